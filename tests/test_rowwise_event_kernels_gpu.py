"""The three event kernels of csrc/tdeq_kernels_rowwise_event.hpp on the MI355X against the CPU oracle
(tests/_rowwise_event_oracle.py): the detection on hand-made controller states, the quartic fit and its evaluation bit
for bit on the scalar and the 16-byte paths, with sentinel borders around every output."""
import numpy as np
import pytest
import torch

from _rowwise_event_oracle import EventOracle
from _rowwise_kernels import F64_VECTORS, I32_VECTORS, I64_VECTORS, SENTINEL, RowVectors, ctrl_for, np_type, seeded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
ALPHA = (0.2, 0.3, 0.8, 1.0)
NO_ERROR = 0x7FFFFFFF
BORDER = 8                                                   # elements: 32 / 64 bytes, so the payload stays 16-byte aligned


@pytest.fixture(scope="module")
def oracle(oracle_kernels):
    return EventOracle(oracle_kernels)


def _detect_inputs(B, dtype):
    """Every combination of (accepted, active, fired before) with g1 of both signs, zero and NaN against both starting
    signs — row r takes combination r of the product, so B = 200 sees all 2 * 2 * 2 * 5 * 2 = 80 of them."""
    r = np.arange(B)
    accepted = r % 2
    active = (r // 2) % 2                                    # 0 with accepted = 1: the step reached the last output time
    fired = (r // 4) % 2
    kind = (r // 8) % 5
    sign0 = np.where((r // 40) % 2 == 0, 1, -1)
    sign0 = np.where((fired == 1) & (r % 3 == 0), 0, sign0)  # (some of the rows that fired did so at t0)
    g1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.75 + r, -0.5 - r, 0.0, -0.0], np.nan)
    state = dict(accepted=accepted, active=active, t0=1.0 + 0.125 * r, tprev=0.5 + 0.125 * r)
    return state, torch.tensor(g1, dtype=F64).to(dtype), torch.tensor(sign0, dtype=torch.int32), \
        torch.tensor(fired, dtype=torch.int32)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("B", [1, 64, 65, 200])
def test_detect(B, dtype, sign, hip_kernels, oracle):
    state, g1, sign0, fired0 = _detect_inputs(B, dtype)
    ctrl = ctrl_for(ALPHA, 5, sign, np_type(dtype))
    n_active = int(state["active"].sum())
    results = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        rv = RowVectors(device, B, 3, np.stack([np.zeros(B), np.full(B, 100.0)]), **state)
        rv.v["status"].copy_(torch.tensor([n_active, NO_ERROR], dtype=torch.int32))
        fired = fired0.clone().to(device)
        fired_now = torch.full((B,), 7, dtype=torch.int32, device=device)
        lo = torch.full((B,), SENTINEL, dtype=F64, device=device)
        hi = torch.full((B,), SENTINEL, dtype=F64, device=device)
        # the buffers of the next trial step inside sentinel borders
        dts_buf = torch.full((B + 2 * BORDER,), SENTINEL, dtype=dtype, device=device)
        times_buf = torch.full((len(ALPHA) * B + 2 * BORDER,), SENTINEL, dtype=dtype, device=device)
        dts = dts_buf[BORDER:BORDER + B]
        times = times_buf[BORDER:BORDER + len(ALPHA) * B].view(len(ALPHA), B)
        dts.copy_(torch.arange(B, dtype=F64).to(dtype) * 0.5 + 0.25)
        times.copy_((torch.arange(len(ALPHA) * B, dtype=F64).to(dtype) + 3.0).view(len(ALPHA), B))
        kern.row_event_detect(g1.to(device), sign0.to(device), ctrl, rv.st, dts, times, fired, fired_now, lo, hi)
        if device != "cpu":
            torch.cuda.synchronize()
        out = rv.cpu()
        out.update(fired=fired.cpu(), fired_now=fired_now.cpu(), lo=lo.cpu(), hi=hi.cpu(), dts_buf=dts_buf.cpu(),
                   times_buf=times_buf.cpu())
        results.append(out)
    ref, got = results
    # what the oracle must have done, stated once more from the rule
    s1 = (g1 > 0).to(torch.int32) - (g1 < 0).to(torch.int32)
    now = torch.tensor(state["accepted"] != 0) & (fired0 == 0) & (s1 != sign0)
    assert torch.equal(ref["fired_now"], now.to(torch.int32)) and torch.equal(ref["fired"], fired0 | now.to(torch.int32))
    leave = now & torch.tensor(state["active"] != 0)
    assert int(ref["status"][0]) == n_active - int(leave.sum()) and int(ref["status"][1]) == NO_ERROR
    if B == 200:
        assert int(now.sum()) > 10 and int(leave.sum()) > 5 and int((now & ~leave).sum()) > 5
    for name in sorted(ref):
        assert torch.equal(got[name].view(torch.uint8), ref[name].view(torch.uint8)), name      # (bit for bit: NaN fillers too)
    # untouched: every vector of the state but `active` and `status`, the brackets of the other rows, the borders
    pristine = RowVectors("cpu", B, 3, np.stack([np.zeros(B), np.full(B, 100.0)]), **state).cpu()
    for name in F64_VECTORS + I32_VECTORS + I64_VECTORS + ("tgrid",):
        if name != "active":
            assert torch.equal(got[name], pristine[name]), name
    assert bool((got["lo"][~now] == SENTINEL).all()) and bool((got["hi"][~now] == SENTINEL).all())
    assert torch.equal(got["lo"][now], torch.tensor(state["tprev"])[now]) and torch.equal(got["hi"][now], torch.tensor(state["t0"])[now])
    for buf in ("dts_buf", "times_buf"):
        assert bool((got[buf][:BORDER] == SENTINEL).all()) and bool((got[buf][-BORDER:] == SENTINEL).all())
    frozen = (torch.tensor(state["t0"]) * sign).to(dtype)
    times = got["times_buf"][BORDER:-BORDER].view(len(ALPHA), B)
    assert bool((got["dts_buf"][BORDER:-BORDER][leave] == 0).all()) and bool((times[:, leave] == frozen[leave]).all())
    keep = ~leave
    assert torch.equal(got["dts_buf"][BORDER:-BORDER][keep], (torch.arange(B, dtype=F64).to(dtype) * 0.5 + 0.25)[keep])


def _bordered(shape, dtype, device, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER,), fill, dtype=dtype, device=device)
    return buf, buf[BORDER:BORDER + n].view(*shape)


def _borders_intact(buf):
    return bool((buf[:BORDER] == SENTINEL).all()) and bool((buf[-BORDER:] == SENTINEL).all())


# the term counts of c_mid: bosh3 / fehlberg2 / adaptive_heun 1, dopri5 6, tsit5 7, dopri8 10; 14: the most the entry point takes
@pytest.mark.parametrize("nt", [1, 6, 7, 10, 14])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 8, 1028])
def test_fit_and_eval(L, dtype, nt, hip_kernels, oracle):
    """L = 3: scalar elements; 8, 1028: 16-byte elements (1028: more than one workgroup for the five rows)."""
    B = 5
    y0, y1, f0, f1 = (seeded((B, L), dtype, 10 + i) for i in range(4))
    ks = [seeded((B, L), dtype, 20 + j) for j in range(nt)]
    coefs = [0.37 / (j + 1) * (-1) ** j for j in range(nt)]
    dts = torch.tensor([0.125, -0.3, 0.0, 0.07, 1.5], dtype=F64).to(dtype)
    fired_now = torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32)
    x = torch.tensor([0.0, 0.3, 0.5, 0.77, 1.0], dtype=F64).to(dtype)
    mask = torch.tensor([1, 1, 0, 0, 1], dtype=torch.int32)      # (row 1 evaluates a row of q that was never fitted)
    outs = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        to = lambda t: t.to(device)      # noqa: E731
        q_buf, q = _bordered((5, B, L), dtype, device)
        kern.row_event_fit(q, to(fired_now), to(y0), to(y1), to(f0), to(f1), [to(k) for k in ks], coefs, to(dts))
        out_buf, out = _bordered((B, L), dtype, device)
        kern.row_event_eval(out, q, to(x), to(mask))
        if device != "cpu":
            torch.cuda.synchronize()
        outs.append((q_buf.cpu(), out_buf.cpu()))
    (q_ref, out_ref), (q_got, out_got) = outs
    assert torch.equal(q_got, q_ref) and torch.equal(out_got, out_ref)
    assert _borders_intact(q_got) and _borders_intact(out_got)
    q = q_got[BORDER:-BORDER].view(5, B, L)
    out = out_got[BORDER:-BORDER].view(B, L)
    assert bool((q[:, fired_now == 0] == SENTINEL).all()) and bool((out[mask == 0] == SENTINEL).all())
    assert not bool((q[:, fired_now == 1] == SENTINEL).any())
    # the quartic's ends: e = y0; at x = 0 the value is y0, at x = 1 it is y1 to rounding
    assert torch.equal(q[0, 0], y0[0]) and torch.equal(out[0], y0[0])
    scale = float(max(y0.abs().max(), y1.abs().max(), f0.abs().max(), f1.abs().max()))
    eps = torch.finfo(dtype).eps
    assert float((out[4] - y1[4]).abs().max()) <= 200 * (1 + abs(float(dts[4]))) * (1 + sum(abs(c) for c in coefs)) * scale * eps
