"""`min_step`, `max_step`, `step_t`, `jump_t` per row on the MI355X: the HIP kernels against the torch-op host path, batch
invariance, compaction for the three entry points, and a refresh call whose output is NaN for every row that did not
jump."""
import pytest
import torch

from _rowwise_steps_oracle import (METHODS, assert_device_matches_host, device_problem, device_tolerances, quiet,  # noqa: F401
                                   switched_problem)

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
NAN = float("nan")


@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 129])
@pytest.mark.parametrize("method", METHODS)
def test_hip_matches_host_path(method, L, dtype, direction):
    """The problem of tests/test_rowwise_steps.py::test_device_driver_matches_host_path, where the driver on the oracle —
    the kernels' arithmetic — leaves no fp32 row with other counts than the host path."""
    y0, f, t, options = device_problem(dtype, L, direction)
    kw = dict(method=method, options=options, return_stats=True, **device_tolerances(dtype))
    host, sh = tda.odeint_rowwise(f, y0, t, **kw)
    y0d, fd, td, _ = device_problem(dtype, L, direction, DEV)
    dev, sd = tda.odeint_rowwise(fd, y0d, td, **kw)
    assert dev.device.type == "cuda"
    assert_device_matches_host(dev, sd, host, sh, dtype, method)


def _batch64(dtype):
    B = 64
    y0, make, _ = switched_problem(B, 5, dtype, 9, DEV)
    g = torch.Generator().manual_seed(3)
    jump = 0.1 + 0.8 * torch.rand(2, B, generator=g, dtype=F64)
    jump[1, ::3] = NAN
    step = 0.05 + 0.9 * torch.rand(1, B, generator=g, dtype=F64)
    step[0, ::4] = NAN
    lo, hi = torch.full((B,), 1e-6, dtype=F64), 0.05 + 0.5 * torch.rand(B, generator=g, dtype=F64)
    tg = torch.linspace(0, 1, 3, dtype=F64)[:, None] * torch.linspace(0.3, 1.0, B, dtype=F64)
    return y0, make, jump, step, lo, hi, tg


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_hip_batch_invariance(dtype):
    y0, make, jump, step, lo, hi, tg = _batch64(dtype)
    kw = dict(return_stats=True, **device_tolerances(dtype))
    full, sf = tda.odeint_rowwise(make(jump), y0, tg.to(DEV), options={"jump_t": jump, "step_t": step, "min_step": lo,
                                                                       "max_step": hi}, **kw)
    assert int(sf["n_accepted"].sum()) > 3 * 64
    rows = torch.randperm(64, generator=torch.Generator().manual_seed(5))[:23].sort().values
    part, sp = tda.odeint_rowwise(make(jump, rows_of=rows.to(DEV)), y0[rows.to(DEV)], tg[:, rows].to(DEV),
                                  options={"jump_t": jump[:, rows], "step_t": step[:, rows], "min_step": lo[rows],
                                           "max_step": hi[rows]}, **kw)
    assert torch.equal(part, full[:, rows.to(DEV)])
    assert torch.equal(sp["n_accepted"], sf["n_accepted"][rows]) and torch.equal(sp["n_rejected"], sf["n_rejected"][rows])


def test_hip_compaction_is_bit_exact():
    dtype = torch.float32
    y0, make, jump, step, lo, hi, tg = _batch64(dtype)
    tg = tg.to(DEV)
    options = {"jump_t": jump, "step_t": step, "min_step": lo, "max_step": hi}
    kw = dict(options=options, return_stats=True, **device_tolerances(dtype))
    plain, rows = make(jump), make(jump, by_rows=True)
    a, sa = tda.odeint_rowwise(plain, y0, tg, **kw)
    b, sb = tda.odeint_rowwise(rows, y0, tg, compact=1.0, **kw)
    assert torch.equal(a, b) and torch.equal(sa["n_accepted"], sb["n_accepted"]) and sb["n_repacks"] > 0
    level = y0[:, 0] * 0.5 + 0.4
    ea, xa, ta = tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=lambda t, y: y[:, 0] - level, t_end=tg[-1], **kw)
    eb, xb, tb = tda.odeint_rowwise_event(rows, y0, 0.0, event_fn=lambda t, y, r: y[:, 0] - level[r], t_end=tg[-1],
                                          compact=1.0, **kw)
    assert torch.equal(ea, eb) and torch.equal(xa, xb) and torch.equal(ta["n_accepted"], tb["n_accepted"])
    assert 0 < int(ta["fired"].sum()) and tb["n_repacks"] > 0
    da, ua = tda.odeint_rowwise_dense(plain, y0, 0.0, tg[-1], **kw)
    db, ub = tda.odeint_rowwise_dense(rows, y0, 0.0, tg[-1], compact=1.0, **kw)
    for name in ("offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(da, name), getattr(db, name)), name
    assert torch.equal(ua["n_accepted"], ub["n_accepted"]) and ub["n_repacks"] > 0
    q = (tg[-1] * 0.37)[None]
    assert torch.equal(da(q), tda.odeint_rowwise(plain, y0, torch.cat([tg[:1], q, tg[-1:]]), **kw)[0][1:2])


def test_hip_poisoned_refresh():
    """A finished row and a row that did not jump get NaN from `func` in every refresh call (the calls at a time just
    behind a jump point of SOME row): the result keeps its bits — the pattern of test_hip_finished_rows_ignore_nan."""
    B, L, dtype = 6, 129, torch.float64
    y0, make, _ = switched_problem(B, L, dtype, 11, DEV)
    jump = torch.tensor([[0.5, NAN, 0.3, NAN, 0.7, 0.45]], dtype=F64)
    tg = (torch.linspace(0, 1, 3, dtype=F64)[:, None] * torch.tensor([1.0, 1.0, 1.0, 0.2, 1.0, 0.4], dtype=F64)).to(DEV)
    f = make(jump)
    behind = torch.nextafter(jump[0].to(DEV), torch.full((B,), 2.0, dtype=F64, device=DEV))      # NaN where there is none
    calls = [0]

    def poisoned(t, y):
        out = f(t, y)
        refresh = t == behind                                # the rows of this call that sit just behind their own point
        if bool(refresh.any()):
            calls[0] += 1
            out = torch.where(refresh[:, None], out, torch.full_like(out, NAN))
        return out

    kw = dict(options={"jump_t": jump}, return_stats=True, rtol=1e-6, atol=1e-8)
    clean, sc = tda.odeint_rowwise(f, y0, tg, **kw)
    dirty, sd = tda.odeint_rowwise(poisoned, y0, tg, **kw)
    assert calls[0] >= 3
    assert torch.equal(dirty, clean) and bool(torch.isfinite(dirty).all())
    assert torch.equal(sd["n_accepted"], sc["n_accepted"]) and torch.equal(sd["n_rejected"], sc["n_rejected"])
    assert sd["nfe"] == sc["nfe"]
