"""The two kernels of a compacted event solve (csrc/tdeq_kernels_rowwise_event.hpp: `row_event_fit_mapped`,
`row_event_eval_mapped`) on the MI355X against the CPU oracle (tests/_rowwise_event_compact_oracle.py): bit for bit on the
scalar and the 16-byte paths, through a non-monotone row map, with sentinel borders around every output and every row
that is not addressed still sentinel.  Shapes, seeds and borders are those of tests/test_rowwise_event_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from _rowwise_event_compact_oracle import EventCompactOracle
from _rowwise_kernels import SENTINEL, seeded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
BORDER = 8                                                   # elements: 32 / 64 bytes, so the payload stays 16-byte aligned
N, Q_ROWS = 5, 9
ROW_MAP = [7, 0, 3, 8, 4]                                    # compact row -> row of q
FIRED_NOW = [1, 0, 1, 0, 1]


@pytest.fixture(scope="module")
def oracle(oracle_kernels):
    return EventCompactOracle(oracle_kernels)


def _bordered(shape, dtype, device, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER,), fill, dtype=dtype, device=device)
    return buf, buf[BORDER:BORDER + n].view(*shape)


def _borders_intact(buf):
    return bool((buf[:BORDER] == SENTINEL).all()) and bool((buf[-BORDER:] == SENTINEL).all())


def _i32(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


# the term counts of c_mid: bosh3 / fehlberg2 / adaptive_heun 1, dopri5 6, tsit5 7, dopri8 10; 14: the most the entry point takes
@pytest.mark.parametrize("nt", [1, 6, 7, 10, 14])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 8, 1028])
def test_fit_mapped_and_eval_mapped(L, dtype, nt, hip_kernels, oracle):
    """L = 3: scalar elements; 8, 1028: 16-byte elements (1028: more than one workgroup for the five rows)."""
    y0, y1, f0, f1 = (seeded((N, L), dtype, 10 + i) for i in range(4))
    ks = [seeded((N, L), dtype, 20 + j) for j in range(nt)]
    coefs = [0.37 / (j + 1) * (-1) ** j for j in range(nt)]
    dts = torch.tensor([0.125, -0.3, 0.0, 0.07, 1.5], dtype=F64).to(dtype)
    fitted = [ROW_MAP[r] for r in range(N) if FIRED_NOW[r]]                     # rows 7, 3, 4 of q
    src = [4, 7, 3]                                                             # the index list: in another order
    x = torch.tensor([1.0, 0.0, 0.77], dtype=F64).to(dtype)
    dst = [5, 0, 2]                                                             # rows of a 6-row output
    outs = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        to = lambda t: t.to(device)      # noqa: E731
        q_buf, q = _bordered((5, Q_ROWS, L), dtype, device)
        kern.row_event_fit_mapped(q, _i32(ROW_MAP, device), _i32(FIRED_NOW, device), to(y0), to(y1), to(f0), to(f1),
                                  [to(k) for k in ks], coefs, to(dts))
        compact_buf, compact = _bordered((3, L), dtype, device)                  # dst_map = NULL: the rows of the list
        kern.row_event_eval_mapped(compact, None, q, _i32(src, device), to(x))
        full_buf, full = _bordered((6, L), dtype, device)
        kern.row_event_eval_mapped(full, _i32(dst, device), q, _i32(src, device), to(x))
        none_buf, none = _bordered((6, L), dtype, device)                        # n_idx == 0: nothing is written
        kern.row_event_eval_mapped(none, _i32([], device), q, _i32([], device), to(x[:0]))
        if device != "cpu":
            torch.cuda.synchronize()
        outs.append([b.cpu() for b in (q_buf, compact_buf, full_buf, none_buf)])
    ref, got = outs
    for r, g in zip(ref, got):
        assert torch.equal(g, r) and _borders_intact(g)
    q = got[0][BORDER:-BORDER].view(5, Q_ROWS, L)
    others = [r for r in range(Q_ROWS) if r not in fitted]
    assert bool((q[:, others] == SENTINEL).all()) and not bool((q[:, fitted] == SENTINEL).any())
    compact = got[1][BORDER:-BORDER].view(3, L)
    full = got[2][BORDER:-BORDER].view(6, L)
    assert not bool((compact == SENTINEL).any())
    assert torch.equal(full[dst], compact) and bool((full[[1, 3, 4]] == SENTINEL).all())
    assert bool((got[3] == SENTINEL).all())
    # the quartic's ends: e = y0 (compact row 0 went to row 7 of q); at x = 0 the value is y0, at x = 1 it is y1 to rounding
    assert torch.equal(q[0, 7], y0[0]) and torch.equal(compact[1], y0[0])
    scale = float(max(y0.abs().max(), y1.abs().max(), f0.abs().max(), f1.abs().max()))
    eps = torch.finfo(dtype).eps
    assert float((compact[0] - y1[4]).abs().max()) <= 200 * (1 + abs(float(dts[4]))) * (1 + sum(abs(c) for c in coefs)) * scale * eps


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_fit_mapped_with_the_identity_map_is_fit(dtype, hip_kernels):
    """row_map = arange(n) into a q of n rows: the bits of `row_event_fit`."""
    L, nt = 8, 6
    y0, y1, f0, f1 = (seeded((N, L), dtype, 10 + i).to(DEV) for i in range(4))
    ks = [seeded((N, L), dtype, 20 + j).to(DEV) for j in range(nt)]
    coefs = [0.37 / (j + 1) * (-1) ** j for j in range(nt)]
    dts = torch.tensor([0.125, -0.3, 0.0, 0.07, 1.5], dtype=F64).to(dtype).to(DEV)
    fired_now = _i32(FIRED_NOW, DEV)
    a = torch.full((5, N, L), SENTINEL, dtype=dtype, device=DEV)
    b = a.clone()
    hip_kernels.row_event_fit(a, fired_now, y0, y1, f0, f1, ks, coefs, dts)
    hip_kernels.row_event_fit_mapped(b, _i32(list(range(N)), DEV), fired_now, y0, y1, f0, f1, ks, coefs, dts)
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), b.cpu())
