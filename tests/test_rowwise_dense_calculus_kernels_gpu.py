"""`row_dense_prefix` and `row_dense_calc` (csrc/tdeq_kernels_rowwise_dense.hpp) on the MI355X against the numpy oracle of
tests/_rowwise_dense_calculus_oracle.py, bit for bit, on synthetic records: ragged rows (one segment next to about 700),
row lengths on both sides of the 16-byte element, batches that end inside a wave, both dtypes, both directions, coefficients
of mixed sign and magnitude — every output inside sentinel borders."""
import functools

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import ANTIDERIVATIVE, DERIVATIVE, INTEGRAL, np_calc, np_prefix, same_bits
from _rowwise_dense_oracle import NONE
from _rowwise_kernels import SENTINEL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
BORDER = 8                                                   # elements: the payload stays 16-byte aligned
LONG = 700


def _bordered(shape, dtype, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER + shift,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[BORDER + shift:BORDER + shift + n].view(*shape)


def _payload_only(buf, shape, shift=0):
    n = int(np.prod(shape))
    host = buf.cpu()
    return bool((host[:BORDER + shift] == SENTINEL).all()) and bool((host[BORDER + shift + n:] == SENTINEL).all())


def _counts(B):
    """Rows of 1 .. 4 segments, one-segment rows next to the one long row in the middle."""
    counts = [1 + (r * 5) % 4 for r in range(B)]
    mid = B // 2
    counts[mid] = LONG
    for r in (mid - 1, mid + 1):
        if 0 <= r < B:
            counts[r] = 1
    return counts


@functools.lru_cache(maxsize=None)
def _record(B, L, dtype):
    """A synthetic record and its queries, with the numpy reference of everything — computed once per shape.  Queries per
    row [7, B]: t0, t1, an interior breakpoint (t1 again for a one-segment row), three interior points, one out of range
    (below t0, beyond t1 or NaN in turn)."""
    g = torch.Generator().manual_seed(1000 * B + L)
    counts = _counts(B)
    n_seg = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ta, tb, t0, t1 = np.empty(n_seg), np.empty(n_seg), np.empty(B), np.empty(B)
    for r, n in enumerate(counts):
        edges = 0.1 * r + np.concatenate([[0.0], np.cumsum(0.01 + 0.05 * torch.rand(n, generator=g, dtype=F64).numpy())])
        ta[off[r]:off[r + 1]], tb[off[r]:off[r + 1]] = edges[:-1], edges[1:]
        t0[r], t1[r] = edges[0], edges[-2] + 0.75 * (edges[-1] - edges[-2])
    scale = 10.0 ** (6 * torch.rand(5, n_seg, L, generator=g, dtype=F64) - 3)
    coeffs = (torch.randn(5, n_seg, L, generator=g, dtype=F64) * scale).to(dtype).numpy()
    q = np.empty((7, B))
    for r in range(B):
        lo, hi = off[r], off[r + 1]
        span = t1[r] - t0[r]
        q[:, r] = [t0[r], t1[r], tb[lo + (hi - lo) // 2 - 1] if hi - lo > 1 else t1[r], t0[r] + 0.3 * span, t0[r] + 0.6 * span,
                   t0[r] + 0.9 * span, (t0[r] - 1e-3, t1[r] + (tb[hi - 1] - t1[r]) / 2, np.nan)[r % 3]]
    q2 = q[[3, 0, 1, 5, 2, 6, 4]]                                            # the integral's other ends (row 5: out of range)
    return dict(off=off, ta=ta, tb=tb, t0=t0, t1=t1, coeffs=coeffs, q=q, q2=q2, P=np_prefix(coeffs, off, ta, tb))


def _search(hip_kernels, rec, q, dtype):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    n = q.size
    seg = torch.empty(n, dtype=torch.int32, device=DEV)
    x = torch.empty(n, dtype=dtype, device=DEV)
    status = torch.tensor([NONE], dtype=torch.int32, device=DEV)
    hip_kernels.row_dense_search(dev(q), dev(rec["off"]), dev(rec["ta"]), dev(rec["tb"]), dev(rec["t0"]), dev(rec["t1"]), seg, x,
                                 status)
    return seg, x, dev(q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3, 67])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 130])
def test_prefix_and_calc_equal_the_oracle(L, B, dtype, hip_kernels):
    """L = 1, 3, 5: scalar elements; 4: one 16-byte element of fp32 (two of fp64); 130: scalar for fp32, 65 elements of fp64 —
    more than one wave per row.  B = 3, 67: the last wave is partial.  The long row's 700 segments are walked by one lane per
    element next to rows of one segment."""
    rec = _record(B, L, dtype)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    n_seg = rec["ta"].size
    coeffs, off, ta, tb = dev(rec["coeffs"]), dev(rec["off"]), dev(rec["ta"]), dev(rec["tb"])
    p_buf, P = _bordered((n_seg, L), F64)
    hip_kernels.row_dense_prefix(P, coeffs, off, ta, tb)
    torch.cuda.synchronize()
    assert _payload_only(p_buf, (n_seg, L))
    assert same_bits(P, torch.from_numpy(rec["P"]))
    seg, x, tq = _search(hip_kernels, rec, rec["q"], dtype)
    seg2, x2, tq2 = _search(hip_kernels, rec, rec["q2"], dtype)
    n = rec["q"].size
    host = [t.cpu().numpy().reshape(-1) for t in (seg, x, tq, seg2, x2, tq2)]
    bad = np.zeros((7, B), dtype=bool)
    bad[6] = True
    for sign in (1.0, -1.0):
        for mode in (DERIVATIVE, ANTIDERIVATIVE, INTEGRAL):
            o_buf, out = _bordered((n, L), dtype)
            hip_kernels.row_dense_calc(out, mode, coeffs, ta, tb, None if mode == DERIVATIVE else P, sign, seg, x,
                                       *((tq, seg2, x2, tq2) if mode == INTEGRAL else (tq,) if mode else ()))
            torch.cuda.synchronize()
            assert _payload_only(o_buf, (n, L)), (sign, mode)
            want = np_calc(mode, rec["coeffs"], rec["P"], rec["ta"], rec["tb"], sign, *host[:6 if mode == INTEGRAL else 3])
            assert same_bits(out, torch.from_numpy(want)), (sign, mode)
            nan_rows = torch.isnan(out.cpu()).view(7, B, L).all(dim=2).numpy()
            both = bad | bad[[3, 0, 1, 5, 2, 6, 4]] if mode == INTEGRAL else bad
            assert np.array_equal(nan_rows, both), (sign, mode)                # out of range: a row of NaN, and no other
    # t0: F == 0 exactly; an interior breakpoint (x = 1 of the earlier segment): T(sign * P[s + 1])
    out = torch.empty(n, L, dtype=dtype, device=DEV)
    hip_kernels.row_dense_calc(out, ANTIDERIVATIVE, coeffs, ta, tb, P, 1.0, seg, x, tq)
    F = out.cpu().view(7, B, L)
    assert bool((F[0] == 0).all())
    for r in range(B):
        s = int(host[0][2 * B + r])
        if s + 1 < rec["off"][r + 1]:
            assert float(host[1][2 * B + r]) == 1.0 and same_bits(F[2, r], torch.from_numpy(rec["P"][s + 1]).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shifted", ["prefix", "out"])
def test_misaligned_base_takes_the_scalar_path(shifted, dtype, hip_kernels):
    """L = 4 allows 16-byte elements, but a `prefix` or `out` one element off a 16-byte boundary must take scalar elements:
    the same bits, nothing outside the payload."""
    B, L = 3, 4
    rec = _record(B, L, dtype)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    n_seg, n = rec["ta"].size, rec["q"].size
    coeffs, off, ta, tb = dev(rec["coeffs"]), dev(rec["off"]), dev(rec["ta"]), dev(rec["tb"])
    p_shift, o_shift = (1, 0) if shifted == "prefix" else (0, 1)
    p_buf, P = _bordered((n_seg, L), F64, p_shift)
    assert (P.data_ptr() % 16 != 0) == (shifted == "prefix")
    hip_kernels.row_dense_prefix(P, coeffs, off, ta, tb)
    seg, x, tq = _search(hip_kernels, rec, rec["q"], dtype)
    host = [t.cpu().numpy().reshape(-1) for t in (seg, x, tq)]
    torch.cuda.synchronize()
    assert _payload_only(p_buf, (n_seg, L), p_shift) and same_bits(P, torch.from_numpy(rec["P"]))
    for mode in (DERIVATIVE, ANTIDERIVATIVE):
        o_buf, out = _bordered((n, L), dtype, o_shift)
        assert (out.data_ptr() % 16 != 0) == (shifted == "out")
        hip_kernels.row_dense_calc(out, mode, coeffs, ta, tb, P, 1.0, seg, x, tq)
        torch.cuda.synchronize()
        assert _payload_only(o_buf, (n, L), o_shift)
        assert same_bits(out, torch.from_numpy(np_calc(mode, rec["coeffs"], rec["P"], rec["ta"], rec["tb"], 1.0, *host)))
