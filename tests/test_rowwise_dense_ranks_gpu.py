"""`RowDenseOutput.ranks` on the MI355X: `row_dense_ranks` and `row_dense_ranks_weighted` themselves on the hand-made record
of the moments test (about one row in eight has left) against the host path; on the bit patterns of the quantiles test, where
keys tie, with the rank identity against `row_dense_quantiles`; and on a real solve against the host path, sliced and whole.
Every comparison is of int64 counts, exact."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, tolerances
from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_moments_gpu import _record
from test_rowwise_dense_quantiles_gpu import _population, _record as _bit_record, _run as _run_quantiles
from test_rowwise_dense_wquantiles import dyadic_weights

import torchdiffeq_amd as tda
from torchdiffeq_amd import rowwise_dense
from torchdiffeq_amd._native import TDEQ_ROW_RANKS_GROUP_VALUES as G
from torchdiffeq_amd.rowwise import HostRowKernels

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345


def _run(k, coeffs, seg, x, values, Q, w=None):
    """The kernel wrappers into bordered outputs -> (below, equal[, total]) on the host; the borders are intact."""
    (V, _, L), B = values.shape, seg.numel() // Q
    sizes = [V * Q * L, V * Q * L] + [Q] * (w is not None)
    flats = [torch.full((n + 16,), SENTINEL, dtype=torch.int64, device=DEV) for n in sizes]
    outs = [f[8:8 + n] for f, n in zip(flats, sizes)]
    outs[:2] = [o.view(V, Q, L) for o in outs[:2]]
    if w is None:
        k.row_dense_ranks(*outs, values, coeffs, seg, x)
    else:
        work = torch.empty(k.row_dense_ranks_weighted_workspace_bytes(Q, B), dtype=torch.uint8, device=DEV)
        k.row_dense_ranks_weighted(*outs, values, coeffs, seg, x, work, w.to(DEV))
    assert all(bool((torch.cat([f[:8], f[8 + n:]]) == SENTINEL).all()) for f, n in zip(flats, sizes))
    return [o.cpu() for o in outs]


def _host(coeffs, seg, x, values, Q, w=None):
    args = (coeffs.cpu(), seg.cpu(), x.cpu(), values.cpu()) + (() if w is None else (w,))
    return (HostRowKernels.quartic_ranks if w is None else HostRowKernels.quartic_ranks_weighted)(*args, Q, seg.numel() // Q)


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1, G + 1, 16])
@pytest.mark.parametrize("B", [1, 2, 1025, 2051])
@pytest.mark.parametrize("L", [1, 3, 65, 36, 68])
def test_kernel_against_host_path(hip_kernels, L, B, V, dtype):
    """B = 1025: the slab boundary, 2051: three slabs.  L = 1, 3: the scalar form; 65: the tile boundary at 64; 36, 68: the
    16-byte form over one and two tiles.  V = G + 1: a second, partial threshold group; 16: four.  Thresholds: values of the
    record's own rows (so `equal` counts), and a NaN and both infinities in single elements.  Unweighted (a row that has left
    is a NaN value), then under per-time weights with zeros among them."""
    Q = 2
    coeffs, seg, x = _record(Q, B, L, dtype)
    rows = torch.randint(0, B, (V,), generator=torch.Generator().manual_seed(V * 100 + B))
    values = coeffs[0].view(Q, B, L)[:, rows.to(DEV)].transpose(0, 1).contiguous()
    values[0, 0, 0], values[-1, -1, -1], values[V // 2, 0, L // 2] = float("nan"), float("inf"), -float("inf")
    got = _run(hip_kernels, coeffs, seg, x, values, Q)
    assert _same(got, _host(coeffs, seg, x, values, Q))
    assert V < 16 or B < 3 or int(got[1].sum()) > 0                   # (16 rows' values: some of those rows are in range)
    w = dyadic_weights((Q, B), B * 100 + L, 2.0 ** 5)
    assert _same(_run(hip_kernels, coeffs, seg, x, values, Q, w), _host(coeffs, seg, x, values, Q, w))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 36])
def test_ties_zeros_infinities_and_nans(hip_kernels, L, dtype):
    """A population drawn from 33 bit patterns (both zeros, the infinities, NaNs, a subnormal), B = 67, so keys tie.  The
    thresholds are what `row_dense_quantiles` selects for 14 ranks: the host path's bits, the rank identity below <= k < below
    + equal, the same under weights (one set for all times), and an invalid weight that zeroes its time alone."""
    Q, B = 2, 67
    coeffs, seg, x = _bit_record(_population(dtype, Q, B, L), dtype)
    ranks = list(range(0, B, 5))
    picked, _ = _run_quantiles(hip_kernels, coeffs, seg, x, ranks, Q)
    values = torch.from_numpy(picked.view(np.float32 if dtype == F32 else np.float64)).to(DEV)
    below, equal = _run(hip_kernels, coeffs, seg, x, values, Q)
    assert _same((below, equal), _host(coeffs, seg, x, values, Q))
    k = torch.tensor(ranks)[:, None, None]
    assert bool(((below <= k) & (k < below + equal)).all()) and int(equal.max()) > 1
    w = dyadic_weights((B,), L + 1)
    good = _run(hip_kernels, coeffs, seg, x, values, Q, w)
    assert _same(good, _host(coeffs, seg, x, values, Q, w))
    w = w.expand(Q, B).clone()
    w[1, 5] = float("inf")
    bad = _run(hip_kernels, coeffs, seg, x, values, Q, w)
    assert _same(bad, _host(coeffs, seg, x, values, Q, w)) and bad[2].tolist() == [int(good[2][0]), 0]
    assert not bool(bad[0][:, 1].any() or bad[1][:, 1].any()) and _same([v[:, 0] for v in bad[:2]], [v[:, 0] for v in good[:2]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_solve_against_host_path_whole_and_sliced(monkeypatch, dtype):
    """Per-row `t1`, B = 67, shared times beyond some rows' `t1` with `check=False`, thresholds per element from the record's
    own rows: the host path on the device's record, unweighted and weighted (a row that has left carries a NaN weight), and the
    same counts when the weighted times run one by one."""
    B, L = 67, 8
    y0, func, _ = decay_problem(B, L, dtype, 3, DEV)
    t1 = per_row_t1(B)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1.to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    twin, shared = _on_host(dense), torch.tensor([0.1, 0.45, 0.55], dtype=F64)
    values = dense(0.1)[[3, 20, 41, 60, 66]]                                             # [V, L] on the device
    w = dyadic_weights((3, B), 21)
    w[2, 0] = float("nan")                                                               # t1[0] = 0.3 < 0.55: not inspected
    for kw in (dict(), dict(weights=w)):
        whole = dense.ranks(shared.to(DEV), values, check=False, **kw)
        assert all(v.device.type == DEV.type for v in whole) and whole.below.shape == (5, 3, L)
        assert _same([v.cpu() for v in whole], twin.ranks(shared, values.cpu(), check=False, **kw))
        assert torch.equal(dense.cdf(shared.to(DEV), values, check=False, **kw).cpu(), twin.cdf(shared, values, check=False, **kw))
        monkeypatch.setattr(rowwise_dense, "QUANTILES_WORKSPACE_BYTES", 1)
        assert _same(dense.ranks(shared.to(DEV), values, check=False, **kw), whole)
        monkeypatch.undo()
        with pytest.raises(ValueError, match=r"dense.ranks\(t\): query 1 of row 0 \(t = 0.45"):
            dense.ranks(shared.to(DEV), values, **kw)
        assert kw or (whole.total.tolist() == [B] * 3 and int(whole.equal[:, 0].min()) >= 1)
    assert whole.total.tolist() != [B] * 3
