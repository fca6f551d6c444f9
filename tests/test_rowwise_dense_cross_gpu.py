"""`RowDenseOutput.cross_covariance` on the MI355X: `row_dense_cross` itself on the hand-made record of the moments test
against the two-pass numpy.longdouble reference of tests/test_rowwise_dense_cross.py (its docstring derives the bound) on the
values the `dense(t)` kernel gives that record; `count` and `ybar` with the bits of `row_dense_moments`; the same bits from run
to run and for any slicing of the times; and the device against the host path and a cross-time reference on a real solve.
`other` is 50 + scale_m * randn and the values are 1e3 + scale_el * randn, so a one-pass E[yz] - E[y] E[z] would be off by
about n * 2^-53 * 5e4 against covariances of order 1."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, tolerances
from test_rowwise_dense_cross import reference
from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_moments_gpu import _close, _record, _values

import torchdiffeq_amd as tda
from torchdiffeq_amd._native import TDEQ_ROW_MOMENTS_SLAB_ROWS as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345


def _other(B, M, took):
    """z [B, M] fp64 on the device; NaN in the rows that are in no time's population."""
    g = torch.Generator().manual_seed(B * 100 + M)
    z = 50 + torch.linspace(0.5, 2.0, M, dtype=F64) * torch.randn(B, M, generator=g, dtype=F64)
    z[torch.from_numpy(~took.any(axis=0))] = float("nan")
    return z.to(DEV)


def _run(k, coeffs, seg, x, z, Q, correction):
    """`row_dense_cross` into bordered outputs -> (out [Q, L, M], count [Q], ybar [Q, L]) as numpy arrays; the borders are
    intact."""
    L, B, M = coeffs.shape[2], seg.numel() // Q, z.shape[1]
    shapes = [((Q, L, M), F64), ((Q,), torch.int64), ((Q, L), F64)]
    flats = [torch.full((int(np.prod(s)) + 16,), SENTINEL, dtype=t, device=DEV) for s, t in shapes]
    outs = [f[8:-8].view(s) for f, (s, _) in zip(flats, shapes)]
    work = torch.empty(k.row_dense_cross_workspace_bytes(Q, B, L, M, coeffs.dtype), dtype=torch.uint8, device=DEV)
    k.row_dense_cross(*outs, z, correction, coeffs, seg, x, work)
    for f in flats:
        assert bool((torch.cat([f[:8], f[-8:]]) == SENTINEL).all())
    return [o.cpu().numpy() for o in outs]


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 67, R + 1])
@pytest.mark.parametrize("M", [1, 16, 17, 70])
@pytest.mark.parametrize("L", [5, 8, 70])
def test_kernel_against_longdouble(hip_kernels, L, M, B, Q, dtype):
    """L = 5: scalar loads; 8: 16-byte loads; 70: two element tiles, the second a tail.  M = 1: the 16-column block with one
    column; 16: that block full; 17: the first shape of the 64-column block; 70: two covariate tiles, the second a tail.  B = 1:
    an empty divisor with correction = 1; 3: fewer rows than a k-step; 67: several chunks and a partial one; R + 1: two slabs.
    About one row in eight has left; where it has left every time its `other` entries are NaN."""
    coeffs, seg, x = _record(Q, B, L, dtype)
    y, took = _values(hip_kernels, coeffs, seg, x, Q)
    z = _other(B, M, took)
    count, mean, var = torch.empty(Q, dtype=torch.int64, device=DEV), *torch.empty(2, Q, L, dtype=F64, device=DEV)
    work = torch.empty(hip_kernels.row_dense_moments_workspace_bytes(False, Q, B, L, dtype), dtype=torch.uint8, device=DEV)
    hip_kernels.row_dense_moments(count, mean, var, None, 1, coeffs, seg, x, work)
    for correction in (0, 1):
        out, n, ybar = _run(hip_kernels, coeffs, seg, x, z, Q, correction)
        assert np.array_equal(n, count.cpu().numpy()) and _same_bits(ybar, mean.cpu().numpy())
        for j in range(Q):
            n_ref, ref, tol = reference(y[j], z.cpu().numpy(), took[j], correction)
            assert n[j] == n_ref and _close(out[j], ref, tol), j


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [16, 70])
def test_same_bits_twice_and_for_sliced_times(hip_kernels, M, dtype):
    """The same call twice, and Q = 3 against three calls of Q = 1 (two slabs, both block shapes): the same bits."""
    Q, B, L = 3, R + 1, 70
    coeffs, seg, x = _record(Q, B, L, dtype)
    z = _other(B, M, np.ones((1, B), dtype=bool))
    whole = _run(hip_kernels, coeffs, seg, x, z, Q, 1)
    again = _run(hip_kernels, coeffs, seg, x, z, Q, 1)
    assert all(_same_bits(a, b) for a, b in zip(whole, again))
    for j in range(Q):
        part = _run(hip_kernels, coeffs, seg[j * B:(j + 1) * B], x[j * B:(j + 1) * B], z, 1, 1)
        assert all(_same_bits(a[j:j + 1], b) for a, b in zip(whole, part)), j


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_solve_against_host_path_and_across_time(dtype):
    """Per-row `t1`, B = 67, shared times beyond some rows' `t1` with `check=False`: the device against the longdouble
    reference on its own `dense(t)` within the bound and against the host path on its record within twice the bound — with
    sampled covariates on the CPU and, for the covariance across time, with `dense(t_ref)`; `check=True` raises."""
    B, L = 67, 8
    y0, func, k = decay_problem(B, L, dtype, 3, DEV)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, per_row_t1(B).to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    twin = _on_host(dense)
    shared = torch.tensor([0.1, 0.45, 0.55], dtype=F64)
    y = dense(shared.to(DEV), check=False).cpu().numpy()
    took = ~np.isnan(y[:, :, 0])
    assert took[0].all() and 2 <= took[2].sum() < B
    for other in (torch.cat([k.cpu().double(), y0.cpu().double()[:, :2]], dim=1), dense(0.1).reshape(B, L)):
        got = dense.cross_covariance(shared.to(DEV), other, check=False)
        assert got.device.type == DEV.type and got.dtype == F64 and got.shape == (3, L, other.shape[1])
        host = twin.cross_covariance(shared, other.cpu(), check=False).numpy().astype(np.longdouble)
        for j in range(3):
            _, ref, tol = reference(y[j], other.cpu().double().numpy(), took[j], 1)
            assert _close(got[j].cpu().numpy(), ref, tol) and _close(got[j].cpu().numpy(), host[j], tol, 2), j
    with pytest.raises(ValueError, match=r"dense.cross_covariance\(t, other\): query 1 of row 0 \(t = 0.45"):
        dense.cross_covariance(shared.to(DEV), other)
    one = dense.cross_covariance(0.1, other)
    assert one.shape == (L, L) and torch.equal(one, got[0])
