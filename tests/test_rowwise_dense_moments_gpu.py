"""`RowDenseOutput.moments` on the MI355X: `row_dense_moments` itself on a hand-made record against a two-pass reference in
numpy.longdouble on the values the `dense(t)` kernel gives that record; the same bits from run to run and the same answer
however the rows fall into slabs; and the device against the reference and the host path on a real solve.

Tolerances (derived, not measured), with u = 2^-53, n = count, d the reference deviations and A_i = mean_r |y_ri|:
    |mean_i - ref| <= 2 n u A_i
    |cov_ij - ref| <= 2 ((n + 3) u sum_r |d_ri d_rj| + n (n u)^2 A_i A_j) / (n - correction)      (variance: i = j)
the bound of a sum of n rounded products in any order plus the second-order term of the rounded mean (the first-order term
vanishes: deviations from the exact mean sum to zero), with a factor 2 of headroom.  Values are 1e3 + scale_el * randn, so a
one-pass E[x^2] - E[x]^2 would be off by about n * 2^-53 * 1e6 against variances of order 1."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, tolerances
from test_rowwise_dense_level_gpu import _on_host

import torchdiffeq_amd as tda
from torchdiffeq_amd._native import TDEQ_ROW_MOMENTS_SLAB_ROWS as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345
U = 2.0 ** -53
LD = np.longdouble


def _reference(y, took, correction):
    """y [Q, B, L] floats, took [Q, B] bool -> per time (count, mean, cov, mean_tol, cov_tol) of the rows that took part, two
    passes in longdouble; the divisor max(n - correction, 0), a zero one by IEEE division."""
    out = []
    with np.errstate(all="ignore"):
        for yq, tq in zip(y, took):
            v = yq[tq].astype(LD)
            n = len(v)
            mean = v.sum(axis=0) / LD(n)
            d = v - mean
            div = LD(max(n - correction, 0))
            A = np.abs(v).sum(axis=0) / LD(max(n, 1))
            cov_tol = 2 * ((n + 3) * U * (np.abs(d).T @ np.abs(d)) + n * (n * U) ** 2 * np.outer(A, A)) / max(n - correction, 1)
            out.append((n, mean, (d.T @ d) / div, 2 * n * U * A, cov_tol))
    return out


def _close(got, ref, tol, slack=1):
    """Within `slack * tol` where the reference is finite, and the same NaN / inf elsewhere."""
    finite = np.isfinite(ref.astype(np.float64))
    return (np.array_equal(got[~finite], ref[~finite].astype(np.float64), equal_nan=True)
            and bool((np.abs(got[finite].astype(LD) - ref[finite]) <= slack * tol[finite]).all()))


def _check(got, ref, covariance, slack=1):
    """got: (count, mean, variance, covariance) as numpy arrays with Q in front, against `_reference`."""
    count, mean, var, cov = got
    for j, (n, r_mean, r_cov, mean_tol, cov_tol) in enumerate(ref):
        assert count[j] == n
        assert _close(mean[j], r_mean, mean_tol, slack), ("mean", j)
        assert _close(var[j], np.diagonal(r_cov), np.diagonal(cov_tol), slack), ("variance", j)
        if covariance:
            assert _close(cov[j], r_cov, cov_tol, slack), ("covariance", j)
            assert np.array_equal(cov[j], cov[j].T, equal_nan=True)                       # the mirror: bit for bit
            assert np.array_equal(np.diagonal(cov[j]), var[j], equal_nan=True)            # the diagonal rule


def _record(Q, B, L, dtype):
    """The record whose (query, row) value is y[q, r] exactly: plane e holds the values, the planes d .. a are zero, seg =
    arange, x = 0, or NaN for about one row in eight, which has left -> (coeffs [5, Q * B, L], seg, x)."""
    g = torch.Generator().manual_seed(B * 1000 + L * 10 + Q)
    y = 1e3 + torch.linspace(0.5, 2.0, L, dtype=F64) * torch.randn(Q * B, L, generator=g, dtype=F64)
    coeffs = torch.zeros(5, Q * B, L, dtype=dtype, device=DEV)
    coeffs[0] = y.to(dtype).to(DEV)
    left = torch.rand(Q, B, generator=g) < 0.125
    left[:, :2] &= B < 3                                                          # (B >= 3: at least two rows stay)
    x = torch.where(left.reshape(-1), float("nan"), 0.0).to(dtype).to(DEV)
    return coeffs, torch.arange(Q * B, dtype=torch.int32, device=DEV), x


def _values(k, coeffs, seg, x, Q):
    """What the kernel of `dense(t)` gives the queries -> (y [Q, B, L] numpy, took part [Q, B])."""
    y = torch.empty(seg.numel(), coeffs.shape[2], dtype=coeffs.dtype, device=DEV)
    k.row_event_eval_mapped(y, None, coeffs, seg, x)
    return y.cpu().numpy().reshape(Q, -1, coeffs.shape[2]), ~x.isnan().cpu().numpy().reshape(Q, -1)


def _run(k, coeffs, seg, x, Q, correction, covariance, offset=0):
    """`row_dense_moments` into bordered outputs `offset` elements off a 16-byte boundary -> (count, mean, variance, covariance
    or None) as numpy arrays; the borders are intact."""
    L, B = coeffs.shape[2], seg.numel() // Q
    shapes = [((Q,), torch.int64), ((Q, L), F64), ((Q, L), F64)] + ([((Q, L, L), F64)] if covariance else [])
    flats = [torch.full((int(np.prod(s)) + 16,), SENTINEL, dtype=t, device=DEV) for s, t in shapes]
    outs = [f[8 + offset:f.numel() - 8 + offset].view(s) for f, (s, _) in zip(flats, shapes)] + [None] * (not covariance)
    work = torch.empty(k.row_dense_moments_workspace_bytes(covariance, Q, B, L, coeffs.dtype), dtype=torch.uint8, device=DEV)
    k.row_dense_moments(*outs, correction, coeffs, seg, x, work)
    for f in flats:
        assert bool((torch.cat([f[:8 + offset], f[f.numel() - 8 + offset:]]) == SENTINEL).all())
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 67, R + 1])
@pytest.mark.parametrize("L", [5, 8, 70])
def test_kernel_against_longdouble(hip_kernels, L, B, Q, dtype):
    """L = 5: scalar loads; 8: 16-byte loads; 70: two element tiles, the second a tail, three tile pairs and the off-diagonal
    block.  B = 1: an empty divisor with correction = 1; 3: fewer rows than one k step of the matrix instruction; 67: several
    chunks and a partial one; R + 1: two slabs.  In one case the outputs sit one element off a 16-byte boundary."""
    coeffs, seg, x = _record(Q, B, L, dtype)
    y, took = _values(hip_kernels, coeffs, seg, x, Q)
    assert B < 3 or took.sum(axis=1).min() >= 2
    for correction in (0, 1):
        ref = _reference(y, took, correction)
        for covariance in (False, True):
            got = _run(hip_kernels, coeffs, seg, x, Q, correction, covariance, offset=int(B == 67 and Q == 3))
            _check(got, ref, covariance)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_twice_and_any_slabs(hip_kernels, dtype):
    """The same call twice: the same bits in every output.  67 rows scattered over R + 1 rows whose other rows have left (two
    slabs): the count and, within the bound, the values of the 67 rows alone."""
    B, L = 67, 70
    coeffs, seg, _ = _record(1, B, L, dtype)
    x = torch.zeros(B, dtype=dtype, device=DEV)
    at = torch.linspace(0, R, B).round().long().to(DEV)                           # rows 0 and R included: both slabs hold some
    spread_seg = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    spread_x = torch.full((R + 1,), float("nan"), dtype=dtype, device=DEV)
    spread_seg[at], spread_x[at] = seg, x
    y, took = _values(hip_kernels, coeffs, seg, x, 1)
    ref = _reference(y, took, 1)
    alone = _run(hip_kernels, coeffs, seg, x, 1, 1, True)
    again = _run(hip_kernels, coeffs, seg, x, 1, 1, True)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(alone, again))
    spread = _run(hip_kernels, coeffs, spread_seg, spread_x, 1, 1, True)
    _check(alone, ref, True)
    _check(spread, ref, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
def test_real_solve_against_its_own_dense(L, dtype):
    """Per-row `t1`, B = 67, shared times beyond some rows' `t1` with `check=False`: `count` is the number of rows with `t1 >=
    t`; the moments agree with the longdouble reference on the non-NaN rows of the device's own `dense(t, check=False)` within
    the bound and with the host path on the device's record within twice the bound; `check=True` raises like `dense(t)`."""
    B = 67
    y0, func, _ = decay_problem(B, L, dtype, 3, DEV)
    t1 = per_row_t1(B)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1.to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    twin = _on_host(dense)
    shared = torch.tensor([0.1, 0.45, 0.55], dtype=F64)
    y = dense(shared.to(DEV), check=False).cpu().numpy()
    took = ~np.isnan(y[:, :, 0])
    assert took.sum(axis=1).tolist() == [int((t1 >= v).sum()) for v in shared] and took.sum(axis=1)[2] >= 2
    for correction in (0, 1):
        ref = _reference(y, took, correction)
        for covariance in (False, True):
            got = dense.moments(shared.to(DEV), covariance=covariance, correction=correction, check=False)
            assert got.mean.device.type == DEV.type and got.mean.shape == (3, L) and (got.covariance is None) == (not covariance)
            got = [None if v is None else v.cpu().numpy() for v in got]
            _check(got, ref, covariance)
            host = twin.moments(shared, covariance=covariance, correction=correction, check=False)
            assert np.array_equal(got[0], host.count.numpy())
            for j, (_, _, _, mean_tol, cov_tol) in enumerate(ref):
                assert _close(got[1][j], host.mean[j].numpy().astype(LD), mean_tol, 2)
                assert _close(got[2][j], host.variance[j].numpy().astype(LD), np.diagonal(cov_tol), 2)
                assert not covariance or _close(got[3][j], host.covariance[j].numpy().astype(LD), cov_tol, 2)
    with pytest.raises(ValueError, match=r"dense.moments\(t\): query 1 of row 0 \(t = 0.45"):
        dense.moments(shared.to(DEV))
    one = dense.moments(0.1, covariance=True)
    assert one.count.shape == () and one.mean.shape == (L,) and one.covariance.shape == (L, L)
    assert np.array_equal(one.covariance.cpu().numpy(), got[3][0]) and int(one.count) == B
