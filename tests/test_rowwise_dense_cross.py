"""`RowDenseOutput.cross_covariance` without a GPU: the host path on a small real solve against a two-pass numpy.longdouble
reference on its own `dense(t)`, the out-of-range rule, the argument errors, and the refusals of `tdeq_row_dense_cross`.

Tolerance (derived, not measured), with u = 2^-53, n the population's size, d and e the reference deviations of y and of
`other`, A_i = mean_r |y_ri| and Z_m = mean_r |z_rm|:
    |out_im - ref| <= 2 ((n + 3) u sum_r |d_ri e_rm| + n (n u)^2 A_i Z_m) / max(n - correction, 1)
the bound of a sum of n rounded products in any order plus the second-order term of the two rounded means (the first-order
terms vanish: deviations from an exact mean sum to zero), with a factor 2 of headroom."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, tolerances
from test_rowwise_dense_moments_gpu import _close

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -53
LD = np.longdouble
B, L = 9, 5


def reference(y, z, took, correction):
    """y [B, L], z [B, M] floats, took [B] bool -> (n, cov [L, M], tol [L, M]) of the rows that took part, two passes in
    longdouble; the divisor max(n - correction, 0), a zero one by IEEE division."""
    v, w = y[took].astype(LD), z[took].astype(LD)
    n = len(v)
    with np.errstate(all="ignore"):
        d, e = v - v.sum(axis=0) / LD(n), w - w.sum(axis=0) / LD(n)
        A, Z = np.abs(v).sum(axis=0) / LD(max(n, 1)), np.abs(w).sum(axis=0) / LD(max(n, 1))
        tol = 2 * ((n + 3) * U * (np.abs(d).T @ np.abs(e)) + n * (n * U) ** 2 * np.outer(A, Z)) / max(n - correction, 1)
        return n, (d.T @ e) / LD(max(n - correction, 0)), tol


def _solve(dtype, t1=0.5):
    y0, func, _ = decay_problem(B, L, dtype, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tda.odeint_rowwise_dense(func, y0, 0.0, t1, **tolerances("dopri5", dtype))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("correction", [0, 1])
def test_host_path_against_longdouble(dtype, correction):
    dense = _solve(dtype)
    t = torch.tensor([0.0, 0.2, 0.5], dtype=F64)
    y = dense(t).double().numpy()
    g = torch.Generator().manual_seed(5)
    for other in (50 + torch.randn(B, 3, generator=g, dtype=F64), torch.arange(B) ** 2, torch.rand(B, generator=g)):
        z = other.double().reshape(B, -1).numpy()
        got = dense.cross_covariance(t, other, correction=correction)
        assert got.dtype == F64 and got.shape == (3, L, z.shape[1])
        one = dense.cross_covariance(0.2, other, correction=correction)                  # a single time drops Q
        assert one.shape == (L, z.shape[1])
        for j in range(3):
            _, ref, tol = reference(y[j], z, np.ones(B, dtype=bool), correction)
            assert _close(got[j].numpy(), ref, tol), j
            assert j != 1 or _close(one.numpy(), ref, tol)


def test_out_of_range_rows_leave_the_population():
    t1 = torch.full((B,), 0.5, dtype=F64)
    t1[0] = 0.2
    dense = _solve(F64, t1)
    z = 50 + torch.randn(B, 2, generator=torch.Generator().manual_seed(6), dtype=F64)
    with pytest.raises(ValueError, match=r"dense.cross_covariance\(t, other\): query 1 of row 0 \(t = 0.4\) is outside"):
        dense.cross_covariance(torch.tensor([0.1, 0.4], dtype=F64), z)
    lone = torch.tensor([[0.1] + [2.0] * (B - 1)])                                       # one row: 0 / 0 with correction = 1
    assert bool(dense.cross_covariance(lone, z, check=False).isnan().all())
    assert torch.equal(dense.cross_covariance(lone, z, correction=0, check=False), torch.zeros(1, L, 2, dtype=F64))
    z[0] = float("nan")                                                                  # masked, not multiplied
    got = dense.cross_covariance(0.4, z, check=False).numpy()
    _, ref, tol = reference(dense(0.4, check=False).numpy(), z.numpy(), np.arange(B) > 0, 1)   # row 0 dropped from both
    assert np.isfinite(got).all() and _close(got, ref, tol)


@pytest.mark.parametrize("other", [torch.zeros(B, dtype=torch.bool), torch.zeros(B, 2, dtype=torch.complex64), torch.zeros(B + 1),
                                   torch.zeros(B, 2, 2), torch.zeros(B, 0), torch.tensor(1.0), [0.0] * B,
                                   torch.zeros(B, 64 * _native.TDEQ_ROW_CROSS_MAX_BLOCKS + 1)])
def test_bad_other_is_refused(other):
    with pytest.raises(ValueError, match=r"dense.cross_covariance\(t, other\)"):
        _solve(F64).cross_covariance(0.2, other)


def test_bad_correction_and_gradients_are_refused():
    dense = _solve(F64)
    for correction in (2, True, 1.0):
        with pytest.raises(ValueError, match=r"dense.cross_covariance\(t, other\): correction"):
            dense.cross_covariance(0.2, torch.zeros(B), correction=correction)
    with pytest.raises(NotImplementedError):
        dense.cross_covariance(0.2, torch.zeros(B, requires_grad=True))
    with pytest.raises(NotImplementedError):
        dense.cross_covariance(torch.tensor(0.2, requires_grad=True), torch.zeros(B))


def test_abi_38_refusals_without_gpu():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38
    f64 = _native.dtype_code(F64)
    # 8 n_q (sum_slabs (1 + L + M) + M + slabs blocks 64 W): two slabs of both kinds at 1025 rows
    assert lib.tdeq_row_dense_cross_workspace_bytes(3, 1025, 70, 17, f64) == (24 * (2 * 88 + 17 + 2 * 2 * 64 * 64) + 15) // 16 * 16
    assert lib.tdeq_row_dense_cross_workspace_bytes(3, 1025, 70, 16, _native.dtype_code(F32)) == 24 * (2 * 87 + 16 + 2 * 2 * 64 * 16)
    assert lib.tdeq_row_dense_cross_workspace_bytes(1, 8, 70, 0, f64) == 0
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(out=p, count=p, ybar=p, other=p, n_cols=2, correction=1, coeffs=p, n_seg=2, seg=p, x=p, n_q=1, n_rows=4, row_len=3,
              workspace=p, workspace_bytes=8, dtype=f64)

    def call(**kw):
        return lib.tdeq_row_dense_cross(*{**ok, **kw}.values(), None)
    for name in ("out", "count", "ybar", "other", "coeffs", "seg", "x", "workspace"):
        assert call(**{name: None}) == -1, name
    for kw in (dict(n_cols=0), dict(n_cols=-1), dict(row_len=64 * 1024 + 1), dict(row_len=64 * 512 + 1, n_cols=65), dict(dtype=7),
               dict(dtype=_native.TDEQ_BF16), dict(correction=2), dict(correction=-1), dict(n_seg=0), dict(n_q=-1),
               dict(n_rows=-1), dict(workspace=p + 8), dict(n_q=2 ** 16, n_rows=2 ** 15)):
        assert call(**kw) == -1, kw
    assert call() == -2                                                                  # workspace too small
    assert call(n_q=0) == 0 and call(n_rows=0, workspace_bytes=64) == 0
