"""`weights=` of `RowDenseOutput.moments` / `.cross_covariance` without a GPU: the host path on a small real solve against a
two-pass numpy.longdouble reference of the definition (and numpy.cov(aweights=, ddof=) in one case), the out-of-range rule,
the argument errors, and the refusals of the four weighted entry points.

Tolerances (derived, not measured), for weights >= 0, with u = 2^-53, n the population's size, W1 = sum w, W2 = sum w^2, D =
W1 - correction W2 / W1, d and e the reference deviations of y and of `other`, A_i = sum_r w_r |y_ri| / W1 (Z_m likewise):
    |mean_i - ref| <= 4 (n + 1) u A_i
the bound of n rounded products summed in any order, plus the n u relative error of W1 and one division, with a factor 2 of
headroom; so the computed mean is off by at most E_i = 2 (n + 1) u A_i, and
    |cov_ij - ref| <= 2 (((n + 4) u sum_r w_r |d_ri d_rj| + W1 E_i E_j) / D + |ref| (rel_D + u))     (variance: i = j)
    rel_D = (2 n + 4) u (W1 + correction W2 / W1) / D
the existing bound with w inside both sums and one more rounding per term for w * dev (the first-order term of the rounded
means vanishes: weighted deviations from the exact mean sum to zero), and the relative error of D: W1 and W2 are sums of n
rounded terms, then a division and a subtraction, whose cancellation is the factor (W1 + correction W2 / W1) / D.  The tests'
weights keep the effective sample size W1^2 / W2 well above `correction` (asserted on the reference), so that factor is small;
a population of one row takes a power of two as its weight, for which D = 0 exactly.  The cross-covariance has e, Z_m and E_m
= 2 (n + 1) u Z_m on its second side."""
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


def reference(y, w, took, correction, z=None):
    """y [B, L], w [B], took [B] bool (, z [B, M]) -> (n, mean, cov, mean_tol, cov_tol) of the rows that took part, two passes
    in longdouble; with `z` the cov is the cross-covariance [L, M]."""
    v, ww = y[took].astype(LD), w[took].astype(LD)[:, None]
    n = len(v)
    with np.errstate(all="ignore"):
        W1, W2 = ww.sum(), (ww * ww).sum()
        assert n < 2 or W1 * W1 / W2 >= 1.5, "the effective sample size stays well above correction"
        D = W1 - correction * W2 / W1
        D = D if D > 0 else LD(0)
        mean, A = (ww * v).sum(axis=0) / W1, (ww * np.abs(v)).sum(axis=0) / W1
        d, E = v - mean, 2 * (n + 1) * U * A
        e, F = d, E
        if z is not None:
            s = z[took].astype(LD)
            e, F = s - (ww * s).sum(axis=0) / W1, 2 * (n + 1) * U * (ww * np.abs(s)).sum(axis=0) / W1
        cov = (ww * d).T @ e / D
        rel_D = (2 * n + 4) * U * (W1 + correction * W2 / W1) / D
        tol = 2 * (((n + 4) * U * ((ww * np.abs(d)).T @ np.abs(e)) + W1 * np.outer(E, F)) / D + np.abs(cov) * (rel_D + U))
        return n, mean, cov, 4 * (n + 1) * U * A, tol


def check_moments(got, y, w, took, correction, slack=1):
    """got: (count, mean, variance, covariance or None) numpy arrays of ONE time against `reference`."""
    n, mean, cov, mean_tol, tol = reference(y, w, took, correction)
    assert got[0] == n and _close(got[1], mean, mean_tol, slack) and _close(got[2], np.diagonal(cov), np.diagonal(tol), slack)
    if got[3] is not None:
        assert _close(got[3], cov, tol, slack) and np.array_equal(got[3], got[3].T, equal_nan=True)
        assert np.array_equal(np.diagonal(got[3]), got[2], equal_nan=True)


def _solve(dtype, t1=0.5):
    y0, func, _ = decay_problem(B, L, dtype, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tda.odeint_rowwise_dense(func, y0, 0.0, t1, **tolerances("dopri5", dtype))


def _weights(Q):
    w = 0.5 + torch.rand(Q, B, generator=torch.Generator().manual_seed(7), dtype=F64)
    w[:, 2], w[0, 7] = 0.0, 0.0                                                          # exact zeros: a subgroup
    return w


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("correction", [0, 1])
def test_host_path_against_longdouble(dtype, correction):
    dense = _solve(dtype)
    t = torch.tensor([0.0, 0.2, 0.5], dtype=F64)
    y = dense(t).double().numpy()
    z = 50 + torch.randn(B, 3, generator=torch.Generator().manual_seed(5), dtype=F64)
    took = np.ones(B, dtype=bool)
    for w in (_weights(3), _weights(1)[0], _weights(1)[0].float(), torch.arange(1, B + 1)):
        wq = w.double().expand(3, B).numpy()
        for covariance in (False, True):
            got = dense.moments(t, covariance=covariance, correction=correction, weights=w)
            assert got.mean.dtype == F64 and got.count.tolist() == [B] * 3
            for j in range(3):
                check_moments([None if f is None else f[j].numpy() for f in got], y[j], wq[j], took, correction)
        cross = dense.cross_covariance(t, z, correction=correction, weights=w)
        for j in range(3):
            _, _, ref, _, tol = reference(y[j], wq[j], took, correction, z.numpy())
            assert _close(cross[j].numpy(), ref, tol), j
    one = dense.moments(0.2, covariance=True, correction=correction, weights=_weights(3)[1:2])   # [1, B] for a single time
    assert one.covariance.shape == (L, L)
    check_moments([f.numpy() for f in one], y[1], _weights(3)[1].numpy(), took, correction)
    if dtype == F64:
        keep = _weights(3)[1].numpy() > 0                                                # (numpy.cov refuses a zero sum only)
        assert np.allclose(one.covariance.numpy(), np.cov(y[1][keep].T, aweights=_weights(3)[1].numpy()[keep], ddof=correction),
                           rtol=1e-12, atol=0)


def test_out_of_range_rows_leave_the_population():
    t1 = torch.full((B,), 0.5, dtype=F64)
    t1[0] = 0.2
    dense = _solve(F64, t1)
    w, z = _weights(1)[0], torch.randn(B, 2, generator=torch.Generator().manual_seed(6), dtype=F64)
    with pytest.raises(ValueError, match=r"dense.moments\(t\): query 1 of row 0 \(t = 0.4\) is outside"):
        dense.moments(torch.tensor([0.1, 0.4], dtype=F64), weights=w)
    w[0] = float("nan")                                                                  # selected away, not multiplied
    y, took = dense(0.4, check=False).numpy(), np.arange(B) > 0
    got = dense.moments(0.4, covariance=True, weights=w, check=False)
    assert int(got.count) == B - 1 and all(bool(f.isfinite().all()) for f in got[1:])
    check_moments([f.numpy() for f in got], y, w.numpy(), took, 1)
    cross = dense.cross_covariance(0.4, z, weights=w, check=False).numpy()
    _, _, ref, _, tol = reference(y, w.numpy(), took, 1, z.numpy())
    assert np.isfinite(cross).all() and _close(cross, ref, tol)
    none = dense.moments(0.1, weights=torch.zeros(B))                                    # a total weight of 0
    assert int(none.count) == B and bool(none.mean.isnan().all()) and bool(none.variance.isnan().all())
    assert bool(dense.cross_covariance(0.1, z, weights=torch.zeros(B)).isnan().all())


@pytest.mark.parametrize("weights", [torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.complex64), torch.zeros(B + 1),
                                     torch.zeros(2, B), torch.zeros(B, 1), torch.tensor(1.0), [1.0] * B, 1.0])
def test_bad_weights_are_refused(weights):
    dense = _solve(F64)
    with pytest.raises(ValueError, match=r"dense.moments\(t\): weights"):
        dense.moments(0.2, weights=weights)
    with pytest.raises(ValueError, match=r"dense.cross_covariance\(t, other\): weights"):
        dense.cross_covariance(0.2, torch.zeros(B), weights=weights)


def test_gradients_are_refused():
    dense = _solve(F64)
    for call in (lambda w: dense.moments(0.2, weights=w), lambda w: dense.cross_covariance(0.2, torch.zeros(B), weights=w)):
        with pytest.raises(NotImplementedError, match="weights requires grad"):
            call(torch.ones(B, requires_grad=True))
        with torch.no_grad():
            call(torch.ones(B, requires_grad=True))


def test_weighted_entry_points_refuse_without_gpu():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38
    names = ["tdeq_row_dense_moments_weighted_workspace_bytes", "tdeq_row_dense_moments_weighted",
             "tdeq_row_dense_cross_weighted_workspace_bytes", "tdeq_row_dense_cross_weighted"]
    assert all(name in _native.ABI_SIGNATURES for name in names)
    f64 = _native.dtype_code(F64)
    # the twin's bytes + 16 n_q (sum_slabs + 1) before rounding: two slabs at 1025 rows
    for cov in (0, 1):
        assert lib.tdeq_row_dense_moments_weighted_workspace_bytes(cov, 3, 1025, 70, f64) == \
            lib.tdeq_row_dense_moments_workspace_bytes(cov, 3, 1025, 70, f64) + 16 * 3 * 3
    assert lib.tdeq_row_dense_cross_weighted_workspace_bytes(3, 1025, 70, 17, f64) == \
        (24 * (2 * 88 + 17 + 2 * 2 * 64 * 64) + 16 * 3 * 3 + 15) // 16 * 16
    assert lib.tdeq_row_dense_cross_weighted_workspace_bytes(1, 8, 70, 0, f64) == 0
    assert lib.tdeq_row_dense_moments_weighted_workspace_bytes(1, 1, 8, 1025, f64) == 0
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    tail = dict(coeffs=p, n_seg=2, seg=p, x=p, n_q=1, n_rows=4, row_len=3, workspace=p, workspace_bytes=8, dtype=f64, stream=None,
                weights=p, w_stride=0)
    entries = [(lib.tdeq_row_dense_moments_weighted, dict(count=p, mean=p, variance=p, covariance=None, correction=1, **tail), ()),
               (lib.tdeq_row_dense_cross_weighted, dict(out=p, count=p, ybar=p, other=p, n_cols=2, correction=1, **tail),
                (dict(n_cols=0), dict(row_len=64 * 1024 + 1)))]
    for entry, ok, more in entries:
        def call(**kw):
            return entry(*{**ok, **kw}.values())
        for name in [k for k, v in ok.items() if v == p and k != "covariance"]:
            assert call(**{name: None}) == -1, name
        for kw in (dict(w_stride=1), dict(w_stride=-4), dict(w_stride=8), dict(dtype=7), dict(dtype=_native.TDEQ_BF16),
                   dict(correction=2), dict(correction=-1), dict(n_seg=0), dict(n_q=-1), dict(n_rows=-1), dict(workspace=p + 8),
                   dict(n_q=2 ** 16, n_rows=2 ** 15, w_stride=2 ** 15)) + more:
            assert call(**kw) == -1, kw
        assert call() == -2 and call(w_stride=4) == -2                                  # workspace too small
        assert call(n_q=0) == 0 and call(n_rows=0, workspace_bytes=64) == 0
    assert entries[0][0](*{**entries[0][1], "covariance": p, "row_len": 1025}.values()) == -1
