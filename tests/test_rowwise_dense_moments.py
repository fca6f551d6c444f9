"""`RowDenseOutput.moments` on the host path: against torch.mean / torch.var / torch.cov of `dense(t)`, the out-of-range rule,
exact symmetry and the diagonal rule, the argument errors."""
import warnings

import pytest
import torch

import torchdiffeq_amd as tda
from torchdiffeq_amd._native import TDEQ_ROW_MOMENTS_MAX_COV_LEN

F64 = torch.float64


def _solve(dtype, sign, B=7, L=5, t1=1.0):
    g = torch.Generator().manual_seed(3)
    A = torch.randn(L, L, generator=g, dtype=dtype) * 0.5
    y0 = torch.randn(B, L, generator=g, dtype=dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tda.odeint_rowwise_dense(lambda t, y: y @ A.T, y0, 0.0, t1 * sign if isinstance(t1, float) else t1)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("dtype", [torch.float32, F64])
@pytest.mark.parametrize("correction", [0, 1])
def test_moments_are_those_of_dense(dtype, sign, correction):
    dense = _solve(dtype, sign)
    t = torch.tensor([0.0, 0.3, 0.77, 1.0], dtype=F64) * sign
    y = dense(t).double()                                                        # [Q, B, L]
    got = dense.moments(t, covariance=True, correction=correction)
    plain = dense.moments(t, correction=correction)
    assert isinstance(got, tda.RowDenseMoments) and plain.covariance is None
    assert got.count.dtype == torch.int64 and got.count.tolist() == [7] * 4
    assert got.mean.shape == (4, 5) and got.variance.shape == (4, 5) and got.covariance.shape == (4, 5, 5)
    assert all(v.dtype == F64 for v in (*got[1:], *plain[1:3]))
    tol = dict(rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(got.mean, y.mean(dim=1), **tol)
    torch.testing.assert_close(plain.mean, got.mean, rtol=0, atol=0)
    torch.testing.assert_close(plain.variance, y.var(dim=1, correction=correction), **tol)
    for j in range(4):
        torch.testing.assert_close(got.covariance[j], torch.cov(y[j].T, correction=correction), **tol)
    assert torch.equal(got.covariance, got.covariance.transpose(1, 2))           # exactly symmetric
    assert torch.equal(torch.diagonal(got.covariance, dim1=1, dim2=2), got.variance)
    one = dense.moments(0.3 * sign, covariance=True, correction=correction)    # a single time drops Q
    assert one.count.shape == () and one.mean.shape == (5,) and one.covariance.shape == (5, 5)
    assert torch.equal(one.covariance, got.covariance[1]) and torch.equal(one.mean, got.mean[1])


def test_out_of_range_rows_leave_the_population():
    t1 = torch.tensor([0.2, 0.4, 0.6, 0.8, 1.0, 1.0, 1.0], dtype=F64)
    dense = _solve(F64, 1, t1=t1)
    t = torch.tensor([0.1, 0.5, 0.9, 1.5])
    with pytest.raises(ValueError, match=r"dense.moments\(t\): query 1 of row 0 \(t = 0.5\) is outside"):
        dense.moments(t)
    got = dense.moments(t, covariance=True, check=False)
    assert got.count.tolist() == [7, 5, 3, 0]
    y = dense(t, check=False)
    for j, n in enumerate([7, 5, 3]):
        torch.testing.assert_close(got.mean[j], y[j, 7 - n:].mean(dim=0), rtol=1e-13, atol=0)
        torch.testing.assert_close(got.covariance[j], torch.cov(y[j, 7 - n:].T), rtol=1e-13, atol=1e-16)
    assert all(bool(v[3].isnan().all()) for v in got[1:])                        # the empty population
    lone = dense.moments(torch.tensor([[0.1] + [2.0] * 6]), check=False)         # one row: 0 / 0 with correction = 1
    assert int(lone.count) == 1 and torch.equal(lone.mean[0], y[0, 0]) and bool(lone.variance.isnan().all())
    assert torch.equal(dense.moments(torch.tensor([[0.1] + [2.0] * 6]), correction=0, check=False).variance, torch.zeros(1, 5, dtype=F64))


@pytest.mark.parametrize("kwargs", [{"correction": 2}, {"correction": True}, {"correction": 1.0}, {"covariance": 1}])
def test_argument_errors(kwargs):
    with pytest.raises(ValueError, match=r"dense.moments\(t\)"):
        _solve(F64, 1).moments(0.5, **kwargs)


def test_long_rows_and_gradients_are_refused():
    dense = _solve(torch.float32, 1, B=2, L=TDEQ_ROW_MOMENTS_MAX_COV_LEN + 1, t1=0.01)
    with pytest.raises(ValueError, match=rf"dense.moments\(t\): covariance=True takes rows of at most {TDEQ_ROW_MOMENTS_MAX_COV_LEN}"):
        dense.moments(0.005, covariance=True)
    assert dense.moments(0.005).variance.shape == (TDEQ_ROW_MOMENTS_MAX_COV_LEN + 1,)
    with pytest.raises(NotImplementedError):
        dense.moments(torch.tensor(0.005, requires_grad=True))
