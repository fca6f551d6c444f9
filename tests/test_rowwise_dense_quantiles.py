"""`RowDenseOutput.quantiles` on the host path: against a plain sort of `dense(t)`, the probs -> rank rule, the argument errors."""
import warnings

import pytest
import torch

import torchdiffeq_amd as tda


def _solve(dtype, sign, B=7, L=5):
    g = torch.Generator().manual_seed(3)
    A = torch.randn(L, L, generator=g, dtype=dtype) * 0.5
    y0 = torch.randn(B, L, generator=g, dtype=dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tda.odeint_rowwise_dense(lambda t, y: y @ A.T, y0, 0.0, 1.0 * sign)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_all_ranks_are_the_sort_of_dense(dtype, sign):
    dense = _solve(dtype, sign)
    t = torch.tensor([0.0, 0.3, 0.77, 1.0], dtype=torch.float64) * sign
    want = torch.sort(dense(t).double(), dim=1).values.to(dtype).transpose(0, 1)
    got = dense.quantiles(t, ranks=range(7))
    assert got.shape == (7, 4, 5) and got.dtype == dtype
    assert torch.equal(got, want)
    assert torch.equal(dense.quantiles(0.3 * sign, ranks=[6, 0, 0]), want[[6, 0, 0], 1])       # a single time, a duplicate


@pytest.mark.parametrize("B", [7, 8])
def test_probs_take_the_lower_rank(B):
    dense = _solve(torch.float64, 1, B=B)
    by_rank = dense.quantiles(0.5, ranks=range(B))
    assert torch.equal(dense.quantiles(0.5, [0, 1, 0.5]), by_rank[[0, B - 1, (B - 1) // 2]])
    assert torch.equal(dense.quantiles(0.5, probs=(1.0, 0.0)), by_rank[[B - 1, 0]])


@pytest.mark.parametrize("kwargs", [
    {}, {"probs": [0.5], "ranks": [1]}, {"probs": []}, {"ranks": []}, {"ranks": list(range(7)) * 3}, {"probs": 0.5},
    {"probs": "0.5"}, {"probs": [1.5]}, {"probs": [-0.1]}, {"probs": [float("nan")]}, {"probs": [True]}, {"ranks": [7]},
    {"ranks": [-1]}, {"ranks": [1.0]}, {"ranks": [False]}])
def test_argument_errors(kwargs):
    dense = _solve(torch.float64, 1)
    with pytest.raises(ValueError, match="quantiles"):
        dense.quantiles(0.5, **kwargs)


def test_queries_are_those_of_dense():
    dense = _solve(torch.float64, 1)
    with pytest.raises(ValueError, match=r"query 1 of row 0 \(t = 1.5\) is outside"):
        dense.quantiles(torch.tensor([0.5, 1.5]), [0.5])
    got = dense.quantiles(torch.tensor([0.5, 1.5]), [0.5], check=False)
    assert not got[:, 0].isnan().any() and got[:, 1].isnan().all()
    with pytest.raises(NotImplementedError):
        dense.quantiles(torch.tensor(0.5, requires_grad=True), [0.5])
