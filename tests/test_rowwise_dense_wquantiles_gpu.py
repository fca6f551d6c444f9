"""`RowDenseOutput.quantiles(weights=)` on the MI355X: `row_dense_quantiles_weighted` itself on the hand-made record of the
moments test (about one row in eight has left) against the host path and against numpy's weighted `inverted_cdf` quantile of
the values `dense(t)` gives; on the bit patterns of the quantiles test, where keys tie; and on a real solve against the host
path, sliced and whole.  Every comparison is bit for bit."""
import math

import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, tolerances
from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_moments_gpu import _record, _values
from test_rowwise_dense_quantiles_gpu import _population, _record as _bit_record, _run as _run_ranks
from test_rowwise_dense_wquantiles import PROBS, dyadic_weights, same_bits

import torchdiffeq_amd as tda
from torchdiffeq_amd import rowwise_dense
from torchdiffeq_amd.rowwise import HostRowKernels

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345.0
PROBS16 = PROBS + PROBS + (0.5, 0.25, 0.75, 1)                                           # duplicates


def _run(k, coeffs, seg, x, probs, w, Q):
    """`row_dense_quantiles_weighted` into a bordered output -> [P, Q, L] on the host; the border is intact."""
    P, L, dtype, B = len(probs), coeffs.shape[2], coeffs.dtype, seg.numel() // Q
    flat = torch.full((P * Q * L + 16,), SENTINEL, dtype=dtype, device=DEV)
    out = flat[8:8 + P * Q * L].view(P, Q, L)
    work = torch.empty(k.row_dense_quantiles_weighted_workspace_bytes(P, Q, B, L, dtype), dtype=torch.uint8, device=DEV)
    k.row_dense_quantiles_weighted(out, torch.tensor(probs, dtype=F64, device=DEV), coeffs, seg, x, work, w.to(DEV))
    assert bool((torch.cat([flat[:8], flat[8 + P * Q * L:]]) == SENTINEL).all())
    return out.cpu()


def _host(coeffs, seg, x, probs, w, Q):
    return HostRowKernels.quartic_quantiles_weighted(coeffs.cpu(), seg.cpu(), x.cpu(), list(probs), w, Q, seg.numel() // Q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("probs", [(0.5,), PROBS16], ids=["P1", "P16"])
@pytest.mark.parametrize("B", [1, 2, 1025, 2051])
@pytest.mark.parametrize("L", [1, 3, 33, 36, 68])
def test_kernel_against_host_path_and_numpy(hip_kernels, L, B, probs, dtype):
    """B = 1025: the slab boundary, 2051: three slabs.  L = 1, 3: the scalar form; 33: the tile boundary at 32; 36, 68: the
    16-byte form over two and three tiles.  Per-time weights, zeros among them; a time whose population is empty or has no
    weight is all NaN."""
    Q = 2
    coeffs, seg, x = _record(Q, B, L, dtype)
    w = dyadic_weights((Q, B), B * 100 + L, 2.0 ** 5)
    got = _run(hip_kernels, coeffs, seg, x, probs, w, Q)
    assert same_bits(got, _host(coeffs, seg, x, probs, w, Q))
    y, took = _values(hip_kernels, coeffs, seg, x, Q)
    for j in range(Q):
        wj = w[j].numpy()[took[j]]
        if wj.sum() == 0:
            assert bool(got[:, j].isnan().all())
        else:
            want = np.quantile(y[j][took[j]], probs, axis=0, weights=wj, method="inverted_cdf")
            assert same_bits(got[:, j], torch.from_numpy(want).to(dtype)), j


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 36])
def test_ties_zeros_infinities_and_nans(hip_kernels, L, dtype):
    """A population drawn from 33 bit patterns (both zeros, the infinities, NaNs, a subnormal), B = 67, so keys tie: the host
    path's bits, the same bits from a second call, one set of weights for all times, and for weights of 1.0 the ranks
    max(ceil(p B) - 1, 0) of the unweighted kernel."""
    Q, B = 2, 67
    coeffs, seg, x = _bit_record(_population(dtype, Q, B, L), dtype)
    for w in (dyadic_weights((Q, B), L), dyadic_weights((B,), L + 1), torch.ones(B, dtype=F64)):
        got = _run(hip_kernels, coeffs, seg, x, PROBS16, w, Q)
        assert same_bits(got, _host(coeffs, seg, x, PROBS16, w, Q)) and same_bits(got, _run(hip_kernels, coeffs, seg, x, PROBS16, w, Q))
    ranks = [max(math.ceil(p * B) - 1, 0) for p in PROBS16]
    by_rank, _ = _run_ranks(hip_kernels, coeffs, seg, x, ranks, Q)
    assert np.array_equal(got.numpy().view(by_rank.dtype), by_rank)
    w = dyadic_weights((Q, B), L + 2)
    w[1, 5] = float("inf")                                                               # invalid: that time alone is NaN
    bad = _run(hip_kernels, coeffs, seg, x, PROBS16, w, Q)
    assert bool(bad[:, 1].isnan().all()) and same_bits(bad, _host(coeffs, seg, x, PROBS16, w, Q))


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_solve_against_host_path_whole_and_sliced(monkeypatch, dtype):
    """Per-row `t1`, B = 67, shared times beyond some rows' `t1` with `check=False` (those rows have left; one of them carries
    a NaN weight), per-time weights: the host path on the device's record, and the same bits when the times run one by one."""
    B, L = 67, 8
    y0, func, _ = decay_problem(B, L, dtype, 3, DEV)
    t1 = per_row_t1(B)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1.to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    shared = torch.tensor([0.1, 0.45, 0.55], dtype=F64)
    w = dyadic_weights((3, B), 21)
    w[2, 0] = float("nan")                                                               # t1[0] = 0.3 < 0.55: not inspected
    whole = dense.quantiles(shared.to(DEV), PROBS, weights=w, check=False)
    assert whole.device.type == DEV.type and not bool(whole.isnan().any())
    assert same_bits(whole.cpu(), _on_host(dense).quantiles(shared, PROBS, weights=w, check=False))
    monkeypatch.setattr(rowwise_dense, "QUANTILES_WORKSPACE_BYTES", 1)
    assert same_bits(dense.quantiles(shared.to(DEV), PROBS, weights=w.to(DEV), check=False), whole)
    with pytest.raises(ValueError, match=r"dense.quantiles\(t\): query 1 of row 0 \(t = 0.45"):
        dense.quantiles(shared.to(DEV), PROBS, weights=w)
