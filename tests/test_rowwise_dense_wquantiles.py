"""`RowDenseOutput.quantiles(weights=)` without a GPU: the host path against numpy's weighted `inverted_cdf` quantile of
`dense(t)` for dyadic weights (for which numpy's own sums are exact), the identities of the definition, the argument errors and
the refusals of the two entry points.  Every comparison is bit for bit."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
B, L = 11, 5
PROBS = (0, 0.05, 1 / 3, 0.5, 0.95, 1)


def _solve(dtype, t1=0.5, rows=slice(None)):
    y0, func, k = decay_problem(B, L, dtype, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tda.odeint_rowwise_dense(lambda t, y: -k[rows] * y * (1 + t)[:, None], y0[rows], 0.0, t1, **tolerances("dopri5", dtype))


def dyadic_weights(shape, seed, scale=2.0 ** -3):
    """Integers in [0, 1024) over 1024 times a power of two, about one in five exactly 0."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(1, 1024, shape, generator=g).double() / 1024 * scale
    return torch.where(torch.rand(shape, generator=g) < 0.2, 0.0, w)


def same_bits(a, b):
    I = torch.int32 if a.dtype == F32 else torch.int64
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(I), b.contiguous().view(I))


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("per_time", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
def test_host_path_against_numpy(dtype, per_time, per_row):
    dense = _solve(dtype)
    t = torch.tensor([0.0, 0.2, 0.5], dtype=F64)
    if per_row:
        t = random_queries(3, torch.zeros(B, dtype=F64), torch.full((B,), 0.5, dtype=F64), 5)
    w = dyadic_weights((3, B) if per_time else (B,), 7)
    got = dense.quantiles(t, PROBS, weights=w)                                           # a TypeError without the feature
    y = dense(t).numpy()
    assert got.shape == (len(PROBS), 3, L) and got.dtype == dtype
    for j in range(3):
        want = np.quantile(y[j], PROBS, axis=0, weights=w.expand(3, B)[j].numpy(), method="inverted_cdf")
        assert same_bits(got[:, j], torch.from_numpy(want).to(dtype)), j
    if not per_row:                                                                      # a single time takes [B] or [1, B]
        assert same_bits(dense.quantiles(t[1], PROBS, weights=w[1:2] if per_time else w), got[:, 1])
    assert same_bits(dense.quantiles(t, PROBS, weights=w * 2.0 ** 1000), got)                       # a power of two: no bit
    assert same_bits(dense.quantiles(t, PROBS, weights=(w * 2.0 ** -1040) * 2.0 ** -20), got)       # (exact: subnormal units)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_identities(dtype):
    dense, t = _solve(dtype), torch.tensor([0.1, 0.4], dtype=F64)
    for weight in (1.0, 0.25, 4):                                                        # equal powers of two: a rank rule
        ranks = [max(math.ceil(p * B) - 1, 0) for p in PROBS]
        assert same_bits(dense.quantiles(t, PROBS, weights=torch.full((B,), weight)), dense.quantiles(t, ranks=ranks))
    keep = torch.arange(B) % 3 != 1                                                      # 0/1 weights: the record of those rows
    part = _solve(dtype, rows=keep)
    assert same_bits(part(t), dense(t)[:, keep])
    assert same_bits(dense.quantiles(t, PROBS, weights=keep.long()), part.quantiles(t, PROBS, weights=torch.ones(int(keep.sum()))))
    w = torch.where(keep, dyadic_weights((B,), 9) + 2.0 ** -13, 0.0)                    # a weight of 0: without that row
    assert same_bits(dense.quantiles(t, PROBS, weights=w.float()), part.quantiles(t, PROBS, weights=w[keep]))


@pytest.mark.parametrize("bad", [-1.0, -2.0 ** -1074, float("nan"), float("inf")])
def test_an_invalid_weight_is_nan_for_its_time_alone(bad):
    dense, t = _solve(F64), torch.tensor([0.1, 0.4, 0.5], dtype=F64)
    w = dyadic_weights((3, B), 11)
    good = dense.quantiles(t, PROBS, weights=w)
    w[1, 4] = bad
    got = dense.quantiles(t, PROBS, weights=w)
    assert bool(got[:, 1].isnan().all()) and same_bits(got[:, [0, 2]], good[:, [0, 2]])
    w[1], w[2, 3] = 0.0, -0.0                                                            # a total of 0; -0.0 is a zero
    got = dense.quantiles(t, PROBS, weights=w)
    assert bool(got[:, 1].isnan().all()) and not bool(got[:, [0, 2]].isnan().any())


def test_a_row_out_of_range_has_left():
    t1 = torch.full((B,), 0.5, dtype=F64)
    t1[0] = 0.2
    dense, w = _solve(F64, t1), dyadic_weights((B,), 13) + 2.0 ** -13
    with pytest.raises(ValueError, match=r"dense.quantiles\(t\): query 1 of row 0 \(t = 0.4\) is outside"):
        dense.quantiles(torch.tensor([0.1, 0.4], dtype=F64), [0.5], weights=w)
    want = np.quantile(dense(0.4, check=False).numpy()[1:], PROBS, axis=0, weights=w.numpy()[1:], method="inverted_cdf")
    for w0 in (float("nan"), -1.0, 1e300):                                               # its weight is not inspected
        w[0] = w0
        assert same_bits(dense.quantiles(0.4, PROBS, weights=w, check=False), torch.from_numpy(want))
    assert bool(dense.quantiles(0.4, [1.0], check=False).isnan().all())                  # unweighted: a NaN value at the top


@pytest.mark.parametrize("kwargs, error", [
    (dict(ranks=[1], weights=torch.ones(B)), ValueError), (dict(weights=torch.ones(B)), ValueError),
    (dict(probs=[0.5], ranks=[1], weights=torch.ones(B)), ValueError), (dict(probs=[1.5], weights=torch.ones(B)), ValueError),
    (dict(probs=[0.5] * 17, weights=torch.ones(B)), ValueError), (dict(probs=[0.5], weights=torch.ones(B + 1)), ValueError),
    (dict(probs=[0.5], weights=torch.ones(2, B)), ValueError), (dict(probs=[0.5], weights=[1.0] * B), ValueError),
    (dict(probs=[0.5], weights=torch.ones(B, dtype=torch.bool)), ValueError),
    (dict(probs=[0.5], weights=torch.ones(B, dtype=torch.complex64)), ValueError),
    (dict(probs=[0.5], weights=torch.ones(B, requires_grad=True)), NotImplementedError)])
def test_argument_errors(kwargs, error):
    with pytest.raises(error, match="quantiles|weights requires grad"):
        _solve(F64).quantiles(0.2, **kwargs)


def test_entry_points_refuse_without_gpu():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38
    f32, f64 = _native.dtype_code(F32), _native.dtype_code(F64)
    space = lib.tdeq_row_dense_quantiles_weighted_workspace_bytes
    # the histograms of 32-element tiles, 32 bytes per time, prefix and remainder, the units
    assert space(3, 2, 1025, 70, f32) == 4 * 2 * 3 * 65536 + 32 * 2 + 16 * 3 * 2 * 70 + 8 * 2 * 1025
    assert space(3, 5, 1025, 70, f64) == 5 * space(3, 1, 1025, 70, f64)                  # linear in the times
    assert space(0, 1, 8, 8, f64) == space(17, 1, 8, 8, f64) == space(1, 1, -1, 8, f64) == space(1, 2 ** 16, 2 ** 15, 8, f64) == 0
    assert space(1, 1, 8, 8, _native.TDEQ_BF16) == 0
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(out=p, probs=p, n_ranks=2, coeffs=p, n_seg=2, seg=p, x=p, n_q=1, n_rows=4, row_len=3, workspace=p, workspace_bytes=8,
              dtype=f64, stream=None, weights=p, w_stride=0)

    def call(**kw):
        return lib.tdeq_row_dense_quantiles_weighted(*{**ok, **kw}.values())
    for name in [k for k, v in ok.items() if v == p]:
        assert call(**{name: None}) == -1, name
    for kw in (dict(w_stride=1), dict(w_stride=-4), dict(w_stride=8), dict(dtype=7), dict(dtype=_native.TDEQ_BF16), dict(n_ranks=0),
               dict(n_ranks=17), dict(n_seg=0), dict(n_q=-1), dict(n_rows=-1), dict(row_len=-1), dict(workspace=p + 8),
               dict(n_q=2 ** 16, n_rows=2 ** 15, w_stride=2 ** 15)):
        assert call(**kw) == -1, kw
    assert call() == -2 and call(w_stride=4) == -2                                      # workspace too small
    assert call(n_q=0) == 0 and call(n_rows=0, workspace_bytes=2 ** 20) == 0 and call(row_len=0, workspace_bytes=128) == 0
