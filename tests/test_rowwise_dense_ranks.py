"""`RowDenseOutput.ranks` / `cdf` without a GPU: the host path against a brute force on `dense(t)` (numpy keys, `<` / `==`,
integer sums), the rank identity with `quantiles`, the weighted identities, the forms of `values`, the argument errors and the
refusals of the entry points.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from test_rowwise_dense_wquantiles import B, L, _solve, dyadic_weights

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
T2 = torch.tensor([0.1, 0.4], dtype=F64)


def np_keys(a):
    """A numpy float array -> the ordered unsigned keys of the kernel: -0.0 before +0.0, every NaN all ones."""
    U = np.uint32 if a.dtype == np.float32 else np.uint64
    bits = np.ascontiguousarray(a).view(U)
    sign = U(1) << U(8 * bits.itemsize - 1)
    return np.where(np.isnan(a), U(~U(0)), np.where(bits & sign, ~bits, bits | sign))


def brute(y, values, m=None):
    """y [Q, B, L], values [V, Q, L] (numpy, one dtype), m int64 [Q, B] or None -> (below, equal) int64 [V, Q, L]."""
    key, level = np_keys(y)[None], np_keys(values)[:, :, None, :]
    m = np.ones(y.shape[:2], dtype=np.int64) if m is None else m
    return ((key < level) * m[None, :, :, None]).sum(axis=2), ((key == level) * m[None, :, :, None]).sum(axis=2)


def _same(r, below, equal, total):
    return all(g.dtype == torch.int64 and np.array_equal(g.numpy(), w) for g, w in zip(r, (below, equal, total)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_host_path_against_brute_force(dtype):
    """Per-row `t1`: at t = 0.4 two rows are out of range and count as NaN values with `check=False`.  Thresholds: the
    record's own values (so `equal` is nonzero), a NaN and both infinities, one set per time and element."""
    t1 = torch.full((B,), 0.5, dtype=F64)
    t1[0], t1[7] = 0.2, 0.3
    dense = _solve(dtype, t1)
    y = dense(T2, check=False)
    values = torch.cat([y[:, [1, 0, 5]].transpose(0, 1), torch.tensor([float("nan"), float("inf"), -float("inf")],
                                                                       dtype=dtype)[:, None, None].expand(3, 2, L)])
    r = dense.ranks(T2, values, check=False)
    below, equal = brute(y.numpy(), values.numpy())
    assert _same(r, below, equal, [B, B]) and equal[:3].min() >= 1 and np.array_equal(equal[3], [[0] * L, [2] * L])
    assert torch.equal(dense.cdf(T2, values, check=False), (r.below + r.equal).double() / B)
    with pytest.raises(ValueError, match=r"dense.ranks\(t\): query 1 of row 0 \(t = 0.4\) is outside"):
        dense.ranks(T2, values)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_rank_identity_with_quantiles(dtype):
    dense = _solve(dtype)
    r = dense.ranks(T2, dense.quantiles(T2, ranks=range(B)))
    k = torch.arange(B)[:, None, None]
    assert bool(((r.below <= k) & (k < r.below + r.equal)).all())


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("per_time", [False, True])
def test_weighted_identities(dtype, per_time):
    dense = _solve(dtype)
    y = dense(T2).numpy().astype(np.float64)
    w = dyadic_weights((2, B) if per_time else (B,), 7)
    values = torch.from_numpy(np.sort(y, axis=1)[:, [2, 6, 9]].transpose(1, 0, 2)).to(dtype)
    wq = w.expand(2, B).numpy()[None, :, :, None]
    want = (wq * (y[None] <= values.double().numpy()[:, :, None, :])).sum(axis=2) / wq.sum(axis=2)      # dyadic: exact sums
    r = dense.ranks(T2, values, weights=w)
    assert np.array_equal(dense.cdf(T2, values, weights=w).numpy(), want) and bool((r.total > 0).all())
    for scaled in (w * 2.0 ** 1000, (w * 2.0 ** -1040) * 2.0 ** -20, w.float()):                       # a power of two: no bit
        assert all(torch.equal(a, b) for a, b in zip(dense.ranks(T2, values, weights=scaled), r))
    keep = w.expand(2, B)[0] != 0                                                        # a weight of 0: without that row
    if not per_time:
        part = _solve(dtype, rows=keep)
        assert torch.equal(part.cdf(T2, values, weights=w[keep]), dense.cdf(T2, values, weights=w))
    bad = w.expand(2, B).clone()
    bad[1, 4] = float("inf")                                                             # invalid: that time alone is zeroed
    z = dense.ranks(T2, values, weights=bad)
    assert all(torch.equal(a[..., 0, :], b[..., 0, :]) and not bool(a[..., 1, :].any()) for a, b in zip(z[:2], r[:2]))
    assert z.total.tolist() == [int(r.total[0]), 0] and bool(dense.cdf(T2, values, weights=bad)[:, 1].isnan().all())


def test_forms_of_values():
    dense = _solve(F64)
    y = dense(T2)
    full = torch.stack([y[:, 3], y[:, 8]])                                               # [V, Q, L]
    r = dense.ranks(T2, full)
    assert _same(r, *brute(y.numpy(), full.numpy()), [B, B])
    per_el = dense.ranks(T2, full[:, 0])                                                 # [V, L]: the same set at every time
    assert _same(per_el, *brute(y.numpy(), full[:, :1].expand(2, 2, L).numpy()), [B, B])
    assert all(torch.equal(a, b) for a, b in zip(dense.ranks(T2, full[:, :1]), per_el))  # [V, 1, L] broadcasts
    flat = torch.tensor([0.25, 1])                                                       # [V], fp32: rounded to the state's dtype
    by_v = dense.ranks(T2, flat)
    assert _same(by_v, *brute(y.numpy(), flat.double()[:, None, None].expand(2, 2, L).numpy()), [B, B])
    one = dense.ranks(0.4, 1)                                                            # a number, a single time: Q is dropped
    assert one.below.shape == (1, L) and torch.equal(one.below[0], by_v.below[1, 1]) and one.total.tolist() == [B]
    assert torch.equal(dense.ranks(T2, torch.tensor([1])).equal, by_v.equal[1:])         # an integer tensor
    assert dense.cdf(0.4, flat).shape == (2, L) and torch.equal(dense.cdf(0.4, full[:, 1:]), dense.cdf(T2, full)[:, 1])


@pytest.mark.parametrize("values, error", [
    (torch.empty(0), ValueError), (torch.zeros(17), ValueError), (torch.zeros(2, L + 1), ValueError),
    (torch.zeros(2, 3, L), ValueError), (torch.zeros(2, 2, 2, L), ValueError), (torch.zeros(2, dtype=torch.bool), ValueError),
    (torch.zeros(2, dtype=torch.complex64), ValueError), (True, ValueError), ([0.5], ValueError),
    (torch.zeros(2, requires_grad=True), NotImplementedError)])
def test_argument_errors(values, error):
    with pytest.raises(error, match=r"dense.ranks\(t\): values|values requires grad"):
        _solve(F64).ranks(T2, values)


def test_names_and_entry_points_refuse_without_gpu():
    names = ["tdeq_row_dense_ranks", "tdeq_row_dense_ranks_weighted", "tdeq_row_dense_ranks_weighted_workspace_bytes"]
    assert all(n in _native.ABI_SIGNATURES for n in names) and "RowDenseRanks" in tda.__all__
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38 and _native.TDEQ_ROW_RANKS_MAX_VALUES == 16
    space = lib.tdeq_row_dense_ranks_weighted_workspace_bytes
    assert space(2, 1025) == 32 * 2 + 8 * 2 * 1025 and space(5, 70) == 5 * space(1, 70)  # linear in the times
    assert space(-1, 8) == space(1, -1) == space(2 ** 16, 2 ** 15) == 0
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(below=p, equal=p, total=p, values=p, n_values=2, coeffs=p, n_seg=2, seg=p, x=p, n_q=1, n_rows=4, row_len=3,
              workspace=p, workspace_bytes=8, dtype=_native.dtype_code(F64), stream=None, weights=p, w_stride=0)
    plain = [k for k in ok if k not in ("total", "workspace", "workspace_bytes", "weights", "w_stride")]

    def call(**kw):
        return lib.tdeq_row_dense_ranks_weighted(*{**ok, **kw}.values())

    def call_plain(**kw):
        return lib.tdeq_row_dense_ranks(*[{**ok, **kw}[k] for k in plain])
    for name in [k for k, v in ok.items() if v == p]:
        assert call(**{name: None}) == -1 and (name not in plain or call_plain(**{name: None}) == -1), name
    for kw in (dict(dtype=7), dict(dtype=_native.TDEQ_BF16), dict(n_values=0), dict(n_values=17), dict(n_seg=0), dict(n_q=-1),
               dict(n_rows=-1), dict(row_len=-1), dict(n_q=2 ** 16, n_rows=2 ** 15)):
        assert call(**kw) == -1 and call_plain(**kw) == -1, kw
    for kw in (dict(w_stride=1), dict(w_stride=8), dict(workspace=p + 8)):
        assert call(**kw) == -1, kw
    assert call() == -2 and call(w_stride=4) == -2                                      # workspace too small
    assert call(n_q=0) == 0 and call(n_rows=0, workspace_bytes=64) == 0 and call(row_len=0, workspace_bytes=64) == 0
    assert call_plain(n_q=0) == 0 and call_plain(n_rows=0) == 0 and call_plain(row_len=0) == 0
