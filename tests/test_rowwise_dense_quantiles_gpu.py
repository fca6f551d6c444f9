"""`RowDenseOutput.quantiles` on the MI355X: `row_dense_quantiles` itself on a hand-made record whose population is a set of
chosen bit patterns, against a numpy sort of the integer keys, bit for bit; the device against its own `dense(t)` and against
the host path on a real solve; and the same population counted by one workgroup and by two."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances
from test_rowwise_dense_level_gpu import _on_host

import torchdiffeq_amd as tda
from torchdiffeq_amd._native import TDEQ_ROW_QUANTILES_SLAB_ROWS as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345.0


def _pool(dtype):
    """The bit patterns of the population, as unsigned integers: both signs, the two zeros, a subnormal, the infinities, two
    NaNs, duplicates, a block that differs only in the lowest byte of the key and one that differs only in the highest."""
    F, U, top = (np.float32, np.uint32, 24) if dtype == F32 else (np.float64, np.uint64, 56)
    vals = np.array([1.5, -1.5, 3.0, -3.0, 1e-3, -2e30, 0.0, -0.0, np.inf, -np.inf, 1.5, -3.0], dtype=F).view(U)
    one = np.array([1.0], dtype=F).view(U)[0]
    nan = np.array([np.nan], dtype=F).view(U)[0]
    low = np.array([1.25], dtype=F).view(U)[0] + np.arange(8, dtype=U)
    high = (np.array([0x00, 0x01, 0x3f, 0x40, 0x7f], dtype=U) << U(top)) | U(0x345678)
    return np.concatenate([vals, [U(1) << U(11), nan | U(5), nan | (U(1) << U(top + 7)) | U(9), one], low, high])


def _sorted_by_key(bits, ranks):
    """bits [Q, B, L] unsigned -> the bits of rank `ranks` along B in the order of the kernel's key, [P, Q, L]."""
    U = bits.dtype.type
    n = 8 * bits.itemsize
    sign, ones = U(1) << U(n - 1), U(~U(0))
    inf, quiet = (U(0x7f800000), U(0x7fc00000)) if n == 32 else (U(0x7ff0000000000000), U(0x7ff8000000000000))
    key = np.where(bits & sign, ~bits, bits | sign)
    key = np.where((bits & ~sign) > inf, ones, key)
    key = np.sort(key, axis=1)[:, ranks].transpose(1, 0, 2)
    return np.where(key == ones, quiet, np.where(key & sign, key ^ sign, ~key))


def _record(bits, dtype, offset=0):
    """The record whose (query, row) value is `bits[q, r]` exactly: plane e holds the patterns, the planes d .. a are -0.0
    (so that e = -0.0 keeps its sign), seg = arange, x = 0 -> (coeffs [5, Q * B, L] on the device, `offset` elements off a
    16-byte boundary, seg, x)."""
    Q, B, L = bits.shape
    flat = torch.full((5 * Q * B * L + 8,), -0.0, dtype=dtype, device=DEV)
    coeffs = flat[offset:offset + 5 * Q * B * L].view(5, Q * B, L)
    coeffs[0] = torch.from_numpy(bits.view(np.float32 if dtype == F32 else np.float64).reshape(Q * B, L)).to(DEV)
    return coeffs, torch.arange(Q * B, dtype=torch.int32, device=DEV), torch.zeros(Q * B, dtype=dtype, device=DEV)


def _run(k, coeffs, seg, x, ranks, Q, offset=0):
    """`row_dense_quantiles` into a bordered output -> (the bits as a numpy array [P, Q, L], the border is intact)."""
    P, L, dtype = len(ranks), coeffs.shape[2], coeffs.dtype
    flat = torch.full((P * Q * L + 16,), SENTINEL, dtype=dtype, device=DEV)
    out = flat[8 + offset:8 + offset + P * Q * L].view(P, Q, L)
    work = torch.empty(k.row_dense_quantiles_workspace_bytes(P, Q, L, dtype), dtype=torch.uint8, device=DEV)
    k.row_dense_quantiles(out, torch.tensor(ranks, dtype=torch.int32, device=DEV), coeffs, seg, x, work)
    border = torch.cat([flat[:8 + offset], flat[8 + offset + P * Q * L:]])
    return out.cpu().numpy().view(np.uint32 if dtype == F32 else np.uint64), bool((border == SENTINEL).all())


def _population(dtype, Q, B, L):
    pool = _pool(dtype)
    return pool[np.random.default_rng(B * 1000 + L * 10 + Q).integers(0, len(pool), size=(Q, B, L))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("B", [1, 3, 67, R + 1])
@pytest.mark.parametrize("L", [5, 8, 70])
def test_kernel_selects_the_rank_of_the_key(hip_kernels, L, B, Q, dtype):
    """L = 5: scalar loads; 8: 16-byte loads; 70: two tiles of 64 elements, the second a tail.  B = 1, 3: a partial wave step;
    67: several; R + 1: two slabs, merged in the global histogram.  Ranks: the ends, the middle, a duplicate.  The population
    is also what the kernel of `dense(t)` gives these queries (subnormals, zeros and infinities included), bit for bit."""
    bits = _population(dtype, Q, B, L)
    ranks = [0, B - 1, B // 2, B // 2]
    coeffs, seg, x = _record(bits, dtype)
    got, intact = _run(hip_kernels, coeffs, seg, x, ranks, Q)
    assert intact and np.array_equal(got, _sorted_by_key(bits, ranks))
    values = torch.empty(Q * B, L, dtype=dtype, device=DEV)
    hip_kernels.row_event_eval_mapped(values, None, coeffs, seg, x)
    assert np.array_equal(got, _sorted_by_key(values.cpu().numpy().view(bits.dtype).reshape(Q, B, L), ranks))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_off_a_16_byte_boundary(hip_kernels, dtype):
    """`coeffs` and `out` one element off: L = 8 takes the scalar loads, and nothing around `out` is touched."""
    bits = _population(dtype, 2, 67, 8)
    ranks = list(range(0, 67, 5))
    got, intact = _run(hip_kernels, *_record(bits, dtype, offset=1), ranks, 2, offset=1)
    assert intact and np.array_equal(got, _sorted_by_key(bits, ranks))


@pytest.mark.parametrize("dtype", DTYPES)
def test_result_does_not_depend_on_the_slab_count(hip_kernels, dtype):
    """The 67 rows of one record as one slab, and spread over two slabs of a population of R + 1 rows whose other rows all
    name a NaN segment: the ranks 0 .. 66 select the same bits."""
    B, L = 67, 70
    bits = _population(dtype, 1, B + 1, L)
    bits[0, B] = _pool(dtype)[13]                                            # the extra segment: NaN in every element
    bits[0, :B] = np.where(np.isnan(bits[0, :B].view(np.float32 if dtype == F32 else np.float64)), bits[0, 0, 0], bits[0, :B])
    coeffs, seg, x = _record(bits, dtype)
    spread = torch.full((R + 1,), B, dtype=torch.int32, device=DEV)
    spread[torch.linspace(0, R, B).round().long().to(DEV)] = seg[:B]        # rows 0 and R included: both slabs hold some
    for first in range(0, B, 16):
        ranks = list(range(first, min(first + 16, B)))
        one, _ = _run(hip_kernels, coeffs, seg[:B].contiguous(), x[:B].contiguous(), ranks, 1)
        two, _ = _run(hip_kernels, coeffs, spread, torch.zeros(R + 1, dtype=dtype, device=DEV), ranks, 1)
        assert np.array_equal(one, two) and np.array_equal(one, _sorted_by_key(bits[:, :B], ranks))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
def test_device_equals_its_own_dense_sorted(L, dtype):
    """Per-row times and per-row `t1` on a real solve, B = 67: every rank is the device's `dense(t)` sorted along B (in fp64 on
    the host, NaN last) and the host path on the device's record, bit for bit; with `check=False` and times beyond some rows'
    `t1` those rows are NaNs at the top ranks; with `check=True` the call raises like `dense(t)`."""
    B, I = 67, torch.int64 if dtype == F64 else torch.int32
    y0, func, _ = decay_problem(B, L, dtype, 3, DEV)
    t1 = per_row_t1(B)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1.to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    twin = _on_host(dense)
    shared = torch.tensor([0.1, 0.45, 0.55], dtype=F64)                      # beyond t1 of the rows with t1 < 0.45, < 0.55
    n_bad = [int((t1 < v).sum()) for v in shared]
    assert n_bad[0] == 0 < n_bad[1] < n_bad[2] < B
    for t, check in ((random_queries(3, torch.zeros(B, dtype=F64), t1, 5), True), (shared, False)):
        want = torch.sort(dense(t.to(DEV), check=check).cpu().double(), dim=1).values.to(dtype).transpose(0, 1)
        want = torch.where(want.isnan(), torch.full_like(want, float("nan")), want)          # (the canonical NaN)
        for first in range(0, B, 16):
            ranks = range(first, min(first + 16, B))
            got = dense.quantiles(t.to(DEV), ranks=ranks, check=check)
            assert got.device.type == DEV.type and got.shape == (len(ranks), 3, L)
            assert torch.equal(got.cpu().view(I), want[first:first + 16].view(I))
            assert torch.equal(got.cpu().view(I), twin.quantiles(t, ranks=ranks, check=check).view(I))
    for j, n in enumerate(n_bad):
        assert int(want[:, j, 0].isnan().sum()) == n and bool(want[B - n:, j].isnan().all())
    with pytest.raises(ValueError, match=r"dense.quantiles\(t\): query 1 of row 0 \(t = 0.45"):
        dense.quantiles(shared.to(DEV), [0.05, 0.5, 0.95])
    by_prob = dense.quantiles(shared[:1].to(DEV), [0.05, 0.5, 0.95])
    assert torch.equal(by_prob.cpu(), want[[3, 33, 62], :1])
