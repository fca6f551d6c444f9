"""Kernel parity of tdeq_row_reduce_tol (the row reductions with a tolerance pair per row) at the row lengths that name
every reduction geometry, with the inputs, the sentinel-bordered buffers and the bounds of
tests/test_rowwise_kernels_gpu.py:

(a) against the CPU row oracle wrapped by tests/_rowwise_tol_oracle.py (each row reduced alone with its two floats): a row
    sum is an fp64 accumulation of L terms against the correctly rounded sum, |got - ref| <= (L + 1) * 2^-53 * |sum|; the
    non-finite census is exact; inactive rows report zeros;
(b) constant vectors give the bits of tdeq_row_reduce with the scalar (the same element arithmetic, the same tree);
(c) a row reduced alone with its own tolerances has the bits it has in the batch;
(d) nothing is written outside `part`, and no input is touched."""
import pytest
import torch

from _rowwise_kernels import BAND_NV, LONG_NV, MANY_PARTIALS_NV, SENTINEL, SHORT_NV, lane_elems, row_lengths
from _rowwise_tol_oracle import TolOracle
from test_rowwise_kernels_gpu import (ATOL_, MODES, RTOL_, _batches, _bits_equal, _check_sums, _device_reduce, _partials,
                                      _Placed, _reduce_case, _to_dev)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]


def _lengths(dtype):
    """Every geometry class, and one length of more than 64 partials per row."""
    return row_lengths(dtype, SHORT_NV + BAND_NV + LONG_NV) + row_lengths(dtype, MANY_PARTIALS_NV[:1])[:1]


def _row_tolerances(B, dtype, seed):
    """rtol over four decades (1e-6 .. 1e-2) in a seeded order, atol = rtol / 100: [B] tensors of the state's dtype."""
    g = torch.Generator().manual_seed(seed)
    rtol = 10.0 ** (-6.0 + 4.0 * torch.rand(B, generator=g, dtype=torch.float64))
    if B > 1:
        rtol[0], rtol[B - 1] = 1e-6, 1e-2
    return rtol.to(dtype), (rtol * 1e-2).to(dtype)


def _device_reduce_tol(kern, mode, args, B, nch, rtol_rows, atol_rows, offset=0):
    """_device_reduce of tests/test_rowwise_kernels_gpu.py through the per-row entry point -> part [3, B, nch]."""
    put = _Placed(offset)
    dev = _to_dev(args, put)
    dev[5] = None if args[5] is None else args[5].cuda()        # dts, active: plain device vectors
    dev[6] = None if args[6] is None else args[6].cuda()
    words = 3 * B * nch
    part = torch.full((words + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    tol = _Placed(0)
    kern.row_reduce_tol(mode, part[:words], *dev, tol(rtol_rows), tol(atol_rows))
    assert put.intact() and tol.intact()
    part = part.cpu()
    assert bool((part[words:] == SENTINEL).all()), "written behind 3 * B * nch words"
    return part[:words].view(3, B, nch)


def _slice_rows(args, r):
    return [a[r:r + 1].clone() if isinstance(a, torch.Tensor) else
            [k[r:r + 1].clone() for k in a] if isinstance(a, list) and a and isinstance(a[0], torch.Tensor) else a
            for a in args]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode,with_partial", MODES, ids=["err", "err_partial", "init01", "init2"])
def test_row_reduce_tol(hip_kernels, oracle_kernels, mode, with_partial, dtype):
    oracle = TolOracle(oracle_kernels)
    for L in _lengths(dtype):
        nch = _partials(L, dtype)
        for B in _batches(L, dtype):
            args = _reduce_case(mode, with_partial, B, L, dtype, 7 * L + B)
            rtol, atol = _row_tolerances(B, dtype, 13 * L + B)
            # (a) the oracle, row by row
            ref = torch.zeros(3 * B * nch, dtype=torch.float64)
            oracle.row_reduce_tol(mode, ref, *args, rtol, atol)
            got = _device_reduce_tol(hip_kernels, mode, args, B, nch, rtol, atol)          # (d) inside
            _check_sums(got, ref.view(3, B, nch), L, (mode, with_partial, L, B))
            if mode == 0:
                inactive = args[6] == 0
                assert bool((got[:, inactive] == 0).all()), "an inactive row reports zeros"
            # (b) constant vectors: the scalar entry point's bits
            const = _device_reduce_tol(hip_kernels, mode, args, B, nch, torch.full((B,), RTOL_, dtype=torch.float64).to(dtype),
                                       torch.full((B,), ATOL_, dtype=torch.float64).to(dtype))
            assert _bits_equal(const, _device_reduce(hip_kernels, mode, args, B, nch)), (mode, L, B)
            # (c) a row alone
            for r in sorted({0, B // 2, B - 1}):
                one = _device_reduce_tol(hip_kernels, mode, _slice_rows(args, r), 1, nch, rtol[r:r + 1].clone(),
                                         atol[r:r + 1].clone())
                assert _bits_equal(one[:, 0], got[:, r]), (mode, L, B, r)
            # the tolerances are looked at: another pair moves the sums of the rows that are reduced
            if B > 1:
                live = torch.ones(B, dtype=torch.bool) if mode != 0 else args[6] != 0
                assert bool((const[0, live] != got[0, live]).any()), (mode, L, B)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_reduce_tol_term_counts(hip_kernels, oracle_kernels, dtype):
    """1 and 14 error terms, the fewest and the most the entry point takes (the cases above have 2 and 3), with and
    without `partial`, 3 rows of one 16-byte element and of 5 scalar ones: (a) of the test above."""
    oracle = TolOracle(oracle_kernels)
    for nt in (1, 14):
        for L in (lane_elems(dtype), 5):
            for with_partial in (False, True):
                args = _reduce_case(0, with_partial, 3, L, dtype, nt + L, nt)
                rtol, atol = _row_tolerances(3, dtype, nt + L)
                ref = torch.zeros(3 * 3, dtype=torch.float64)
                oracle.row_reduce_tol(0, ref, *args, rtol, atol)
                got = _device_reduce_tol(hip_kernels, 0, args, 3, 1, rtol, atol)
                _check_sums(got, ref.view(3, 3, 1), L, (nt, L, with_partial))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode,with_partial", MODES, ids=["err", "err_partial", "init01", "init2"])
def test_row_reduce_tol_scalar_fallback(hip_kernels, mode, with_partial, dtype):
    """A scalar-element row on buffers one element off 16-byte alignment gives the bits of the aligned run; a row of
    16-byte elements on such buffers is refused (the geometry must not depend on alignment)."""
    lv = lane_elems(dtype)
    B, L = 5, 4 * lv + 1
    args = _reduce_case(mode, with_partial, B, L, dtype, L)
    rtol, atol = _row_tolerances(B, dtype, L)
    assert _bits_equal(_device_reduce_tol(hip_kernels, mode, args, B, 1, rtol, atol, offset=1),
                       _device_reduce_tol(hip_kernels, mode, args, B, 1, rtol, atol))
    args = _reduce_case(mode, with_partial, B, 4 * lv, dtype, 3)
    with pytest.raises(RuntimeError, match="code -1"):
        _device_reduce_tol(hip_kernels, mode, args, B, 1, rtol, atol, offset=1)
