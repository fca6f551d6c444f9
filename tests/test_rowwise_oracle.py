"""The row kernels without a GPU: the device driver of `odeint_rowwise` (`HipRowKernels`: plan interpreter, held partial
rows, `RowState` plumbing, the two polled words) run on CPU tensors with the CPU row oracle in place of the HIP kernels
— against the reference's per-row fixtures and against the torch-op host path — and the argument validation of the four
forward entry points, which precedes any launch."""
import contextlib
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from _rowwise_cases import ATOL, GOLDEN, RTOL, Batched, cases
from _rowwise_kernels import RowVectors

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native, rowwise

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ["dopri5", "bosh3", "tsit5", "fehlberg2", "adaptive_heun", "dopri8"]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """Inside `with device_driver():` a CPU state is solved by `HipRowKernels` on the oracle's row operations."""
    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: oracle_kernels)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# -- a. the device driver on the reference's fixtures ---------------------------------------------------------------------
@pytest.mark.parametrize("case", list(range(8)))
def test_device_driver_matches_reference_rows(case, device_driver):
    """What tests/test_rowwise.py::test_matches_reference_rows asserts of the host path, of the device driver."""
    golden = np.load(os.path.join(HERE, "golden", GOLDEN))
    problem, method, kind, params, y0, t, expected, n_acc, n_rej = list(cases(golden))[case]
    func = Batched(problem, params)
    with torch.no_grad(), device_driver():
        sol, stats = tda.odeint_rowwise(func, torch.tensor(y0), torch.tensor(t), rtol=RTOL, atol=ATOL, method=method,
                                        return_stats=True)
    assert stats["n_accepted"].tolist() == n_acc.tolist()
    assert stats["n_rejected"].tolist() == n_rej.tolist()
    for r in range(y0.shape[0]):
        bound = 1e-12 if n_acc[r] < 100 else 0.1 * RTOL
        assert _rel(sol[:, r], expected[:, r]) < bound, (problem, method, kind, r)


# -- b. the device driver against the host path -----------------------------------------------------------------------------
def _random_problem(B, L, dtype, seed):
    """tests/test_rowwise_gpu.py::_random_problem: rows of different stiffness, coupled inside a row only."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].to(dtype)
    w = (torch.rand(B, 1, generator=g, dtype=torch.float64) * 4).to(dtype)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64).to(dtype)

    def f(t, y):
        return -k * y + torch.sin(w * t[:, None]) * torch.roll(y, 1, dims=1)
    return y0, f


def _both(device_driver, f, y0, t, **kw):
    host, sh = tda.odeint_rowwise(f, y0, t, return_stats=True, **kw)
    with device_driver():
        dev, sd = tda.odeint_rowwise(f, y0, t, return_stats=True, **kw)
    return host, sh, dev, sd


@pytest.mark.parametrize("method", METHODS)
def test_device_driver_matches_host_path_fp64(method, device_driver):
    """The bounds of tests/test_rowwise_gpu.py::test_hip_matches_host_path_fp64 (adaptive_heun, whose order-2 rows take
    thousands of steps through the row-by-row oracle, on 12 rows instead of 96)."""
    B = 12 if method == "adaptive_heun" else 96
    y0, f = _random_problem(B, 5, torch.float64, 1)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    host, sh, dev, sd = _both(device_driver, f, y0, t, rtol=1e-6, atol=1e-8, method=method)
    assert sd["n_accepted"].tolist() == sh["n_accepted"].tolist()
    assert sd["n_rejected"].tolist() == sh["n_rejected"].tolist()
    assert sd["nfe"] == sh["nfe"]
    bound = 1e-7 if method == "dopri8" else 1e-12
    for r in range(B):
        assert _rel(dev[:, r], host[:, r]) < bound, r


def test_device_driver_matches_host_path_fp32(device_driver):
    """The bounds of tests/test_rowwise_gpu.py::test_hip_matches_host_path_fp32, its cap on rows whose counts differ (a
    ratio within a rounding of 1 may decide differently on differently ordered fp64 sums) included."""
    y0, f = _random_problem(200, 8, torch.float32, 2)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float32)
    host, sh, dev, sd = _both(device_driver, f, y0, t, rtol=1e-4, atol=1e-6)
    differ = (sd["n_accepted"] != sh["n_accepted"]) | (sd["n_rejected"] != sh["n_rejected"])
    assert int(differ.sum()) <= 2          # at most 1 % of the rows
    for r in range(200):
        if not differ[r]:
            assert _rel(dev[:, r], host[:, r]) < 1e-5, r


# one length from each band of one-chunk long rows (1024 < nv <= 2048), per dtype: 16-byte and scalar elements
_LENGTHS = {torch.float64: [1, 3, 4, 2050, 1025], torch.float32: [1, 3, 4, 4100, 1501]}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["t1d", "t2d", "decreasing", "first_step"])
def test_device_driver_row_lengths_and_grids(kind, dtype, device_driver, oracle_kernels):
    """`[T]` and `[T, B]` grids, decreasing time and per-row first steps at row lengths 1, 3, 4 and one length of each
    one-chunk long-row band (the part workspace is sized by `row_partials`).  fp64: equal counts and 1e-12; fp32: the
    1e-5 of the fp32 comparison on rows with equal counts, which these inputs give for every row."""
    B = 5
    for L in _LENGTHS[dtype]:
        y0, f = _random_problem(B, L, dtype, 10 + L)
        t = torch.linspace(0, 1.2, 4, dtype=dtype)
        opts = None
        if kind == "t2d":
            t = t[:, None] * torch.linspace(0.4, 1.0, B, dtype=dtype) + 0.05 * torch.arange(B).to(dtype)
        elif kind == "decreasing":
            t = torch.linspace(1, 0, 4, dtype=dtype)
        elif kind == "first_step":
            opts = {"first_step": torch.tensor([1e-3, 2e-3, 3e-3, 4e-3, 5e-3], dtype=torch.float64)}
        rtol, atol = (1e-7, 1e-9) if dtype == torch.float64 else (1e-4, 1e-6)
        host, sh, dev, sd = _both(device_driver, f, y0, t, rtol=rtol, atol=atol, options=opts)
        assert sd["n_accepted"].tolist() == sh["n_accepted"].tolist(), (L, kind)
        assert sd["n_rejected"].tolist() == sh["n_rejected"].tolist(), (L, kind)
        assert sd["nfe"] == sh["nfe"]
        for r in range(B):
            assert _rel(dev[:, r], host[:, r]) < (1e-12 if dtype == torch.float64 else 1e-5), (L, kind, r)


def test_device_driver_max_num_steps_names_the_row(device_driver):
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=torch.float64)
    y0 = torch.ones(4, 1, dtype=torch.float64)
    with device_driver(), pytest.raises(AssertionError, match=r"max_num_steps exceeded \(\d+>=50\) in row 2"):
        tda.odeint_rowwise(lambda t, y: -k * (y - torch.sin(t)[:, None]), y0, torch.tensor([0.0, 5.0]),
                           rtol=1e-5, atol=1e-7, options={"max_num_steps": 50})


def test_device_driver_finished_rows_ignore_nan(device_driver):
    B = 8
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[:, None]
    y0 = torch.randn(B, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    tg = torch.linspace(0, 1, 5, dtype=torch.float64)[:, None] * torch.linspace(0.3, 1.0, B, dtype=torch.float64)
    last, frozen_seen = [None], [0]

    def f(t, y, poison):
        out = -k * y + torch.cos(t)[:, None]
        if last[0] is not None:
            same = t == last[0]
            frozen_seen[0] += int(same.sum())
            if poison:
                out[same] = float("nan")
        last[0] = t.clone()
        return out
    host = tda.odeint_rowwise(lambda t, y: f(t, y, False), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    with device_driver():
        last[0], frozen_seen[0] = None, 0
        clean = tda.odeint_rowwise(lambda t, y: f(t, y, False), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
        assert frozen_seen[0] > 0
        last[0] = None
        poisoned = tda.odeint_rowwise(lambda t, y: f(t, y, True), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    assert torch.equal(clean, poisoned)
    assert _rel(clean, host) < 1e-12


# -- c. argument validation of the forward entry points (no launch is reached) ------------------------------------------------
EINVAL, EWORKSPACE = -1, -2
F32, F64, BF16 = _native.TDEQ_F32, _native.TDEQ_F64, _native.TDEQ_BF16


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _buffers():
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 14)(*([p] * 14))
    return buf, p, ptrs


def _outs(p, n, mask=1):
    outs = (_native.MultiOut * max(n, 1))()
    for o in range(n):
        outs[o].out, outs[o].mask, outs[o].add_y0 = p, mask, 1
    return outs


def test_row_combine_argument_errors(lib):
    buf, p, ptrs = _buffers()
    ok = _outs(p, 1)
    call = lambda **kw: lib.tdeq_row_combine(*[kw.get(n, d) for n, d in (       # noqa: E731
        ("outs", ok), ("n_out", 1), ("y0", p), ("acc_in", None), ("k", ptrs), ("n_terms", 1), ("dts", p), ("active", p),
        ("n_rows", 2), ("row_len", 4), ("dtype", F64), ("stream", None))])
    for name in ("outs", "y0", "k", "dts", "active"):
        assert call(**{name: None}) == EINVAL, name
    assert call(k=(ctypes.c_void_p * 14)()) == EINVAL                    # a null stage stream
    assert call(n_terms=0) == EINVAL and call(n_terms=15) == EINVAL
    assert call(n_out=0) == EINVAL and call(n_out=_native.TDEQ_MAX_MULTI_OUT + 1, outs=_outs(p, 16)) == EINVAL
    assert call(outs=_outs(None, 1)) == EINVAL                           # a null output
    assert call(outs=_outs(p, 1, mask=0)) == EINVAL                      # a zero mask
    assert call(outs=_outs(p, 1, mask=0b10)) == EINVAL                   # a mask bit at n_terms
    assert call(outs=_outs(p, 1, mask=0b101), n_terms=2) == EINVAL       # ... and above it
    assert call(row_len=0) == EINVAL and call(n_rows=-1) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    assert call(n_rows=0) == 0


def test_row_reduce_argument_errors(lib):
    buf, p, ptrs = _buffers()
    call = lambda **kw: lib.tdeq_row_reduce(*[kw.get(n, d) for n, d in (        # noqa: E731
        ("mode", 0), ("y0", p), ("y1", p), ("partial", None), ("k", ptrs), ("coef", buf), ("n_terms", 1), ("dts", p),
        ("active", p), ("rtol", 1e-3), ("atol", 1e-6), ("n_rows", 2), ("row_len", 4), ("part", p), ("part_bytes", 48),
        ("dtype", F64), ("stream", None))])
    for name in ("y0", "y1", "part"):
        assert call(**{name: None}) == EINVAL, name
    assert call(mode=-1) == EINVAL and call(mode=3) == EINVAL
    assert call(n_terms=15) == EINVAL and call(n_terms=-1) == EINVAL
    for name in ("k", "coef", "dts", "active"):                          # mode 0 needs them all, and a term
        assert call(**{name: None}) == EINVAL, name
    assert call(n_terms=0) == EINVAL
    assert call(k=(ctypes.c_void_p * 14)()) == EINVAL
    for mode in (1, 2):
        assert call(mode=mode, n_terms=1, partial=p) == EINVAL           # the initial-step norms take no terms
        assert call(mode=mode, n_terms=0, partial=None) == EINVAL        # ... and need `b`
    assert call(row_len=0) == EINVAL and call(n_rows=-1) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    assert call(part_bytes=47) == EWORKSPACE
    # one-chunk long rows and chunked rows: 3 * B * nch doubles
    assert call(row_len=2050, part_bytes=47) == EWORKSPACE
    assert call(row_len=4098, dtype=F64, part_bytes=3 * 2 * 2 * 8 - 1) == EWORKSPACE
    assert call(row_len=1 << 20, dtype=F32, part_bytes=3 * 2 * 128 * 8 - 1) == EWORKSPACE
    assert call(n_rows=0, part_bytes=0) == 0
    assert call(mode=1, n_terms=0, partial=p, n_rows=0, part_bytes=0) == 0


def _state(B=2, L=4, n_out=2):
    return RowVectors("cpu", B, L, torch.zeros(n_out, B))


def test_row_control_argument_errors(lib):
    buf, p, _ = _buffers()
    ctrl = _native.step_ctrl([0.0, 0.5, 1.0], [False, False, True], 3, 0.9, 10.0, 0.2, 0.0, float("inf"), 1.0, 1)
    rows = _state()

    def call(mode=0, part=p, c=ctrl, st=rows.st, dts=p, times=p, dtype=F64):
        return lib.tdeq_row_control(mode, part, None if c is None else ctypes.byref(c),
                                    None if st is None else ctypes.byref(st), dts, times, dtype, None)
    assert call(part=None) == EINVAL and call(c=None) == EINVAL and call(st=None) == EINVAL
    assert call(dts=None) == EINVAL and call(times=None) == EINVAL
    assert call(mode=-1) == EINVAL and call(mode=4) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    for n_times in (0, _native.TDEQ_MAX_STAGE_TIMES + 1):
        bad = type(ctrl).from_buffer_copy(ctrl)
        bad.n_times = n_times
        assert call(c=bad) == EINVAL, n_times
    for field, value in (("status", None), ("row_len", 0), ("n_rows", -1), ("n_out", 0)):
        st = type(rows.st).from_buffer_copy(rows.st)
        setattr(st, field, value)
        assert call(st=st) == EINVAL, field


def test_row_dense_commit_argument_errors(lib):
    buf, p, ptrs = _buffers()
    rows = _state()

    def call(st=rows.st, **kw):
        args = [kw.get(n, d) for n, d in (("sol", p), ("y0", p), ("y1", p), ("f0", p), ("f1", p), ("k", ptrs),
                                          ("coef", buf), ("n_terms", 1), ("dts", p))]
        return lib.tdeq_row_dense_commit(*args, None if st is None else ctypes.byref(st), kw.get("dtype", F64), None)
    for name in ("sol", "y0", "y1", "f0", "f1", "k", "coef", "dts"):
        assert call(**{name: None}) == EINVAL, name
    assert call(st=None) == EINVAL
    assert call(k=(ctypes.c_void_p * 14)()) == EINVAL
    assert call(n_terms=0) == EINVAL and call(n_terms=15) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    for field, value in (("row_len", 0), ("n_rows", -1)):
        st = type(rows.st).from_buffer_copy(rows.st)
        setattr(st, field, value)
        assert call(st=st) == EINVAL, field
    st = type(rows.st).from_buffer_copy(rows.st)
    st.n_rows = 0
    assert call(st=st) == 0


def test_row_scale_many_and_multi_dot_term_counts(lib):
    """The term counts of the two backward entry points (tests/test_rowwise_grad_gpu.py has their other answers)."""
    buf, p, ptrs = _buffers()
    for n in (0, 15, -1):
        assert lib.tdeq_row_scale_many(ptrs, n, p, p, 2, 4, F64, None) == EINVAL, n
        assert lib.tdeq_row_multi_dot(p, ptrs, n, 2, 4, p, None, 0, F64, None) == EINVAL, n
    assert lib.tdeq_row_scale_many(ptrs, 14, p, p, 0, 4, F64, None) == 0
    assert lib.tdeq_row_multi_dot(p, ptrs, 14, 0, 4, p, None, 0, F64, None) == 0


# (L, dtype code) -> partials per row: short rows, the one-chunk long rows, chunked rows
_PARTIALS = [(1, F32, 1), (1, F64, 1), (3, F32, 1), (4, F32, 1), (1024, F32, 1), (1024, F64, 1), (1023, F64, 1),
             (4096, F32, 1), (2048, F64, 1),                       # nv = 1024: the top of the short rows
             (4100, F32, 1), (8192, F32, 1), (1025, F32, 1), (1501, F32, 1), (2047, F32, 1),      # the fp32 bands
             (2050, F64, 1), (4096, F64, 1), (1025, F64, 1), (2047, F64, 1),                       # the fp64 bands
             (2049, F32, 2), (2049, F64, 2), (8196, F32, 2), (4098, F64, 2), (3 * 2048 + 1, F64, 4),
             (1 << 20, F32, 128), (1 << 20, F64, 256), (64 * 2048 + 1, F32, 65)]


def test_row_partials_table(lib, oracle_kernels):
    for L, code, nch in _PARTIALS:
        dtype = torch.float32 if code == F32 else torch.float64
        assert lib.tdeq_row_partials(L, code) == nch, (L, code)
        assert oracle_kernels.row_partials(L, dtype) == nch, (L, code)
    assert lib.tdeq_row_partials(0, F32) == EINVAL and lib.tdeq_row_partials(4, BF16) == EINVAL
    # the workspace of the row dots: none while a row has one partial (one-chunk long rows write `out` directly)
    assert lib.tdeq_row_dots_workspace_bytes(4, 4100, 3, F32) == 0
    assert lib.tdeq_row_dots_workspace_bytes(4, 2049, 3, F64) == 3 * 4 * 2 * 8
