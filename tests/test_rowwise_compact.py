"""`odeint_rowwise(compact=...)` without a GPU: the torch-op host path and, through `device_driver`, `HipRowKernels` on
the CPU row oracle.  A compacted solve must give the bits of the plain one — a row's arithmetic does not depend on the
batch it sits in — while `func` sees fewer and fewer rows, on the schedule the policy prescribes (the simulator of
tests/_rowwise_compact_oracle.py, written from the policy's text)."""
import contextlib
import ctypes

import pytest
import torch

from _rowwise_compact_oracle import (METHODS, assert_same_solve, decay_problem, device_driver, quiet,  # noqa: F401
                                     random_problem, simulate, solve_both)
from _rowwise_kernels import RowVectors

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

BACKENDS = ["host", "oracle"]
# repacks of c = 0.5 on the random problem (96 rows; adaptive_heun 12), from the plain host solve's trial counts
REPACKS_HALF = {"dopri5": 5, "tsit5": 5, "bosh3": 6, "fehlberg2": 6, "dopri8": 6, "adaptive_heun": 3}


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


_PLAIN = {}


def _plain_random(backend, method, device_driver):
    """The plain solve of the random problem, computed once per (backend, method) and left unchanged."""
    key = (backend, method)
    if key not in _PLAIN:
        B = 12 if method == "adaptive_heun" else 96
        y0, plain, by_rows, subset = random_problem(B, 5, torch.float64, 1)
        t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
        with torch.no_grad(), _backend(backend, device_driver):
            res = tda.odeint_rowwise(plain, y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
        _PLAIN[key] = (y0, t, by_rows, subset, res)
    return _PLAIN[key]


# -- 1. bit-identity on the random problem ------------------------------------------------------------------------------------
# (adaptive_heun, thousands of steps through the row-by-row oracle, runs on the host path only)
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("backend,method", [(b, m) for b in BACKENDS for m in METHODS if (b, m) != ("oracle", "adaptive_heun")])
def test_compact_equals_plain_fp64(backend, method, c, device_driver):
    y0, t, by_rows, _, plain = _plain_random(backend, method, device_driver)
    with torch.no_grad(), _backend(backend, device_driver):
        compact = tda.odeint_rowwise(by_rows, y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True, compact=c)
    _, repacks = assert_same_solve(plain, compact, c, method)
    assert repacks >= 3
    if c == 0.5 and backend == "host":
        assert repacks == REPACKS_HALF[method]


@pytest.mark.parametrize("method", METHODS)
def test_plain_rows_do_not_depend_on_the_batch(method, device_driver):
    """What compaction rests on, on the plain path: a subset of the rows solved alone has the bits it has in the batch."""
    y0, t, _, subset, (sol, stats) = _plain_random("host", method, device_driver)
    idx = torch.arange(y0.shape[0])[1::3]
    with torch.no_grad():
        part, sp = tda.odeint_rowwise(subset(idx), y0[idx], t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
    assert torch.equal(part, sol[:, idx])
    assert torch.equal(sp["n_accepted"], stats["n_accepted"][idx]) and torch.equal(sp["n_rejected"], stats["n_rejected"][idx])


# -- 2. fp32, a func without transcendentals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("backend", BACKENDS)
def test_compact_equals_plain_fp32(backend, c, device_driver):
    y0, plain, by_rows = decay_problem(64, 8, 1)
    t = torch.tensor([0.0, 0.5, 1.0])
    with _backend(backend, device_driver):
        res = solve_both(plain, by_rows, y0, t, c, rtol=1e-5, atol=1e-7)
    trials, repacks = assert_same_solve(*res, c, "dopri5")
    assert repacks >= 3
    if backend == "host":
        assert (min(trials), max(trials)) == (3, 38)
        if c == 0.5:
            assert repacks == 5


# -- 3. grids and options ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("kind", ["t2d", "decreasing", "first_step"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_compact_grids_and_options(backend, kind, c, device_driver):
    B = 12
    y0, plain, by_rows, _ = random_problem(B, 3, torch.float64, 7)
    t = torch.linspace(0, 1.2, 4, dtype=torch.float64)
    opts = None
    if kind == "t2d":            # rows that end at different times
        t = t[:, None] * torch.linspace(0.2, 1.0, B, dtype=torch.float64) + 0.05 * torch.arange(B).to(torch.float64)
    elif kind == "decreasing":
        t = torch.linspace(1, 0, 4, dtype=torch.float64)
    else:
        opts = {"first_step": torch.linspace(1e-3, 5e-3, B, dtype=torch.float64)}
    with _backend(backend, device_driver):
        res = solve_both(plain, by_rows, y0, t, c, rtol=1e-6, atol=1e-8, options=opts)
    _, repacks = assert_same_solve(*res, c, "dopri5", first_step_given=kind == "first_step")
    assert repacks >= 1


# -- 4. what func sees ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_contract(backend, c, device_driver):
    B, S = 24, 6
    y0, plain, by_rows, _ = random_problem(B, 3, torch.float64, 5)
    t = torch.linspace(0, 1.5, 3, dtype=torch.float64)
    seen = []

    def func(t_rows, y, rows):
        assert rows.dtype == torch.int64 and rows.device == y.device and rows.dim() == 1
        assert len(rows) == y.shape[0] == t_rows.shape[0] and y.shape[1:] == y0.shape[1:]
        assert bool((rows[1:] > rows[:-1]).all())
        seen.append(rows.tolist())
        return by_rows(t_rows, y, rows)
    with torch.no_grad(), _backend(backend, device_driver):
        _, stats = tda.odeint_rowwise(func, y0, t, rtol=1e-6, atol=1e-8, return_stats=True, compact=c)
    trials = (stats["n_accepted"] + stats["n_rejected"]).tolist()
    assert len(seen) == stats["nfe"] and sum(len(r) for r in seen) == stats["row_evals"]
    assert seen[0] == seen[1] == list(range(B))                      # f(t0, y0) and the initial step's probe
    lengths = [len(r) for r in seen]
    assert all(a >= b for a, b in zip(lengths, lengths[1:]))
    assert trials.index(max(trials)) in seen[-1] and lengths[-1] < B
    # the calls of trial step i (S each) carry the rows the schedule says, and those rows are the longest-running ones
    carried, _ = simulate(trials, c)
    assert lengths[2:] == [n for n in carried for _ in range(S)]
    for i, n in enumerate(carried):
        rows = seen[2 + S * i]
        assert all(rows == seen[2 + S * i + s] for s in range(S))
        if c == 1.0 and n < B:
            # after the first repack no call holds a row that was inactive at the poll before it
            assert rows == [r for r in range(B) if trials[r] > i]
        else:
            assert set(rows) >= {r for r in range(B) if trials[r] > i}


# -- 5. an error after a repack names the original row -------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_max_num_steps_names_the_original_row(backend, device_driver):
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=torch.float64)
    y0 = torch.ones(4, 1, dtype=torch.float64)
    lengths = []

    def func(t, y, rows):
        lengths.append(len(rows))
        return -k[rows] * (y - torch.sin(t)[:, None])
    with _backend(backend, device_driver), \
            pytest.raises(AssertionError, match=r"max_num_steps exceeded \(\d+>=50\) in row 2"):
        tda.odeint_rowwise(func, y0, torch.tensor([0.0, 5.0]), rtol=1e-5, atol=1e-7, options={"max_num_steps": 50},
                           compact=1.0)
    assert lengths[-1] == 1                                           # the stiff row was alone by then: compact row 0


# -- 6. validation -------------------------------------------------------------------------------------------------------------------
def test_compact_validation():
    y0 = torch.ones(3, 2, dtype=torch.float64)
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    for bad in (0, 1.5, -0.1, "x"):
        with pytest.raises(ValueError, match="compact"):
            tda.odeint_rowwise(lambda t_, y, rows: -y, y0, t, compact=bad)
    with pytest.raises(NotImplementedError, match="compact"):
        tda.odeint_rowwise(lambda t_, y, rows: -y, y0.clone().requires_grad_(True), t, differentiable=True, compact=0.5)
    for off in (None, False):
        with torch.no_grad():
            _, stats = tda.odeint_rowwise(lambda t_, y: -y, y0, t, return_stats=True, compact=off)     # two arguments
        assert sorted(stats) == ["n_accepted", "n_rejected", "nfe"]
    with torch.no_grad():                                             # True is 0.5; under no_grad `differentiable` is inert
        k = torch.tensor([[0.1], [30.0], [1.0]], dtype=torch.float64)
        _, stats = tda.odeint_rowwise(lambda t_, y, rows: -k[rows] * y, y0, t, return_stats=True, compact=True,
                                      differentiable=True)
        _, half = tda.odeint_rowwise(lambda t_, y, rows: -k[rows] * y, y0, t, return_stats=True, compact=0.5)
    assert stats["row_evals"] == half["row_evals"] and stats["n_repacks"] == half["n_repacks"] >= 1


# -- 7. argument validation of the two entry points (no launch is reached) ----------------------------------------------------------
EINVAL = -1
F32, F64, BF16 = _native.TDEQ_F32, _native.TDEQ_F64, _native.TDEQ_BF16


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _buffers():
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    return buf, p, (ctypes.c_void_p * 14)(*([p] * 14))


def test_row_gather_argument_errors(lib):
    buf, p, ptrs = _buffers()
    call = lambda **kw: lib.tdeq_row_gather(*[kw.get(n, d) for n, d in (        # noqa: E731
        ("dst", ptrs), ("src", ptrs), ("n_src", 2), ("idx", p), ("n_idx", 3), ("row_len", 4), ("dtype", F64),
        ("stream", None))])
    for name in ("dst", "src", "idx"):
        assert call(**{name: None}) == EINVAL, name
    one_null = (ctypes.c_void_p * 14)(p, None, p, p)
    assert call(dst=one_null) == EINVAL and call(src=one_null) == EINVAL
    assert call(n_src=0) == EINVAL and call(n_src=5) == EINVAL and call(n_src=-1) == EINVAL
    assert call(n_idx=-1) == EINVAL
    assert call(row_len=0) == EINVAL and call(row_len=-4) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    for n_src in (1, 2, 3, 4):
        assert call(n_src=n_src, n_idx=0) == 0                         # no row: no launch
    assert call(dst=one_null, n_src=1, n_idx=0) == 0                   # (a null behind n_src is not looked at)


def test_row_dense_commit_mapped_argument_errors(lib):
    buf, p, ptrs = _buffers()
    rows = RowVectors("cpu", 2, 4, torch.zeros(2, 2))

    def call(st=rows.st, **kw):
        args = [kw.get(n, d) for n, d in (("sol", p), ("row_map", p), ("sol_rows", 7), ("y0", p), ("y1", p), ("f0", p),
                                          ("f1", p), ("k", ptrs), ("coef", buf), ("n_terms", 1), ("dts", p))]
        return lib.tdeq_row_dense_commit_mapped(*args, None if st is None else ctypes.byref(st), kw.get("dtype", F64), None)
    for name in ("sol", "row_map", "y0", "y1", "f0", "f1", "k", "coef", "dts"):
        assert call(**{name: None}) == EINVAL, name
    assert call(st=None) == EINVAL
    assert call(k=(ctypes.c_void_p * 14)()) == EINVAL
    assert call(n_terms=0) == EINVAL and call(n_terms=15) == EINVAL
    assert call(dtype=BF16) == EINVAL and call(dtype=7) == EINVAL
    assert call(sol_rows=0) == EINVAL and call(sol_rows=1) == EINVAL  # fewer solution rows than compact rows
    for field, value in (("row_len", 0), ("n_rows", -1)):
        st = type(rows.st).from_buffer_copy(rows.st)
        setattr(st, field, value)
        assert call(st=st) == EINVAL, field
    st = type(rows.st).from_buffer_copy(rows.st)
    st.n_rows = 0
    assert call(st=st) == 0


def test_row_gather_wrapper_takes_no_rows(lib):
    """Empty tensors have null pointers, which the entry point refuses: the wrapper returns before the call."""
    out, src = torch.empty(0, 8), torch.ones(4, 8)
    _native.HipKernels(lib).row_gather([out], [src], torch.empty(0, dtype=torch.int32))
    assert lib.tdeq_row_gather((ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_void_p * 1)(src.data_ptr()), 1, None, 0, 8,
                               F32, None) == EINVAL
