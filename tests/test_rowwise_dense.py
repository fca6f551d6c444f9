"""`odeint_rowwise_dense` without a GPU: the host path (`HostRowKernels`) and `HipRowKernels` on the CPU row oracle
(tests/_rowwise_dense_oracle.py).  The contract: for queries inside a row's interval, `dense(q)` is bit for bit what
`odeint_rowwise` gives on the per-row grid [t0, the queries sorted, t1] — plus the structure of the store, `compact`,
forced small chunks, the out-of-range rules, errors, validation and the argument checks of the three new entry points.

Accepted steps per row at the settings of `tolerances` on `decay_problem(12, 5, dtype, 3)` with t1 = linspace(0.3, 0.6):
fp64 — dopri5 4 .. 60, tsit5 4 .. 58, dopri8 2 .. 17; fp32 at (1e-6, 1e-8) — dopri5 4 .. 39, tsit5 4 .. 38, dopri8 3 .. 13;
both dtypes at (1e-3, 1e-5) — bosh3 3 .. 22, fehlberg2 4 .. 16, adaptive_heun 11 .. 158."""
import contextlib
import ctypes
import functools
import math

import pytest
import torch

from _rowwise_dense_oracle import (METHODS, decay_problem, device_driver, grid_reference, per_row_t1, quiet,  # noqa: F401
                                   random_queries, tolerances)

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native, rowwise_dense

F32, F64 = torch.float32, torch.float64
BACKENDS = ["host", "oracle"]
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, L, SEED, Q = 12, 5, 3, 7
T1 = {"number": 0.45, "vector": per_row_t1(B)}


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _t1_rows(t1):
    return t1 if isinstance(t1, torch.Tensor) else torch.full((B,), float(t1), dtype=F64)


def _dense(func, y0, t0, t1, **kw):
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, t1, return_stats=True, **kw)


def _grid_solver(func, y0, **kw):
    def solve(grid):
        with torch.no_grad():
            return tda.odeint_rowwise(func, y0, grid, **kw)
    return solve


@functools.lru_cache(maxsize=None)
def _solved(backend_key, method, dtype, t1_key):
    """One dense solve per (backend, method, dtype, t1), shared by the tests that only evaluate it.  Called inside the
    backend's context; the dense object keeps the backend it was solved on."""
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    return _dense(func, y0, 0.0, T1[t1_key], method=method, **tolerances(method, dtype))


def _assert_equals_grid(dense, q, func, y0, t0, t1, **kw):
    got = dense(q)
    ref = grid_reference(_grid_solver(func, y0, **kw), q, t0, t1)
    assert got.shape == ref.shape == (q.shape[0], *y0.shape)
    assert torch.equal(got, ref)
    return got


# -- 1. the contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t1_key", ["number", "vector"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_dense_equals_the_grid_solve(backend, device_driver, method, dtype, t1_key):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1[t1_key])
    q = random_queries(Q, t0, t1, seed=11)                                   # unsorted per row
    with _backend(backend, device_driver):
        dense, stats = _solved(backend, method, dtype, t1_key)
        _assert_equals_grid(dense, q, func, y0, t0, t1, method=method, **tolerances(method, dtype))
        # and the solve is the solve on [t0, t1]: the same counters
        with torch.no_grad():
            _, plain = tda.odeint_rowwise(func, y0, torch.stack([t0, t1]), method=method, return_stats=True,
                                          **tolerances(method, dtype))
    for name in ("n_accepted", "n_rejected", "nfe"):
        assert torch.equal(torch.as_tensor(stats[name]), torch.as_tensor(plain[name])), name
    assert stats["n_segments"] == int(stats["n_accepted"].sum()) == dense.n_segments
    print(f"accepted per row {int(stats['n_accepted'].min())} .. {int(stats['n_accepted'].max())}, chunks {stats['n_chunks']}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_query_forms(backend, device_driver, dtype):
    """Repeated queries, a shared [Q] list, a scalar, a 0-dim tensor and an fp32 query tensor."""
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1["vector"])
    kw = dict(method="dopri5", **tolerances("dopri5", dtype))
    q = random_queries(4, t0, t1, seed=5)
    q = torch.cat([q, q[[2, 0, 2]]])                                         # repeats, out of order
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)               # inside every row's interval
    with _backend(backend, device_driver):
        dense, _ = _solved(backend, "dopri5", dtype, "vector")
        got = _assert_equals_grid(dense, q, func, y0, t0, t1, **kw)
        assert torch.equal(got[4], got[2]) and torch.equal(got[5], got[0])
        by_list = dense(shared)
        assert torch.equal(by_list, _assert_equals_grid(dense, shared[:, None].expand(-1, B).contiguous(), func, y0, t0, t1, **kw))
        assert by_list.shape == (4, B, L)
        one = dense(0.21)
        assert one.shape == (B, L) and torch.equal(one, by_list[0]) and torch.equal(dense(torch.tensor(0.21, dtype=F64)), one)
        q32 = shared.to(F32)                                                 # cast to fp64 as odeint_rowwise casts its grid
        assert torch.equal(dense(q32), dense(q32.to(F64)))
        assert dense(torch.empty(0, dtype=F64)).shape == (0, B, L)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["dopri5", "bosh3", "dopri8"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_ends_and_breakpoints(backend, device_driver, method, dtype):
    """t0, t1 and EVERY breakpoint of every row (from `seg_end`; a row with fewer of them repeats its own): a breakpoint
    belongs to the earlier step (x = 1) exactly as the grid solve places an output time that equals a step's end."""
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1["vector"])
    with _backend(backend, device_driver):
        dense, stats = _solved(backend, method, dtype, "vector")
        off = dense.offsets.tolist()
        inner = [dense.seg_end[off[r]:off[r + 1] - 1] for r in range(B)]     # (the last end is t1 or beyond it)
        assert all(bool((b < t1[r]).all()) for r, b in enumerate(inner))
        n = max(len(b) for b in inner)
        cols = [b[torch.arange(n) % len(b)] if len(b) else t1[r].expand(n) for r, b in enumerate(inner)]
        q = torch.cat([t0[None], t1[None], torch.stack(cols, dim=1)])
        got = _assert_equals_grid(dense, q, func, y0, t0, t1, method=method, **tolerances(method, dtype))
    assert torch.equal(got[0], y0)                                           # x = 0 of the first segment: e = y0
    assert n >= 10 or method == "dopri8"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_decreasing_time_row_tolerances_and_first_step(backend, device_driver, dtype):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t0 = torch.full((B,), 0.3, dtype=F64)
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
    rtol = torch.logspace(-4, -6, B, dtype=F64)
    atol = (rtol * 1e-2).tolist()
    first = torch.linspace(1e-3, 5e-3, B, dtype=F64)
    q = random_queries(Q, t0, t1, seed=2)
    for kw in (dict(method="dopri5", **tolerances("dopri5", dtype)),                               # decreasing time
               dict(method="tsit5", rtol=rtol, atol=atol),                                         # [B] tolerances
               dict(method="bosh3", options={"first_step": first}, **tolerances("bosh3", dtype))):  # per-row first_step
        with _backend(backend, device_driver):
            dense, stats = _dense(func, y0, 0.3, t1, **kw)
            _assert_equals_grid(dense, q, func, y0, t0, t1, **kw)
            ends = torch.stack([t0, t1])
            _assert_equals_grid(dense, ends, func, y0, t0, t1, **kw)
        assert torch.equal(dense.t0, t0) and torch.equal(dense.t1, t1)
        assert bool((dense.seg_end < dense.seg_start).all())                 # true time


# -- 2. the store ------------------------------------------------------------------------------------------------------------------
def _same_dense(a, b):
    for name in ("t0", "t1", "offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.n_segments == b.n_segments


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_structure(backend, device_driver, method, dtype):
    with _backend(backend, device_driver):
        dense, stats = _solved(backend, method, dtype, "vector")
    t1 = _t1_rows(T1["vector"])
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(stats["n_accepted"], 0)
    assert torch.equal(dense.offsets, off) and dense.offsets.dtype == torch.int64
    assert dense.coeffs.shape == (5, int(off[-1]), L) and dense.coeffs.dtype == dtype
    assert dense.seg_start.dtype == dense.seg_end.dtype == dense.t0.dtype == F64
    for r in range(B):
        a, b = dense.seg_start[off[r]:off[r + 1]], dense.seg_end[off[r]:off[r + 1]]
        assert float(a[0]) == 0.0 and torch.equal(a[1:], b[:-1]) and bool((b > a).all())
        assert float(b[-1]) >= float(t1[r]) and (len(b) == 1 or float(b[-2]) < float(t1[r]))
    assert torch.equal(dense.t0, torch.zeros(B, dtype=F64)) and torch.equal(dense.t1, t1)


@pytest.mark.parametrize("compact", [True, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_compact_equals_plain(backend, device_driver, method, dtype, compact):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1["vector"])
    q = torch.cat([random_queries(Q, t0, t1, seed=4), t0[None], t1[None]])
    with _backend(backend, device_driver):
        plain, st_p = _solved(backend, method, dtype, "vector")
        dense, st_c = _dense(func, y0, 0.0, T1["vector"], method=method, compact=compact, **tolerances(method, dtype))
        assert torch.equal(dense(q), plain(q))
    _same_dense(dense, plain)
    for name in ("n_accepted", "n_rejected"):
        assert torch.equal(st_c[name], st_p[name]), name
    assert st_c["nfe"] == st_p["nfe"] and st_c["n_segments"] == st_p["n_segments"]
    assert "n_repacks" not in st_p and "row_evals" not in st_p
    assert st_c["n_repacks"] >= 1 and st_c["row_evals"] < B * st_c["nfe"]


@pytest.mark.parametrize("compact", [None, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_small_chunks_pack_to_the_same_arrays(backend, device_driver, dtype, compact):
    """`dense_chunk_rows=1` is raised to B = 12 slots: the 299 (fp32: 199) quartics of the dopri5 solve need many chunks;
    4096 slots hold them all."""
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    kw = dict(method="dopri5", compact=compact, **tolerances("dopri5", dtype))
    with _backend(backend, device_driver):
        one, st_one = _dense(func, y0, 0.0, T1["vector"], options={"dense_chunk_rows": 4096}, **kw)
        many, st_many = _dense(func, y0, 0.0, T1["vector"], options={"dense_chunk_rows": 1}, **kw)
    assert st_one["n_chunks"] == 1 and st_many["n_chunks"] >= 3
    assert st_many["n_chunks"] >= math.ceil(st_many["n_segments"] / B)
    _same_dense(many, one)


def test_chunk_policy():
    assert rowwise_dense._chunk_rows({}, 12, 5, 8) == 48                                       # a few B
    assert rowwise_dense._chunk_rows({}, 65536, 128, 4) == (256 << 20) // (5 * 128 * 4)        # bounded by bytes
    assert rowwise_dense._chunk_rows({}, 65536, 4096, 8) == 65536                              # never fewer than B
    assert rowwise_dense._chunk_rows({"dense_chunk_rows": 3}, 12, 5, 8) == 12
    assert rowwise_dense._chunk_rows({"dense_chunk_rows": 100}, 12, 5, 8) == 100


# -- 3. out of range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_out_of_range(backend, device_driver, dtype):
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1["vector"])
    good = random_queries(3, t0, t1, seed=9)
    with _backend(backend, device_driver):
        dense, _ = _solved(backend, "dopri5", dtype, "vector")
        want = dense(good)
        last_end = dense.seg_end[dense.offsets[4 + 1] - 1]
        assert float(last_end) > float(t1[4])                                # row 4's last step reaches beyond its t1
        cases = {"below t0": (1, 7, -1e-9), "beyond t1": (2, 4, float(t1[4] + (last_end - t1[4]) / 2)),
                 "nan": (0, 11, float("nan")), "next after t1": (1, 0, math.nextafter(float(t1[0]), math.inf))}
        for name, (j, r, v) in cases.items():
            q = good.clone()
            q[j, r] = v
            with pytest.raises(ValueError, match=rf"query {j} of row {r} "):
                dense(q)
            got = dense(q, check=False)
            assert bool(torch.isnan(got[j, r]).all()), name
            got[j, r] = want[j, r]
            assert torch.equal(got, want), name                              # every other row unchanged
        # several: the smallest flat index (j, r) is named
        q = good.clone()
        q[2, 1], q[1, 9], q[1, 3] = float("nan"), 5.0, -2.0
        with pytest.raises(ValueError, match=r"query 1 of row 3 "):
            dense(q)
        got = dense(q, check=False)
        bad = torch.isnan(got).all(dim=2)
        assert bad.nonzero().tolist() == [[1, 3], [1, 9], [2, 1]] and not bool(torch.isnan(got[~bad]).any())
        # t1 itself is valid (the reference's closure raises IndexError there), shared queries beyond the shortest row are not
        assert not bool(torch.isnan(dense(t1[None])).any())
        with pytest.raises(ValueError, match=r"query 0 of row 0 "):
            dense(0.5)


# -- 4. errors and validation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_max_num_steps_names_the_original_row_after_a_repack(backend, device_driver):
    """Rows 0 and 1 reach their t1 within a few steps and leave; the stiff row 2, then first of the carried rows, runs into
    max_num_steps: the message names row 2."""
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=F64)
    sizes = []

    def f(t, y, rows):
        sizes.append(rows.tolist())
        return -k[rows] * (y - torch.sin(t)[:, None])
    with _backend(backend, device_driver):
        with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(50>=50\) in row 2"):
            _dense(f, torch.ones(4, 1, dtype=F64), 0.0, torch.tensor([0.01, 0.01, 5.0, 5.0], dtype=F64), rtol=1e-5, atol=1e-7,
                   options={"max_num_steps": 50}, compact=1.0)
    assert sizes[0] == [0, 1, 2, 3] and sizes[-1] in ([2], [2, 3])


def test_gradients_are_refused():
    y0, func, k = decay_problem(B, L, F64, SEED)
    for kw in (dict(y0=y0.clone().requires_grad_(True)), dict(t0=torch.tensor(0.0, requires_grad=True)),
               dict(t1=torch.full((B,), 0.4, dtype=F64, requires_grad=True))):
        args = dict(y0=y0, t0=0.0, t1=0.4)
        args.update(kw)
        with pytest.raises(NotImplementedError, match="odeint_rowwise_dense"):
            tda.odeint_rowwise_dense(func, **args)
        with torch.no_grad():
            tda.odeint_rowwise_dense(func, **args, rtol=1e-3, atol=1e-5)
    class Field(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(L, L).double()

        def forward(self, t, y):
            return self.lin(y)
    with pytest.raises(NotImplementedError, match="odeint_rowwise_dense"):       # a parameter of func
        tda.odeint_rowwise_dense(Field(), y0, 0.0, 0.4)
    kp = k.clone().requires_grad_(True)                                      # a closure: caught at the first evaluation
    with pytest.raises(NotImplementedError):
        tda.odeint_rowwise_dense(lambda t, y: -kp * y, y0, 0.0, 0.4)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, 0.4, rtol=1e-3, atol=1e-5)
    with pytest.raises(NotImplementedError, match="gradients"):
        dense(torch.tensor([0.1], dtype=F64, requires_grad=True))
    assert "differentiable" not in tda.odeint_rowwise_dense.__code__.co_varnames


def test_validation():
    y0, func, _ = decay_problem(B, L, F64, SEED)
    two = lambda t, y: func(t, y)      # noqa: E731
    with torch.no_grad():
        for t0, t1 in ((0.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0), (0.0, torch.linspace(-0.1, 0.3, B)),
                       (torch.zeros(B), torch.cat([torch.zeros(1), torch.ones(B - 1)])), (0.0, torch.ones(B + 1)),
                       (0.0, torch.ones(B, 1)), ("0", 1.0), (0.0, None), (0.0, True), (0.0, torch.ones(B, dtype=torch.complex64))):
            with pytest.raises(ValueError, match="odeint_rowwise_dense: t"):
                tda.odeint_rowwise_dense(two, y0, t0, t1)
        for bad in (0.0, -0.5, 1.5, 2, "yes", [0.5]):
            with pytest.raises(ValueError, match="compact"):
                tda.odeint_rowwise_dense(func, y0, 0.0, 0.4, compact=bad)
        for bad in (0, -3, 2.5, "8", True):
            with pytest.raises(ValueError, match="dense_chunk_rows"):
                tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, options={"dense_chunk_rows": bad})
        with pytest.raises(ValueError, match="unsupported option"):
            tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, options={"dense_rows": 4})
        with pytest.raises(ValueError, match="method"):
            tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, method="rk4")
        for bad_y0 in (y0.half(), y0.to(torch.complex64), (y0, y0), torch.tensor(1.0)):
            with pytest.raises(ValueError):
                tda.odeint_rowwise_dense(two, bad_y0, 0.0, 0.4)
        with pytest.raises(TypeError):                                       # compact: func takes `rows`
            tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, compact=True)
        dense = tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, rtol=1e-3, atol=1e-5)
        assert not isinstance(dense, tuple)
        for bad_t in (torch.zeros(2, B + 1), torch.zeros(2, B, 1), "0.1", None, torch.zeros(3, dtype=torch.bool)):
            with pytest.raises(ValueError, match=r"dense\(t\)"):
                dense(bad_t)
        _, stats = tda.odeint_rowwise_dense(two, y0, 0.0, 0.4, rtol=1e-3, atol=1e-5, return_stats=True)
        assert sorted(stats) == ["n_accepted", "n_chunks", "n_rejected", "n_segments", "nfe"]
    assert "odeint_rowwise_dense" in tda.__all__


# -- 5. against the closed form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_closed_form(method, dtype):
    """y = y0 exp(-k (t + t^2 / 2)).  The bound is no fixed number: per row, FACTOR times the largest error
    `odeint_rowwise` itself shows on the same problem at 33 uniform interior output times — those are values of the same
    interpolants, so 7 random times can exceed that maximum only by what 33 samples miss of a smooth error curve's peaks; 4
    covers it with room (plus one rounding of the exact value in the state's dtype)."""
    FACTOR = 4.0
    y0, func, k = decay_problem(B, L, dtype, SEED)
    t0, t1 = torch.zeros(B, dtype=F64), _t1_rows(T1["vector"])
    kw = dict(method=method, **tolerances(method, dtype))
    exact = lambda t: y0.double()[None] * torch.exp(-k.double()[None] * (t + t * t / 2)[:, :, None])      # noqa: E731
    grid = t0[None] + torch.linspace(0, 1, 35, dtype=F64)[:, None] * (t1 - t0)[None]
    with torch.no_grad():
        ref = tda.odeint_rowwise(func, y0, grid, **kw)
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1, **kw)
    own = (ref.double() - exact(grid)).abs().amax(dim=(0, 2))                                  # [B]
    q = random_queries(Q, t0, t1, seed=21)
    err = (dense(q).double() - exact(q)).abs().amax(dim=(0, 2))
    bound = FACTOR * own + torch.finfo(dtype).eps * y0.double().abs().amax(dim=1)
    print("largest error / bound per row:", [f"{float(e):.2e}/{float(b):.2e}" for e, b in zip(err, bound)])
    assert bool((own > 0).all()) and bool((err <= bound).all())


# -- 6. the argument checks of the three new entry points ------------------------------------------------------------------------
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _caller(fn, names, base):
    return lambda **kw: fn(*[kw.get(n, base[n]) for n in names])


def _row_state(p, n_rows):
    st = _native.RowState()
    for name in ("t0", "tprev", "accepted", "n_acc"):
        setattr(st, name, p)
    st.n_rows = n_rows
    return st


def test_row_dense_slots_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    names = ("st", "row_map", "cap", "counter", "slot_row", "slot_ord", "slot_ta", "slot_tb", "slot", "mask", "stream")
    base = dict(st=ctypes.byref(_row_state(p, 4)), row_map=p, cap=8, counter=p, slot_row=p, slot_ord=p, slot_ta=p, slot_tb=p,
                slot=p, mask=p, stream=None)
    slots = _caller(lib.tdeq_row_dense_slots, names, base)
    for name in ("st", "counter", "slot_row", "slot_ord", "slot_ta", "slot_tb", "slot", "mask"):
        assert slots(**{name: None}) == EINVAL, name
    for field in ("t0", "tprev", "accepted", "n_acc"):
        st = _row_state(p, 4)
        setattr(st, field, None)
        assert slots(st=ctypes.byref(st)) == EINVAL, field
    assert slots(st=ctypes.byref(_row_state(p, -1))) == EINVAL
    assert slots(st=ctypes.byref(_row_state(p, 2 ** 31))) == EINVAL
    for kw in (dict(cap=-1), dict(cap=2 ** 31 - 4), dict(cap=2 ** 40)):      # cap + n_rows must fit an int32
        assert slots(**kw) == EINVAL, kw
    empty = ctypes.byref(_row_state(p, 0))
    assert slots(st=empty) == 0 and slots(st=empty, row_map=None, cap=0) == 0              # no row: no launch
    assert slots(st=empty, mask=None) == EINVAL and slots(st=empty, cap=-1) == EINVAL      # (the checks come first)


def test_row_dense_pack_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    names = ("dst", "dst_rows", "src", "src_rows", "dest", "n_used", "row_len", "dtype", "stream")
    base = dict(dst=p, dst_rows=9, src=p, src_rows=6, dest=p, n_used=4, row_len=4, dtype=_native.TDEQ_F32, stream=None)
    pack = _caller(lib.tdeq_row_dense_pack, names, base)
    for name in ("dst", "src", "dest"):
        assert pack(**{name: None}) == EINVAL, name
    for kw in (dict(dst_rows=-1), dict(dst_rows=0), dict(src_rows=-1), dict(src_rows=3), dict(n_used=-1), dict(n_used=7),
               dict(row_len=0), dict(row_len=-4), dict(dtype=_native.TDEQ_F16), dict(dtype=_native.TDEQ_C64), dict(dtype=9)):
        assert pack(**kw) == EINVAL, kw
    assert pack(n_used=0) == 0 and pack(n_used=0, dst_rows=0, src_rows=0) == 0
    assert pack(n_used=0, dest=None) == EINVAL and pack(n_used=0, src_rows=-1) == EINVAL


def test_row_dense_search_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    names = ("tq", "n_q", "offsets", "seg_ta", "seg_tb", "n_seg", "t0", "t1", "n_rows", "seg", "x", "status", "dtype", "stream")
    base = dict(tq=p, n_q=2, offsets=p, seg_ta=p, seg_tb=p, n_seg=5, t0=p, t1=p, n_rows=3, seg=p, x=p, status=p,
                dtype=_native.TDEQ_F64, stream=None)
    search = _caller(lib.tdeq_row_dense_search, names, base)
    for name in ("tq", "offsets", "seg_ta", "seg_tb", "t0", "t1", "seg", "x", "status"):
        assert search(**{name: None}) == EINVAL, name
    for kw in (dict(n_q=-1), dict(n_rows=-1), dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31), dict(n_q=2 ** 31),
               dict(n_q=2 ** 30, n_rows=2), dict(dtype=_native.TDEQ_BF16), dict(dtype=_native.TDEQ_C128), dict(dtype=6)):
        assert search(**kw) == EINVAL, kw
    assert search(n_q=0) == 0 and search(n_rows=0) == 0 and search(n_q=0, n_seg=0) == 0
    assert search(n_q=0, status=None) == EINVAL and search(n_rows=0, n_seg=-1) == EINVAL
