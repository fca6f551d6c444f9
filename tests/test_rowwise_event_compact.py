"""`odeint_rowwise_event(compact=...)` without a GPU: the host path (`HostRowKernels`) and `HipRowKernels` on the CPU row
oracle (tests/_rowwise_event_compact_oracle.py), each against the SAME call without `compact` on the same backend — every
output bit for bit — plus what makes the comparison worth something (rows did leave, the bisection ran on the rows with
a quartic only), the `rows` argument, the error row after a repack, validation and the argument checks of the two new
entry points."""
import contextlib
import ctypes
import functools

import pytest
import torch

from _rowwise_event_compact_oracle import METHODS, decay_event_problem_rows, device_driver, quiet  # noqa: F401
from _rowwise_event_oracle import decay_event_problem

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
BACKENDS = ["host", "oracle"]
COMPACT = [True, 1.0, 0.25]
B, L, SEED = 12, 5, 3
# fp32 draws its rows from seed 1: one of the seeds (1, 10, 11 of the first twelve) at which all 54 fp32 cases of
# test_compact_equals_plain see a repack — at seed 3 dopri8 with t_end = 0.15 stops its last seven rows in one trial step
SEEDS = {F64: SEED, F32: 1}
T_ENDS = {"none": None, "number": 0.15, "vector": torch.linspace(0.05, 0.4, B, dtype=F64)}
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
# the trial steps per row of the plain fp64 dopri5 solve without t_end at the default tolerances, sorted
DOPRI5_TRIALS = [2, 2, 3, 3, 4, 5, 6, 7, 8, 10, 11, 14]


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _tols(method, dtype):
    """The defaults in fp64 and (1e-6, 1e-8) in fp32: tight enough that also dopri8's rows take different numbers of
    trial steps, so that every threshold has a poll to repack at (with t_end = 0.15 the six unfired rows of a looser
    solve reach t_end in the same trial step as the last fired one).  The order-2 pairs, which take hundreds of steps per
    row at those, get (1e-5, 1e-7) and (1e-4, 1e-6); looser still, fehlberg2's estimate lets an unstable step pass on the
    stiff rows."""
    rtol, atol = (1e-7, 1e-9) if dtype == F64 else (1e-6, 1e-8)
    loosen = 100
    return (rtol * loosen, atol * loosen) if method in ("adaptive_heun", "fehlberg2") else (rtol, atol)


def _solve(func, y0, t0, event_fn, **kw):
    with torch.no_grad():
        return tda.odeint_rowwise_event(func, y0, t0, event_fn=event_fn, return_stats=True, **kw)


def _assert_same(plain, compact, min_repacks=1):
    """(event_t, solution, stats) of the plain call and of the same call with `compact`: every output the same bits, and
    the compact solve did take rows out."""
    (tp, sp, xp), (tc, sc, xc) = plain, compact
    assert torch.equal(tc, tp) and torch.equal(sc, sp)
    for name in ("n_accepted", "n_rejected", "fired"):
        assert torch.equal(xc[name], xp[name]), name
    assert xc["nfe"] == xp["nfe"] and xc["n_event_evals"] == xp["n_event_evals"]
    assert not {"row_evals", "n_repacks", "event_row_evals"} & set(xp)
    n = tp.shape[0]
    print(f"n_repacks {xc['n_repacks']}, row_evals {xc['row_evals']} of {n * xc['nfe']}, event_row_evals "
          f"{xc['event_row_evals']} of {n * xc['n_event_evals']}")
    assert xc["n_repacks"] >= min_repacks
    assert xc["row_evals"] < n * xc["nfe"]
    assert xc["event_row_evals"] < n * xc["n_event_evals"]


@functools.lru_cache(maxsize=None)
def _plain(backend_key, method, dtype, t_end_key):
    """The plain solve of one (backend, method, dtype, t_end): computed once, shared by the three `compact` values."""
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEEDS[dtype])
    rtol, atol = _tols(method, dtype)
    two = lambda f: (lambda t, y: f(t, y))      # noqa: E731  (strictly two arguments: a third would be a TypeError)
    return _solve(two(func), y0, 0.0, two(event_fn), t_end=T_ENDS[t_end_key], rtol=rtol, atol=atol, method=method)


def _compact_against_plain(backend, device_driver, method, dtype, t_end_key, compact):
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEEDS[dtype])
    rtol, atol = _tols(method, dtype)
    with _backend(backend, device_driver):
        plain = _plain(backend, method, dtype, t_end_key)
        got = _solve(func, y0, 0.0, event_fn, t_end=T_ENDS[t_end_key], rtol=rtol, atol=atol, method=method, compact=compact)
    _assert_same(plain, got)
    return plain, got


def test_three_argument_problem_is_the_two_argument_problem():
    for dtype in (F64, F32):
        y0, func, event_fn, k = decay_event_problem(B, L, dtype, SEED)
        y0r, func_r, event_r, kr, _ = decay_event_problem_rows(B, L, dtype, SEED)
        t = torch.linspace(0, 1, B, dtype=F64).to(dtype)
        assert torch.equal(y0, y0r) and torch.equal(k, kr)
        for rows in (None, torch.arange(B)):
            assert torch.equal(func_r(t, y0, rows), func(t, y0)) and torch.equal(event_r(t, y0, rows), event_fn(t, y0))
        rows = torch.tensor([1, 4, 9])
        assert torch.equal(func_r(t[rows], y0[rows], rows), func(t, y0)[rows])
        assert torch.equal(event_r(t[rows], y0[rows], rows), event_fn(t, y0)[rows])


# -- 1. / 3. compact against plain, on both backends ------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", COMPACT, ids=["half", "every", "quarter"])
@pytest.mark.parametrize("t_end", list(T_ENDS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_compact_equals_plain(backend, method, dtype, t_end, compact, device_driver):
    plain, got = _compact_against_plain(backend, device_driver, method, dtype, t_end, compact)
    fired = plain[2]["fired"]
    if t_end == "none":
        assert bool(fired.all())
    else:
        assert 0 < int(fired.sum()) < B                      # both kinds of row stop and leave
    if t_end == "number" and method == "dopri5" and dtype == F64:
        assert int(fired.sum()) == 6


# -- 4. not vacuous ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_leave_whenever_one_stops(backend, device_driver):
    """compact = 1.0 on the fp64 dopri5 problem: the rows take 2 .. 14 trial steps, 75 together where the batch pays
    12 x 14; a repack after every trial step that stopped a row."""
    plain, got = _compact_against_plain(backend, device_driver, "dopri5", F64, "none", 1.0)
    trials = (plain[2]["n_accepted"] + plain[2]["n_rejected"]).tolist()
    assert sorted(trials) == DOPRI5_TRIALS
    x = got[2]
    assert x["n_repacks"] >= 5
    # func: once at t0 and once for the initial step's probe with every row, then 6 stages per trial step a row takes
    # before it leaves (a row leaves at the poll after the step that stopped it)
    assert x["row_evals"] == 2 * B + 6 * sum(trials)
    assert x["row_evals"] < B * x["nfe"] and x["event_row_evals"] < B * x["n_event_evals"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_bisection_is_called_with_the_rows_that_have_a_quartic(backend, device_driver):
    """Two rows fired at t0 (no step, no quartic) and a t_end that stops some rows unfired: every bisection round calls
    event_fn with exactly the rows that fired after t0, in ascending original order."""
    y0, func, _, _, level = decay_event_problem_rows(B, L, F64, SEED)
    level = level.clone()
    level[[2, 7]] = y0[[2, 7], 0]
    seen = []

    def event_fn(t, y, rows):
        seen.append((rows.clone(), y.shape[0], t.shape[0]))
        return y[:, 0] - level[rows]
    with _backend(backend, device_driver):
        plain = _solve(lambda t, y: func(t, y), y0, 0.0, lambda t, y: y[:, 0] - level, t_end=0.15)
        got = _solve(func, y0, 0.0, event_fn, t_end=0.15, compact=True)
    _assert_same(plain, got)
    x = got[2]
    at_start = torch.zeros(B, dtype=torch.bool)
    at_start[[2, 7]] = True
    has_q = torch.nonzero(x["fired"] & ~at_start).view(-1)
    assert bool(x["fired"][at_start].all()) and 0 < has_q.numel() < int(x["fired"].sum()) < B
    trial_steps = int((x["n_accepted"] + x["n_rejected"]).max())
    rounds = x["n_event_evals"] - 1 - trial_steps
    assert rounds >= 10 and len(seen) == x["n_event_evals"]
    for rows, n_y, n_t in seen[-rounds:]:
        assert torch.equal(rows, has_q) and n_y == n_t == has_q.numel()
    assert seen[-rounds - 1][0].numel() != has_q.numel() or not torch.equal(seen[-rounds - 1][0], has_q)
    assert x["event_row_evals"] == sum(n for _, n, _ in seen)


# -- 2. the other variants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [True, 1.0], ids=["half", "every"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_decreasing_time_with_rows_fired_at_t0(backend, compact, device_driver):
    """The mirror image of the problem (y' = k (1 - t) y from 0 towards t_end = -3), rows 2 and 9 with g(t0) == 0: they
    are never active and leave at the first repack."""
    y0, _, _, k, _ = decay_event_problem_rows(B, L, F64, 5)
    q = torch.linspace(0.9, 0.2, B, dtype=F64)[torch.randperm(B, generator=torch.Generator().manual_seed(6))]
    q[[2, 9]] = 1.0
    level = (y0[:, 0] * q).clone()
    kw = dict(t_end=-3.0, rtol=1e-6, atol=1e-8)
    with _backend(backend, device_driver):
        plain = _solve(lambda t, y: k * y * (1 - t)[:, None], y0, 0.0, lambda t, y: y[:, 0] - level, **kw)
        got = _solve(lambda t, y, rows: k[rows] * y * (1 - t)[:, None], y0, 0.0, lambda t, y, rows: y[:, 0] - level[rows],
                     compact=compact, **kw)
    _assert_same(plain, got)
    event_t, sol, x = got
    assert bool(x["fired"].all()) and bool((event_t[[2, 9]] == 0.0).all()) and torch.equal(sol[1][[2, 9]], y0[[2, 9]])
    assert bool((event_t[[r for r in range(B) if r not in (2, 9)]] < 0.0).all())


@pytest.mark.parametrize("compact", [True, 1.0], ids=["half", "every"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_row_tolerances_and_first_steps(backend, dtype, compact, device_driver):
    """[B] tolerances (re-selected at a repack by `_Problem.keep_rows`, and read for ALL rows by the bisection) and a
    per-row first_step."""
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEED)
    lo, hi = (-4, -8) if dtype == F64 else (-2, -5)
    g = torch.Generator().manual_seed(11)
    rtol = torch.logspace(lo, hi, B, dtype=F64)[torch.randperm(B, generator=g)]
    atol = rtol * 1e-2
    fs = torch.linspace(1e-3, 5e-3, B, dtype=F64)
    with _backend(backend, device_driver):
        for opts in (None, {"first_step": fs}):
            plain = _solve(lambda t, y: func(t, y), y0, 0.0, lambda t, y: event_fn(t, y), t_end=0.3, rtol=rtol, atol=atol,
                           options=opts)
            got = _solve(func, y0, 0.0, event_fn, t_end=0.3, rtol=rtol, atol=atol, options=opts, compact=compact)
            _assert_same(plain, got)
            assert 0 < int(plain[2]["fired"].sum()) < B


# -- 5. the third argument ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", COMPACT, ids=["half", "every", "quarter"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_handed_to_func_and_event_fn(backend, compact, device_driver):
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, F64, SEED)
    f_rows, e_rows = [], []

    def check(rows, t, y):
        assert rows.dtype == torch.int64 and rows.device == y0.device and rows.dim() == 1
        assert rows.shape[0] == y.shape[0] == t.shape[0] and y.shape[1:] == y0.shape[1:]
        assert bool((rows[1:] > rows[:-1]).all()) and int(rows[0]) >= 0 and int(rows[-1]) < B
        return rows.clone()

    def f(t, y, rows):
        f_rows.append(check(rows, t, y))
        return func(t, y, rows)

    def ev(t, y, rows):
        e_rows.append(check(rows, t, y))
        return event_fn(t, y, rows)
    with _backend(backend, device_driver):
        event_t, sol, x = _solve(f, y0, 0.0, ev, t_end=0.15, compact=compact)
    assert len(f_rows) == x["nfe"] and len(e_rows) == x["n_event_evals"]
    assert x["row_evals"] == sum(r.numel() for r in f_rows) and x["event_row_evals"] == sum(r.numel() for r in e_rows)
    everyone = torch.arange(B)
    # t0, the initial step's probe and the first trial step's six stages come before the first repack can
    assert all(torch.equal(r, everyone) for r in f_rows[:2]) and torch.equal(e_rows[0], everyone)
    trial_steps = int((x["n_accepted"] + x["n_rejected"]).max())
    stepping = e_rows[:1 + trial_steps]
    for calls in (f_rows, stepping):
        for before, after in zip(calls, calls[1:]):
            assert set(after.tolist()) <= set(before.tolist())          # the set only shrinks
    assert f_rows[-1].numel() < B and stepping[-1].numel() < B
    assert len({r.numel() for r in f_rows}) == x["n_repacks"] + 1
    # a row is carried until the poll after the step that stopped it, never beyond the next repack at compact = 1.0
    if compact is not True and compact == 1.0:
        trials = (x["n_accepted"] + x["n_rejected"])
        for i in range(trial_steps):
            assert set(f_rows[2 + 6 * i].tolist()) == set(torch.nonzero(trials > i).view(-1).tolist())
    # the bisection: the rows that fired (none at t0 here), whether or not they are still carried
    has_q = torch.nonzero(x["fired"]).view(-1)
    assert len(e_rows) > 1 + trial_steps and all(torch.equal(r, has_q) for r in e_rows[1 + trial_steps:])


# -- 6. the error row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_max_num_steps_names_the_original_row_after_a_repack(backend, device_driver):
    """Rows 0 and 1 fire within a few steps and leave; the stiff row 2, then first of the carried rows, runs into
    max_num_steps: the message names row 2.  And the controller's error still wins over an event in the same trial step:
    y' = -1 in steps of 0.1 — row 0 passes 0.95 in its first step and leaves, rows 1 and 2 pass 0.75 in their third."""
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=F64)
    level = torch.tensor([0.9999, 0.9999, -10.0, -10.0], dtype=F64)
    sizes = []

    def f(t, y, rows):
        sizes.append(rows.tolist())
        return -k[rows] * (y - torch.sin(t)[:, None])
    ev = lambda t, y, rows: y[:, 0] - level[rows]          # noqa: E731
    with _backend(backend, device_driver):
        with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(50>=50\) in row 2"):
            _solve(f, torch.ones(4, 1, dtype=F64), 0.0, ev, t_end=5.0, rtol=1e-5, atol=1e-7, options={"max_num_steps": 50},
                   compact=1.0)
        # row 2 sat at position 0 when it failed (row 3, far from stiff, may have reached t_end and left as well)
        assert sizes[0] == [0, 1, 2, 3] and sizes[-1] in ([2], [2, 3])
        y0 = torch.ones(3, 1, dtype=F64)
        levels = torch.tensor([0.95, 0.75, 0.75], dtype=F64)
        carried = []

        def fall(t, y, rows):
            carried.append(rows.tolist())
            return -torch.ones_like(y)
        ev = lambda t, y, rows: y[:, 0] - levels[rows]     # noqa: E731
        kw = dict(rtol=1e-6, atol=1e-9, compact=1.0)
        event_t, _, ok = _solve(fall, y0, 0.0, ev, options={"first_step": 0.1, "ifactor": 1.0, "max_num_steps": 4}, **kw)
        assert ok["fired"].tolist() == [True] * 3 and ok["n_accepted"].tolist() == [1, 3, 3] and ok["n_repacks"] == 1
        assert float((event_t - torch.tensor([0.05, 0.25, 0.25], dtype=F64)).abs().max()) <= 1e-9
        del carried[:]
        with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(3>=3\) in row 1"):
            _solve(fall, y0, 0.0, ev, options={"first_step": 0.1, "ifactor": 1.0, "max_num_steps": 3}, **kw)
        assert carried[0] == [0, 1, 2] and carried[-1] == [1, 2]


# -- 7. validation -------------------------------------------------------------------------------------------------------------
def test_validation():
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, F64, SEED)
    with torch.no_grad():
        for bad in (0.0, -0.5, 1.5, 2, "yes", [0.5], torch.tensor(0.5)):
            with pytest.raises(ValueError, match="compact"):
                tda.odeint_rowwise_event(func, y0, 0.0, event_fn=event_fn, compact=bad)
        # off: func and event_fn keep two arguments, and the stats their five entries
        two = lambda f: (lambda t, y: f(t, y))      # noqa: E731
        for off in (None, False):
            out = tda.odeint_rowwise_event(two(func), y0, 0.0, event_fn=two(event_fn), compact=off, return_stats=True)
            assert sorted(out[2]) == ["fired", "n_accepted", "n_event_evals", "n_rejected", "nfe"]
        # on: three, the first call included
        with pytest.raises(TypeError):
            tda.odeint_rowwise_event(func, y0, 0.0, event_fn=two(event_fn), compact=True)
        with pytest.raises(TypeError):
            tda.odeint_rowwise_event(two(func), y0, 0.0, event_fn=event_fn, compact=True)
        assert len(tda.odeint_rowwise_event(func, y0, 0.0, event_fn=event_fn, compact=True)) == 2
        # every row fired at t0: no step, no func call, nothing to repack
        event_t, sol, x = tda.odeint_rowwise_event(func, y0, 0.25, event_fn=lambda t, y, rows: y[:, 0] - y0[rows, 0],
                                                   compact=True, return_stats=True)
        assert x["nfe"] == 0 and x["n_event_evals"] == 1 and x["n_repacks"] == 0 and x["row_evals"] == 0
        assert x["event_row_evals"] == B and bool((event_t == 0.25).all()) and torch.equal(sol[1], y0)
    with pytest.raises(OverflowError, match="in row"):
        with torch.no_grad():
            tda.odeint_rowwise_event(func, y0, 0.0, event_fn=event_fn, t_end=1.5, atol=0.0, rtol=1e-6, compact=True)


EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _caller(fn, names, base):
    return lambda **kw: fn(*[kw.get(n, base[n]) for n in names])


def test_row_event_fit_mapped_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 14)(*([p] * 14))
    names = ("q", "row_map", "q_rows", "fired_now", "y0", "y1", "f0", "f1", "k", "coef", "n_terms", "dts", "n_rows",
             "row_len", "dtype", "stream")
    base = dict(q=p, row_map=p, q_rows=3, fired_now=p, y0=p, y1=p, f0=p, f1=p, k=ptrs, coef=buf, n_terms=3, dts=p, n_rows=2,
                row_len=4, dtype=_native.TDEQ_F32, stream=None)
    fit = _caller(lib.tdeq_row_event_fit_mapped, names, base)
    for name in ("q", "row_map", "fired_now", "y0", "y1", "f0", "f1", "k", "coef", "dts"):
        assert fit(**{name: None}) == EINVAL, name
    for kw in (dict(n_terms=0), dict(n_terms=15), dict(n_terms=-1), dict(n_rows=-1), dict(row_len=0), dict(row_len=-4),
               dict(q_rows=0), dict(q_rows=-1), dict(q_rows=1), dict(dtype=_native.TDEQ_F16), dict(dtype=_native.TDEQ_C64),
               dict(dtype=9), dict(k=(ctypes.c_void_p * 14)(p, None, p))):
        assert fit(**kw) == EINVAL, kw
    assert fit(n_rows=0) == 0 and fit(n_rows=0, q_rows=0) == 0                   # no row: no launch
    assert fit(n_rows=0, q=None) == EINVAL and fit(n_rows=0, q_rows=-1) == EINVAL      # (the checks come first)


def test_row_event_eval_mapped_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    names = ("out", "dst_map", "out_rows", "q", "src_map", "q_rows", "x", "n_idx", "row_len", "dtype", "stream")
    base = dict(out=p, dst_map=p, out_rows=3, q=p, src_map=p, q_rows=3, x=p, n_idx=2, row_len=4, dtype=_native.TDEQ_F64,
                stream=None)
    ev = _caller(lib.tdeq_row_event_eval_mapped, names, base)
    for name in ("out", "q", "src_map", "x"):
        assert ev(**{name: None}) == EINVAL, name
    for kw in (dict(n_idx=-1), dict(row_len=0), dict(row_len=-1), dict(q_rows=0), dict(q_rows=-1), dict(out_rows=0),
               dict(out_rows=-1), dict(dst_map=None, out_rows=1), dict(dtype=_native.TDEQ_BF16), dict(dtype=_native.TDEQ_C128),
               dict(dtype=6)):
        assert ev(**kw) == EINVAL, kw
    assert ev(n_idx=0) == 0 and ev(n_idx=0, dst_map=None) == 0 and ev(n_idx=0, q_rows=0, out_rows=0) == 0
    assert ev(n_idx=0, src_map=None) == EINVAL and ev(n_idx=0, out_rows=-1) == EINVAL
