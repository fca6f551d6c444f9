"""`odeint_rowwise_event` without a GPU: the host path (`HostRowKernels`) and `HipRowKernels` on the CPU row oracle
(tests/_rowwise_event_oracle.py) — row independence, the two backends against each other, the package's own
`odeint_event` row by row, a closed form, the edge rules, validation and the argument checks of the three entry points."""
import contextlib
import ctypes
import math

import pytest
import torch

from _rowwise_event_oracle import METHODS, device_driver, quiet, random_problem, threshold_event  # noqa: F401

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
BACKENDS = ["host", "oracle"]
B, L = 12, 5


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _tols(dtype):
    return (1e-6, 1e-8) if dtype == F64 else (1e-4, 1e-6)


def _solve(func, y0, t0, event_fn, **kw):
    with torch.no_grad():
        return tda.odeint_rowwise_event(func, y0, t0, event_fn=event_fn, return_stats=True, **kw)


def _same(a, b):
    """(event_t, solution, stats) twice: the same bits, counts and flags."""
    (ta, sa, xa), (tb, sb, xb) = a, b
    assert torch.equal(ta, tb) and torch.equal(sa, sb)
    for name in ("n_accepted", "n_rejected", "fired"):
        assert torch.equal(xa[name], xb[name]), name
    assert xa["nfe"] == xb["nfe"] and xa["n_event_evals"] == xb["n_event_evals"]


def _assert_row(one, full, r):
    (t1, s1, x1), (t, s, x) = one, full
    assert torch.equal(t1[0], t[r]), (r, float(t1[0]), float(t[r]))
    assert torch.equal(s1[:, 0], s[:, r]), r
    for name in ("n_accepted", "n_rejected", "fired"):
        assert x1[name][0] == x[name][r], (name, r)


def _tols_of(method, dtype):
    """(the order-2 pairs take hundreds of steps per row at the tight pair: a looser one keeps the row-by-row solves quick)"""
    rtol, atol = _tols(dtype)
    return (rtol * 100, atol * 100) if method in ("adaptive_heun", "fehlberg2") else (rtol, atol)


def _mixed(dtype, L=L):
    """12 x 5 rows of different stiffness (`random_problem`) and the crossing y[:, 0] = 0.7 y0[:, 0]: the stiff rows fire
    within a few steps, the slow ones later or not before t_end = 1.5."""
    y0, plain, _, subset = random_problem(B, L, dtype, 3)
    c = (y0[:, 0] * 0.7).clone()
    return y0, plain, subset, c


# -- 1. a row alone is the row in the batch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", METHODS)
def test_row_alone_equals_row_in_batch(method, dtype):
    y0, plain, subset, c = _mixed(dtype)
    rtol, atol = _tols_of(method, dtype)
    full = _solve(plain, y0, 0.0, threshold_event(c), t_end=1.5, rtol=rtol, atol=atol, method=method)
    event_t, sol, stats = full
    trials = (stats["n_accepted"] + stats["n_rejected"])[stats["fired"]]
    print(f"{method} {dtype}: event_t {event_t.tolist()}, fired {stats['fired'].tolist()}, trials of the fired rows {trials.tolist()}")
    assert int(stats["fired"].sum()) >= 6 and len(set(trials.tolist())) >= (2 if method == "dopri8" else 3)
    assert event_t.dtype == F64 and sol.shape == (2, B, L) and torch.equal(sol[0], y0)
    # the rows that fired sit on their threshold (to the accuracy of the solve), the others at t_end
    hit = (sol[1, :, 0] - c).abs()[stats["fired"]]
    assert float(hit.max()) <= 100 * rtol * float(y0.abs().max())
    assert bool((event_t[~stats["fired"]] == 1.5).all())
    for r in range(B):
        one = _solve(subset(slice(r, r + 1)), y0[r:r + 1], 0.0, threshold_event(c[r:r + 1]), t_end=1.5, rtol=rtol, atol=atol,
                     method=method)
        _assert_row(one, full, r)


# -- 2. the two backends ------------------------------------------------------------------------------------------------------
# The order-2 pairs in fp64 get their first step size as an option.  The initial-step heuristic ends in h ** (1 / order),
# a square root for order 2: the host path asks ATen's CPU sqrt for it (as the reference does; `_scalars._aten_sqrt`: not
# correctly rounded, ~1 % of fp64 arguments differ in the last bit), the kernels and their oracle take the IEEE sqrt.  Row
# 11 of this problem is such an argument (0x1.779d58ce9765fp-11 against 0x1.779d58ce97660p-11), so already the PLAIN
# odeint_rowwise solve differs there, whatever L is; with `first_step` given no square root is taken and every bit agrees.
BITWISE = [(m, d) for d in (F64, F32) for m in METHODS]
GIVEN_FIRST_STEP = {("fehlberg2", F64), ("adaptive_heun", F64)}


@pytest.mark.parametrize("method,dtype", BITWISE, ids=[f"{m}-{'f64' if d == F64 else 'f32'}" for m, d in BITWISE])
def test_host_path_equals_oracle_driver(method, dtype, device_driver):
    """Bit for bit, on rows of TWO elements.  The two backends add a row's squares in different orders (the host path
    pairwise, the oracle correctly rounded: tests/test_rowwise_oracle.py compares them to a bound for that reason); with
    L = 2 a row's sum is one addition, the same on both, so every decision and every bit after it has to agree — the
    event detection, the kept quartics and the bisection included.  The premise is checked first: the plain solve of the
    same problem is equal on the two backends."""
    y0, plain, _, c = _mixed(dtype, L=2)
    rtol, atol = _tols_of(method, dtype)
    kw = dict(rtol=rtol, atol=atol, method=method)
    if (method, dtype) in GIVEN_FIRST_STEP:
        kw["options"] = {"first_step": torch.logspace(-4, -3, B, dtype=F64)}
    grid = torch.tensor([0.0, 1.5], dtype=F64)
    with torch.no_grad():
        plain_host = tda.odeint_rowwise(plain, y0, grid, **kw)
        with device_driver():
            plain_oracle = tda.odeint_rowwise(plain, y0, grid, **kw)
    assert torch.equal(plain_host, plain_oracle)
    kw["t_end"] = 1.5
    host = _solve(plain, y0, 0.0, threshold_event(c), **kw)
    with device_driver():
        oracle = _solve(plain, y0, 0.0, threshold_event(c), **kw)
    print(f"{method} {dtype}: fired {host[2]['fired'].tolist()}, trials {(host[2]['n_accepted'] + host[2]['n_rejected']).tolist()}")
    _same(host, oracle)
    assert int(host[2]["fired"].sum()) >= 6


@pytest.mark.parametrize("method,L", [("dopri5", 5), ("fehlberg2", 2), ("adaptive_heun", 2)])
def test_host_path_against_oracle_driver_bounded(method, L, device_driver):
    """fp64 where the two backends differ in their last bits (12 x 5: the row sums; the order-2 pairs: see above): the
    bounds of tests/test_rowwise_oracle.py — equal counts, the states within S = 1e-12 max|y| — and for a row that fired
    the event time within atol + S / |dg/dt| (each bisection ends within atol / 2 of its own interpolant's root, the
    interpolants are S apart), the state there within S plus the trajectory's speed times that."""
    y0, plain, _, c = _mixed(F64, L=L)
    rtol, atol = _tols_of(method, F64)
    kw = dict(t_end=1.5, rtol=rtol, atol=atol, method=method)
    host = _solve(plain, y0, 0.0, threshold_event(c), **kw)
    with device_driver():
        oracle = _solve(plain, y0, 0.0, threshold_event(c), **kw)
    for name in ("n_accepted", "n_rejected", "fired"):
        assert torch.equal(host[2][name], oracle[2][name])
    fired = host[2]["fired"]
    assert int(fired.sum()) >= 6
    speed = plain(host[0], host[1][1]).abs()
    S = 1e-12 * float(host[1].abs().max())
    bound = torch.where(fired, atol + S / speed[:, 0], torch.zeros(B, dtype=F64))      # an unfired row: t_end exactly
    diff = (host[0] - oracle[0]).abs()
    print(f"{method} L={L}: |event_t difference| {diff.tolist()}, bound {bound.tolist()}")
    assert bool((diff <= bound).all())
    assert bool(((host[1][1] - oracle[1][1]).abs().max(dim=1).values <= S + speed.max(dim=1).values * bound).all())


# -- 3. against odeint_event, one row at a time ------------------------------------------------------------------------------
def _linear_rows():
    g = torch.Generator().manual_seed(1)
    A = torch.randn(4, 4, generator=g, dtype=F64) * 0.5
    y0 = torch.randn(3, 4, generator=g, dtype=F64)
    c = torch.tensor([0.6, 3.0, 0.0], dtype=F64)          # crossings of y[:, 0] near t = 2.0, 0.55 and 0.85
    return A, y0, c


@pytest.mark.parametrize("method", METHODS)
def test_rows_match_odeint_event(method):
    """Row r against `odeint_event` on that row alone (fp64, reference-exact on the CPU): the same accepted and rejected
    steps, and |event_t - ref| <= 2 atol + S / |dg/dt| — each bisection ends within atol of the root of its interpolant,
    and the interpolants differ by the solution bound S of tests/test_rowwise.py::test_single_row_matches_odeint."""
    A, y0, c = _linear_rows()
    rtol, atol = 1e-6, 1e-8
    event_t, sol, stats = _solve(lambda t, y: torch.sin(t)[:, None] * (y @ A.T) - 0.3 * y, y0, 0.0, threshold_event(c),
                                 rtol=rtol, atol=atol, method=method)
    assert bool(stats["fired"].all())
    rel = 0.1 * rtol if method == "dopri8" else 1e-13
    for r in range(3):
        n_acc, n_rej = [0], [0]

        def f(t, y):
            return torch.sin(t) * (y @ A.T) - 0.3 * y
        f.callback_accept_step = lambda *a: n_acc.__setitem__(0, n_acc[0] + 1)
        f.callback_reject_step = lambda *a: n_rej.__setitem__(0, n_rej[0] + 1)
        with torch.no_grad():
            ref_t, ref = tda.odeint_event(f, y0[r], torch.tensor(0.0, dtype=F64), event_fn=lambda t, y: y[0] - c[r],
                                          rtol=rtol, atol=atol, method=method)
            slope = abs(float(f(ref_t, ref[-1])[0]))
        assert slope >= 0.1
        if method != "dopri8":
            assert [int(stats["n_accepted"][r]), int(stats["n_rejected"][r])] == [n_acc[0], n_rej[0]]
        S = rel * float(ref.abs().max())
        diff = abs(float(event_t[r] - ref_t))
        print(f"{method} row {r}: event_t {float(event_t[r])!r}, |diff| {diff:.3e}, bound {2 * atol + S / slope:.3e}")
        assert diff <= 2 * atol + S / slope
        # the state at the event: the solution bound plus the trajectory's speed times the bound on the event time
        assert float((sol[1, r] - ref[-1]).abs().max()) <= S + float(f(ref_t, ref[-1]).abs().max()) * (2 * atol + S / slope)


# -- 4. closed form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_falling_balls_closed_form(dtype, backend, device_driver):
    """h'' = -g from rest at height h_r: the ground is reached at sqrt(2 h_r / g).  dopri5 integrates a quadratic exactly
    and its mid-point is exact for it, so the quartic is the trajectory and the bisection's atol is the whole error."""
    grav = 9.81
    h = torch.tensor([0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 0.01], dtype=F64)
    y0 = torch.stack([h, torch.zeros_like(h)], dim=1).to(dtype)
    rtol, atol = _tols(dtype)
    b = 1e-13 if dtype == F64 else 1e-5

    def f(t, y):
        return torch.stack([y[:, 1], torch.full_like(y[:, 1], -grav)], dim=1)
    with _backend(backend, device_driver):
        event_t, sol, stats = _solve(f, y0, 0.0, lambda t, y: y[:, 0], rtol=rtol, atol=atol, method="dopri5")
    exact = torch.sqrt(2 * y0[:, 0].double() / grav)
    err = (event_t - exact).abs()
    print(f"{dtype} {backend}: event_t {event_t.tolist()}, |err| {err.tolist()}")
    assert bool(stats["fired"].all())
    assert bool((err <= atol + b * exact).all())
    assert float((sol[1, :, 1].double() + grav * event_t).abs().max()) <= (1e-12 if dtype == F64 else 1e-4)


# -- 5. the edge rules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_t_end_number_and_vector(backend, device_driver):
    y0, plain, subset, c = _mixed(F64)
    ends = torch.linspace(0.05, 1.5, B, dtype=F64)
    with _backend(backend, device_driver):
        number = _solve(plain, y0, 0.0, threshold_event(c), t_end=0.2, rtol=1e-6, atol=1e-8)
        tensor0 = _solve(plain, y0, torch.tensor(0.0), threshold_event(c), t_end=torch.full((B,), 0.2, dtype=F64), rtol=1e-6,
                         atol=1e-8)
        vector = _solve(plain, y0, torch.zeros(B, dtype=F64), threshold_event(c), t_end=ends, rtol=1e-6, atol=1e-8)
        _same(number, tensor0)
        event_t, sol, stats = number
        assert 0 < int(stats["fired"].sum()) < B                                     # both kinds of row
        assert bool((event_t[~stats["fired"]] == 0.2).all()) and bool((event_t[stats["fired"]] < 0.2).all())
        # an unfired row is the row of the plain solve to its t_end
        plain_sol, plain_stats = tda.odeint_rowwise(plain, y0, torch.tensor([0.0, 0.2], dtype=F64), rtol=1e-6, atol=1e-8,
                                                    return_stats=True)
        un = ~stats["fired"]
        assert torch.equal(sol[1][un], plain_sol[1][un])
        assert torch.equal(stats["n_accepted"][un], plain_stats["n_accepted"][un])
        event_t, sol, stats = vector
        assert 0 < int(stats["fired"].sum()) < B
        assert torch.equal(event_t[~stats["fired"]], ends[~stats["fired"]])
        for r in (0, 5, 11):
            one = _solve(subset(slice(r, r + 1)), y0[r:r + 1], 0.0, threshold_event(c[r:r + 1]), t_end=float(ends[r]),
                         rtol=1e-6, atol=1e-8)
            _assert_row(one, vector, r)


@pytest.mark.parametrize("backend", BACKENDS)
def test_event_beyond_t_end_does_not_count(backend, device_driver):
    """y' = -1 from 1 with first_step 0.6: the step [0, 0.6] is exact and accepted, crosses t_end AND the threshold.  The
    threshold 0.45 is reached at 0.55: beyond t_end = 0.5 the row is a row that reached t_end; with t_end = 0.58 it fired."""
    y0 = torch.ones(2, 1, dtype=F64)
    f = lambda t, y: -torch.ones_like(y)      # noqa: E731
    kw = dict(rtol=1e-6, atol=1e-9, options={"first_step": 0.6})
    with _backend(backend, device_driver):
        event_t, sol, stats = _solve(f, y0, 0.0, threshold_event(torch.tensor([0.45, 0.45], dtype=F64)),
                                     t_end=torch.tensor([0.5, 0.58], dtype=F64), **kw)
    assert stats["n_accepted"].tolist() == [1, 1] and stats["n_rejected"].tolist() == [0, 0]
    assert stats["fired"].tolist() == [False, True]
    assert float(event_t[0]) == 0.5 and abs(float(sol[1, 0, 0]) - 0.5) <= 1e-13
    assert abs(float(event_t[1]) - 0.55) <= 1e-9 and abs(float(sol[1, 1, 0]) - 0.45) <= 2e-9


@pytest.mark.parametrize("backend", BACKENDS)
def test_decreasing_time(backend, device_driver):
    """Backwards from t0 = 1: event_fn sees true time, and the solve is the forward solve of the mirrored problem."""
    y0, plain, _, c = _mixed(F64)
    seen = []

    def ev(t, y):
        seen.append(t.clone())
        return y[:, 0] - c
    mirrored = lambda t, y: -plain(1.0 - t, y)      # noqa: E731
    with _backend(backend, device_driver):
        back = _solve(mirrored, y0, 1.0, ev, t_end=-0.5, rtol=1e-6, atol=1e-8)
        fwd = _solve(plain, y0, 0.0, threshold_event(c), t_end=1.5, rtol=1e-6, atol=1e-8)
    assert all(bool((t <= 1.0).all()) for t in seen) and float(seen[-1].min()) < 1.0
    assert torch.equal(back[2]["fired"], fwd[2]["fired"]) and int(fwd[2]["fired"].sum()) >= 6
    assert float((back[0] - (1.0 - fwd[0])).abs().max()) <= 1e-6
    assert float((back[1] - fwd[1]).abs().max()) <= 1e-5


@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_fired_at_t0(backend, device_driver):
    y0, plain, subset, c = _mixed(F64)
    c0 = c.clone()
    c0[[2, 7]] = y0[[2, 7], 0]                                # g(t0) == 0 for rows 2 and 7
    calls = [0]

    def counted(t, y):
        calls[0] += 1
        return plain(t, y)
    with _backend(backend, device_driver):
        some = _solve(plain, y0, 0.25, threshold_event(c0), t_end=1.5, rtol=1e-6, atol=1e-8)
        ref = _solve(plain, y0, 0.25, threshold_event(c), t_end=1.5, rtol=1e-6, atol=1e-8)
        every = _solve(counted, y0, 0.25, threshold_event(y0[:, 0].clone()), t_end=1.5, rtol=1e-6, atol=1e-8)
    event_t, sol, stats = some
    for r in (2, 7):
        assert float(event_t[r]) == 0.25 and bool(stats["fired"][r]) and torch.equal(sol[1, r], y0[r])
        assert int(stats["n_accepted"][r]) == 0 and int(stats["n_rejected"][r]) == 0
    others = [r for r in range(B) if r not in (2, 7)]
    assert torch.equal(event_t[others], ref[0][others]) and torch.equal(sol[1][others], ref[1][1][others])
    event_t, sol, stats = every
    assert calls[0] == 0 and stats["nfe"] == 0 and stats["n_event_evals"] == 1
    assert bool((event_t == 0.25).all()) and bool(stats["fired"].all()) and torch.equal(sol[1], y0)
    assert int(stats["n_accepted"].sum()) == 0 and int(stats["n_rejected"].sum()) == 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_row_tolerances_and_first_steps(dtype, backend, device_driver):
    """[B] tolerances and a per-row first_step: row r is the one-row solve with rtol[r], atol[r], first_step[r]."""
    y0, plain, subset, c = _mixed(dtype)
    lo, hi = (-4, -8) if dtype == F64 else (-2, -5)
    g = torch.Generator().manual_seed(11)
    rtol = torch.logspace(lo, hi, B, dtype=F64)[torch.randperm(B, generator=g)]
    atol = rtol * 1e-2
    fs = torch.linspace(1e-3, 5e-3, B, dtype=F64)
    with _backend(backend, device_driver):
        for opts in (None, {"first_step": fs}):
            full = _solve(plain, y0, 0.0, threshold_event(c), t_end=1.5, rtol=rtol, atol=atol, options=opts)
            assert int(full[2]["fired"].sum()) >= 6
            for r in range(B):
                o_r = None if opts is None else {"first_step": fs[r:r + 1]}
                one = _solve(subset(slice(r, r + 1)), y0[r:r + 1], 0.0, threshold_event(c[r:r + 1]), t_end=1.5,
                             rtol=float(rtol[r]), atol=float(atol[r]), options=o_r)
                _assert_row(one, full, r)


@pytest.mark.parametrize("backend", BACKENDS)
def test_max_num_steps_names_the_original_row(backend, device_driver):
    """Every trial step counts (there is no output time to start again from), and the controller's error wins over an
    event in the same trial step: y' = -1 in steps of 0.1 passes 0.75 in its 3rd step — fine with max_num_steps = 4, an
    error with 3 (the reference would return the event)."""
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=F64)
    f = lambda t, y: -k * (y - torch.sin(t)[:, None])      # noqa: E731
    never = lambda t, y: y[:, 0] + 10.0                    # noqa: E731
    with _backend(backend, device_driver):
        with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(50>=50\) in row 2"):
            _solve(f, torch.ones(4, 1, dtype=F64), 0.0, never, t_end=5.0, rtol=1e-5, atol=1e-7, options={"max_num_steps": 50})
        y0 = torch.ones(1, 1, dtype=F64)
        fall = lambda t, y: -torch.ones_like(y)            # noqa: E731
        ev = threshold_event(torch.tensor([0.75], dtype=F64))
        kw = dict(rtol=1e-6, atol=1e-9)
        event_t, _, ok = _solve(fall, y0, 0.0, ev, options={"first_step": 0.1, "ifactor": 1.0, "max_num_steps": 4}, **kw)
        assert ok["fired"].tolist() == [True] and ok["n_accepted"].tolist() == [3] and abs(float(event_t[0]) - 0.25) <= 1e-9
        with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(3>=3\) in row 0"):
            _solve(fall, y0, 0.0, ev, options={"first_step": 0.1, "ifactor": 1.0, "max_num_steps": 3}, **kw)


@pytest.mark.parametrize("backend", BACKENDS)
def test_nan_from_event_fn(backend, device_driver):
    """sign(NaN) = 0: at t0 the row counts as fired there; after an accepted step 0 != s0 fires the row in that step."""
    y0, plain, _, c = _mixed(F64)

    def nan_at_start(t, y):
        g = y[:, 0] - c
        g[3] = float("nan")
        return g

    def nan_later(t, y):
        g = y[:, 0] - c
        return torch.where((torch.arange(B) == 8) & (t > 0.3), torch.full_like(g, float("nan")), g)
    with _backend(backend, device_driver):
        ref = _solve(plain, y0, 0.0, threshold_event(c), t_end=1.5, rtol=1e-6, atol=1e-8)
        start = _solve(plain, y0, 0.0, nan_at_start, t_end=1.5, rtol=1e-6, atol=1e-8)
        later = _solve(plain, y0, 0.0, nan_later, t_end=1.5, rtol=1e-6, atol=1e-8)
    assert float(start[0][3]) == 0.0 and bool(start[2]["fired"][3]) and torch.equal(start[1][1, 3], y0[3])
    assert not bool(ref[2]["fired"][8])                       # row 8 does not reach its threshold before t_end ...
    assert bool(later[2]["fired"][8]) and 0.29 < float(later[0][8]) < 1.5      # ... the NaN stops it
    assert bool(torch.isfinite(later[1]).all())
    others = [r for r in range(B) if r != 8]
    assert torch.equal(later[0][others], ref[0][others]) and torch.equal(later[1][:, others], ref[1][:, others])


def test_event_fn_is_called_under_no_grad_with_true_time():
    y0, plain, _, c = _mixed(F32)
    seen = []

    def ev(t, y):
        seen.append((torch.is_grad_enabled(), t.dtype, t.shape, y.shape))
        return y[:, 0].double() - c.double()                  # (a real tensor of another dtype is cast)
    event_t, sol, stats = tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=ev, t_end=1.5, rtol=1e-4, atol=1e-6,
                                                   return_stats=True)
    assert stats["n_event_evals"] == len(seen) and all(s == (False, F32, (B,), (B, L)) for s in seen)
    trials = int((stats["n_accepted"] + stats["n_rejected"]).max())
    assert len(seen) >= 1 + trials
    out = tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=ev, t_end=1.5, rtol=1e-4, atol=1e-6)
    assert len(out) == 2 and torch.equal(out[0], event_t) and torch.equal(out[1], sol)


# -- 6. validation -------------------------------------------------------------------------------------------------------------
def test_validation():
    y0, plain, _, c = _mixed(F64)
    ev = threshold_event(c)
    run = lambda **kw: tda.odeint_rowwise_event(plain, kw.pop("y0", y0), kw.pop("t0", 0.0), event_fn=kw.pop("event_fn", ev), **kw)  # noqa: E731
    with torch.no_grad():
        for bad in (dict(t_end=0.0), dict(t_end=torch.cat([torch.ones(B - 1), -torch.ones(1)])), dict(t_end=torch.ones(B + 1)),
                    dict(t0=torch.zeros(3)), dict(t0=torch.zeros(B, 1)), dict(t0="0"), dict(t_end=[1.0] * B),
                    dict(t0=float("nan")), dict(t_end=float("nan")), dict(event_fn=None), dict(method="rk4"),
                    dict(options={"step_size": 0.1}), dict(rtol=torch.ones(B + 1)), dict(y0=(y0, y0)), dict(y0=y0.to(torch.float16)),
                    dict(t0=torch.zeros(B, dtype=torch.complex64))):
            with pytest.raises(ValueError):
                run(**bad)
        for bad, exc in ((lambda t, y: 1.0, TypeError), (lambda t, y: y[:, :1], RuntimeError), (lambda t, y: y[0, 0], RuntimeError),
                         (lambda t, y: (y[:, 0] - c).to("meta"), RuntimeError),
                         (lambda t, y: torch.complex(y[:, 0], y[:, 0]), RuntimeError)):
            with pytest.raises(exc):
                run(event_fn=bad)
        with pytest.raises(TypeError):
            tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=ev, compact=True)
        with pytest.raises(TypeError):
            tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=ev, differentiable=True)
        with pytest.raises(OverflowError):
            run(t_end=1.5, atol=0.0, rtol=1e-6)
    with pytest.raises(NotImplementedError):
        run(y0=y0.clone().requires_grad_(True), t_end=1.5)
    with pytest.raises(NotImplementedError):
        run(t0=torch.zeros(B, dtype=F64, requires_grad=True), t_end=1.5)
    lin = torch.nn.Linear(L, L).double()
    with pytest.raises(NotImplementedError):
        tda.odeint_rowwise_event(lambda t, y: lin(y), y0, 0.0, event_fn=ev, t_end=1.5)
    # odeint_rowwise itself still refuses an event function
    with pytest.raises(ValueError, match="event_fn is not supported"):
        tda.odeint_rowwise(plain, y0, torch.tensor([0.0, 1.0]), event_fn=ev)


# -- 7. argument validation of the entry points (no launch is reached) ---------------------------------------------------------
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def _caller(fn, names, base):
    return lambda **kw: fn(*[kw.get(n, base[n]) for n in names])


def _state(p, n_rows=2):
    st = _native.RowState()
    for name in ("t0", "tprev", "dt", "h0", "tgrid", "active", "accepted", "out_lo", "out_hi", "next_out", "since", "bad_y",
                 "code", "n_acc", "n_rej", "ratio", "status"):
        setattr(st, name, p)
    st.n_rows, st.row_len, st.max_num_steps, st.n_out, st.order = n_rows, 4, 10, 2, 4
    return st


def test_row_event_detect_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ctrl = _native.step_ctrl([0.5, 1.0], [False, True], 5, 0.9, 10.0, 0.2, 0.0, math.inf, 1.0, n_norm_seg=1)
    names = ("g1", "sign0", "ctrl", "st", "dts", "times", "fired", "fired_now", "lo", "hi", "dtype", "stream")
    base = dict(g1=p, sign0=p, ctrl=ctypes.byref(ctrl), st=ctypes.byref(_state(p)), dts=p, times=p, fired=p, fired_now=p, lo=p,
                hi=p, dtype=_native.TDEQ_F64, stream=None)
    call = _caller(lib.tdeq_row_event_detect, names, base)
    for name in names[:10]:
        assert call(**{name: None}) == EINVAL, name
    for dtype in (_native.TDEQ_BF16, _native.TDEQ_C64, 7, -1):
        assert call(dtype=dtype) == EINVAL
    assert call(st=ctypes.byref(_state(p, n_rows=-1))) == EINVAL
    for name in ("accepted", "tprev", "t0", "active", "status"):
        st = _state(p)
        setattr(st, name, None)
        assert call(st=ctypes.byref(st)) == EINVAL, name
    for n_times in (0, _native.TDEQ_MAX_STAGE_TIMES + 1):
        bad = _native.step_ctrl([0.5], [False], 5, 0.9, 10.0, 0.2, 0.0, math.inf, 1.0, n_norm_seg=1)
        bad.n_times = n_times
        assert call(ctrl=ctypes.byref(bad)) == EINVAL
    assert call(st=ctypes.byref(_state(p, n_rows=0))) == 0                        # no row: no launch
    assert call(st=ctypes.byref(_state(p, n_rows=0)), g1=None) == EINVAL          # (the null check comes first)


def test_row_event_fit_and_eval_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 14)(*([p] * 14))
    names = ("q", "fired_now", "y0", "y1", "f0", "f1", "k", "coef", "n_terms", "dts", "n_rows", "row_len", "dtype", "stream")
    base = dict(q=p, fired_now=p, y0=p, y1=p, f0=p, f1=p, k=ptrs, coef=buf, n_terms=3, dts=p, n_rows=2, row_len=4,
                dtype=_native.TDEQ_F32, stream=None)
    fit = _caller(lib.tdeq_row_event_fit, names, base)
    for name in ("q", "fired_now", "y0", "y1", "f0", "f1", "k", "coef", "dts"):
        assert fit(**{name: None}) == EINVAL, name
    for kw in (dict(n_terms=0), dict(n_terms=15), dict(n_terms=-1), dict(n_rows=-1), dict(row_len=0), dict(row_len=-4),
               dict(dtype=_native.TDEQ_F16), dict(dtype=9), dict(k=(ctypes.c_void_p * 14)(p, None, p))):
        assert fit(**kw) == EINVAL, kw
    assert fit(n_rows=0) == 0 and fit(n_rows=0, q=None) == EINVAL
    names = ("out", "q", "x", "mask", "n_rows", "row_len", "dtype", "stream")
    base = dict(out=p, q=p, x=p, mask=p, n_rows=2, row_len=4, dtype=_native.TDEQ_F64, stream=None)
    ev = _caller(lib.tdeq_row_event_eval, names, base)
    for name in ("out", "q", "x", "mask"):
        assert ev(**{name: None}) == EINVAL, name
    for kw in (dict(n_rows=-1), dict(row_len=0), dict(dtype=_native.TDEQ_BF16), dict(dtype=_native.TDEQ_C128), dict(dtype=6)):
        assert ev(**kw) == EINVAL, kw
    assert ev(n_rows=0) == 0 and ev(n_rows=0, mask=None) == EINVAL
