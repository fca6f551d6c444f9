"""`min_step`, `max_step`, `step_t`, `jump_t` per row in the rowwise family, without a GPU: the host path against `odeint`
row by row, row independence, the equivalences between the accepted forms, the breakpoints of the dense output, events and
compaction, the device driver on the CPU row oracle against the host path, and the validation."""
import numpy as np
import pytest
import torch

from _rowwise_steps_oracle import (METHODS, assert_device_matches_host, device_driver, device_problem,  # noqa: F401
                                   device_tolerances, quiet, switched_problem)

import torchdiffeq_amd as tda
from torchdiffeq_amd import rowwise
from torchdiffeq_amd.solvers._common import optimal_step_size

NAN = float("nan")
F64 = torch.float64


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# -- 1. one row against odeint -------------------------------------------------------------------------------------------------
SWITCH = [0.5, 1.3]
ONE_ROW_OPTIONS = {
    "step_t": {"step_t": [0.3, 1.1]},
    "jump_t": {"jump_t": SWITCH},
    "both": {"step_t": [0.3, 1.1], "jump_t": SWITCH},
    "max_step": {"max_step": 0.05},
    "min_step": {"min_step": 0.2},
}
# per method: a ceiling below the steps its controller takes at these tolerances, a floor above them
BOUNDS = {"max_step": {"dopri5": 0.05, "tsit5": 0.05, "dopri8": 0.05, "bosh3": 0.01, "fehlberg2": 0.002, "adaptive_heun": 0.002},
          "min_step": {"dopri5": 0.7, "tsit5": 0.7, "dopri8": 1.0, "bosh3": 0.2, "fehlberg2": 0.2, "adaptive_heun": 0.2}}
MIN_STEP_F32 = {"dopri5": 1.0, "tsit5": 1.0, "dopri8": 1.5}          # (fp32 runs at looser tolerances: a higher floor)


def _one_row_pair(dtype, switch):
    """The one-row problem as `odeint_rowwise` and as `odeint` take it, with a shared call counter: the field of
    tests/test_rowwise.py::test_single_row_matches_odeint plus a forcing that changes sign at the times of `switch`."""
    g = torch.Generator().manual_seed(1)
    A = (torch.randn(4, 4, generator=g, dtype=F64) * 0.5).to(dtype)
    y0 = torch.randn(1, 4, generator=g, dtype=F64).to(dtype)
    switch = switch.to(dtype)
    calls = [0]

    def forcing(t_):
        return 1 - 2 * (((t_ >= switch[0]).to(dtype) + (t_ >= switch[1]).to(dtype)) % 2)

    def f_rows(t_, y):
        calls[0] += 1
        return torch.sin(t_)[:, None] * (y @ A.T) - 0.3 * y + forcing(t_)[:, None]

    def f_ode(t_, y):
        calls[0] += 1
        return torch.sin(t_) * (y @ A.T) - 0.3 * y + forcing(t_)
    return y0, f_rows, f_ode, calls


def _assert_matches_odeint(y0, f_rows, f_ode, calls, t, method, dtype, rtol, atol, options):
    """Equal counts and nfe, and the solution within the bounds of tests/test_rowwise.py::test_single_row_matches_odeint."""
    sol, stats = tda.odeint_rowwise(f_rows, y0, t, rtol=rtol, atol=atol, method=method, options=options, return_stats=True)
    nfe_rows, calls[0] = calls[0], 0
    n_acc, n_rej = [0], [0]
    f_ode.callback_accept_step = lambda *a: n_acc.__setitem__(0, n_acc[0] + 1)
    f_ode.callback_reject_step = lambda *a: n_rej.__setitem__(0, n_rej[0] + 1)
    ref = tda.odeint(f_ode, y0, t, rtol=rtol, atol=atol, method=method, options=options)
    assert stats["nfe"] == nfe_rows == calls[0]
    assert stats["n_accepted"].tolist() == n_acc and stats["n_rejected"].tolist() == n_rej
    if method == "dopri8":
        bound = 0.1 * rtol if dtype == torch.float64 else 10 * rtol
    else:
        bound = 1e-13 if dtype == torch.float64 else 1e-5
    assert _rel(sol, ref) < bound
    return stats


@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", list(ONE_ROW_OPTIONS))
@pytest.mark.parametrize("method", METHODS)
def test_single_row_matches_odeint(method, which, dtype, direction, monkeypatch):
    """The forcing changes sign at the jump points of the case, so a solve that does not re-evaluate f0 behind a jump point
    takes other steps.  (The options go in as tensors: `odeint` maps only a tensor to decreasing time, as the reference.)

    The fp64 cases of the five methods below order 8 carry the case's options and nothing else.  fp32 and dopri8 add
    `first_step` and `ifactor = 2`: the stage sums are formed left to right here and by ATen's `torch.sum` on odeint's host
    path, and a step much shorter than the controller would take — the heuristic's first one, one cut at a point — has an
    error estimate at the rounding level of the state there, which those two orders turn into growth factors percents
    apart.  Capped at 2, such a step grows by the same factor in both.

    The `max_step` case must bind and the `min_step` case must force an acceptance: seen in the (dt, ratio) pairs the
    controller of the rowwise solve hands to `optimal_step_size`."""
    options = {name: torch.tensor(v, dtype=F64) for name, v in ONE_ROW_OPTIONS[which].items()}
    if which in BOUNDS:                                      # the bound at which this method's controller is overruled
        value = BOUNDS[which][method]
        if which == "min_step" and dtype == torch.float32:
            value = MIN_STEP_F32.get(method, value)
        options[which] = torch.tensor(value, dtype=F64)
    if dtype == torch.float32 or method == "dopri8":
        options["first_step"], options["ifactor"] = 0.23, 2.0
    y0, f_rows, f_ode, calls = _one_row_pair(dtype, options.get("jump_t", torch.tensor([10.0, 11.0], dtype=F64)))
    t = torch.linspace(0, 2, 5, dtype=dtype)
    if direction < 0:
        t = t.flip(0)
    rtol, atol = (1e-6, 1e-8) if dtype == torch.float64 else (1e-4, 1e-6)
    trials = []
    monkeypatch.setattr(rowwise, "optimal_step_size",
                        lambda dt, ratio, *a: trials.append((dt, ratio)) or optimal_step_size(dt, ratio, *a))
    _assert_matches_odeint(y0, f_rows, f_ode, calls, t, method, dtype, rtol, atol, options)
    bound = float(options[which]) if which in BOUNDS else None
    if which == "max_step":
        assert sum(1 for dt, _ in trials if dt == bound) > 10 and max(dt for dt, _ in trials) <= bound
    if which == "min_step":
        assert min(dt for dt, _ in trials) >= bound
        assert any(dt == bound and ratio > 1 for dt, ratio in trials)     # accepted although the error says no


def test_point_hit_exactly_matches_odeint():
    """The quirk of rk_common.py:292-296 itself: a point with `p == t0 + dt` is not cut (`t0 < p < t0 + dt` fails), the
    step is no `on_step_t` step, so the index stays on that point and no later point of the list is ever stepped onto.
    With `first_step = 0.125` the first step ends on step_t[0] = 0.125 exactly; `odeint` agrees on counts, nfe and solution,
    and the dense output shows 0.125 as a breakpoint but none at 0.6 or 1.1."""
    dtype = torch.float64
    options = {"step_t": torch.tensor([0.125, 0.6, 1.1], dtype=F64), "first_step": 0.125}
    y0, f_rows, f_ode, calls = _one_row_pair(dtype, torch.tensor([10.0, 11.0], dtype=F64))
    t = torch.linspace(0, 2, 5, dtype=dtype)
    stats = _assert_matches_odeint(y0, f_rows, f_ode, calls, t, "dopri5", dtype, 1e-6, 1e-8, options)
    dense = tda.odeint_rowwise_dense(f_rows, y0, 0.0, 2.0, rtol=1e-6, atol=1e-8, options=options)
    assert float(dense.seg_end[0]) == 0.125                  # the first step was accepted whole
    assert dense.n_segments == int(stats["n_accepted"])
    assert not bool(((dense.seg_end == 0.6) | (dense.seg_end == 1.1)).any())
    # the same list behind a first step that does not hit it: every point is a breakpoint
    cut = tda.odeint_rowwise_dense(f_rows, y0, 0.0, 2.0, rtol=1e-6, atol=1e-8, options=dict(options, first_step=0.1))
    assert all(bool((cut.seg_end == p).any()) for p in (0.125, 0.6, 1.1))


# -- 2. row independence --------------------------------------------------------------------------------------------------------
B7 = 7
# columns: no points | a point equal to t0 | a point beyond the row's end | a point the first step hits exactly (0.125 =
# t0 + first_step: not cut, and the index stays) | rows with one, two and three points
STEP7 = torch.tensor([[NAN, 0.0, 3.0, 0.125, 0.4, 0.2, 0.15],
                      [NAN, 0.45, NAN, 0.6, NAN, 0.9, 0.35],
                      [NAN, NAN, NAN, NAN, NAN, NAN, 0.85]], dtype=F64)
JUMP7 = torch.tensor([[NAN, 0.3, NAN, 0.5, 0.7, 0.55, 0.6],
                      [NAN, NAN, NAN, NAN, 0.25, 5.0, 0.0]], dtype=F64)
FIRST7 = torch.tensor([0.05, 0.02, 0.03, 0.125, 0.01, 0.04, 0.02], dtype=F64)


def _problem7(dtype, direction=1):
    y0, make, _ = switched_problem(B7, 3, dtype, 4)
    t = torch.linspace(0, 1, 4, dtype=F64) * direction
    return y0, make, t, STEP7 * direction, JUMP7 * direction


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_rows_are_independent(method, dtype):
    y0, make, t, step, jump = _problem7(dtype)
    lo, hi = torch.linspace(1e-5, 1e-3, B7, dtype=F64), torch.linspace(0.05, 0.6, B7, dtype=F64)
    kw = dict(rtol=1e-5, atol=1e-7, method=method, return_stats=True)
    full, st = tda.odeint_rowwise(make(jump), y0, t, options={"step_t": step, "jump_t": jump, "first_step": FIRST7,
                                                              "min_step": lo, "max_step": hi}, **kw)
    for r in range(B7):
        one, s1 = tda.odeint_rowwise(make(jump, rows_of=[r]), y0[r:r + 1], t,
                                     options={"step_t": step[:, r:r + 1], "jump_t": jump[:, r:r + 1],
                                              "first_step": FIRST7[r:r + 1], "min_step": float(lo[r]),
                                              "max_step": float(hi[r])}, **kw)
        assert torch.equal(one[:, 0], full[:, r]), r
        assert (int(s1["n_accepted"]), int(s1["n_rejected"])) == (int(st["n_accepted"][r]), int(st["n_rejected"][r])), r


# -- 3. equivalences ---------------------------------------------------------------------------------------------------------------
def _same(a, b, with_nfe=True):
    (sa, ta), (sb, tb) = a, b
    assert torch.equal(sa, sb)
    assert torch.equal(ta["n_accepted"], tb["n_accepted"]) and torch.equal(ta["n_rejected"], tb["n_rejected"])
    if with_nfe:
        assert ta["nfe"] == tb["nfe"]


@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
def test_equivalent_forms(direction):
    y0, make, t, _, _ = _problem7(F64, direction)
    shared = torch.tensor([0.3, 0.7], dtype=F64) * direction
    f = make(shared)
    kw = dict(rtol=1e-6, atol=1e-8, return_stats=True)
    for name in ("step_t", "jump_t"):
        _same(tda.odeint_rowwise(f, y0, t, options={name: shared}, **kw),
              tda.odeint_rowwise(f, y0, t, options={name: shared[:, None].expand(-1, B7)}, **kw))
        _same(tda.odeint_rowwise(f, y0, t, options={name: shared}, **kw),
              tda.odeint_rowwise(f, y0, t, options={name: shared.tolist()}, **kw))
    _same(tda.odeint_rowwise(f, y0, t, options={"min_step": 1e-3, "max_step": 0.04}, **kw),
          tda.odeint_rowwise(f, y0, t, options={"min_step": [1e-3] * B7, "max_step": np.full(B7, 0.04)}, **kw))
    _same(tda.odeint_rowwise(f, y0, t, options={"max_step": 0.04}, **kw),
          tda.odeint_rowwise(f, y0, t, options={"max_step": torch.full((B7,), 0.04, dtype=F64)}, **kw))
    _same(tda.odeint_rowwise(f, y0, t, **kw),
          tda.odeint_rowwise(f, y0, t, options={"min_step": 0, "max_step": float("inf"), "step_t": []}, **kw))


# -- 4. breakpoints of the dense output ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
def test_dense_breakpoints_and_contract(direction):
    y0, make, t, step, jump = _problem7(F64, direction)
    options = {"step_t": step, "jump_t": jump, "max_step": torch.linspace(0.05, 0.6, B7, dtype=F64)}
    kw = dict(rtol=1e-6, atol=1e-8, options=options)
    dense = tda.odeint_rowwise_dense(make(jump), y0, 0.0, 1.0 * direction, **kw)
    for r in range(B7):
        ends = dense.seg_end[dense.offsets[r]:dense.offsets[r + 1]]
        inside = [float(x) for x in torch.cat([step[:, r], jump[:, r]]) if x == x and 0 < float(x) * direction < 1]
        assert r == 0 or r == 2 or inside
        for pt in inside:
            assert bool((ends == pt).any()), (r, pt)
    q = torch.tensor([0.1, 0.3, 0.5, 0.77], dtype=F64) * direction
    grid = torch.cat([t[:1], q, t[-1:]])
    sol = tda.odeint_rowwise(make(jump), y0, grid, **kw)
    assert torch.equal(dense(q), sol[1:-1])


# -- 5. events and compaction ---------------------------------------------------------------------------------------------------------
def _event(level, by_rows=False):
    if by_rows:
        return lambda t, y, rows: y[:, 0] - level[rows]
    return lambda t, y: y[:, 0] - level


def test_event_rows_with_jumps_are_independent():
    y0, make, t, step, jump = _problem7(F64)
    level = y0[:, 0] * 0.5 + 0.4
    kw = dict(t_end=1.0, rtol=1e-6, atol=1e-8, return_stats=True)
    et, sol, st = tda.odeint_rowwise_event(make(jump), y0, 0.0, event_fn=_event(level), options={"jump_t": jump}, **kw)
    assert 0 < int(st["fired"].sum()) < B7
    for r in range(B7):
        e1, s1, t1 = tda.odeint_rowwise_event(make(jump, rows_of=[r]), y0[r:r + 1], 0.0, event_fn=_event(level[r:r + 1]),
                                              options={"jump_t": jump[:, r:r + 1]}, **kw)
        assert torch.equal(e1[0], et[r]) and torch.equal(s1[:, 0], sol[:, r]), r
        assert (int(t1["n_accepted"]), int(t1["n_rejected"])) == (int(st["n_accepted"][r]), int(st["n_rejected"][r])), r


@pytest.mark.parametrize("c", [0.5, 1.0])
def test_compaction_is_bit_exact(c):
    y0, make, t, step, jump = _problem7(F64)
    tg = t[:, None] * torch.linspace(0.3, 1.0, B7, dtype=F64)          # rows finish at different times
    options = {"step_t": step, "jump_t": jump, "min_step": torch.linspace(1e-5, 1e-3, B7, dtype=F64),
               "max_step": torch.linspace(0.05, 0.6, B7, dtype=F64)}
    kw = dict(rtol=1e-6, atol=1e-8, options=options, return_stats=True)
    plain, rows = make(jump), make(jump, by_rows=True)
    _same(tda.odeint_rowwise(plain, y0, tg, **kw), tda.odeint_rowwise(rows, y0, tg, compact=c, **kw), with_nfe=False)
    level = y0[:, 0] * 0.5 + 0.4
    ea, sa, ta = tda.odeint_rowwise_event(plain, y0, 0.0, event_fn=_event(level), t_end=tg[-1], **kw)
    eb, sb, tb = tda.odeint_rowwise_event(rows, y0, 0.0, event_fn=_event(level, True), t_end=tg[-1], compact=c, **kw)
    assert torch.equal(ea, eb)
    _same((sa, ta), (sb, tb), with_nfe=False)
    da, ta = tda.odeint_rowwise_dense(plain, y0, 0.0, tg[-1], **kw)
    db, tb = tda.odeint_rowwise_dense(rows, y0, 0.0, tg[-1], compact=c, **kw)
    assert tb["n_repacks"] > 0
    for name in ("offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(da, name), getattr(db, name)), name
    _same((da.coeffs, ta), (db.coeffs, tb), with_nfe=False)


# -- 6. the device driver on the row oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 129])
@pytest.mark.parametrize("method", METHODS)
def test_device_driver_matches_host_path(method, L, dtype, direction, device_driver):  # noqa: F811
    """`HipRowKernels` on the oracle has the kernels' arithmetic: the problem of the GPU comparison leaves no fp32 row
    whose counts differ, so the GPU test's allowance of one such row is headroom for the device's summation order only."""
    y0, f, t, options = device_problem(dtype, L, direction)
    kw = dict(method=method, options=options, return_stats=True, **device_tolerances(dtype))
    host, sh = tda.odeint_rowwise(f, y0, t, **kw)
    with device_driver():
        dev, sd = tda.odeint_rowwise(f, y0, t, **kw)
    assert assert_device_matches_host(dev, sd, host, sh, dtype, method) == 0


@pytest.mark.parametrize("entry", ["event", "dense"])
def test_device_driver_events_dense_and_compaction(entry, device_driver):  # noqa: F811
    """The hooks see the step before the refresh, and a repack re-selects every new vector and table column: both
    backends, with and without `compact`, give the host path's counts and (1e-12) values."""
    y0, make, t, step, jump = _problem7(F64)
    options = {"step_t": step, "jump_t": jump, "max_step": torch.linspace(0.05, 0.6, B7, dtype=F64)}
    kw = dict(rtol=1e-6, atol=1e-8, options=options, return_stats=True)
    t_end = torch.linspace(0.3, 1.0, B7, dtype=F64)
    level = y0[:, 0] * 0.5 + 0.4
    q = torch.tensor([0.1, 0.25], dtype=F64)

    def run(compact):
        f = make(jump, by_rows=compact is not None)
        if entry == "event":
            et, sol, st = tda.odeint_rowwise_event(f, y0, 0.0, event_fn=_event(level, compact is not None), t_end=t_end,
                                                   compact=compact, **kw)
            return torch.cat([et[None, :, None].expand(1, B7, 3), sol]), st
        dense, st = tda.odeint_rowwise_dense(f, y0, 0.0, t_end, compact=compact, **kw)
        return dense(q), st
    host, sh = run(None)
    with device_driver():
        dev, sd = run(None)
        devc, sdc = run(1.0)
    assert sd["n_accepted"].tolist() == sh["n_accepted"].tolist() and sd["n_rejected"].tolist() == sh["n_rejected"].tolist()
    assert sd["nfe"] == sh["nfe"]
    assert _rel(dev, host) < 1e-12
    assert torch.equal(devc, dev) and torch.equal(sdc["n_accepted"], sd["n_accepted"]) and sdc["n_repacks"] > 0


# -- 7. validation ---------------------------------------------------------------------------------------------------------------------
def test_validation():
    y0, make, t, step, jump = _problem7(F64)
    f = make(jump)
    for name in ("step_t", "jump_t"):
        for bad in (torch.zeros(2, B7 + 1), torch.zeros(2, 2, B7), torch.zeros(2, dtype=torch.complex64),
                    torch.zeros(2, dtype=torch.bool), np.zeros(2, dtype=bool), [True, False], "0.5", 0.5):
            with pytest.raises(ValueError, match=name):
                tda.odeint_rowwise(f, y0, t, options={name: bad})
    for name in ("min_step", "max_step"):
        for bad in (torch.zeros(B7 + 1), torch.zeros(2, B7), torch.zeros(B7, dtype=torch.complex64),
                    torch.zeros(B7, dtype=torch.bool), [0.1] * (B7 - 1), "1"):
            with pytest.raises(ValueError, match=name):
                tda.odeint_rowwise(f, y0, t, options={name: bad})
    dup = step.clone()
    dup[1, 4] = 0.7                                          # row 4: 0.7 is one of its jump points
    with pytest.raises(ValueError, match=r"must not have any repeated elements between them \(row 4\)"):
        tda.odeint_rowwise(f, y0, t, options={"step_t": dup, "jump_t": jump})
    twice = step.clone()
    twice[2, 5] = 0.2                                        # row 5: 0.2 twice in its step points
    with pytest.raises(ValueError, match=r"repeated elements between them \(row 5\)"):
        tda.odeint_rowwise(f, y0, t, options={"step_t": twice})
    for options in ({"min_step": 0.0}, {"max_step": 1.0}, {"step_t": [0.5]}, {"jump_t": [0.5]}):
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match="recorded solve"):
                tda.odeint_rowwise(f, y0, t, options=options, differentiable=True)
        with torch.no_grad():
            tda.odeint_rowwise(f, y0, t, options=options, differentiable=True)
