"""`odeint_rowwise_event`: a batch of independent IVPs, each row stopped by its own terminal event.

`odeint_event` treats a batched state as one system with one scalar event; here row r of `y0[B, *row_shape]` is
integrated by the per-row controller of `odeint_rowwise` until `event_fn(t, y)[r]` changes sign (or the row reaches
`t_end[r]`), and the event time of every row is then located by ONE bisection over the quartics of the rows' last steps.

What an event solve adds to a rowwise trial step is the step hook `RowEvents` (rowwise.py: the driver and both backends
take one), which runs between the controller and the dense-output commit: one call of `event_fn`, the
detection (`tdeq_row_event_detect`: a row that fires leaves the active rows like a finished one) and the quartic of the
rows that fired in this step (`tdeq_row_event_fit`), kept in a [5, B, L] buffer because the commit overwrites y0 and f0.
The bisection evaluates the kept quartics (`tdeq_row_event_eval`); its [B] bracket arithmetic is a handful of fp64 torch
ops, the same expressions on both backends.

With `compact=` a row that has stopped — fired, reached `t_end`, or fired at `t0` — leaves the batch at the next repack
(the driver's rule).  The quartics stay in the [5, B, L] buffer at their ORIGINAL row (`tdeq_row_event_fit_mapped`),
`RowEvents.keep_rows` parks the event state of the rows that leave, and the bisection runs on the rows that have a quartic
only (`tdeq_row_event_eval_mapped`).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import rowwise
from ._native import device_guard
from .rowwise import _Problem

__all__ = ["odeint_rowwise_event"]


_NAME = "odeint_rowwise_event"


def _sign(g: torch.Tensor) -> torch.Tensor:
    """(g > 0) - (g < 0) as int32: 0 for a zero and for a NaN (the expression of tdeq_row_event_detect)."""
    return (g > 0).to(torch.int32) - (g < 0).to(torch.int32)


def _event_grid(t0, t_end, B: int) -> torch.Tensor:
    """The [2, B] fp64 grid [t0, t_end] of the solve (+inf for `t_end=None`)."""
    for v in (t0, t_end):
        if isinstance(v, torch.Tensor) and v.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("odeint_rowwise_event does not propagate gradients (t0 / t_end requires grad); "
                                      "detach them or call it under torch.no_grad()")
    start = rowwise._row_times(_NAME, "t0", t0, B)
    if not bool(torch.isfinite(start).all()):
        raise ValueError("odeint_rowwise_event: t0 must be finite")
    if t_end is None:
        return torch.stack([start, torch.full((B,), math.inf, dtype=torch.float64)])
    return rowwise._row_grid(_NAME, start, "t_end", rowwise._row_times(_NAME, "t_end", t_end, B))


class RowEvents:
    """The event state of one solve, shared by both backends: the starting signs, which rows fired (ever / in the last
    trial step), their brackets in solver time and the quartic of the step each row fired in.

    `coef` is a [5, B, L] tensor of the state's dtype on its device — FIVE TIMES THE STATE, held for the whole solve,
    and indexed by ORIGINAL row also after a repack (`compact=`); the [B] vectors are then those of the rows carried,
    and `all_fired` / `all_lo` / `all_hi` hold what the rows that left had (`keep_rows`, `full`)."""

    def __init__(self, p: _Problem, event_fn):
        dev, B = p.device, p.B
        self.p, self.event_fn = p, event_fn
        self.n_evals = 0
        self.row_evals = 0                                   # the sum of y.shape[0] over the calls of event_fn
        self.atol_rows = p.atol_rows                         # all B rows' (`_Problem.keep_rows` re-selects its own at a repack)
        self.all_sign0 = self.all_fired = self.all_lo = self.all_hi = None      # [B], from the first repack on
        self.sign0 = torch.zeros(B, dtype=torch.int32, device=dev)
        self.fired = torch.zeros(B, dtype=torch.int32, device=dev)
        self.fired_now = torch.zeros(B, dtype=torch.int32, device=dev)
        self.lo = torch.zeros(B, dtype=torch.float64, device=dev)
        self.hi = torch.zeros(B, dtype=torch.float64, device=dev)
        self.coef = torch.empty(5, B, p.L, dtype=p.dtype, device=dev)

    def call(self, t_rows: torch.Tensor, y: torch.Tensor, rows=None) -> torch.Tensor:
        """event_fn(t_rows [b] true time, y [b, *row_shape]) -> [b] contiguous in the state's dtype; with `compact` set
        event_fn also gets the original indices of the rows of this call: those now carried, or `rows` (the bisection)."""
        self.n_evals += 1
        self.row_evals += y.shape[0]
        p = self.p
        if p.rows is None:
            g = self.event_fn(t_rows, y.view(y.shape[0], *p.shape[1:]))
        else:
            g = self.event_fn(t_rows, y.view(y.shape[0], *p.shape[1:]), p.rows if rows is None else rows)
        if not isinstance(g, torch.Tensor):
            raise TypeError("odeint_rowwise_event: event_fn must return a Tensor, got {}".format(type(g).__name__))
        if g.shape != (y.shape[0],):
            raise RuntimeError("odeint_rowwise_event: event_fn returned shape {} for {} rows (one value per row: [{}])".format(
                tuple(g.shape), y.shape[0], y.shape[0]))
        if g.device != p.device:
            raise RuntimeError(f"odeint_rowwise_event: event_fn returned a tensor on '{g.device}', the state lives on "
                               f"'{p.device}'")
        if g.is_complex():
            raise RuntimeError("odeint_rowwise_event: event_fn must return a real tensor")
        return g.detach().to(p.dtype).contiguous()

    def step_times(self, t0: torch.Tensor) -> torch.Tensor:
        """The end of each row's trial step in true time, in the state's dtype (t0: the fp64 solver times after the
        controller — the end of an accepted step; the value of any other row is ignored)."""
        return (t0 * self.p.sign).to(self.p.dtype)

    # -- compact=: what a repack does to the event state ------------------------------------------------------------------
    def _park(self) -> None:
        """`fired`, `lo`, `hi` of the rows now carried -> the [B] vectors, at their original indices (as
        `HipRowKernels._park_counts` keeps the counters of the rows that leave)."""
        rows = self.p.rows
        self.all_fired.index_copy_(0, rows, self.fired)
        self.all_lo.index_copy_(0, rows, self.lo)
        self.all_hi.index_copy_(0, rows, self.hi)

    def keep_rows(self, keep: torch.Tensor) -> None:
        """A repack, before `_Problem.keep_rows`: the carried rows `keep` (int64 positions in the current batch,
        ascending, on the state's device) stay.  Tiny [B] torch ops, like the other vectors of `repack`."""
        if self.all_fired is None:
            self.all_sign0 = self.sign0                      # (never written after t0: the first batch's vector is the full one)
            self.all_fired, self.all_lo, self.all_hi = (torch.zeros_like(v) for v in (self.fired, self.lo, self.hi))
        self._park()
        for name in ("sign0", "fired", "fired_now", "lo", "hi"):
            setattr(self, name, getattr(self, name).index_select(0, keep))

    def full(self):
        """(sign0, fired, lo, hi) as [B] vectors indexed by original row, for `_locate`."""
        if self.all_fired is None:
            return self.sign0, self.fired, self.lo, self.hi
        self._park()
        return self.all_sign0, self.all_fired, self.all_lo, self.all_hi

    # -- the step hook (rowwise.py) ---------------------------------------------------------------------------------------
    @property
    def stopped_now(self) -> torch.Tensor:
        return self.fired_now

    def before_step(self, n_active: int) -> None:
        pass

    def device_step(self, kern, y, y1, f0, f1, mid, coefs, dts) -> None:
        g1 = self.call(self.step_times(kern.t0), y1)
        kern.k.row_event_detect(g1, self.sign0, kern.ctrl, kern.st, kern.dts, kern.times, self.fired, self.fired_now,
                                self.lo, self.hi)
        if kern.row_map is None:
            kern.k.row_event_fit(self.coef, self.fired_now, y, y1, f0, f1, mid, coefs, dts)
        else:                                                # a compacted batch: the quartic goes to the row's original index
            kern.k.row_event_fit_mapped(self.coef, kern.row_map, self.fired_now, y, y1, f0, f1, mid, coefs, dts)

    def host_step(self, kern, accepted, y, y1, f0, f1, ks, dts) -> None:
        """The same decisions as torch / numpy ops; the row leaves the active ones after the controller's `prepare`."""
        g1 = self.call(self.step_times(torch.from_numpy(kern.t0.copy())), y1)
        s1, s0 = _sign(g1).numpy(), self.sign0.numpy()
        fired, now, lo, hi = self.fired.numpy(), self.fired_now.numpy(), self.lo.numpy(), self.hi.numpy()
        now[:] = 0
        rows = [r for r, _, _ in accepted if not fired[r] and s1[r] != s0[r]]
        if not rows:
            return
        now[rows] = 1
        fired[rows] = 1
        lo[rows], hi[rows] = kern.tprev[rows], kern.t0[rows]
        idx = torch.tensor(rows)
        at = idx if kern.row_map is None else torch.from_numpy(kern.row_map[rows])
        self.coef[:, at] = kern.step_quartic(idx, y, y1, f0, f1, ks, dts)


def _bisection_rounds(width: torch.Tensor, has_q: torch.Tensor) -> np.ndarray:
    """nitrs_r = max(0, ceil(log(width_r) / log 2)) of the rows with a quartic, 0 elsewhere (a NaN counts as 0), formed
    on the host in fp64 so that both backends get the same integers (event_handling.py:8)."""
    with np.errstate(all="ignore"):
        n = np.ceil(np.log(width.cpu().numpy()) / math.log(2.0))
    n = np.where(np.isnan(n), 0.0, np.maximum(n, 0.0))
    return np.where(has_q.cpu().numpy(), n, 0.0)


def _atol_rows(p: _Problem, atol_rows) -> torch.Tensor:
    """Each row's atol rounded to the state's dtype, as fp64 [B] on the state's device (`atol_rows`: the [B] vector of a
    solve with per-row tolerances, else None)."""
    if atol_rows is not None:
        return atol_rows.to(torch.float64)
    return torch.full((p.B,), float(p.np_dtype(p.atol)), dtype=torch.float64, device=p.device)


def _locate(p: _Problem, ev: RowEvents, kern, sol, at_start):
    """The one bisection after every row has stopped -> (event time [B] fp64 in solver time, fired [B] bool);
    solution row 1 of the rows that fired is overwritten with the quartic at the event time.

    It runs over a SELECTION of the rows.  Without `compact`: all B rows, those without a quartic masked out ([B] vectors,
    a [B, L] `y_mid`, `event_fn` called without `rows`).  With `compact`: the rows that have a quartic only, gathered in
    ascending original order ([n_q] vectors, a [n_q, L] `y_mid`, `event_fn` called with `rows = idx`)."""
    dev = p.device
    sign0, fired, lo_all, hi_all = ev.full()
    fired = fired.bool()
    has_q = fired & ~at_start                                # (a row that fired at t0 took no step: it keeps y0)
    atol = _atol_rows(p, ev.atol_rows)
    if p.compact is None:
        idx, live, s0 = None, has_q, sign0
        ta, tb = lo_all.clone(), hi_all.clone()              # the step the row fired in: the quartic's interval
        lo, hi = lo_all, hi_all
        mask = has_q.to(torch.int32)
        y_mid = p.y0.clone()                                 # (rows without a quartic keep y0; their values are ignored)
    else:
        idx = torch.nonzero(has_q).view(-1)
        ta, tb = lo_all.index_select(0, idx), hi_all.index_select(0, idx)
        atol, live = atol.index_select(0, idx), torch.ones_like(idx, dtype=torch.bool)
        lo, hi, s0 = ta, tb, sign0.index_select(0, idx)
        src = idx.to(torch.int32)
        y_mid = torch.empty(idx.numel(), p.L, dtype=p.dtype, device=dev)

    def quartics_at(out, x, fired=None):
        """out <- the selected rows' quartics at x; `fired` ([B] bool): only those rows, written at their original row."""
        if idx is None:
            kern.event_eval(out, ev.coef, x, mask if fired is None else (has_q & fired).to(torch.int32))
        elif fired is None:
            kern.event_eval_mapped(out, None, ev.coef, src, x)
        else:
            sel = fired.index_select(0, idx)
            at = src[sel]
            kern.event_eval_mapped(out, at, ev.coef, at, x[sel])

    n = _bisection_rounds((tb - ta) / atol, live)            # (0 for a row without a quartic)
    if np.isinf(n).any():
        r = int(np.flatnonzero(np.isinf(n))[0])
        raise OverflowError("odeint_rowwise_event: cannot bisect to a tolerance of 0 (atol must be positive) in row {}".format(
            r if idx is None else int(idx[r])))
    nitrs = torch.from_numpy(n.astype(np.int64)).to(dev)
    width = tb - ta
    for i in range(int(n.max()) if n.size else 0):
        t_mid = (lo + hi) / 2
        quartics_at(y_mid, ((t_mid - ta) / width).to(p.dtype))
        same = _sign(ev.call((t_mid * p.sign).to(p.dtype), y_mid, idx)) == s0
        update = nitrs > i
        lo, hi = torch.where(update & same, t_mid, lo), torch.where(update & ~same, t_mid, hi)
    mid = (lo + hi) / 2
    event_s = mid if idx is None else ((lo_all + hi_all) / 2).index_copy_(0, idx, mid)
    t_end = p.tgrid[1].to(dev)
    fired = fired & (event_s <= t_end)                       # a final step that crossed both: the event must come first
    quartics_at(sol[1], ((mid - ta) / width).to(p.dtype), fired)
    return torch.where(fired, event_s, t_end), fired


def odeint_rowwise_event(func, y0, t0, *, event_fn, t_end=None, rtol=1e-7, atol=1e-9, method="dopri5", options=None,
                         return_stats=False, compact=None):
    """Integrate B independent IVPs `dy_r/dt = func(t, y)[r]` from `t0`, each row until ITS terminal event: the first
    sign change of `event_fn(t, y)[r]` — or until `t_end[r]`, whichever comes first.  Returns `(event_t, solution)`.

    `y0` is `[B, *row_shape]` (fp32 / fp64); `func(t_rows, y)` is the func of `odeint_rowwise` (`t_rows` a `[b]` tensor of
    stage times in the state's dtype).  `t0` is a number, a 0-dim tensor or a `[B]` tensor.  `t_end` is None (increasing
    time, no end), a number or a `[B]` tensor; it must differ from `t0` in every row, in the same direction for all rows
    (`t_end < t0`: decreasing time), else ValueError.  `rtol`, `atol` (numbers or `[B]` vectors), `method` and `options`
    (`first_step`, `safety`, `ifactor`, `dfactor`, `max_num_steps`, `min_step`, `max_step`, `step_t`, `jump_t`) are those of
    `odeint_rowwise`; the event of a step onto a jump point is tested before `f0` is re-evaluated behind it.  `jump_dy`
    raises NotImplementedError: an impulse can flip the sign of the event function with no root inside any step.

    `event_fn(t_rows [b], y [b, *row_shape]) -> [b]` returns one real value per row on the state's device; it always gets
    TRUE time (also for decreasing time), in the state's dtype, and is called under `torch.no_grad()`; its value is cast
    to the state's dtype.  A wrong type, shape or device raises as it does for `func`.

    Per row r (the reference's `_advance_until_event` + `find_event`, row by row):
      * `s0 = sign(event_fn(t0, y0))[r]` with `sign(g) = (g > 0) - (g < 0)` (a NaN gives 0).  `s0 == 0`: the row has fired
        at `t0` — it takes no step and keeps `y0`.
      * after every trial step `event_fn` is called once for all rows with the end of each row's step and the state
        there.  A row whose step was accepted and whose sign is `!= s0` fires: it stops, frozen like a row that reached
        its last output time (`func` and `event_fn` keep being called for it, the values are ignored).
      * a row that reaches `t_end[r]` first stops there: `event_t[r] = t_end[r]`, `solution[1, r] = y(t_end[r])`,
        `fired[r] = False`.
      * once every row has stopped, ONE bisection locates all events: row r takes
        `nitrs_r = max(0, ceil(log2((hi - lo) / atol_r)))` halvings of the step `[lo, hi]` it fired in (`atol_r` the row's
        atol rounded to the state's dtype), each on the quartic dense output of that step, and `max_r nitrs_r` rounds are
        run with one `event_fn` call each; `event_t[r] = (lo + hi) / 2` and `solution[1, r]` is the quartic there.
      * a final step that crosses `t_end[r]` AND changes sign is bisected like any other; the row counts as fired only if
        the located time is not beyond `t_end[r]`, else it is a row that reached `t_end[r]`.
    A row's bits do not depend on B or on the other rows (as long as `func` and `event_fn` treat rows independently).

    Errors are those of `odeint_rowwise`, per row.  `max_num_steps` counts ALL trial steps of a row (there are no output
    times in between to start the count again).  The one deviation from the reference: an error the controller reports
    for a row (max_num_steps, dt underflow, a non-finite state) wins even if that row fires in the same trial step.
    With `t_end=None` a row that never fires ends in one of those errors, or never.

    Returns `event_t` (`[B]` fp64, true time, on the state's device) and `solution` (`[2, *y0.shape]`: `solution[0] = y0`,
    `solution[1, r]` = row r at `event_t[r]`); with `return_stats=True` also `stats`: `n_accepted`, `n_rejected` (int64
    `[B]`), `nfe`, `fired` (bool `[B]`, on the CPU like the counters) and `n_event_evals` (calls of `event_fn`: one at `t0`,
    one per trial step, one per bisection round).

    `compact` (default None / False: off; `True` = 0.5; a float c in (0, 1]; anything else ValueError) takes the rows that
    have stopped out of the batch by `odeint_rowwise`'s rule: after every poll, the one after the initial step included,
    with `cur` rows carried and `n_active` of them still active, `0 < n_active < cur` and `n_active <= c * cur` repacks the
    batch to the active rows.  A row that fired, a row that reached `t_end` and a row that fired at `t0` are all simply
    not active (the rows fired at `t0` leave at the first poll).  With `compact` set `func` is called as
    `func(t_rows, y, rows)` and `event_fn` as `event_fn(t_rows, y, rows)` — every call, the ones at `t0` and those of the
    bisection included: `rows` is an int64 `[b]` tensor on the state's device with the original indices of the rows of
    the call, ascending (`arange(B)` before the first repack); per-row parameters must be indexed with it.  The final
    bisection then runs on the rows that have a quartic only (those that fired after `t0`), with the same number of
    rounds.  `event_t`, `solution`, `n_accepted`, `n_rejected`, `fired`, `nfe` and `n_event_evals` are bit for bit those of
    the same call without `compact` (as long as `func` and `event_fn` treat rows independently), errors name the
    original row, and `stats` gains `row_evals` (the sum of `y.shape[0]` over the calls of `func`), `n_repacks` and
    `event_row_evals` (that sum over the calls of `event_fn`).

    Memory: besides the buffers of `odeint_rowwise` the solve holds the quartic coefficients of every row, a `[5, B, L]`
    tensor of the state's dtype — five times the state.

    Out of scope (raises or is not offered): gradients (with grad mode on and anything requiring grad this raises
    NotImplementedError; there is no `differentiable` argument), several event functions, non-terminal events, 16-bit or
    complex states, captured (hipGraph) steps.
    """
    if not callable(event_fn):
        raise ValueError("odeint_rowwise_event: event_fn must be callable: event_fn(t_rows [b], y [b, *row_shape]) -> [b]")
    if options is not None and dict(options).get("jump_dy") is not None:
        raise NotImplementedError("odeint_rowwise_event: jump_dy is not supported: an impulse can flip the sign of the "
                                  "event function with no root inside any step")
    B = rowwise._batch_rows(y0)
    p = _Problem(func, y0, None if B is None else _event_grid(t0, t_end, B), rtol, atol, method, options, None, False, compact)
    ev = RowEvents(p, event_fn)
    with torch.no_grad(), device_guard(p.device):
        ev.sign0 = _sign(ev.call((p.tgrid[0] * p.sign).to(p.dtype).to(p.device), p.y0))      # at t0 in true time
        at_start = ev.sign0 == 0
        ev.fired.copy_(at_start)
        ev.lo.copy_(p.tgrid[0])
        ev.hi.copy_(p.tgrid[0])
        sol = torch.empty(2, p.B, p.L, dtype=p.dtype, device=p.device)
        sol[0].copy_(p.y0)
        sol[1].copy_(p.y0)
        stepping = not bool(at_start.all())                  # every row fired at t0: no step, no func call
    n_acc = n_rej = None
    event_s, fired = p.tgrid[0].to(p.device), at_start
    if stepping:
        f0 = p.first_call(p.y0)
        with torch.no_grad(), device_guard(p.device):
            kern, n_acc, n_rej = rowwise._solve(p, p.y0, f0, sol, ev, at_start)
            event_s, fired = _locate(p, ev, kern, sol, at_start)
    event_t = event_s * p.sign
    solution = sol.view(2, *p.shape)
    if not return_stats:
        return event_t, solution
    stats = dict(rowwise._stats(p, n_acc, n_rej), fired=fired.cpu(), n_event_evals=ev.n_evals)
    if p.compact is not None:
        stats["event_row_evals"] = ev.row_evals
    return event_t, solution, stats
