"""`odeint_rowwise`: a batch of independent IVPs, each row with its own adaptive step controller.

`odeint` treats a batched state as ONE system: the error ratio is the RMS over every element of the batch, so every
row takes the same step sizes and the same accept / reject decisions, and a row's answer depends on its batch mates.
Here row r of `y0[B, *row_shape]` is its own IVP: its own error norm (the RMS over its L = prod(row_shape) elements),
its own step size, accept / reject decision, counters and output times, and — with `rtol` / `atol` given as [B] vectors —
its own tolerances.  A row's bits do not depend on B or on the other rows (as long as `func` itself treats rows
independently).

On a ROCm device every state-sized operation is a HIP kernel of csrc/tdeq_kernels_rowwise.hpp and the per-row
controller runs on the device (the host reads two words per trial step, three with per-row bounds or points); CPU
states run the same row operations as torch ops (`HostRowKernels`, one `HostPathWarning`).

The structure.  ONE DRIVER, `_solve`, serves the three entry points (`odeint_rowwise` here, `odeint_rowwise_event` in
rowwise_event.py, `odeint_rowwise_dense` in rowwise_dense.py): it chooses the backend, runs the initial step and then the
loop poll -> row error -> repack rule (`compact=`, `_compact_fraction`) -> trial step, and reads the counters; `_stats`
assembles what all three report.  An entry point validates its arguments (`_Problem`; `_row_times` / `_row_grid` for a
solve between two times per row), evaluates `func` once in the caller's grad mode (`_Problem.first_call`) and turns what
the driver leaves behind into its result.

The TWO BACKENDS, `HipRowKernels` and `HostRowKernels`, offer the driver the same methods — `initial_step`, `trial_step`,
`poll`, `counts`, `repack`, `deactivate_rows`, `n_jumped` / `refresh_after_jump` (a step onto a `jump_t` point), for a
recorded solve `begin_recording` / `recorded_solution` — and the entry points the operations on kept quartics,
`event_eval` / `event_eval_mapped` / `pack_quartics`.  WHAT IS LAUNCHED in a
trial step is `HipRowKernels.trial_step`: one interpreter of the tableau's launch plan (`tableaus.launch_plan`: the carry
plan of dopri5 / dopri8 / tsit5, row by row for the others), then the error norm, the controller, the hook and the
dense-output commit.

ONE STEP HOOK (None in a plain solve; one slot, hooks do not combine) is what an event or a dense solve adds to a step.  The
backends and the driver use exactly these members of it:
  * `before_step(n_active)`: the driver, before every trial step;
  * `device_step(kern, y, y1, f0, f1, mid, coefs, dts)` / `host_step(kern, accepted, y, y1, f0, f1, ks, dts)`: the backend,
    between the controller and the commit (the commit overwrites y and f0);
  * `keep_rows(keep)`: the backend, at a repack, before `_Problem.keep_rows`;
  * `stopped_now`: the rows the hook took out of the active ones in this trial step (int32 [n]), or None for a hook that
    stops none — `poll` and the end of the host trial step read it.

WHAT IS RECORDED for `differentiable=True` lives in rowwise_autodiff.py: the device backend hands its finished launches
to a `RowRecorder` (None in a plain solve), the host backend records plain torch ops; `_Problem.grad_mode` is the one
place that turns grad mode on for a recorded solve.
"""
from __future__ import annotations

import contextlib
import math
from typing import List

import numpy as np
import torch

from . import _fallback, _native
from . import rowwise_autodiff as rad
from ._native import device_guard
from ._scalars import nextafter, power, rdiv, scalar_type
from .solvers._common import _clamp, optimal_step_size
from .solvers.adaptive import (STEP_CALLBACKS, AdaptiveHeunSolver, Bosh3Solver, Dopri5Solver, Dopri8Solver, Fehlberg2,
                               Tsit5Solver)
from .tableaus import SparseRow, launch_plan

__all__ = ["odeint_rowwise"]

_METHODS = {"dopri5": Dopri5Solver, "bosh3": Bosh3Solver, "tsit5": Tsit5Solver, "fehlberg2": Fehlberg2,
            "adaptive_heun": AdaptiveHeunSolver, "dopri8": Dopri8Solver}
_OPTIONS = ("first_step", "safety", "ifactor", "dfactor", "max_num_steps", "min_step", "max_step", "step_t", "jump_t",
            "jump_dy")
_STEP_OPTIONS = ("min_step", "max_step", "step_t", "jump_t", "jump_dy")
_NO_ERROR_ROW = 0x7FFFFFFF


class _Method:
    """Host-side constants of one tableau, shared by both backends."""

    def __init__(self, name: str, np_dtype):
        cls = _METHODS[name]
        tab = cls.tableau
        self.name, self.order, self.tableau = name, cls.order, tab
        self.beta = tab.beta_rows()
        self.c_sol = SparseRow.from_dense(tab.c_sol)
        self.c_err = SparseRow.from_dense(tab.c_error)
        self.c_mid = SparseRow.from_dense(tab.c_mid)
        self.fsal = tab.fsal_solution
        self.alpha = [np_dtype(a) for a in tab.alpha]
        self.alpha_is_one = [a == 1.0 for a in tab.alpha]
        self.n_stages = len(self.beta)


def _compact_fraction(compact):
    """`compact=` of odeint_rowwise -> None (off) or the fraction c in (0, 1]: after a poll that finds n_active of the
    `cur` carried rows still active, 0 < n_active < cur and n_active <= c * cur, the batch is repacked to those rows."""
    if compact is None or compact is False:
        return None
    if compact is True:
        return 0.5
    if isinstance(compact, (int, float)) and 0.0 < compact <= 1.0:
        return float(compact)
    raise ValueError(f"odeint_rowwise: compact must be None, a bool or a fraction in (0, 1], got {compact!r}")


def _tolerance(name: str, tol, B: int):
    """`rtol` / `atol` of odeint_rowwise -> (float, None) for a number or a one-element tensor, (None, fp64 CPU tensor
    [B]) for a per-row vector (a 1-D real tensor, a 1-D numpy array, a list or a tuple of numbers with B entries).  A
    tensor is detached: no gradient flows to a tolerance.  The values are not looked at."""
    if isinstance(tol, torch.Tensor) and tol.numel() == 1 and not tol.is_complex():
        return float(tol), None
    if isinstance(tol, (int, float)) and not isinstance(tol, bool):
        return float(tol), None
    if isinstance(tol, torch.Tensor):
        shape, ok = tuple(tol.shape), tol.dim() == 1 and not tol.is_complex()
        vec = tol.detach().to("cpu", torch.float64) if ok else None
    elif isinstance(tol, np.ndarray):
        shape, ok = tol.shape, tol.ndim == 1 and tol.dtype.kind in "fiu"
        vec = torch.as_tensor(np.ascontiguousarray(tol), dtype=torch.float64) if ok else None
    elif isinstance(tol, (list, tuple)):
        shape = (len(tol),)
        ok = all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in tol)
        vec = torch.as_tensor([float(x) for x in tol], dtype=torch.float64) if ok else None
    else:
        raise ValueError(f"odeint_rowwise: {name} must be a number or a per-row vector [B] = [{B}] (a 1-D tensor, numpy "
                         f"array, list or tuple of numbers), got {type(tol).__name__}")
    if not ok or shape != (B,):
        raise ValueError(f"odeint_rowwise: {name} must be a number or a per-row vector of exactly B = {B} real entries, "
                         f"got shape {tuple(shape)}; a vector of another length and tolerances per element of a row "
                         "([B, *row_shape], [*row_shape]) are not supported")
    return None, vec


def _step_bound(name: str, v, B: int):
    """`min_step` / `max_step` -> (float, None) or (None, fp64 CPU tensor [B]): the forms of `_tolerance`.  The values are
    not looked at, as the reference does not validate them."""
    if isinstance(v, torch.Tensor) and v.dtype == torch.bool:
        v = None
    try:
        return _tolerance(name, v, B)
    except ValueError:
        raise ValueError(f"odeint_rowwise: {name} must be a number, a 0-dim tensor or a real per-row vector of exactly "
                         f"B = {B} entries (a 1-D tensor, numpy array, list or tuple of numbers)") from None


class _RowPoints:
    """One of the two point tables of a rowwise solve (`step_t`, `jump_t`) as the controllers take it: `table` [K, B] fp64
    numpy in solver time, every column sorted ascending and padded with +inf, `count` [B] the points of each row, `next`
    [B] the index each row starts with (rk_common.py:223-241 row by row; -1 for a row without points)."""

    def __init__(self, table: np.ndarray, count: np.ndarray, nxt: np.ndarray):
        self.table, self.count, self.next = table, count, nxt


def _points(name: str, v, B: int) -> "np.ndarray | None":
    """`step_t` / `jump_t` -> fp64 numpy [K, B] in the caller's time (NaN: no point), or None for K = 0."""
    bad = None
    if isinstance(v, torch.Tensor):
        if v.is_complex() or v.dtype == torch.bool:
            bad = f"a {v.dtype} tensor"
        else:
            a = v.detach().to("cpu", torch.float64).numpy()
    elif isinstance(v, (np.ndarray, list, tuple)):
        try:
            a = np.asarray(v)
        except ValueError:
            a = np.empty(0, dtype=object)
        if a.size == 0 and a.ndim == 1:
            a = a.astype(np.float64)
        if a.dtype.kind not in "fiu":
            bad = f"values of kind {a.dtype}"
        else:
            a = a.astype(np.float64)
    else:
        bad = type(v).__name__
    if bad is None and not (a.ndim == 1 or (a.ndim == 2 and a.shape[1] == B)):
        bad = f"shape {tuple(a.shape)}"
    if bad is not None:
        raise ValueError(f"odeint_rowwise: {name} must be real times [K] (shared by all rows) or [K, B] = [K, {B}] (a "
                         f"column per row): a tensor, a numpy array or a list of numbers; got {bad}")
    if a.shape[0] == 0:
        return None
    return np.ascontiguousarray(np.broadcast_to(a[:, None], (a.shape[0], B)) if a.ndim == 1 else a)


def _impulses(v, jump, sign: float, t0: np.ndarray, y0: torch.Tensor) -> torch.Tensor:
    """`jump_dy` -> a contiguous [K, B or 1, L] tensor of the state's dtype on its device, entry k the impulse of the
    caller's `jump_t[k]` (`jump`: that table as `_points` returns it, [K, B] in the caller's time, or None)."""
    B, row_shape = y0.shape[0], tuple(y0.shape[1:])
    if jump is None:
        raise ValueError("odeint_rowwise: jump_dy needs jump_t: one impulse for every entry of it")
    try:
        dy = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"odeint_rowwise: jump_dy must be a real tensor, numpy array or nested list of numbers, got "
                         f"{type(v).__name__}") from None
    if dy.is_complex() or dy.dtype == torch.bool:
        raise ValueError(f"odeint_rowwise: jump_dy must be real, got a {dy.dtype} tensor")
    K = jump.shape[0]
    per_row, shared = (K, B) + row_shape, (K,) + row_shape
    if dy.dim() == y0.dim() + 1 and tuple(dy.shape) == per_row:
        rows = B
    elif dy.dim() == y0.dim() and tuple(dy.shape) == shared:
        rows = 1
    else:
        raise ValueError(f"odeint_rowwise: jump_dy must be [K, B, *row_shape] = {list(per_row)} (an impulse per row) or "
                         f"[K, *row_shape] = {list(shared)} (shared by all rows), entry for entry the impulses of jump_t "
                         f"(K = {K}); got shape {list(dy.shape)}")
    dy = dy.detach().to(device=y0.device, dtype=y0.dtype).reshape(K, rows, -1).contiguous()
    live = jump == jump                                      # (the dy of a NaN time is ignored)
    finite = torch.isfinite(dy).all(dim=2).cpu().numpy()
    bad = live & ~finite
    if bad.any():
        k, r = (int(x[0]) for x in np.nonzero(bad))
        raise ValueError(f"odeint_rowwise: jump_dy[{k}] is not finite for row {r}, whose jump_t[{k}] is a time")
    with np.errstate(invalid="ignore"):
        at_start = (jump * sign == t0[None, :]) & (dy != 0).any(dim=2).cpu().numpy()
    if at_start.any():
        k, r = (int(x[0]) for x in np.nonzero(at_start))
        raise ValueError(f"odeint_rowwise: jump_t[{k}] of row {r} is the row's start time and its jump_dy is not zero: no "
                         "step ends there, so the impulse would never be applied; add it to y0")
    return dy


def _row_points(step, jump, sign: float, t0: np.ndarray, index: bool = False):
    """The two tables of `_points` -> (`_RowPoints` or None) each: per row the points >= t0_r in solver time, sorted; a
    value that occurs twice in a row's two lists together is refused (rk_common.py:229-232).  Whole-table numpy ops: the
    set-up of B rows costs no Python loop over them.  `index`: the jump table also gets `.index`, int32 [K', B]: the entry
    of the caller's table that sits at each sorted position (-1: padding), the argsort of the sort done here."""
    kept = []
    for tab in (step, jump):
        if tab is None:
            kept.append(None)
            continue
        a = tab * sign
        with np.errstate(invalid="ignore"):
            a = np.where(a >= t0[None, :], a, np.nan)        # (a NaN entry is padding; a point before t0_r is dropped)
        kept.append(np.sort(a, axis=0))                      # ascending, NaN last
    both = [a for a in kept if a is not None]
    if both:
        merged = np.sort(np.concatenate(both, axis=0), axis=0)
        twice = (merged[1:] == merged[:-1]).any(axis=0)      # (NaN != NaN: padding never counts)
        if twice.any():
            raise ValueError("`step_t` and `jump_t` must not have any repeated elements between them (row {}).".format(
                int(np.flatnonzero(twice)[0])))
    out = []
    for a in kept:
        count = None if a is None else (a == a).sum(axis=0).astype(np.int32)
        if a is None or count.max(initial=0) == 0:
            out.append(None)
            continue
        # bisect_right(points, t0_r) counts the points equal to t0_r (none is smaller); then min(., n - 1), -1 without points
        nxt = np.minimum((a == t0[None, :]).sum(axis=0), count - 1).astype(np.int32)
        table = np.where(a == a, a, np.inf)[:int(count.max())]
        out.append(_RowPoints(np.ascontiguousarray(table), count, nxt))
    if index and out[1] is not None:
        with np.errstate(invalid="ignore"):
            raw = np.where(jump * sign >= t0[None, :], jump * sign, np.nan)      # the table before its sort (kept[1])
        order = np.argsort(raw, axis=0, kind="stable")       # (NaN last, as np.sort; no two equal times in a column)
        a = kept[1][:out[1].table.shape[0]]
        out[1].index = np.ascontiguousarray(np.where(a == a, order[:a.shape[0]], -1).astype(np.int32))
    return out


def _batch_rows(y0):
    """B of a y0 that has a batch, else None: the entry points that build their grid from B pass `t=None` then, and
    `_Problem` refuses that y0 with its own message before it looks at t."""
    return y0.shape[0] if isinstance(y0, torch.Tensor) and y0.dim() >= 1 and y0.shape[0] >= 1 else None


def _row_times(fn: str, name: str, v, B: int) -> torch.Tensor:
    """A start or end time of `fn` -> fp64 CPU tensor [B]: a number, a 0-dim tensor or a [B] tensor."""
    if isinstance(v, torch.Tensor):
        if v.is_complex() or v.dtype == torch.bool or v.dim() > 1 or (v.dim() == 1 and v.shape[0] != B):
            raise ValueError(f"{fn}: {name} must be a number, a 0-dim tensor or a real [B] = [{B}] tensor, "
                             f"got a {v.dtype} tensor of shape {tuple(v.shape)}")
        v = v.detach().to("cpu", torch.float64)
        return v.expand(B).clone() if v.dim() == 0 else v.clone()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return torch.full((B,), float(v), dtype=torch.float64)
    raise ValueError(f"{fn}: {name} must be a number, a 0-dim tensor or a [B] = [{B}] tensor, got "
                     f"{type(v).__name__}")


def _row_grid(fn: str, start: torch.Tensor, name: str, end: torch.Tensor) -> torch.Tensor:
    """The [2, B] fp64 grid [t0, end] of a solve between two times per row (`name`: what `fn` calls the end)."""
    if not (bool((end > start).all()) or bool((end < start).all())):
        raise ValueError(f"{fn}: {name} must differ from t0 in every row, in the same direction for all rows")
    return torch.stack([start, end])


def _func_parameters_require_grad(func) -> bool:
    params = getattr(func, "parameters", None)
    if callable(params):
        try:
            return any(p.requires_grad for p in params())
        except TypeError:
            return False
    return False


class _Problem:
    """Validated inputs: y [B, L] (contiguous copy), tgrid [T, B] fp64 in solver time (ascending), sign."""

    def __init__(self, func, y0, t, rtol, atol, method, options, event_fn, differentiable=False, compact=None):
        self.compact = _compact_fraction(compact)
        if event_fn is not None:
            raise ValueError("odeint_rowwise: event_fn is not supported (use odeint)")
        if not isinstance(y0, torch.Tensor):
            raise ValueError("odeint_rowwise: tuple states are not supported; y0 must be one tensor [B, *row_shape]")
        if y0.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"odeint_rowwise: the state dtype must be float32 or float64, got {y0.dtype} "
                             "(16-bit, complex and integer states are not supported)")
        if y0.dim() < 1 or y0.shape[0] < 1:
            raise ValueError("odeint_rowwise: y0 must have a leading batch dimension B >= 1")
        (rtol, rtol_rows), (atol, atol_rows) = _tolerance("rtol", rtol, y0.shape[0]), _tolerance("atol", atol, y0.shape[0])
        if method not in _METHODS:
            raise ValueError('odeint_rowwise: method "{}" is not supported; one of {}'.format(
                method, ", ".join(sorted(_METHODS))))
        options = dict(options or {})
        unknown = sorted(set(options) - set(_OPTIONS))
        if unknown:
            raise ValueError("odeint_rowwise: unsupported option(s) {}; supported: {}".format(
                ", ".join(repr(u) for u in unknown), ", ".join(_OPTIONS)))
        for name in STEP_CALLBACKS:
            if getattr(func, name, None) is not None:
                raise ValueError(f"odeint_rowwise: step callbacks ({name}) are not supported")
        if not isinstance(t, torch.Tensor) or not torch.is_floating_point(t):
            raise ValueError("odeint_rowwise: t must be a floating point tensor [T] or [T, B]")
        B = y0.shape[0]
        if t.dim() == 2:
            if t.shape[1] != B:
                raise ValueError(f"odeint_rowwise: a 2-D t must be [T, B] = [T, {B}], got {tuple(t.shape)}")
        elif t.dim() != 1:
            raise ValueError(f"odeint_rowwise: t must be [T] or [T, B], got {t.dim()} dimensions")
        if t.shape[0] < 1:
            raise ValueError("odeint_rowwise: t needs at least one time")
        # record: the solve builds an autograd graph (rowwise_autodiff.py); under no_grad `differentiable` has no effect
        self.record = bool(differentiable) and torch.is_grad_enabled()
        if self.record and t.requires_grad:
            raise NotImplementedError("odeint_rowwise(differentiable=True): time gradients (t.requires_grad) are not "
                                      "supported; detach t, or use odeint")
        if self.record and self.compact is not None:
            raise NotImplementedError("odeint_rowwise: compact is not supported for a recorded solve "
                                      "(differentiable=True with grad mode on)")
        if not self.record and torch.is_grad_enabled() and (y0.requires_grad or t.requires_grad or
                                                            _func_parameters_require_grad(func)):
            raise NotImplementedError("odeint_rowwise does not propagate gradients unless differentiable=True is "
                                      "passed; use that, odeint (backprop through the solver) or odeint_adjoint, or "
                                      "call it under torch.no_grad()")

        self.func, self.shape, self.B = func, y0.shape, B
        self.L = int(math.prod(y0.shape[1:]))
        self.dtype, self.device = y0.dtype, y0.device
        self.np_dtype = scalar_type(y0.dtype)
        tg = t.detach().to(torch.float64)
        tg = tg[:, None].expand(-1, B) if tg.dim() == 1 else tg
        tg = tg.to("cpu")
        n_t = tg.shape[0]
        sign = 1.0
        if n_t > 1:
            inc, dec = bool((tg[1:] > tg[:-1]).all()), bool((tg[1:] < tg[:-1]).all())
            if not (inc or dec):
                raise ValueError("odeint_rowwise: every row of t must be strictly monotone, all in the same direction")
            sign = 1.0 if inc else -1.0
        # times as the solver sees them: the grid cast to the state's type and back (odeint: t.to(y0.dtype)), negated
        # for decreasing time (misc.py `_ReverseFunc`)
        self.tgrid = (tg * sign).contiguous()
        self.sign = sign
        self.y0 = y0.detach().reshape(B, self.L).contiguous()
        self.y0_graph = y0.reshape(B, self.L) if self.record else None
        # the tolerances: two floats, or — as soon as one of them is a per-row vector — two [B] tensors in the state's
        # dtype on its device (the other filled to [B]), rounded as the kernels round a scalar: T(x) of the fp64 value
        self.rtol, self.atol = rtol, atol
        self.rtol_rows = self.atol_rows = None
        if rtol_rows is not None or atol_rows is not None:
            rows = [torch.full((B,), x, dtype=torch.float64) if v is None else v
                    for x, v in ((rtol, rtol_rows), (atol, atol_rows))]
            self.rtol_rows, self.atol_rows = (v.to(self.dtype).to(self.device).contiguous() for v in rows)
            self.rtol = self.atol = None
        self.method = _Method(method, self.np_dtype)
        fs = options.get("first_step")
        if fs is not None:
            fs = torch.as_tensor(fs, dtype=torch.float64).detach().reshape(-1).cpu()
            if fs.numel() == 1:
                fs = fs.expand(B)
            elif fs.numel() != B:
                raise ValueError(f"odeint_rowwise: first_step must be a scalar or a [B] = [{B}] tensor")
            fs = fs.abs()
        self.first_step = fs
        self.safety = float(options.get("safety", 0.9))
        self.ifactor = float(options.get("ifactor", 10.0))
        self.dfactor = float(options.get("dfactor", 0.2))
        self.max_num_steps = int(options.get("max_num_steps", 2 ** 31 - 1))
        # the step options: two bounds (floats, or — as soon as one is a per-row vector — two fp64 [B] numpy vectors) and
        # the two point tables; the clipped step's graph is out of scope for a recorded solve
        (self.min_step, lo_rows), (self.max_step, hi_rows) = (_step_bound(name, options.get(name, default), B)
                                                              for name, default in (("min_step", 0.0), ("max_step", math.inf)))
        self.min_rows = self.max_rows = None
        if lo_rows is not None or hi_rows is not None:
            self.min_rows, self.max_rows = (np.full(B, x) if v is None else v.numpy().copy()
                                            for x, v in ((self.min_step, lo_rows), (self.max_step, hi_rows)))
            self.min_step = self.max_step = None
        step, jump = (_points(name, options.get(name, ()), B) for name in ("step_t", "jump_t"))
        # the impulses of the jump points (`jump_dy`): [K, B or 1, L], never permuted or gathered — `jump_points.index`
        # leads from a position in a row's sorted column to the caller's k; None without the option
        self.jump_dy = None
        if options.get("jump_dy") is not None:
            self.jump_dy = _impulses(options["jump_dy"], jump, sign, self.tgrid[0].numpy(), y0)
        self.step_points, self.jump_points = _row_points(step, jump, sign, self.tgrid[0].numpy(),
                                                         index=self.jump_dy is not None)
        given = [name for name in _STEP_OPTIONS if name in options]
        if self.record and given:                            # (after their validation: a wrong value is a ValueError first)
            raise NotImplementedError("odeint_rowwise: {} not supported for a recorded solve (differentiable=True with "
                                      "grad mode on)".format(", ".join(given) + (" is" if len(given) == 1 else " are")))
        self.n_impulses = None                               # with jump_dy: int64 [B] by original row, after the solve
        self.nfe = 0
        # compact: the original indices of the rows now carried (int64, ascending, on the state's device) — func's third
        # argument — and what the two extra stats count
        self.rows = torch.arange(B, device=self.device) if self.compact is not None else None
        self.row_evals = 0
        self.n_repacks = 0

    def keep_rows(self, idx: torch.Tensor) -> None:
        """A repack: the carried rows `idx` (int64 positions in the current batch, ascending) stay."""
        self.rows = self.rows.index_select(0, idx.to(self.rows.device))
        if self.rtol_rows is not None:
            at = idx.to(self.rtol_rows.device)
            self.rtol_rows, self.atol_rows = self.rtol_rows.index_select(0, at), self.atol_rows.index_select(0, at)
        self.n_repacks += 1

    def tolerances(self):
        """(rtol, atol) as a torch expression over a [b, L] state takes them: the two floats, or the [b, 1] columns of the
        per-row vectors of the rows now carried."""
        if self.rtol_rows is None:
            return self.rtol, self.atol
        return self.rtol_rows[:, None], self.atol_rows[:, None]

    def grad_mode(self):
        """The grad mode the backends step in (inside the driver's no_grad): on for a recorded solve.  The controller is
        outside the graph either way: it works on detached values or under a no_grad of its own."""
        return torch.enable_grad() if self.record else contextlib.nullcontext()

    def call(self, t_rows: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """func(t_rows [b], y [b, *row_shape]) -> [b, L] contiguous in the state's dtype, b the rows now carried (B
        unless the batch was compacted); with `compact` set func also gets their original indices."""
        self.nfe += 1
        self.row_evals += y.shape[0]
        y = y.view(y.shape[0], *self.shape[1:])
        shape = y.shape
        f = self.func(t_rows, y) if self.rows is None else self.func(t_rows, y, self.rows)
        if not isinstance(f, torch.Tensor):
            raise TypeError("odeint_rowwise: func must return a Tensor, got {}".format(type(f).__name__))
        if f.requires_grad and torch.is_grad_enabled() and not self.record:
            raise NotImplementedError("odeint_rowwise does not propagate gradients (func's output requires grad) unless "
                                      "differentiable=True is passed; use that, odeint / odeint_adjoint, or call it "
                                      "under torch.no_grad()")
        if f.shape != shape:
            raise RuntimeError("odeint_rowwise: func returned shape {} for a state of shape {}".format(
                tuple(f.shape), tuple(shape)))
        if f.device != self.device:
            raise RuntimeError(f"odeint_rowwise: func returned a tensor on '{f.device}', the state lives on '{self.device}'")
        f = f.reshape(shape[0], self.L)
        if f.dtype != self.dtype:
            f = f.to(self.dtype)
        return f if f.is_contiguous() and f.data_ptr() % 16 == 0 else f.contiguous(memory_format=torch.contiguous_format).clone()

    def first_call(self, y: torch.Tensor) -> torch.Tensor:
        """func at t0, for the entry points to call in the CALLER's grad mode: a func whose output depends on parameters
        that require grad (closures included) is refused here, never silently detached (unless the solve is recorded)."""
        with device_guard(self.device):
            return self.call((self.tgrid[0] * self.sign).to(self.dtype).to(self.device), y).clone()

    def raise_row_error(self, failure, y) -> None:
        r, code, since, dt, at = failure                     # r: the original row; at: where it sits in y
        if code == 2:
            raise AssertionError("max_num_steps exceeded ({}>={}) in row {}".format(since, self.max_num_steps, r))
        if code == 1:
            raise AssertionError("underflow in dt {} in row {}".format(dt, r))
        raise AssertionError("non-finite values in state `y`: {} in row {}".format(y[at].view(self.shape[1:]), r))


def _row_sum(x: torch.Tensor) -> torch.Tensor:
    """Sum over dim 1 of an fp64 [B, L] tensor in a FIXED order (pairwise halving over a zero-padded power-of-two
    width): each addition is an elementwise op, so a row's sum has the same bits in a batch of any size — unlike
    `sum(dim=-1)`, whose order ATen may choose by shape and thread count."""
    n = x.shape[1]
    w = 1 << max(0, (n - 1).bit_length())
    if w != n:
        x = torch.cat([x, x.new_zeros(x.shape[0], w - n)], dim=1)
    while x.shape[1] > 1:
        h = x.shape[1] // 2
        x = x[:, :h] + x[:, h:]
    return x[:, 0]


def _stopped_now(hook):
    """The rows the hook took out of the active ones in the last trial step (int32 [n], nonzero: stopped), or None."""
    return None if hook is None else hook.stopped_now


class HostRowKernels:
    """The row operations of `odeint_rowwise` as torch ops (CPU states): the per-row controller runs as host scalar
    arithmetic, row by row, with the decisions of the device controller (tdeq_kernels_rowwise.hpp)."""

    k = None                                                 # no kernels object: every operation is a torch expression

    def __init__(self, p: _Problem, hook=None):
        self.p = p
        self.hook = hook                                     # the step hook of an event or dense solve, else None
        T = p.np_dtype
        self.T = T
        B = p.B
        self.n = B                                           # rows now carried (fewer than p.B after a repack)
        self.row_map = None                                  # after a repack: their original indices
        self.t0 = np.zeros(B)
        self.tprev = np.zeros(B)
        self.dt = np.zeros(B)
        self.active = np.ones(B, dtype=bool)
        self.since = np.zeros(B, dtype=np.int64)
        self.next_out = np.ones(B, dtype=np.int64)
        self.bad_y = np.zeros(B, dtype=bool)
        self.n_acc = np.zeros(B, dtype=np.int64)
        self.n_rej = np.zeros(B, dtype=np.int64)
        self.code = np.zeros(B, dtype=np.int64)
        self.tg = p.tgrid.numpy()
        # the step options: the bounds per row, the two point tables with each row's index, and of the prepared step
        # where it was cut (`on_point`: 0 not, 1 at a step point, 2 at a jump point; `clip_t`: the point)
        self.min_r = np.full(B, p.min_step) if p.min_rows is None else p.min_rows.copy()
        self.max_r = np.full(B, p.max_step) if p.max_rows is None else p.max_rows.copy()
        self.step_tab, self.step_cnt, self.step_next = self._table(p.step_points)
        self.jump_tab, self.jump_cnt, self.jump_next = self._table(p.jump_points)
        self.clip_t = np.zeros(B)
        self.on_point = np.zeros(B, dtype=np.int64)
        self.jumped = np.zeros(B, dtype=bool)
        # impulses (`jump_dy`): the jump table is tested with the CLOSED rule t0 < p <= t0 + dt, an accepted step onto a jump
        # point notes the point's position in the row's sorted column, and `refresh_after_jump` adds the impulse
        self.impulse = p.jump_dy is not None and p.jump_points is not None
        self.jump_hit = np.zeros(B, dtype=np.int64) if self.impulse else None
        self.n_imp = np.zeros(B, dtype=np.int64) if self.impulse else None      # by original row
        # record mode: [B] fp64 graphs of the first step sizes (initial-step heuristic) and, from the second trial step
        # on, of the time every later step of the row is anchored to (t0 + dt_first for a row whose first step was accepted)
        self.s_shadow = None
        self.anchor = None

    # -- helpers ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _table(pts):
        if pts is None:
            return None, None, None
        return pts.table.copy(), pts.count.astype(np.int64), pts.next.astype(np.int64)

    def _coef(self, coef: float, dts: torch.Tensor) -> torch.Tensor:
        return torch.tensor(coef, dtype=self.p.dtype) * dts

    def _sum_terms(self, ks, row: SparseRow, dts):
        acc = None
        for j, c in zip(row.idx, row.coef):
            term = ks[j] * self._coef(c, dts)
            acc = term if acc is None else acc + term
        return acc

    def _dts_tensor(self, vals) -> torch.Tensor:
        return torch.tensor(np.asarray(vals, dtype=self.T).astype(np.float64), dtype=self.p.dtype).reshape(-1, 1)

    def _row_norms(self, q: torch.Tensor) -> np.ndarray:
        qd = q.detach().to(torch.float64)
        return _row_sum(qd * qd).numpy()

    def stage_time(self, r: int, i: int):
        m, T = self.p.method, self.T
        t0, dt = self.t0[r], self.dt[r]
        if m.alpha_is_one[i]:
            t1 = T(self.clip_t[r] if self.on_point[r] else t0 + dt)       # a cut step: the point itself
            tt = nextafter(t1, t1 - 1)
        else:
            tt = T(t0) + m.alpha[i] * T(dt)
        return float(self.p.sign * tt)

    def times_tensor(self) -> List[torch.Tensor]:
        p, m = self.p, self.p.method
        out = np.empty((m.n_stages, self.n))
        for r in range(self.n):
            for i in range(m.n_stages):
                out[i, r] = self.stage_time(r, i) if self.active[r] else float(p.sign * self.T(self.t0[r]))
        return list(torch.tensor(out, dtype=p.dtype).unbind(0))

    def prepare(self, r: int) -> None:
        dt, t0 = self.dt[r], self.t0[r]
        if not math.isfinite(dt):
            dt = self.min_r[r]
        dt = _clamp(dt, self.min_r[r], self.max_r[r])
        code = 3 if self.bad_y[r] else 0
        if not t0 + dt > t0:
            code = 1
        if self.since[r] >= self.p.max_num_steps:
            code = 2
        self.code[r] = code
        # the step cut short at the row's next step point, then at its next jump point, which wins (rk_common.py:289-309)
        on = 0
        for kind, tab, cnt, nxt in ((1, self.step_tab, self.step_cnt, self.step_next),
                                    (2, self.jump_tab, self.jump_cnt, self.jump_next)):
            if tab is not None and cnt[r] >= 1:
                pt = tab[nxt[r], r]
                if t0 < pt and (pt <= t0 + dt if kind == 2 and self.impulse else pt < t0 + dt):
                    # (a step that lands on the point keeps its size: pt - t0 may round above dt, hence above max_step)
                    on, dt = kind, (pt - t0 if pt < t0 + dt else dt)
                    self.clip_t[r] = pt
        self.on_point[r] = on
        self.dt[r] = dt

    # -- what the driver calls besides the two steps -------------------------------------------------------------------
    def begin_recording(self, sol, y) -> None:
        sol[0] = y                                           # the host path records the solution rows as in-place writes

    def recorded_solution(self, sol) -> torch.Tensor:
        return sol

    def poll(self):
        # (a row the hook stopped in this trial step was prepared before it left, and its error wins)
        stopped = _stopped_now(self.hook)
        live = self.active if stopped is None else self.active | stopped.numpy().astype(bool)
        r = next((r for r in range(self.n) if live[r] and self.code[r] != 0), None)
        if r is None:
            return int(self.active.sum()), None
        row = r if self.row_map is None else int(self.row_map[r])
        return int(self.active.sum()), (row, int(self.code[r]), int(self.since[r]), float(self.dt[r]), r)

    def counts(self):
        if self.row_map is None:
            return torch.from_numpy(self.n_acc.copy()), torch.from_numpy(self.n_rej.copy())
        self.all_acc[self.row_map], self.all_rej[self.row_map] = self.n_acc, self.n_rej
        return torch.from_numpy(self.all_acc.copy()), torch.from_numpy(self.all_rej.copy())

    _ROW_VECTORS = ("t0", "tprev", "dt", "active", "since", "next_out", "bad_y", "n_acc", "n_rej", "code", "min_r", "max_r",
                    "clip_t", "on_point", "jumped", "jump_hit", "step_cnt", "step_next", "jump_cnt", "jump_next")

    def repack(self, y, f0, n_keep: int):
        """Carry on with the `n_keep` active rows only, in their order: (y, f0) of those rows."""
        if self.row_map is None:
            self.row_map = np.arange(self.p.B)
            self.all_acc = np.zeros(self.p.B, dtype=np.int64)
            self.all_rej = np.zeros(self.p.B, dtype=np.int64)
        self.all_acc[self.row_map], self.all_rej[self.row_map] = self.n_acc, self.n_rej     # the rows that leave keep theirs
        keep = np.flatnonzero(self.active)
        assert len(keep) == n_keep
        for name in self._ROW_VECTORS:
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name)[keep])
        self.tg = self.tg[:, keep]
        for name in ("step_tab", "jump_tab"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name)[:, keep])
        self.row_map = self.row_map[keep]
        idx = torch.from_numpy(keep)
        if self.hook is not None:
            self.hook.keep_rows(idx)
        if self.s_shadow is not None:
            self.s_shadow = self.s_shadow[idx]
        if self.anchor is not None:
            self.anchor = self.anchor[idx]
        self.n = n_keep
        self.p.keep_rows(idx)
        return y[idx], f0[idx]

    # -- initial step ---------------------------------------------------------------------------------------------------
    def initial_step(self, y, f0) -> None:
        p, T = self.p, self.T
        self.t0[:] = p.tgrid[0].numpy()
        rtol, atol = p.tolerances()
        scale = atol + y.detach().abs() * rtol
        bad = (~torch.isfinite(y)).sum(dim=1).numpy()
        self.bad_y[:] = bad != 0
        if p.first_step is not None:
            self.dt[:] = p.first_step.numpy()
        else:
            s0, s1 = self._row_norms(y.detach() / scale), self._row_norms(f0.detach() / scale)
            h0 = np.empty(self.n, dtype=object)
            d1s = []
            with np.errstate(all="ignore"):
                for r in range(self.n):
                    d0, d1 = T(math.sqrt(s0[r] / p.L)), T(math.sqrt(s1[r] / p.L))
                    h = T(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
                    h0[r] = abs(h)
                    d1s.append(d1)
            c = torch.tensor([float(T(float(h) * p.sign)) for h in h0], dtype=p.dtype).reshape(-1, 1)
            shadow = None
            if p.record:
                shadow = rad.FirstStepShadow(_row_sum, y, f0, rtol, atol, p.sign)
                c = rad.stitch_rows(c, shadow.h0, p.sign)
            y1 = y + f0 * c
            t1 = torch.tensor([float(p.sign * T(self.t0[r] + float(h0[r]))) for r in range(self.n)], dtype=p.dtype)
            if shadow is not None:
                t1 = rad.stitch_rows(t1, shadow.h0, p.sign)
            f1 = p.call(t1, y1)
            s2 = self._row_norms((f1.detach() - f0.detach()) / scale)
            if shadow is not None:
                self.s_shadow = shadow.finish(f1, p.method.order - 1)
            order = p.method.order - 1
            with np.errstate(all="ignore"):
                for r in range(self.n):
                    hh, d1 = h0[r], d1s[r]
                    d2 = abs(T(math.sqrt(s2[r] / p.L)) / hh)
                    if d1 <= 1e-15 and d2 <= 1e-15:
                        h1 = max(T(1e-6), hh * 1e-3)
                    else:
                        h1 = power(rdiv(0.01, max(d1, d2)), 1.0 / float(order + 1))
                    h1 = abs(h1)
                    self.dt[r] = float(min(100 * hh, h1))
        for r in range(self.n):
            self.prepare(r)

    # -- trial step -----------------------------------------------------------------------------------------------------
    def trial_step(self, y, f0, sol):
        """One trial step of every active row; returns the (y, f0) of the next one (the same tensors, committed in
        place, unless the solve is recorded)."""
        p, m, T = self.p, self.p.method, self.T
        dts = self._dts_tensor([T(self.dt[r]) * T(p.sign) if self.active[r] else T(0) for r in range(self.n)])
        shadow, self.s_shadow = self.s_shadow, None          # only the first trial step's size carries a graph
        anchor = self.anchor
        if shadow is not None:
            dts = rad.stitch_rows(dts, shadow, p.sign)
        act = torch.from_numpy(self.active.copy()).reshape(-1, 1)
        times = rad.stage_times(self.times_tensor(), m.alpha, p.sign, shadow, anchor)
        ks = [f0]
        yi = None
        for i, row in enumerate(m.beta):
            yi = torch.where(act, y + self._sum_terms(ks, row, dts), y)
            ks.append(p.call(times[i], yi))
        y1 = yi if m.fsal else torch.where(act, y + self._sum_terms(ks, m.c_sol, dts), y)
        f1 = ks[-1]
        with torch.no_grad():                                # the controller is outside the graph
            err = self._sum_terms(ks, m.c_err, dts)
            rtol, atol = p.tolerances()
            tol = atol + rtol * torch.maximum(y.abs(), y1.abs())
            sums = self._row_norms(err / tol)
            bad = ((~torch.isfinite(y)) | (~torch.isfinite(y1))).sum(dim=1).numpy()
        accepted = []
        n_out = self.tg.shape[0]
        self.jumped[:] = False
        with np.errstate(all="ignore"):
            for r in range(self.n):
                if not self.active[r]:
                    continue
                ratio = float(T(math.sqrt(sums[r] / p.L)))
                dt = self.dt[r]
                # rk_common.py:324-332: the error decides, but a step above the ceiling is never taken and one at the
                # floor always
                accept = bool(dt <= self.min_r[r] or (ratio <= 1 and not dt > self.max_r[r]))
                dt_next = _clamp(optimal_step_size(dt, ratio, p.safety, p.ifactor, p.dfactor, m.order), self.min_r[r],
                                 self.max_r[r])
                self.since[r] += 1
                if accept:
                    on = self.on_point[r]
                    t1 = self.clip_t[r] if on else self.t0[r] + dt      # a cut step ends on the point's own bits
                    if on == 1 and self.step_next[r] != self.step_cnt[r] - 1:
                        self.step_next[r] += 1
                    if on == 2:
                        if self.impulse:
                            self.jump_hit[r] = self.jump_next[r]
                        if self.jump_next[r] != self.jump_cnt[r] - 1:
                            self.jump_next[r] += 1
                        self.jumped[r] = True
                    self.tprev[r], self.t0[r] = self.t0[r], t1
                    self.n_acc[r] += 1
                    lo = hi = int(self.next_out[r])
                    while hi < n_out and self.tg[hi, r] <= t1:
                        hi += 1
                    self.next_out[r] = hi
                    if hi > lo:
                        self.since[r] = 0
                    self.bad_y[r] = bad[r] != 0
                    accepted.append((r, lo, hi))
                    if hi >= n_out:
                        self.active[r] = False
                else:
                    self.n_rej[r] += 1
                self.dt[r] = dt_next
        if self.hook is not None:                            # between controller and commit: the commit overwrites y, f0
            self.hook.host_step(self, accepted, y, y1, f0, f1, ks, dts)
        if accepted:
            y, f0 = self._dense_commit(accepted, y, y1, f0, f1, ks, dts, sol, shadow, anchor)
        if shadow is not None and shadow.requires_grad:
            took = torch.zeros(self.n, dtype=torch.float64)
            took[[r for r, _, _ in accepted]] = 1.0
            self.anchor = shadow * took
        for r in range(self.n):
            if self.active[r]:
                self.prepare(r)
        stopped = _stopped_now(self.hook)
        if stopped is not None:
            self.active[stopped.numpy().astype(bool)] = False
        return y, f0

    @property
    def n_jumped(self) -> int:
        """The rows whose accepted step of the last trial step ended on a jump point."""
        return int(self.jumped.sum())

    def refresh_after_jump(self, y, f0):
        """f0 of the rows that jumped <- func just after the point (rk_common.py:352, Perturb.NEXT), one call for the
        carried batch: every other row is evaluated at its frozen time and its f0 keeps its bits.  With `jump_dy` the
        state of a row that jumped first takes the impulse of the point, y_r += dy[k, r] in the state's type, so that the
        call sees the state behind the point."""
        p, T = self.p, self.T
        if self.impulse:
            for r in np.flatnonzero(self.jumped):
                o = int(r if self.row_map is None else self.row_map[r])
                k = int(p.jump_points.index[self.jump_hit[r], o])
                if k >= 0:
                    y[r] += p.jump_dy[k, o if p.jump_dy.shape[1] > 1 else 0]
                self.n_imp[o] += 1
        t_rows = np.empty(self.n)
        for r in range(self.n):
            t0 = T(self.t0[r])
            t_rows[r] = float(T(p.sign) * (nextafter(t0, t0 + 1) if self.jumped[r] else t0))
        f_new = p.call(torch.tensor(t_rows, dtype=p.dtype), y)
        rows = torch.from_numpy(np.flatnonzero(self.jumped))
        f0[rows] = f_new[rows]
        return f0

    def impulse_counts(self) -> torch.Tensor:
        """`n_impulses`: the steps of each original row that ended on a jump point (int64 [B])."""
        return torch.zeros(self.p.B, dtype=torch.int64) if self.n_imp is None else torch.from_numpy(self.n_imp.copy())

    def deactivate_rows(self, mask: torch.Tensor) -> None:
        """Before the initial step: the rows of `mask` (bool [B]) never start."""
        self.active[mask.numpy()] = False

    def event_eval(self, out, q, x, mask) -> None:
        """out[r, :] = the quartic q[:, r] of a [5, B, L] tensor at x[r] for the rows with mask[r]."""
        idx = torch.nonzero(mask).view(-1)
        self.event_eval_mapped(out, idx, q, idx, x[idx])

    def _quartic_planes(self, idx, y, y1, f0, f1, ks, dts):
        """The quartic of the trial step just taken for the rows `idx` (int64 positions in the batch): its planes
        (e, d, c, b, a), [n, L] each — the one place the host states the coefficients (`tdeq_row_event_fit` on the device)."""
        p, m = self.p, self.p.method
        d = dts[idx]
        y0r, y1r, f0r, f1r = y[idx], y1[idx], f0[idx], f1[idx]
        kr = [k[idx] if k is not None else None for k in ks]
        ymid = y0r + self._sum_terms(kr, m.c_mid, d)
        two_dt = torch.tensor(2.0, dtype=p.dtype) * d
        qa = ((f1r - f0r) * two_dt - (y1r + y0r) * 8.0) + ymid * 16.0
        qb = (((f0r * 5.0 - f1r * 3.0) * d + y0r * 18.0) + y1r * 14.0) - ymid * 32.0
        qc = (((f1r - f0r * 4.0) * d - y0r * 11.0) - y1r * 5.0) + ymid * 16.0
        qd = f0r * d
        return y0r, qd, qc, qb, qa

    def step_quartic(self, idx, y, y1, f0, f1, ks, dts) -> torch.Tensor:
        """`_quartic_planes` as one tensor [5, n, L], as the hooks keep it."""
        return torch.stack(self._quartic_planes(idx, y, y1, f0, f1, ks, dts))

    @staticmethod
    def eval_quartics(q, src, x) -> torch.Tensor:
        """The quartics q[:, src[i], :] of a [5, rows, L] tensor at x[i] -> [n, L]."""
        e, d, c, b, a = q[:, src.to(torch.int64)].unbind(0)
        x1 = x[:, None]
        x2 = x1 * x1
        x3 = x2 * x1
        x4 = x3 * x1
        total = e + d * x1
        total = total + c * x2
        total = total + b * x3
        total = total + a * x4
        return total

    # -- calculus on a dense record (rowwise_dense.py; the arithmetic of tdeq_row_dense_prefix / tdeq_row_dense_calc) -----
    @staticmethod
    def _quartic_integral(e, d, c, b, a, x, h):
        """J_s(x) in fp64 (numpy float64 arrays, every product and sum rounded once); the whole segment is x = 1.0."""
        return (((((a * 0.2) * x + b * 0.25) * x + c * (1.0 / 3.0)) * x + d * 0.5) * x + e) * x * h

    @staticmethod
    def quartic_prefix(q, offsets, ta, tb) -> torch.Tensor:
        """The exclusive prefix of the whole-segment integrals of a record `q` [5, n_seg, L] -> fp64 [n_seg, L]: per row
        P[offsets[r]] = 0, P[s + 1] = P[s] + I_s, added left to right (step k of every row at once)."""
        planes = [v.numpy().astype(np.float64) for v in q.unbind(0)]
        h = (tb.numpy() - ta.numpy())[:, None]
        whole = HostRowKernels._quartic_integral(*planes, 1.0, h)
        P = np.zeros_like(whole)
        off = offsets.numpy()
        count = np.diff(off)
        for k in range(1, int(count.max()) if count.size else 0):
            at = off[:-1][count > k] + k
            P[at] = P[at - 1] + whole[at - 1]
        return torch.from_numpy(P)

    @staticmethod
    def quartic_derivatives(q, src, x, w) -> torch.Tensor:
        """d/dt of the quartics q[:, src[i], :] at x[i], in the state's type; `w[i]` = T(sign * (tb - ta)) -> [n, L]."""
        _, d, c, b, a = q[:, src.to(torch.int64)].unbind(0)
        x1 = x[:, None]
        total = d + (c + c) * x1
        xp = x1 * x1
        total = total + (b * 3) * xp
        xp = xp * x1
        total = total + (a * 4) * xp
        return total / w[:, None]

    @staticmethod
    def quartic_antiderivatives(q, prefix, ta, tb, sign: float, src, x, tq) -> torch.Tensor:
        """sign * (P[s] + J_s(x64)) for s = src[i], x64 = (tq[i] - ta[s]) / (tb[s] - ta[s]) in fp64 (NaN where the search
        marked the query out of range with x[i] = NaN) -> fp64 [n, L], not yet rounded to the state's type."""
        s = src.numpy().astype(np.int64)
        planes = [v.numpy().astype(np.float64) for v in q[:, torch.from_numpy(s)].unbind(0)]
        start, h = ta.numpy()[s], tb.numpy()[s] - ta.numpy()[s]
        with np.errstate(all="ignore"):
            x64 = np.where(np.isnan(x.numpy()), np.nan, (tq.numpy().reshape(-1) - start) / h)[:, None]
            total = sign * (prefix.numpy()[s] + HostRowKernels._quartic_integral(*planes, x64, h[:, None]))
        return torch.from_numpy(total)

    # -- the walk over a window of a dense record and the level machine on it, once for the four queries below --------------
    @staticmethod
    def _bisect(phi, lo, hi, on):
        """bisect(phi, lo, hi) of the header on fp64 arrays, where `on` -> (a root was found, the root): every round moves all
        the elements that still bisect."""
        lo, hi = lo.copy(), hi.copy()
        flo, fhi = phi(lo), phi(hi)
        nlo = flo < 0
        found = on & (flo != 0) & (fhi != 0) & (nlo != (fhi < 0))
        live = found.copy()
        for _ in range(64):
            if not live.any():
                break
            mid = 0.5 * (lo + hi)
            live &= (mid != lo) & (mid != hi)
            fm = phi(mid)
            hit = live & (fm == 0)                           # an exact zero is the root: both ends move onto it
            left = live & (hit | ((fm < 0) == nlo))
            right = live & (hit | ~left)
            lo, flo = np.where(left, mid, lo), np.where(left, fm, flo)
            hi, fhi = np.where(right, mid, hi), np.where(right, fm, fhi)
            live &= ~hit
        return found, np.where(np.abs(flo) <= np.abs(fhi), lo, hi)

    class _WindowStep:
        """Step k of the walk of every window that has one (WindowQuartic of the kernels): the windows `idx` on their k-th
        segment.  Coefficients, `xlo` and `xhi` are fp64 [len(idx), L]; the segment `t_a`, `t_b`, `h`, the window's ends
        `t_lo`, `t_hi` and `atA`, `atB` (this is the window's first / last segment) are [len(idx), 1]."""

        def __init__(self, idx, planes, t_a, t_b, atA, atB, t_lo, t_hi):
            self.idx, self.t_a, self.t_b, self.atA, self.atB, self.t_lo, self.t_hi = idx, t_a, t_b, atA, atB, t_lo, t_hi
            self.e, self.d, self.c, self.b, self.a = e, d, c, b, a = planes
            self.h = h = t_b - t_a
            self.xlo = np.broadcast_to(np.where(atA, (t_lo - t_a) / h, 0.0), e.shape)
            self.xhi = np.broadcast_to(np.where(atB, (t_hi - t_a) / h, 1.0), e.shape)
            c2, self.a4 = c + c, 4.0 * a
            b3, b6, a12, a4 = 3.0 * b, 6.0 * b, 12.0 * a, self.a4
            self.p = lambda v: e + v * (d + v * (c + v * (b + v * a)))
            self.g = lambda v: d + v * (c2 + v * (b3 + v * a4))
            self.g1 = lambda v: c2 + v * (b6 + v * a12)

        def time_of(self, z):
            """The time of the candidates `z`: a window's end and a breakpoint are the stored words."""
            return np.where(self.atA & (z == self.xlo), self.t_lo, np.where(self.atB & (z == self.xhi), self.t_hi, np.where(
                z == 0.0, self.t_a, np.where(z == 1.0, self.t_b, self.t_a + z * self.h))))

        def run(self, visit):
            """The isolation: `visit(v, on)` for the candidates in increasing x, `on` the elements that have this one."""
            bisect, xlo, xhi, g, g1 = HostRowKernels._bisect, self.xlo, self.xhi, self.g, self.g1
            every = np.ones(xlo.shape, dtype=bool)
            x1 = (-self.b) / self.a4
            xm = np.where((self.a != 0.0) & (xlo < x1) & (x1 < xhi), x1, xlo)
            f0, root = bisect(g1, xlo, xm, xm > xlo)
            r0 = np.where(f0, root, xlo)
            f1, root = bisect(g1, xm, xhi, every)
            r1 = np.where(f1, root, r0)
            visit(xlo, every)
            for lo, hi in ((xlo, r0), (r0, r1)):
                fz, z = bisect(g, lo, hi, hi > lo)
                visit(z, fz)
                visit(hi, hi > lo)
            fz, z = bisect(g, r1, xhi, every)
            visit(z, fz)
            visit(xhi, every)

    @staticmethod
    def _window_walk(q, ta, tb, src, x, tq, src2, x2, tq2):
        """The walk of the windows between the queries (src, x, tq) and (src2, x2, tq2) of the search over the record `q`
        [5, n_seg, L] (row_dense_walk of the kernels) -> (nan bool [n, L]: the windows with an out-of-range end, which are not
        walked; the later end of every window, fp64 [n, 1]; the `_WindowStep`s: step k of every window's walk at once)."""
        planes, start, end = q.numpy(), ta.numpy(), tb.numpy()
        sa, sb = src.numpy().astype(np.int64), src2.numpy().astype(np.int64)
        qa, qb = tq.numpy().reshape(-1), tq2.numpy().reshape(-1)
        swap = qb < qa
        sa, sb = np.where(swap, sb, sa), np.where(swap, sa, sb)
        qa, qb = np.where(swap, qb, qa), np.where(swap, qa, qb)
        bad = np.isnan(x.numpy()) | np.isnan(x2.numpy()) | (sa > sb)
        count = np.where(bad, 0, sb - sa + 1)

        def steps():
            with np.errstate(all="ignore"):
                for k in range(int(count.max()) if sa.size else 0):
                    idx = np.flatnonzero(count > k)
                    s = sa[idx] + k
                    yield HostRowKernels._WindowStep(
                        idx, [planes[p, s].astype(np.float64) for p in range(5)], start[s][:, None], end[s][:, None],
                        np.full((idx.size, 1), k == 0), (s == sb[idx])[:, None], qa[idx][:, None], qb[idx][:, None])
        return np.repeat(bad[:, None], planes.shape[2], axis=1), qb[:, None], steps()

    @staticmethod
    def _level_walk(q, level, window, cross=None, piece=None, timed=False):
        """The level machine on the walk of `window` (the arguments of `_window_walk` after `q`), for `level` [n_rows, L]
        (query i belongs to row i % n_rows), run under masks (row_dense_level_walk of the kernels) -> (nan bool [n, L]; with
        `timed` the time above the level, fp64 [n, L], else None).  `cross(s, on, tz, ab)`: the elements `on` of step `s` cross at the
        solver times `tz` and are above after it where `ab`.  `piece(s, on, area, over)`: a piece between two candidates,
        split at a crossing, adds `area` = K(v) - K(u) for the elements `on`, above the level where `over`; K is evaluated
        with a `piece` only."""
        H = HostRowKernels
        nan, t_hi, steps = H._window_walk(q, *window)
        n, L = nan.shape
        levels = level.numpy().astype(np.float64)[np.arange(n) % level.shape[0]]
        state, t_up, total = np.zeros((n, L), dtype=bool), np.zeros((n, L)), np.zeros((n, L))
        with np.errstate(all="ignore"):
            for s in steps:
                idx = s.idx
                lev = levels[idx]
                el = s.e - lev
                phi = lambda v: s.p(v) - lev                             # noqa: E731
                K = lambda v: H._quartic_integral(el, s.d, s.c, s.b, s.a, v, s.h)    # noqa: E731
                st, up, tot, nn = state[idx], t_up[idx], total[idx], nan[idx]
                entry = np.ones(st.shape, dtype=bool)                    # the segment's first candidate comes next
                u, fu, ku = s.xlo, np.zeros(st.shape), np.zeros(st.shape)

                def visit(v, on):
                    nonlocal st, up, tot, nn, entry, u, fu, ku
                    fv = phi(v)
                    nn = nn | (on & np.isnan(fv))
                    ab = fv > 0
                    opening = on & entry & s.atA                         # the window's first candidate sets the state
                    crossing = on & ~opening & (ab != st)
                    inside = crossing & ~entry                           # (else: a later segment's first candidate)
                    found, root = H._bisect(phi, u, v, inside & (fu != 0) & (fv != 0))
                    z = np.where(inside & (fu == 0), u, np.where(found, root, v))
                    tz = s.time_of(z)
                    if piece is not None:                                # u -> v, or u -> z under the old state and z -> v
                        kv = K(v)
                        kz = np.where(inside, K(z), ku)
                        piece(s, inside, kz - ku, st)
                        piece(s, on & ~entry, kv - kz, ab)
                        ku = np.where(on, kv, ku)
                    if cross is not None:
                        cross(s, crossing, tz, ab)
                    if timed:
                        tot = np.where(crossing & ~ab, tot + (tz - up), tot)
                        up = np.where(opening, s.t_lo, np.where(crossing & ab, tz, up))
                    st = np.where(opening | crossing, ab, st)
                    entry, u, fu = entry & ~on, np.where(on, v, u), np.where(on, fv, fu)

                s.run(visit)
                state[idx], t_up[idx], total[idx], nan[idx] = st, up, tot, nn
            return nan, np.where(state, total + (t_hi - t_up), total) if timed else None

    # -- queries over a window of a dense record (the arithmetic of tdeq_row_dense_extremum / _level / _level_times /
    #    _exposure, include/tdeq_hip.h) ---------------------------------------------------------------------------------------
    @staticmethod
    def quartic_extrema(q, ta, tb, sign: float, src, x, tq, src2, x2, tq2, maximum: bool):
        """The maximum (or minimum) of the record `q` [5, n_seg, L] on the windows between the queries (src, x, tq) and (src2,
        x2, tq2) of the search, per element, and its time -> (values [n, L] in the state's type, times fp64 [n, L] in true
        time).  Step k of every window's walk at once; the bisection rounds run under masks."""
        nan, _, steps = HostRowKernels._window_walk(q, ta, tb, src, x, tq, src2, x2, tq2)
        best, when, have = np.zeros(nan.shape), np.zeros(nan.shape), np.zeros(nan.shape, dtype=bool)
        with np.errstate(all="ignore"):
            for s in steps:
                idx = s.idx
                bst, whn, hv, nn = best[idx], when[idx], have[idx], nan[idx]

                def consider(v, on):
                    nonlocal bst, whn, hv, nn
                    p = s.p(v)
                    nn = nn | (on & np.isnan(p))
                    take = on & (~hv | ((p > bst) if maximum else (p < bst)))
                    bst, whn, hv = np.where(take, p, bst), np.where(take, s.time_of(v), whn), hv | on

                s.run(consider)
                best[idx], when[idx], have[idx], nan[idx] = bst, whn, hv, nn
            values = np.where(nan, np.nan, best).astype(q.numpy().dtype)
            times = np.where(nan, np.nan, sign * when)
        return torch.from_numpy(values), torch.from_numpy(times)

    @staticmethod
    def quartic_levels(q, level, ta, tb, sign: float, src, x, tq, src2, x2, tq2):
        """The crossings of `level` [n_rows, L] (query i belongs to row i % n_rows) by the record `q` [5, n_seg, L] on the
        windows between the queries (src, x, tq) and (src2, x2, tq2) of the search, per element -> (count int32, first, last
        fp64 in true time, time_above fp64), all [n, L].  Step k of every window's walk at once; the candidates are those of
        `quartic_extrema`, the state machine and the bisection rounds run under masks."""
        shape = (src.numel(), q.shape[2])
        first, last, count = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int32)

        def cross(s, on, tz, ab):
            i = s.idx
            first[i], last[i] = np.where(on & (count[i] == 0), tz, first[i]), np.where(on, tz, last[i])
            count[i] = count[i] + on.astype(np.int32)

        nan, total = HostRowKernels._level_walk(q, level, (ta, tb, src, x, tq, src2, x2, tq2), cross, timed=True)
        with np.errstate(all="ignore"):
            none = nan | (count == 0)
            count = np.where(nan, np.int32(-1), count).astype(np.int32)
            first, last = np.where(none, np.nan, sign * first), np.where(none, np.nan, sign * last)
            total = np.where(nan, np.nan, total)
        return tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in (count, first, last, total))

    @staticmethod
    def quartic_crossing_times(q, level, ta, tb, sign: float, max_count: int, src, x, tq, src2, x2, tq2):
        """The true times of the first `max_count` rising and falling crossings of `level` [n_rows, L] (query i belongs to row
        i % n_rows) by the record `q` [5, n_seg, L] on the windows between the queries (src, x, tq) and (src2, x2, tq2) of the
        search, per element, and the number of crossings of each direction -> (n_rising, n_falling int32 [n, L], rising,
        falling fp64 [max_count, n, L]).  `quartic_levels` with the lists filled under masks: a crossing of the walk goes to
        slot n of its direction's list while n < max_count, and the counter runs on; rising is meant in true time, so the two
        directions of the walk swap for `sign` < 0."""
        n, L, K = src.numel(), q.shape[2], int(max_count)
        n_up, n_dn = (np.zeros((n, L), dtype=np.int32) for _ in range(2))   # crossings of the walk: to above, to not above
        ups, dns = (np.full((K, n, L), np.nan) for _ in range(2))

        def cross(s, on, tz, ab):
            window = np.broadcast_to(s.idx[:, None], on.shape)
            column = np.broadcast_to(np.arange(L)[None, :], on.shape)
            for lst, total, to in ((ups, n_up, on & ab), (dns, n_dn, on & ~ab)):
                cnt = total[s.idx]
                keep = to & (cnt < K)
                lst[cnt[keep], window[keep], column[keep]] = sign * tz[keep]
                total[s.idx] = cnt + to.astype(np.int32)

        nan, _ = HostRowKernels._level_walk(q, level, (ta, tb, src, x, tq, src2, x2, tq2), cross)
        n_up, n_dn = np.where(nan, np.int32(-1), n_up).astype(np.int32), np.where(nan, np.int32(-1), n_dn).astype(np.int32)
        ups, dns = np.where(nan[None], np.nan, ups), np.where(nan[None], np.nan, dns)
        outs = (n_up, n_dn, ups, dns) if sign > 0 else (n_dn, n_up, dns, ups)
        return tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in outs)

    @staticmethod
    def quartic_exposure(q, level, ta, tb, sign: float, src, x, tq, src2, x2, tq2):
        """The area between the record `q` [5, n_seg, L] and `level` [n_rows, L] (query i belongs to row i % n_rows) above and
        below the level on the windows between the queries (src, x, tq) and (src2, x2, tq2) of the search, per element ->
        (area_above, area_below in the state's type, time_above fp64), all [n, L].  The walk and the state machine of
        `quartic_levels`; every piece between two candidates adds its K(v) - K(u) under a mask, split at a crossing.  `sign`
        changes nothing (durations)."""
        a_up, a_dn = (np.zeros((src.numel(), q.shape[2])) for _ in range(2))

        def piece(s, on, area, over):
            i = s.idx
            a_up[i], a_dn[i] = np.where(on & over, a_up[i] + area, a_up[i]), np.where(on & ~over, a_dn[i] - area, a_dn[i])

        nan, total = HostRowKernels._level_walk(q, level, (ta, tb, src, x, tq, src2, x2, tq2), piece=piece, timed=True)
        with np.errstate(all="ignore"):
            above = np.where(nan, np.nan, np.where(a_up < 0, 0.0, a_up)).astype(q.numpy().dtype)
            below = np.where(nan, np.nan, np.where(a_dn < 0, 0.0, a_dn)).astype(q.numpy().dtype)
            total = np.where(nan, np.nan, total)
        return tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in (above, below, total))

    def event_eval_mapped(self, out, dst, q, src, x) -> None:
        """out[dst[i] (None: i), :] = the quartic q[:, src[i]] at x[i], for the index lists `dst`, `src`."""
        if src.numel() == 0:
            return
        total = self.eval_quartics(q, src, x)
        if dst is None:
            out.copy_(total)
        else:
            out[dst.to(torch.int64)] = total

    def pack_quartics(self, coeffs, q, dest, used: int) -> None:
        """coeffs[:, dest[i]] = q[:, i] for the first `used` slots of a chunk of a dense solve."""
        coeffs[:, dest] = q[:, :used]

    def _dense_commit(self, accepted, y, y1, f0, f1, ks, dts, sol, shadow=None, anchor=None):
        p, T = self.p, self.T
        rows = torch.tensor([r for r, _, _ in accepted])
        with_out = [(i, r, lo, hi) for i, (r, lo, hi) in enumerate(accepted) if hi > lo]
        if with_out:
            idx = torch.tensor([r for _, r, _, _ in with_out])
            y0r, qd, qc, qb, qa = self._quartic_planes(idx, y, y1, f0, f1, ks, dts)
            for n, (_, r, lo, hi) in enumerate(with_out):
                ta, tb = self.tprev[r], self.t0[r]
                for j in range(lo, hi):
                    x = T((self.tg[j, r] - ta) / (tb - ta))
                    x2 = x * x
                    x3 = x2 * x
                    x4 = x3 * x
                    if shadow is None and anchor is None:
                        xs = (float(x), float(x2), float(x3), float(x4))
                    else:
                        # the step's ends carry the heuristic's graph, and with them theta = x (interp.py:39-40): the
                        # first step ends at t0 + dt_r (d x / d dt_r = -x / dt_r), a later one is shifted as a whole
                        # (d x / d anchor = -1 / width); the powers keep their T-rounded values
                        val = lambda v: torch.tensor(float(v), dtype=p.dtype)   # noqa: E731
                        moved = shadow[r] * float(x) if shadow is not None else anchor[r]
                        xt = rad.stitch_rows(val(x), moved * (-1.0 / (tb - ta)))
                        xs = (xt, rad.stitch_rows(val(x2), xt * xt), rad.stitch_rows(val(x3), xt * xt * xt),
                              rad.stitch_rows(val(x4), xt * xt * xt * xt))
                    # (not `eval_quartics`: the powers of x are host scalars here, graph scalars in a recorded solve)
                    total = y0r[n] + qd[n] * xs[0]
                    total = total + qc[n] * xs[1]
                    total = total + qb[n] * xs[2]
                    total = total + qa[n] * xs[3]
                    sol[j, r if self.row_map is None else self.row_map[r]] = total
        if p.record:
            mask = torch.zeros(self.n, 1, dtype=torch.bool)
            mask[rows] = True
            return torch.where(mask, y1, y), torch.where(mask, f1, f0)
        y[rows] = y1[rows]
        f0[rows] = f1[rows]
        return y, f0


class HipRowKernels:
    """The row operations of `odeint_rowwise` on the HIP kernels (csrc/tdeq_kernels_rowwise.hpp)."""

    def __init__(self, p: _Problem, hook=None):
        self.p = p
        self.hook = hook                                     # the step hook of an event or dense solve, else None
        self.k = _native.get_kernels(p.device, p.dtype)
        dev, B = p.device, p.B
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.t0 = p.tgrid[0].to(dev).clone()
        self.tprev = torch.zeros(B, **f64)
        self.dt = torch.zeros(B, **f64)
        self.h0 = torch.zeros(B, **f64)
        self.ratio = torch.zeros(B, **f64)
        self.tg = p.tgrid.to(dev)
        self.active = torch.ones(B, **i32)
        self.accepted = torch.zeros(B, **i32)
        self.out_lo = torch.zeros(B, **i32)
        self.out_hi = torch.zeros(B, **i32)
        self.next_out = torch.ones(B, **i32)
        self.since = torch.zeros(B, **i32)
        self.bad_y = torch.zeros(B, **i32)
        self.code = torch.zeros(B, **i32)
        self.n_acc = torch.zeros(B, dtype=torch.int64, device=dev)
        self.n_rej = torch.zeros(B, dtype=torch.int64, device=dev)
        # per-row bounds or points: the controller variant (`tdeq_row_control_points`), whose status has a third word
        self.impulse = p.jump_dy is not None and p.jump_points is not None
        self.n_imp = torch.zeros(B, dtype=torch.int64, device=dev) if self.impulse else None      # by original row
        self.pts = self._row_points(f64, i32) if (p.min_rows is not None or p.step_points is not None
                                                   or p.jump_points is not None) else None
        self.n_jumped = 0
        self.status = torch.zeros(2 if self.pts is None else 3, **i32)
        self.nch = self.k.row_partials(p.L, p.dtype)
        self.part = torch.empty(3 * B * self.nch, **f64)
        st = _native.RowState()
        for name in ("t0", "tprev", "dt", "h0", "active", "accepted", "out_lo", "out_hi", "next_out", "since", "bad_y",
                     "code", "n_acc", "n_rej", "ratio", "status"):
            setattr(st, name, getattr(self, name).data_ptr())
        st.tgrid = self.tg.data_ptr()
        st.n_rows, st.row_len, st.max_num_steps = B, p.L, p.max_num_steps
        st.n_out, st.order = self.tg.shape[0], p.method.order - 1
        self.st = st
        m = p.method
        # (scalar bounds ride in the block every controller launch takes; with per-row bounds these two are not read)
        lo, hi = (0.0, math.inf) if p.min_rows is not None else (p.min_step, p.max_step)
        self.ctrl = _native.step_ctrl(m.alpha, m.alpha_is_one, m.order, p.safety, p.ifactor, p.dfactor, lo, hi,
                                      p.sign, n_norm_seg=1)
        self.plan = launch_plan(m.name)
        self.dts = None
        self.times = None
        self.n = B                                           # rows now carried (fewer than p.B after a repack)
        self.row_map = None                                  # after a repack: their original indices, int32 on the device
        # a recorded solve (differentiable=True): every launch below is handed to the recorder and becomes a graph node
        self.rec = rad.RowRecorder(self.k, p, _row_sum) if p.record else None

    _POINT_VECTORS = ("step_count", "jump_count", "next_step", "next_jump", "clip_t", "on_point", "min_step", "max_step",
                      "jumped", "jump_hit")

    def _row_points(self, f64, i32) -> _native.RowPoints:
        """The vectors and tables of `tdeq_row_points` as attributes `pt_<field>` (None: absent), and the block."""
        p, B = self.p, self.p.B
        for kind, src in (("step", p.step_points), ("jump", p.jump_points)):
            for field, val, kw in ((f"{kind}_t", "table", f64), (f"{kind}_count", "count", i32), (f"next_{kind}", "next", i32)):
                setattr(self, "pt_" + field, None if src is None else torch.as_tensor(getattr(src, val), **kw).contiguous())
        self.pt_min_step = None if p.min_rows is None else torch.as_tensor(p.min_rows, **f64)
        self.pt_max_step = None if p.max_rows is None else torch.as_tensor(p.max_rows, **f64)
        self.pt_clip_t = torch.zeros(B, **f64)
        self.pt_on_point, self.pt_jumped = torch.zeros(B, **i32), torch.zeros(B, **i32)
        # impulses (`jump_dy`): the controller's IMPULSE variant — closed rule for the jump table, `jump_hit` — and what
        # `tdeq_row_impulse` reads besides: the index table by ORIGINAL row (a repack re-selects nothing of it or of jump_dy)
        self.pt_jump_hit = torch.zeros(B, **i32) if self.impulse else None
        if self.impulse:
            self.dy_index = torch.as_tensor(p.jump_points.index, **i32).contiguous()
        pts = _native.RowPoints()
        pts.jump_closed = 1 if self.impulse else 0
        pts.n_step = 0 if self.pt_step_t is None else self.pt_step_t.shape[0]
        pts.n_jump = 0 if self.pt_jump_t is None else self.pt_jump_t.shape[0]
        self._point_pointers(pts)
        return pts

    def _point_pointers(self, pts) -> None:
        for field in self._POINT_VECTORS + ("step_t", "jump_t"):
            vec = getattr(self, "pt_" + field)
            setattr(pts, field, None if vec is None else vec.data_ptr())

    def begin_recording(self, sol, y) -> None:
        self.rec.sol_rows = [y] + [None] * (sol.shape[0] - 1)

    def recorded_solution(self, sol) -> torch.Tensor:
        return torch.stack(self.rec.sol_rows)          # (each row is the raw solution row's storage: same bits)

    def poll(self):
        n_active, r, *more = self.status.tolist()            # the words the host reads per trial step: two, or three
        self.n_jumped = more[0] if more else 0               # (per-row bounds or points: the rows that jumped)
        # (a hook that stops rows: a row the controller found in error may have fired and left in the same trial step — its
        #  error wins.  Safe because every control launch (`tdeq_row_control`) first resets both words to {0, no error row},
        #  so status[1] can only name a row of THIS launch, never a stale one; pinned by
        #  tests/test_rowwise_event.py::test_max_num_steps_names_the_original_row)
        if r == _NO_ERROR_ROW or (n_active == 0 and _stopped_now(self.hook) is None):
            return n_active, None
        row = r if self.row_map is None else int(self.row_map[r])
        return n_active, (row, int(self.code[r]), int(self.since[r]), float(self.dt[r]), r)

    def counts(self):
        if self.row_map is None:
            return self.n_acc.cpu(), self.n_rej.cpu()
        self._park_counts()
        return self.all_acc.cpu(), self.all_rej.cpu()

    def _park_counts(self) -> None:
        rows = self.p.rows.to(self.all_acc.device)
        self.all_acc.index_copy_(0, rows, self.n_acc)
        self.all_rej.index_copy_(0, rows, self.n_rej)

    _ROW_VECTORS = ("t0", "tprev", "dt", "h0", "ratio", "active", "accepted", "out_lo", "out_hi", "next_out", "since",
                    "bad_y", "code", "n_acc", "n_rej")

    def repack(self, y, f0, n_keep: int):
        """Carry on with the `n_keep` active rows only, in their order: (y, f0) of those rows in fresh tensors (one
        gather launch), every per-row vector of the state, the running step sizes, stage times and output grid
        re-selected.  The workspace `part` and `status` keep their size; from here on the dense output goes through
        `row_map` (`tdeq_row_dense_commit_mapped`)."""
        p, st = self.p, self.st
        if self.row_map is None:
            self.all_acc, self.all_rej = torch.zeros_like(self.n_acc), torch.zeros_like(self.n_rej)
        self._park_counts()                                  # the rows that leave keep their counters
        keep = torch.nonzero(self.active).view(-1)           # ascending
        assert keep.numel() == n_keep
        y_new, f_new = y.new_empty(n_keep, p.L), f0.new_empty(n_keep, p.L)
        self.k.row_gather([y_new, f_new], [y, f0], keep.to(torch.int32))
        for name in self._ROW_VECTORS:
            vec = getattr(self, name).index_select(0, keep)
            setattr(self, name, vec)
            setattr(st, name, vec.data_ptr())
        self.tg = self.tg.index_select(1, keep)
        st.tgrid = self.tg.data_ptr()
        self.dts, self.times = self.dts.index_select(0, keep), self.times.index_select(1, keep)
        if self.pts is not None:
            for field in self._POINT_VECTORS:
                if getattr(self, "pt_" + field) is not None:
                    setattr(self, "pt_" + field, getattr(self, "pt_" + field).index_select(0, keep))
            for field in ("step_t", "jump_t"):
                if getattr(self, "pt_" + field) is not None:
                    setattr(self, "pt_" + field, getattr(self, "pt_" + field).index_select(1, keep).contiguous())
            self._point_pointers(self.pts)
        st.n_rows = self.n = n_keep
        if self.hook is not None:
            self.hook.keep_rows(keep)
        p.keep_rows(keep)
        self.row_map = p.rows.to(device=self.active.device, dtype=torch.int32)
        return y_new, f_new

    def _control(self, mode: int) -> None:
        p = self.p
        dts = torch.empty(self.n, dtype=p.dtype, device=p.device)
        times = torch.empty(p.method.n_stages, self.n, dtype=p.dtype, device=p.device)
        if self.pts is None:
            self.k.row_control(mode, self.part, self.ctrl, self.st, dts, times, p.dtype)
        else:
            # (mode 0 also writes the [n] times of the evaluation that follows a step onto a jump point)
            self.jump_times = torch.empty(self.n, dtype=p.dtype, device=p.device)
            self.pts.jump_times = self.jump_times.data_ptr()
            self.k.row_control_points(mode, self.part, self.ctrl, self.st, self.pts, dts, times, p.dtype)
        self.dts, self.times = dts, times

    def refresh_after_jump(self, y, f0):
        """f0 of the rows that jumped <- func just after the point, one call for the carried batch at the times the
        controller wrote; `tdeq_row_select` takes the rows that jumped and reads nothing of the others.  With `jump_dy`
        `tdeq_row_impulse` first adds the impulse of the point to the state of those rows, in place."""
        if self.impulse:
            self.k.row_impulse(y, self.p.jump_dy, self.dy_index, self.pt_jump_hit, self.pt_jumped, self.row_map)
        f_new = self.p.call(self.jump_times, y)
        self.k.row_select(f0, f_new, self.pt_jumped)
        if self.impulse:
            hit = self.pt_jumped.ne(0).to(torch.int64)
            if self.row_map is None:
                self.n_imp.add_(hit)
            else:
                self.n_imp.index_add_(0, self.row_map.to(torch.int64), hit)
        return f0

    def impulse_counts(self) -> torch.Tensor:
        """`n_impulses`: the steps of each original row that ended on a jump point (int64 [B])."""
        return torch.zeros(self.p.B, dtype=torch.int64) if self.n_imp is None else self.n_imp.cpu()

    def _reduce(self, mode: int, y0, y1, partial, ks, coefs, dts, active) -> None:
        """The row reduction into `part`: with the two scalar tolerances, or with the [n] vectors of the rows now carried
        (`_Problem.keep_rows` re-selects them at a repack)."""
        p = self.p
        if p.rtol_rows is None:
            self.k.row_reduce(mode, self.part, y0, y1, partial, ks, coefs, dts, active, p.rtol, p.atol)
        else:
            self.k.row_reduce_tol(mode, self.part, y0, y1, partial, ks, coefs, dts, active, p.rtol_rows, p.atol_rows)

    def initial_step(self, y, f0) -> None:
        p, k, rec = self.p, self.k, self.rec
        self._reduce(1, y, y, f0, [], [], None, None)
        if p.first_step is not None:
            self.dt.copy_(p.first_step.to(self.dt.device))
            self._control(3)
            return
        self._control(1)
        y1, t1 = torch.empty_like(y), self.times[0]
        k.row_combine([y1], (((1.0,), 1, True),), y, None, [f0], self.dts, self.active)
        if rec is not None:
            y1, t1 = rec.first_probe(y, f0, y1, self.dts, t1)
        f1 = p.call(t1, y1)
        self._reduce(2, y, f1, f0, [], [], None, None)
        self._control(2)
        if rec is not None:
            rec.first_step_size(f1)

    def trial_step(self, y, f0, sol):
        """One trial step of every active row; returns the (y, f0) of the next one (the same tensors, committed in
        place, unless the solve is recorded: then fresh graph tensors)."""
        p, m, k, plan, rec = self.p, self.p.method, self.k, self.plan, self.rec
        dts, times, act = self.dts, self.times.unbind(0), self.active
        if rec is not None:
            times = rec.begin_step(times)
        ks = [f0]
        held, R, S = {}, len(plan.ops), m.n_stages
        for i in range(R):
            op, row = plan.ops[i], m.beta[i] if i < S else m.c_sol
            if i == 0:                                       # row 0 is no part of a plan: one whole output
                yi = torch.empty_like(y)
                k.row_combine([yi], ((row.coef, (1 << len(row.idx)) - 1, True),), y, None, [ks[j] for j in row.idx],
                              dts, act)
            elif op is None:
                yi = held.pop(i)                             # finished by an earlier launch
            else:
                outs = [torch.empty_like(y) for _ in op.targets]
                k.row_combine(outs, op.spec, y, held.pop(i) if op.continues else None, [ks[j] for j in op.idx], dts, act)
                yi = outs[0]
                for tgt, buf in zip(op.targets[1:], outs[1:]):
                    held[tgt] = buf
            if rec is not None:
                yi = rec.stage(yi, y, ks, row, dts)
            if i < S:
                ks.append(p.call(times[i], yi))
        y1, f1, mid = yi, ks[-1], [ks[j] for j in m.c_mid.idx]
        # the error norm continues the partial error row of the last combine (none: the whole row), then the controller
        self._reduce(0, y, y1, held.pop(R, None), [ks[j] for j in plan.err_idx], plan.err_coef, dts, act)
        # dense output + commit y <- y1, f0 <- f1 of the accepted rows: in place, or, recorded, into fresh tensors (the
        # inputs stay alive for the backward)
        t_start = None if rec is None else self.t0.clone()
        self._control(0)
        if self.hook is not None:                            # between controller and commit: the commit overwrites y, f0
            self.hook.device_step(self, y, y1, f0, f1, mid, m.c_mid.coef, dts)
        y_to, f0_to = (y, f0) if rec is None else (y.detach().clone(), f0.detach().clone())
        if self.row_map is None:
            k.row_dense_commit(sol, y_to, y1, f0_to, f1, mid, m.c_mid.coef, dts, self.st)
        else:                                                # a compacted batch: y, f0 at the compact index, sol at the original
            k.row_dense_commit_mapped(sol, self.row_map, y_to, y1, f0_to, f1, mid, m.c_mid.coef, dts, self.st)
        if rec is None:
            return y, f0
        return rec.commit(self, sol, y, y1, f0, ks, dts, t_start, y_to, f0_to)

    def deactivate_rows(self, mask: torch.Tensor) -> None:
        """Before the initial step: the rows of `mask` (bool [B]) never start."""
        self.active.masked_fill_(mask, 0)

    def event_eval(self, out, q, x, mask) -> None:
        """out[r, :] = the quartic q[:, r] of a [5, B, L] tensor at x[r] for the rows with mask[r] (int32 [B])."""
        self.k.row_event_eval(out, q, x, mask)

    def event_eval_mapped(self, out, dst, q, src, x) -> None:
        """out[dst[i] (None: i), :] = the quartic q[:, src[i]] at x[i]; `dst`, `src` int32 [n] index lists."""
        self.k.row_event_eval_mapped(out, dst, q, src, x)

    def pack_quartics(self, coeffs, q, dest, used: int) -> None:
        """coeffs[:, dest[i]] = q[:, i] for the first `used` slots of a chunk of a dense solve."""
        self.k.row_dense_pack(coeffs, q, dest, used)


def _solve(p: _Problem, y_start, f0, sol, hook=None, never_start=None):
    """The one driver of the rowwise family, called under no_grad: chooses the backend, integrates every row to its last
    output time — or until `hook` stops it — and returns (the backend, n_accepted, n_rejected by original row).

    `y_start` [B, L]: the state at t0 (copied, unless the solve is recorded); `f0`: func there (`_Problem.first_call`), or
    None for a grid of one time — the backend is still chosen then, nothing is integrated and the counters are None.
    `never_start`: a bool [B] mask of rows that are not integrated at all."""
    if p.device.type == "cuda":
        kern = HipRowKernels(p, hook)
    else:
        _fallback.warn_once(f"the state lives on '{p.device}'")
        kern = HostRowKernels(p, hook)
    if f0 is None:
        return kern, None, None
    if never_start is not None:
        kern.deactivate_rows(never_start)
    # private state buffers: the dense-output launch commits y <- y1, f0 <- f1 in place
    y = y_start if p.record else y_start.clone()
    with p.grad_mode():
        if p.record:
            kern.begin_recording(sol, y)
        kern.initial_step(y, f0)
        while True:
            n_active, failure = kern.poll()
            if failure is not None:
                p.raise_row_error(failure, y)
            if p.jump_points is not None and kern.n_jumped:
                f0 = kern.refresh_after_jump(y, f0)          # a step ended on a jump point: f0 from its far side
            if n_active == 0:
                break
            if p.compact is not None and n_active < y.shape[0] and n_active <= p.compact * y.shape[0]:
                y, f0 = kern.repack(y, f0, n_active)
            if hook is not None:
                hook.before_step(n_active)
            y, f0 = kern.trial_step(y, f0, sol)
    if p.jump_dy is not None:
        p.n_impulses = kern.impulse_counts()
    return (kern, *kern.counts())


def _stats(p: _Problem, n_acc, n_rej) -> dict:
    """What every rowwise solve reports (`n_acc`, `n_rej` None: no step was taken)."""
    if n_acc is None:
        n_acc, n_rej = torch.zeros(p.B, dtype=torch.int64), torch.zeros(p.B, dtype=torch.int64)
    stats = {"n_accepted": n_acc.to(torch.int64), "n_rejected": n_rej.to(torch.int64), "nfe": p.nfe}
    if p.compact is not None:
        stats["row_evals"], stats["n_repacks"] = p.row_evals, p.n_repacks
    if p.jump_dy is not None:
        stats["n_impulses"] = torch.zeros(p.B, dtype=torch.int64) if p.n_impulses is None else p.n_impulses
    return stats


def odeint_rowwise(func, y0, t, *, rtol=1e-7, atol=1e-9, method="dopri5", options=None, return_stats=False,
                   event_fn=None, differentiable=False, compact=None):
    """Integrate B independent IVPs `dy_r/dt = func(t, y)[r]`, each row with its own adaptive step controller.

    `y0` is one tensor `[B, *row_shape]` (fp32 / fp64); row r is the IVP of `y0[r]`.  `t` is `[T]` (a grid shared by all
    rows) or `[T, B]` (a grid per row); every row strictly monotone, all in the same direction.

    `func(t_rows, y)` gets `t_rows`, a 1-D tensor `[B]` on y0's device in the state's dtype holding each row's stage time
    (rows see different times: `func` must broadcast it itself, e.g. `t_rows[:, None]`), and `y [B, *row_shape]`; it
    returns dy/dt of the same shape.  A row that has reached its last output time stays frozen at the end of its last
    accepted step and is still evaluated there; its output is ignored (NaN or Inf included).

    Methods: dopri5, bosh3, tsit5, fehlberg2, adaptive_heun, dopri8.  Options: `first_step` (scalar or `[B]`),
    `safety`, `ifactor`, `dfactor`, `max_num_steps` (per row), and the step options below.  Everything else raises
    ValueError.  Error norm per
    row: the RMS over the row's elements of err / (atol + rtol * max(|y0|, |y1|)) — `odeint`'s norm for a one-row
    state — and the reference's controller per row.

    Step options, the reference's row by row (rk_common.py:223-241, 266-361), quirks included.  `min_step`, `max_step`: a
    number, a 0-dim tensor or a real `[B]` vector in the forms of the tolerances (defaults 0 and inf, not validated): the
    bounds of `dt_r`; a step at the floor is always accepted, one above the ceiling never.  `step_t`, `jump_t`: real times
    `[K]` (shared) or `[K, B]` (a column per row) in TRUE time — a tensor on any device, a numpy array or a list; `K = 0`
    means absent, a NaN entry is padding.  Row r must end a step on each of its points: points before `t0_r` are dropped, a
    value that occurs twice in the row's two lists raises ValueError naming the row, a trial step that would pass the
    row's next point `p` (`t0 < p < t0 + dt`) is cut short and, accepted, ends at `p` exactly; a point hit exactly is not
    cut and the row's index stays on it.  After an accepted step onto a jump point `func` is called once more for the
    carried batch — `t_rows[r]` the next representable time behind the point for the rows that jumped, the frozen time of
    every other row — and `f0` of the rows that jumped is taken from it (the other rows' output is ignored, NaN included);
    `nfe` counts the call.  Row r has the bits and counts of the one-row solve with column r.  With `differentiable=True`
    and grad mode on any of the four raises NotImplementedError.

    `jump_dy`: state impulses at the jump points, entry for entry those of `jump_t` as the caller wrote it (before sorting
    and before points are dropped): `[K, B, *row_shape]` (an impulse per row) or `[K, *row_shape]` (shared; the two forms
    are told apart by `dim()` against `y0.dim()`), a tensor on any device, a numpy array or nested lists, converted to the
    state's dtype; real, and finite wherever the matching time is not NaN (the dy of a NaN time is ignored).  When row r's
    accepted step ends on `p = jump_t[k, r]`, `y_r <- y_r + jump_dy[k, r]` — one addition in the state's type, applied in
    the direction of integration (not negated for a descending grid) — and `f0_r` is then re-evaluated behind the point on
    the new state.  Output is LEFT-continuous: an output time equal to `p` holds the state before the impulse (the step
    that ends on `p` writes it), the first value after `p` includes it, and an impulse at a row's last output time is
    therefore not visible in the solution.  A point before `t0_r` is dropped with its impulse; a point equal to `t0_r`
    whose impulse is not all zero raises ValueError naming the row (no step ends there: add it to y0).  In a solve with
    `jump_dy` a jump point is stepped onto when `t0 < p <= t0 + dt` (closed: a step that lands on `p` exactly is a step
    onto it, or that dose and every later one of the row would be lost); `step_t`, and `jump_t` without `jump_dy`, keep
    the reference's open rule.  `stats` gains `n_impulses`, int64 `[B]` by original row: the steps that ended on a jump
    point.  `compact` is supported, bit for bit.  `jump_dy` without `jump_t` or with another K raises ValueError; with
    `differentiable=True` and grad mode on it raises NotImplementedError, as it does in `odeint_rowwise_event`.

    `rtol` and `atol` are each a number (or a one-element tensor), or a per-row vector with exactly `B = y0.shape[0]`
    entries: a 1-D tensor of any real dtype on any device, a 1-D numpy array, a list or a tuple of numbers.  Row r is then
    integrated with `rtol[r]`, `atol[r]`; if only one of the two is a vector the other is filled to `[B]`.  Row r of such a
    solve has the bits, the counts and the error behaviour of the one-row solve with the scalars `float(rtol[r])`,
    `float(atol[r])`, and constant vectors give the bits of the scalar solve (both backends, with `compact` and with
    `differentiable=True`).  A tolerance tensor is detached: no gradient flows to a tolerance.  Values are not validated,
    as scalars are not.  A vector of another length and a tensor of two or more dimensions raise ValueError: tolerances
    per element of a row (`[B, *row_shape]`, `[*row_shape]`) are not supported.

    Returns the solution `[T, *y0.shape]` with `solution[j, r]` = row r at `t[j]` (or `t[j, r]`); with
    `return_stats=True`, `(solution, stats)` where `stats` holds `n_accepted` and `n_rejected` (int64 `[B]`) and
    `nfe` (func calls for the whole batch).

    Gradients: by default none — with grad mode on and `y0`, `t` or a parameter of `func` requiring grad this raises
    NotImplementedError.  `differentiable=True` (with grad mode on) records the solve: the solution carries an autograd
    graph to `y0` and to every tensor `func` uses that requires grad, with the same forward bits, step counts and `nfe`
    as the default.  The controller (error norm, accept / reject, next dt_r) is outside the graph; a row's FIRST step
    size is inside it when it comes from the initial-step heuristic and outside it when `first_step` is given; `t_rows`
    is detached from `t` and carries only that first-step graph (as the reference's stage times do; none with
    `first_step`); a finished or rejected row sends an exactly-zero cotangent into `func`'s backward for that evaluation.
    Every trial step's stage tensors stay alive until the backward, so memory grows with the number of trial
    iterations.  Time gradients (`t.requires_grad`) and second-order gradients (`create_graph=True`) raise
    NotImplementedError; under `torch.no_grad()` the argument has no effect.

    `compact` (default None / False: off) takes the finished rows out of the batch instead of freezing them.  `True`
    means 0.5; a float c in (0, 1] is the threshold: after the initial step and after every trial step, with `cur` rows
    carried and `n_active` of them still active, `0 < n_active < cur` and `n_active <= c * cur` repacks the batch to the
    active rows, in ascending original order (c = 1.0: whenever a row finishes; c = 0.5: at most log2(B) times).  The
    solution, the per-row counters and the row named by an error message stay indexed by ORIGINAL row, and every bit of
    them is what the plain solve gives (as long as `func` treats rows independently).  With `compact` set `func` is
    called with a THIRD argument, `func(t_rows, y, rows)`: `rows` is an int64 `[b]` tensor on y0's device with the
    original indices of the rows of this call, ascending; `t_rows` is `[b]`, `y` and the return value `[b, *row_shape]`.
    Per-row parameters of `func` must be indexed with it (`k[rows]`).  Before the first repack `rows` is `arange(B)`;
    between repacks a finished row is still evaluated and ignored, after the next repack it is gone.  `nfe` stays the
    number of calls of `func`; `stats` gains `row_evals`, the sum of `y.shape[0]` over those calls, and `n_repacks`.
    Anything else for `compact` raises ValueError; with `differentiable=True` and grad mode on it raises
    NotImplementedError.
    """
    p = _Problem(func, y0, t, rtol, atol, method, options, event_fn, differentiable, compact)
    n_t = p.tgrid.shape[0]
    y_start = p.y0
    if p.record:
        # a private, aligned copy that carries y0's graph (the recorded solve never writes into a state tensor)
        y_start = p.y0_graph.clone(memory_format=torch.contiguous_format)
    f0 = p.first_call(y_start) if n_t > 1 else None
    with torch.no_grad(), device_guard(p.device):
        sol = torch.empty(n_t, p.B, p.L, dtype=p.dtype, device=p.device)
        sol[0].copy_(p.y0)
        kern, n_acc, n_rej = _solve(p, y_start, f0, sol)
        if p.record:
            with torch.enable_grad():
                sol = kern.recorded_solution(sol) if n_t > 1 else y_start[None]
                solution = rad.first_order_only(sol.view(n_t, *p.shape))
        else:
            solution = sol.view(n_t, *p.shape)
    return (solution, _stats(p, n_acc, n_rej)) if return_stats else solution
