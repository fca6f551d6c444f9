"""Backprop through `odeint_rowwise(..., differentiable=True)`: the rowwise section of autodiff.py.

Every state-sized operation of a rowwise trial step is linear in its state-sized inputs with one weight PER ROW,

    out[r, :] = sum_m w_m[r] X_m[r, :],

so one `torch.autograd.Function` (`_RowLinearOp`) serves all of them, as `autodiff._LinearOp` does for the whole-batch
kernels.  The forward value is the output of the SAME `tdeq_row_*` launch as in no-grad mode (the node is handed the
finished tensor); the backward is

    grad X_m[r, :] = w_m[r] g[r, :]                      `tdeq_row_scale_many` (g read once; weights that are exactly 0
                                                          for all rows are skipped, exactly 1 for all rows pass g on)
    grad s_r = sum_m dw_m/ds[r] <g[r, :], X_m[r, :]>     `tdeq_row_multi_dot` (first trial step, dense-output nodes)

with s_r the row's first step size when it comes from the initial-step heuristic — the one step size the reference
differentiates.  The controller (error norm, accept / reject, next dt_r) is outside the graph.  Because the later step
sizes are constants, the end of an accepted first step, t0 + dt_r, is the time every later step of the row is anchored
to: the reference's t0 / t1 carry that graph into the stage times handed to func and into the dense output's theta, and
so do `t_rows` and the dense-output nodes here (`anchor`; d theta / d anchor = -1 / step width).  With `first_step`
given there is no such graph and no node has a scalar input.

Node types and their weights (dts[r] = sign * T(dt_r), 0 for a finished row):
  stage input / y1   y + sum_j w_j k_j          w_y = 1,  w_j[r] = fl_T(fl_T(a_j) * dts[r])
  commit             m y1 + (1 - m) y           m[r] = 1 for an accepted trial step, else 0 (same for f0 <- f1)
  dense output       sol[j] = the quartic of the row's accepted step at theta_jr, linear in (y0, y1, f0, f1, k_mid);
                     weights zero for the rows whose step does not contain output time j
A rejected or finished row gets an exactly-zero cotangent through the commit mask.

`RowRecorder` holds everything only a recorded device solve needs (the first-step and anchor graphs, the solution rows'
graph tensors, the tableau-only slot map of the dense-output node) and turns the launches `rowwise.HipRowKernels` hands
it into these nodes; `stage_times` is the one rule, shared with the host backend, for the graph the stage times carry.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

Weight = Union[float, torch.Tensor]      # 0.0 / 1.0 (the same for every row) or a [B] tensor in the state dtype

_SECOND_ORDER = ("odeint_rowwise(differentiable=True) does not support second-order gradients (a backward pass that is "
                 "itself recorded, create_graph=True); use odeint for those")


class _RowSpec:
    __slots__ = ("kernels", "out", "w", "dw")

    def __init__(self, kernels, out, w, dw=None):
        self.kernels = kernels      # HipKernels
        self.out = out              # the finished forward value [B, L]
        self.w = w                  # [M] weights of the state-sized inputs
        self.dw = dw                # [M] d w_m / d s (float or fp64 [B]) when the node has the per-row scalar s


class _RowLinearOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec: _RowSpec, s: Optional[torch.Tensor], *xs):
        ctx.spec = spec
        ctx.need_s = s is not None and ctx.needs_input_grad[1]
        if ctx.need_s:
            ctx.s_dtype = s.dtype
            ctx.save_for_backward(*xs)
        return spec.out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise NotImplementedError(_SECOND_ORDER)
        spec = ctx.spec
        kern = spec.kernels
        g = g.contiguous()
        if g.data_ptr() % 16:
            g = g.clone(memory_format=torch.contiguous_format)
        need_x = ctx.needs_input_grad[2:]
        grads: List[Optional[torch.Tensor]] = [None] * len(spec.w)
        outs, ws = [], []
        for m, (w, need) in enumerate(zip(spec.w, need_x)):
            if not need:
                continue
            if isinstance(w, float):      # the same weight for every row: exactly 0 (skipped) or exactly 1 (g passes)
                if w == 1.0:
                    grads[m] = g
                continue
            grads[m] = torch.empty_like(g)
            outs.append(grads[m])
            ws.append(w)
        for lo in range(0, len(outs), 14):                       # TDEQ_MAX_TERMS outputs per launch
            kern.row_scale_many(outs[lo:lo + 14], g, torch.stack(ws[lo:lo + 14]).contiguous())
        grad_s = None
        if ctx.need_s:
            xs = ctx.saved_tensors
            live = [m for m, d in enumerate(spec.dw) if not (isinstance(d, float) and d == 0.0)]
            for lo in range(0, len(live), 14):
                part = live[lo:lo + 14]
                dots = kern.row_multi_dot(g, [xs[m] for m in part])
                for q, m in enumerate(part):                      # (added in input order, elementwise over the rows)
                    term = dots[q] * spec.dw[m]
                    grad_s = term if grad_s is None else grad_s + term
            if grad_s is not None:
                grad_s = grad_s.to(ctx.s_dtype)
        return (None, grad_s, *grads)


def row_linear(kernels, out: torch.Tensor, xs: Sequence[torch.Tensor], w: Sequence[Weight], s=None, dw=None):
    """`out` (finished, detached) as the value of one graph node over `xs` with per-row weights `w`."""
    with torch.enable_grad():          # (the solver's loop runs under no_grad: the controller is outside the graph)
        return _RowLinearOp.apply(_RowSpec(kernels, out, list(w), None if s is None else list(dw)), s, *xs)


class _StitchRows(torch.autograd.Function):
    """forward: `value`; backward: the gradient goes to `shadow` (same shape, cast to its dtype)."""

    @staticmethod
    def forward(ctx, shadow, value):
        ctx.shadow_dtype = shadow.dtype
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.shadow_dtype), None


def stitch_rows(value: torch.Tensor, shadow: Optional[torch.Tensor], scale: float = 1.0) -> torch.Tensor:
    """`value` with the gradient of `scale * shadow` (the solver's loop runs under no_grad: grad mode is set here)."""
    if shadow is None or not shadow.requires_grad:
        return value
    with torch.enable_grad():
        return _StitchRows.apply((shadow * scale).reshape(value.shape), value)


class _FirstOrderOnly(torch.autograd.Function):
    """Identity on the returned solution that refuses a recorded backward on either backend."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise NotImplementedError(_SECOND_ORDER)
        return g


def first_order_only(x: torch.Tensor) -> torch.Tensor:
    return _FirstOrderOnly.apply(x) if x.requires_grad else x


def dense_weights(x: torch.Tensor, d: torch.Tensor, mid_coef: Sequence[float]):
    """Weights of the quartic dense output (interp.py:17-21, 42-47 expanded) at the per-row abscissa `x` with the signed
    step `d`, both fp64 [B]: (w_y0, w_y1, w_f0, w_f1, [w_mid_j]) and their derivatives with respect to x and d."""
    x2, x3, x4 = x * x, x * x * x, x * x * x * x
    p_f0, dp_f0 = x - 4 * x2 + 5 * x3 - 2 * x4, 1 - 8 * x + 15 * x2 - 8 * x3
    p_f1, dp_f1 = x2 - 3 * x3 + 2 * x4, 2 * x - 9 * x2 + 8 * x3
    p_m, dp_m = 16 * x2 - 32 * x3 + 16 * x4, 32 * x - 96 * x2 + 64 * x3
    w_y1, dw_y1 = -5 * x2 + 14 * x3 - 8 * x4, -10 * x + 42 * x2 - 32 * x3
    zero = torch.zeros_like(x)
    w = [1 - w_y1, w_y1, d * p_f0, d * p_f1] + [c * d * p_m for c in mid_coef]
    dwx = [-dw_y1, dw_y1, d * dp_f0, d * dp_f1] + [c * d * dp_m for c in mid_coef]
    dwd = [zero, zero, p_f0, p_f1] + [c * p_m for c in mid_coef]
    return w, dwx, dwd


class FirstStepShadow:
    """Per-row analogue of `solvers._InitialStepShadow`: the initial-step heuristic (misc.py:36-77) recorded with torch
    ops on per-row quantities, beside the values the backend computed.  The branches are taken from the shadow's own
    norms.  `row_sum` is the backend-independent fixed-order row sum, so that a row's graph does not depend on B."""

    def __init__(self, row_sum, y, f0, rtol, atol, sign: float):
        # rtol, atol: two floats, or the [B, 1] columns of per-row tolerances (`rowwise._Problem.tolerances`)
        self.row_sum, self.sign = row_sum, sign
        self.f0 = f0
        self.L = y.shape[1]
        self.scale = atol + y.abs() * rtol
        self.d0, ok0 = self._norm(y / self.scale)
        self.d1, ok1 = self._norm(f0 / self.scale)
        self.const = (self.d0.detach() < 1e-5) | (self.d1.detach() < 1e-5) | ~ok0 | ~ok1
        one = torch.ones_like(self.d1)
        h0 = (0.01 * self.d0 / torch.where(self.const, one, self.d1)).abs()
        self.h0 = torch.where(self.const, torch.full_like(h0, 1e-6), h0)       # [B], fp64

    def _norm(self, q):
        """(sqrt(mean(q^2)) per row in fp64, the rows where it is differentiable)."""
        ms = self.row_sum(q.double() ** 2) / self.L
        ok = ms.detach() > 0
        return torch.where(ok, ms, torch.ones_like(ms)).sqrt() * ok.to(ms.dtype), ok

    def finish(self, f1, order: int):
        """The [B] fp64 shadow of dt_r = min(100 h0, h1) (its VALUE is not used, only its graph)."""
        d2n, ok2 = self._norm((f1 - self.f0) / self.scale)
        d2 = (d2n / self.h0).abs()
        d1 = self.d1
        floor = (d1.detach() <= 1e-15) & (d2.detach() <= 1e-15)
        d1_is_max = ~(d2.detach() > d1.detach())
        m = torch.where(d1_is_max, d1, d2)
        m = torch.where(floor, torch.ones_like(m), m)
        h1 = torch.where(floor, self.h0 * 1e-3, (0.01 / m) ** (1.0 / float(order + 1))).abs()
        big = 100 * self.h0
        return torch.where(h1.detach() < big.detach(), h1, big)


def stage_times(times, alpha, sign: float, shadow, anchor):
    """The stage times handed to func with the graph they carry: the first trial step's t0 + alpha_i dt_r (`shadow`,
    the row's first step size), a later step's anchor (it is shifted as a whole); plain values without either."""
    if shadow is not None:
        return [stitch_rows(tt, shadow, sign * float(a)) for tt, a in zip(times, alpha)]
    if anchor is not None:
        return [stitch_rows(tt, anchor, sign) for tt in times]
    return times


class RowRecorder:
    """What only a recorded solve on the HIP kernels needs: every launch of `rowwise.HipRowKernels` handed to it becomes
    one `_RowLinearOp` node over the launch's finished output.  It holds the kernels object and the problem, never the
    backend: that owns the recorder, and a cycle would keep the whole recorded graph alive until the cyclic collector
    runs; `commit` is handed the backend (`rows`: its per-row device vectors are read, never written) per call.  The
    solve runs in grad mode (`rowwise._Problem.grad_mode`)."""

    def __init__(self, kernels, problem, row_sum):
        self.k, self.p, self.row_sum = kernels, problem, row_sum
        self.first = None             # FirstStepShadow between the two halves of the initial-step heuristic
        self.s_shadow = None          # [B] fp64 graph of the first step sizes (initial-step heuristic)
        self.shadow = None            # ... while the first trial step runs (only that step's size carries a graph)
        self.anchor = None            # [B] fp64 graph of the time the later steps of a row are anchored to
        self.sol_rows = None          # graph tensors of the solution rows (each the raw row's storage)
        self._coef_t = {}
        # which of (y0, y1, f0 = k_0, f1 = k_S, k_mid...) share an input of the dense-output node: f0 and f1 usually
        # carry a mid weight too.  slot of every c_mid term, and the stages behind the slots from 2 on
        m = self.p.method
        slots = {0: 2, m.n_stages: 3}
        for j in m.c_mid.idx:
            slots.setdefault(j, len(slots) + 2)
        self.mid_slot, self.dense_stages = [slots[j] for j in m.c_mid.idx], list(slots)

    def _coefs(self, row) -> torch.Tensor:
        c = self._coef_t.get(id(row))
        if c is None:
            c = self._coef_t[id(row)] = torch.tensor(row.coef, dtype=self.p.dtype, device=self.p.device)[:, None]
        return c

    def first_probe(self, y, f0, y1, dts, t1):
        """(y1, t1) of the initial-step heuristic's probe y1 = y + h0 f0 at t1 = t0 + h0, as graph tensors."""
        p = self.p
        self.first = FirstStepShadow(self.row_sum, y, f0, *p.tolerances(), p.sign)
        return (row_linear(self.k, y1, [y, f0], [1.0, dts], s=self.first.h0, dw=[0.0, p.sign]),
                stitch_rows(t1, self.first.h0, p.sign))

    def first_step_size(self, f1) -> None:
        self.s_shadow, self.first = self.first.finish(f1, self.p.method.order - 1), None

    def begin_step(self, times):
        """The stage times of this trial step as func gets them."""
        self.shadow, self.s_shadow = self.s_shadow, None
        if self.shadow is not None and not self.shadow.requires_grad:
            self.shadow = None
        return stage_times(times, self.p.method.alpha, self.p.sign, self.shadow, self.anchor)

    def stage(self, raw, y, ks, row, dts):
        """`raw` = y + sum_j fl_T(fl_T(a_j) dts[r]) k_j over the whole tableau row, as one graph node (the carried
        partial sums of the launch are an implementation detail of the forward)."""
        w = (self._coefs(row) * dts[None, :]).unbind(0)          # T products: the kernel's own coefficients
        xs = [y] + [ks[j] for j in row.idx]
        if self.shadow is None:
            return row_linear(self.k, raw, xs, [1.0, *w])
        dw = [0.0] + [float(c) * self.p.sign for c in self._coefs(row)[:, 0].tolist()]
        return row_linear(self.k, raw, xs, [1.0, *w], s=self.shadow, dw=dw)

    def commit(self, rows, sol, y, y1, f0, ks, step_dts, t_start, y_new, f0_new):
        """Graph of the dense output + commit launch that just ran on the fresh (y_new, f0_new); returns them as the
        graph tensors of the next trial step's (y, f0)."""
        p, m = self.p, self.p.method
        shadow, anchor = self.shadow, self.anchor
        acc, lo, hi = rows.accepted != 0, rows.out_lo, rows.out_hi
        hit = acc & (hi > lo)
        n_acc, j_lo, j_hi = torch.stack([acc.sum(), torch.where(hit, lo, torch.iinfo(torch.int32).max).min().long(),
                                         torch.where(hit, hi, 0).max().long()]).tolist()
        if j_hi > j_lo:
            d = step_dts.double()
            width = torch.where(hit, rows.t0 - t_start, torch.ones_like(rows.t0))
            cmid = self._coefs(m.c_mid)[:, 0].double().tolist()
            for j in range(j_lo, j_hi):
                mask = hit & (lo <= j) & (hi > j)
                # theta as the kernel forms it: in the time type, then rounded to T (interp.py:39-40)
                x = torch.where(mask, ((rows.tg[j] - t_start) / width).to(p.dtype).double(), torch.zeros_like(width))
                parts = dense_weights(x, d, cmid)                   # (w, dw/dx, dw/dd) per input
                merged = [list(v[:4]) for v in parts]
                for q, slot in enumerate(self.mid_slot):
                    for lst, src in zip(merged, parts):
                        if slot < 4:
                            lst[slot] = lst[slot] + src[4 + q]
                        else:
                            lst.append(src[4 + q])
                md = mask.double()
                xs = [y, y1] + [ks[jj] for jj in self.dense_stages]
                ws = [(v * md).to(p.dtype) for v in merged[0]]
                prev = self.sol_rows[j]
                if prev is not None:
                    # `prev` and the new node's value are both the storage of sol[j], which later launches rewrite
                    # behind autograd's back: safe only because the chained input has weight 1 and dw = 0, so its
                    # VALUE is never read in a backward (g passes through, no dot is taken with it)
                    xs, ws = [prev] + xs, [1.0] + ws
                if shadow is None and anchor is None:
                    self.sol_rows[j] = row_linear(self.k, sol[j], xs, ws)
                    continue
                if shadow is not None:
                    # the first step: weights depend on dt_r directly (d = sign dt_r) and through theta (-x / dt_r)
                    dw = [(dd * p.sign - dx * x / width) * md for dx, dd in zip(merged[1], merged[2])]
                else:
                    # a later step is shifted as a whole with the row's anchor: d theta / d anchor = -1 / width
                    dw = [-dx / width * md for dx in merged[1]]
                if prev is not None:
                    dw = [0.0] + dw
                self.sol_rows[j] = row_linear(self.k, sol[j], xs, ws, s=shadow if shadow is not None else anchor, dw=dw)
        if shadow is not None:
            self.anchor = shadow * acc.double()
        if n_acc == 0:
            return y, f0
        if n_acc == p.B:
            wm = [1.0, 0.0]
        else:
            mt = acc.to(p.dtype)
            wm = [mt, 1 - mt]
        return row_linear(self.k, y_new, [y1, y], wm), row_linear(self.k, f0_new, [ks[-1], f0], wm)
