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

    def __init__(self, row_sum, y, f0, rtol: float, atol: float, sign: float):
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
