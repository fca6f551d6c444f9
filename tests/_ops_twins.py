"""Plain-torch twins of the operations `torchdiffeq_amd.autodiff.Ops` records (tests/test_ops_autodiff.py).

Every function here is the reference's own expression of one operation — a Runge–Kutta stage combine, the fitted
quartic of `_interp_fit` + `_interp_evaluate`, the 3/8-rule stages, the Adams sums, the cubic Hermite interpolant —
written on fp64 (complex128) tensors and fp64 0-dim scalars, so `torch.autograd.grad` of a twin is the gradient the hand
calculus of autodiff.py has to reproduce.  None of them holds a per-tensor weight table: the weights of `dense_eval`
and of the Hermite basis only exist as what autograd derives from the expressions.

The absolute-value companion `S` of a twin is the SAME function called with `S=True` on the moduli of its inputs: every
subtraction becomes an addition and every constant its modulus, so each product is a product of moduli.  A twin is a
polynomial of its inputs; its companion is that polynomial with every coefficient replaced by its modulus, and so is
every derivative of the companion — `torch.autograd.grad` of `S` at (|inputs|, |grad_output|) is the companion of the
gradient, of any order.  That is the scale a rounding-error bound multiplies.

The one expression that is no polynomial is the Hermite fraction h = (t - t0) / (t1 - t0).  The tests choose times for
which both differences are exact, and the companion keeps their values (`_ExactDiff`, `_PosRecip`) while every
derivative of either takes its modulus.
"""
from __future__ import annotations

from typing import Sequence

import torch


def _sub(S: bool):
    return torch.add if S else torch.sub


def _c(v, S: bool):
    """A constant of the expression: itself, or its modulus in the companion."""
    if isinstance(v, (list, tuple)):
        return [abs(x) if S else x for x in v]
    return abs(v) if S else v


# -- Runge–Kutta stage combines (rk_common.py:79, 110-157) ---------------------------------------------------------------
def combine(y0, ks, cs, dt, S=False):
    """y0 + sum_j c_j dt k_j."""
    out = y0
    for k, c in zip(ks, _c(list(cs), S)):
        out = out + (c * dt) * k
    return out


def fixed_stage(mode, y0, ks, ws, dt, S=False):
    """mode 0: y0 + dt (k_0 w_0 + k_1 w_1 ...); mode 1: y0 + dt k_0 w_0."""
    ws = _c(list(ws), S)
    if mode == 1:
        return y0 + dt * ks[0] * ws[0]
    acc = None
    for k, w in zip(ks, ws):
        acc = k * w if acc is None else acc + k * w
    return y0 + dt * acc


def rk4_stage(stage, y0, k1, k2, k3, k4, dt, third, S=False):
    """The evaluation points and the increment of the 3/8 rule (rk_common.py:115-118); `third` = 1/3 in the state's type."""
    sub = _sub(S)
    if stage == 1:
        return y0 + dt * k1 * third
    if stage == 2:
        return y0 + dt * sub(k2, k1 * third)
    if stage == 3:
        return y0 + dt * (sub(k1, k2) + k3)
    return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def lerp(y0, y1, slope, S=False):
    return y0 + slope * _sub(S)(y1, y0)


def weighted_sum(xs, ws):
    """sum_m w_m x_m; a weight is a number or a 0-dim tensor (the companion gets moduli from its caller)."""
    acc = None
    for x, w in zip(xs, ws):
        acc = x * w if acc is None else acc + x * w
    return acc


# -- dense output (rk_common.py:363-369, interp.py:1-48) -----------------------------------------------------------------
def dense_eval(y0, y1, k: Sequence[torch.Tensor], mid_idx, mid_coef, dt, x, S=False):
    sub = _sub(S)
    f0, f1 = k[0], k[-1]
    acc = None
    for j, c in zip(mid_idx, _c(list(mid_coef), S)):
        acc = c * k[j] if acc is None else acc + c * k[j]
    y_mid = y0 + dt * acc
    a = sub(2 * dt * sub(f1, f0), 8 * (y1 + y0)) + 16 * y_mid
    b = sub(dt * sub(5 * f0, 3 * f1) + 18 * y0 + 14 * y1, 32 * y_mid)
    c = sub(sub(dt * sub(f1, 4 * f0), 11 * y0), 5 * y1) + 16 * y_mid
    d = dt * f0
    e = y0
    total = e + x * d
    x_power = x
    for coefficient in (c, b, a):
        x_power = x_power * x
        total = total + x_power * coefficient
    return total


# -- Adams–Bashforth–Moulton (fixed_adams.py:160-223) --------------------------------------------------------------------
def adams_predict(y0, hist, bash, moulton, dt, S=False):
    """(y0 + dy, dy, delta) with dy = sum_j bash_j dt f_j and delta = dt sum_j m_j f_j (`moulton` None: only y0 + dy)."""
    dy = None
    for f, b in zip(hist, _c(list(bash), S)):
        dy = (b * dt) * f if dy is None else dy + (b * dt) * f
    if moulton is None:
        return y0 + dy, None, None
    sm = None
    for f, m in zip(hist, _c(list(moulton), S)):
        sm = m * f if sm is None else sm + m * f
    return y0 + dy, dy, dt * sm


def adams_correct(y0, f, delta, m0, dt, S=False):
    """(y0 + dy, dy) with dy = m0 dt f + delta."""
    dy = (_c(m0, S) * dt) * f + delta
    return y0 + dy, dy


# -- cubic Hermite interpolant (solvers.py:166-173) ----------------------------------------------------------------------
class _ExactDiff(torch.autograd.Function):
    """a - b where the difference is exact: the companion keeps the value and takes |d/da| = |d/db| = 1."""

    @staticmethod
    def forward(ctx, a, b):
        return a - b

    @staticmethod
    def backward(ctx, g):
        return g, g


class _PosRecip(torch.autograd.Function):
    """1 / x with every derivative replaced by its modulus (d/dx = +1/x^2, and so on)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return 1 / x

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        r = _PosRecip.apply(x)
        return g * r * r


def hermite(t0, t1, t, y0, f0, y1, f1, sign, S=False):
    """solvers.py:166-173 with f0, f1 the raw outputs of a field integrated in the direction `sign` (their weights
    carry it).  In the companion the times are positive and their differences exact (module docstring)."""
    sub = _sub(S)
    if S:
        h = _ExactDiff.apply(t, t0) * _PosRecip.apply(_ExactDiff.apply(t1, t0))
        dt = _ExactDiff.apply(t1, t0)
    else:
        h = (t - t0) / (t1 - t0)
        dt = t1 - t0
    sign = _c(sign, S)
    h00 = (1 + 2 * h) * sub(1, h) * sub(1, h)
    h10 = h * sub(1, h) * sub(1, h)
    h01 = h * h * sub(3, 2 * h)
    h11 = h * h * sub(h, 1)
    return h00 * y0 + h10 * dt * sign * f0 + h01 * y1 + h11 * dt * sign * f1
