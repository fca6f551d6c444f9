"""CPU restatement of the reference's Runge–Kutta step arithmetic for bfloat16 / float16 STATES.

TEST INFRASTRUCTURE ONLY (like rk_oracle.c): the parity oracle of torchdiffeq_amd/csrc/tdeq_kernels_lp.hpp.  Only tests/
may import it; the product never does.

The reference integrates a reduced-precision state with ordinary ATen ops on tensors of that type (every time-like
scalar is cast to `y0.abs().dtype`: torchdiffeq/_impl/rk_common.py:61-65, misc.py:185-187), so the restatement IS the
reference's own torch expressions, evaluated by ATen's CPU kernels on bf16 / fp16 tensors — each function cites the lines
it repeats (paths relative to torchdiffeq/_impl/).  Two deliberate differences, the same the fp32 / fp64 oracle has
(docs/LAB_NOTEBOOK.md §8): a tableau row is summed over its NON-ZERO weights, left to right (`_row_sum`: products rounded to the
state's type, accumulated in float32, rounded once — what `torch.sum(k * c, dim=-1)` does for a reduced-precision
tensor, with the order fixed), and norms are reported as fp64 sums of the rounded squares.

Pinning: tests/test_lowp_oracle.py checks these functions against vectors the imported reference produced on bf16 / fp16
inputs (tests/golden/make_golden_lowp.py -> tests/golden/lowp_kernels.npz).
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch


def _t(x: float, dtype) -> torch.Tensor:
    """A host number as the reference holds it next to a state of `dtype`: a 0-dim tensor of that type."""
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32).to(dtype)


def _row_sum(ks: Sequence[torch.Tensor], coefs: Sequence[float], dt: float) -> torch.Tensor:
    """`torch.sum(k[..., :n] * (beta_i * dt), dim=-1)` (rk_common.py:79, 89, 366) over the non-zero weights: the
    tableau row is cast to the state's type (rk_common.py:201-205), `beta_i * dt` is a product of two tensors of that
    type, `k * c` rounds every product, the sum accumulates them in float32 and rounds once."""
    dtype = ks[0].dtype
    dtT = _t(dt, dtype)
    acc = None
    for k, c in zip(ks, coefs):
        cT = _t(c, dtype) * dtT                       # fl_T(fl_T(c) * fl_T(dt))
        p = (k * cT).float()                          # the rounded product, widened exactly
        acc = p if acc is None else acc + p           # float32 accumulation, left to right
    return acc.to(dtype)


def stage_combine(y0, ks, coefs, dt):
    """yi = y0 + sum(k * (beta_i * dt))        rk_common.py:79 (and :83-85; misc.py:65 with one term)"""
    return y0 + _row_sum(ks, coefs, dt)


def stage_combine_err(y0, ks, coefs, err_coefs, dt):
    """(y1, the error row over the same stages)        rk_common.py:79 / :89"""
    return y0 + _row_sum(ks, coefs, dt), _row_sum(ks, err_coefs, dt)


def error_quotient(y0, y1, ks, coefs, dt, rtol, atol):
    """y1_error / (atol + rtol * max(|y0|, |y1|))        rk_common.py:89, misc.py:80-82.  rtol / atol are 0-dim tensors
    (rk_common.py:186-187) and FIRST operands here: ATen casts them to the state's type."""
    err = _row_sum(ks, coefs, dt)
    dtype = y0.dtype
    tol = _t(atol, dtype) + _t(rtol, dtype) * torch.max(y0.abs(), y1.abs())
    return err / tol


def norm_terms(q) -> Tuple[float, float]:
    """(sum of fl(|q|^2), sum of |q|) in fp64: the terms of `sqrt(mean(|x|^2))` (misc.py:22-23) before the mean."""
    a = q.abs()
    return float(a.pow(2).double().sum()), float(a.double().sum())


def init_quotients(mode, a, b, y, rtol, atol):
    """misc.py:50-66: scale = atol + |y0| * rtol with rtol the SECOND operand (a 0-dim fp64 tensor next to a
    reduced-precision tensor: ATen's CPU kernel takes it at float32), atol cast to the state's type;
    mode 0: (y0 / scale, f0 / scale); mode 1: (f1 - f0) / scale."""
    rt, at = torch.tensor(float(rtol), dtype=torch.float64), _t(atol, y.dtype)
    scale = at + y.abs() * rt
    assert scale.dtype == y.dtype
    if mode == 0:
        return a / scale, b / scale
    return (a - b) / scale, None


def quartic(y0, y1, f0, f1, ks, coefs, dt):
    """rk_common.py:363-369 + interp.py:17-21, literally, with dt a 0-dim tensor of the state's type."""
    dtype = y0.dtype
    dtT = _t(dt, dtype)
    y_mid = y0 + _row_sum(ks, coefs, dt)
    a = 2 * dtT * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dtT * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dtT * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    d = dtT * f0
    e = y0
    return [e, d, c, b, a]


def dense_eval(y0, y1, f0, f1, ks, coefs, dt, x):
    """interp.py:38-48: x cast to the state's type, `total = coefficients[0] + x * coefficients[1]`, then
    `x_power = x_power * x; total = total + x_power * coefficient` for the rest."""
    co = quartic(y0, y1, f0, f1, ks, coefs, dt)
    xT = _t(x, y0.dtype)
    total = co[0] + xT * co[1]
    x_power = xT
    for coefficient in co[2:]:
        x_power = x_power * xT
        total = total + x_power * coefficient
    return total


def _time(x: float) -> torch.Tensor:
    """A time-like scalar of a FIXED-GRID solver: a 0-dim tensor in `t.dtype` (solvers.py:102-128 never casts the grid
    to the state's type) — next to a reduced-precision tensor ATen rounds it to that type as a first operand and takes
    it at float32 as a second operand."""
    return torch.tensor(float(x), dtype=torch.float64)


def rk4_stage(stage, y0, k1, k2, k3, k4, dt):
    """rk_common.py:110-118 (3/8 rule), the stage inputs and the step: dt a 0-dim tensor in the grid's type,
    `_one_third` / 0.125 / 3 Python numbers."""
    dtT = _time(dt)
    third = 1.0 / 3.0
    if stage == 1:
        return y0 + dtT * k1 * third
    if stage == 2:
        return y0 + dtT * (k2 - k1 * third)
    if stage == 3:
        return y0 + dtT * (k1 - k2 + k3)
    return y0 + (k1 + 3 * (k2 + k3) + k4) * dtT * 0.125


def lerp(y0, y1, slope):
    """solvers.py:175-181 `_linear_interp`: y0 + slope * (y1 - y0), slope a 0-dim tensor in the grid's type."""
    return y0 + _time(slope) * (y1 - y0)


def fixed_stage(mode, y0, ks, ws, dt):
    """rk_common.py:121-157 / fixed_grid.py: mode 1 = y0 + dt * k0 * w0; mode 0 = y0 + dt * (k0 * w0 + k1 * w1 ...)
    (dt a 0-dim tensor in the grid's type, the weights Python numbers, the sum a chain of elementwise additions)."""
    dtT = _time(dt)
    if mode == 1:
        return y0 + dtT * ks[0] * ws[0]
    acc = ks[0] * ws[0]
    for k, w in zip(ks[1:], ws[1:]):
        acc = acc + k * w
    return y0 + dtT * acc


def weighted_sum(xs, ws):
    """x0 * w0 + x1 * w1 + ... with the weights 0-dim tensors of the state's type (the Adams / backward helpers)."""
    acc = xs[0] * _t(ws[0], xs[0].dtype)
    for x, w in zip(xs[1:], ws[1:]):
        acc = acc + x * _t(w, x.dtype)
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# The step controller in the state's type, and the look-ahead first stage it selects (the parity oracle of the 16-bit
# branches of norm_finalize_ctrl_kernel in csrc/tdeq_kernels.hpp and of lp::sel_kernel).  Pinned to the reference by
# tests/test_lowp_oracle.py against tests/golden/lowp_controller.npz.
# ---------------------------------------------------------------------------------------------------------------------
def stage_combine_sel(y_acc, f_acc, y_rej, f_rej, coef, accept, dt_T):
    """The first stage of the NEXT trial step, y + f * (beta_00 * dt) (rk_common.py:79 with one term), on the pair the
    controller kept: (y1, f1) after an accepted step, (y0, f0) after a rejected one (rk_common.py:338-357).  `dt_T` is
    the signed step size as a 0-dim tensor of the state's type holds it (rk_common.py:64)."""
    y, f = (y_acc, f_acc) if accept else (y_rej, f_rej)
    return y + f * (_t(coef, y.dtype) * _t(dt_T, y.dtype))


def segment_norm(q, leading_abs: bool = False) -> float:
    """`q.abs().pow(2).mean().sqrt()` (misc.py:22-23) of one segment, from the fp64 sum of the rounded squares the norm
    kernels report: ATen's mean of a reduced-precision tensor is a float32 sum divided by a float32 count, rounded ONCE
    to the type, and the `sqrt` is rounded again.  A one-element segment is |x|, squared in the type — the same
    expression — and with `leading_abs` |x| itself (the adjoint norms take their time component as `t.abs()`,
    adjoint.py:250, 273)."""
    a = q.abs()
    if leading_abs and q.numel() == 1:
        return float(a.reshape(()))
    total = a.pow(2).double().sum()
    mean = (total.to(torch.float32) / torch.tensor(float(q.numel()), dtype=torch.float32)).to(q.dtype)
    return float(mean.sqrt())


def _nan_max(values) -> float:
    """`max(...)` over 0-dim tensors as the controller needs it: a NaN wins wherever it stands."""
    out = 0.0
    for v in values:
        if math.isnan(v) or math.isnan(out):
            out = math.nan
        else:
            out = max(out, v)
    return out


def step_controller(norms, t0, dt, ctrl, dtype):
    """One pass of rk_common.py:323-360 after the norms, and the stage times of the trial step that follows
    (rk_common.py:61-78, 268-273, through misc.py:180-197).

    `norms`: the per-segment values (`segment_norm`); `t0`, `dt`: the trial step just taken, fp64 host numbers, dt > 0;
    `ctrl`: anything with the fields of `tdeq_step_ctrl` (safety, ifactor, dfactor, exponent = 1 / order, min_step,
    max_step, time_sign, alpha — already rounded to the state's type — alpha_is_one, n_times, n_norm_seg).

    -> (accept, dt_next, ratio, t0_next, T(dt') * sign, stage_times[T]) where dt_next is `_optimal_step_size` with a
    fp64 `last_step` (misc.py:85-95) clamped (rk_common.py:359) and dt' is what the next `_adaptive_step` makes of it
    (rk_common.py:269-271: a non-finite step size becomes min_step)."""
    f64 = lambda x: torch.tensor(float(x), dtype=torch.float64)
    ratio = _nan_max([float(v) for v in list(norms)[:ctrl.n_norm_seg]])                  # misc.py:30-33
    t0_, dt_ = f64(t0), f64(dt)
    lo, hi = f64(ctrl.min_step), f64(ctrl.max_step)
    accept = bool(f64(ratio) <= 1)                                                       # rk_common.py:324
    if dt_ > hi:
        accept = False
    if dt_ <= lo:
        accept = True
    error_ratio = f64(ratio)                                                             # misc.py:92 `.type_as(last_step)`
    if error_ratio == 0:                                                                 # misc.py:88-95
        dt_next = dt_ * f64(ctrl.ifactor)
    else:
        dfactor = f64(1.0) if error_ratio < 1 else f64(ctrl.dfactor)
        factor = torch.min(f64(ctrl.ifactor), torch.max(f64(ctrl.safety) / error_ratio ** f64(ctrl.exponent), dfactor))
        dt_next = dt_ * factor
    dt_next = dt_next.clamp(lo, hi)                                                      # rk_common.py:359
    t0_next = t0_ + dt_ if accept else t0_                                               # rk_common.py:340 / 355
    dt_new = dt_next if bool(torch.isfinite(dt_next)) else lo                            # rk_common.py:269-271
    dt_new = dt_new.clamp(lo, hi)
    dt_signed = float(dt_new.to(dtype) * torch.tensor(float(ctrl.time_sign), dtype=dtype))
    return (accept, float(dt_next), ratio, float(t0_next), dt_signed, stage_times(float(t0_next), float(dt_new), ctrl, dtype))


def stage_times(t0, dt, ctrl, dtype):
    """The times `func` sees during the trial step (t0, dt) — fp64 host numbers — of a state of `dtype`
    (rk_common.py:61-78 through misc.py:180-197): t0, dt and t1 = t0 + dt are each cast from fp64, `t0 + alpha_i * dt` is
    arithmetic on 0-dim tensors of the type, a stage at alpha == 1 sits at nextafter(t1, t1 - 1), and a solve in
    decreasing time negates the result (misc.py:165, exact)."""
    f64 = lambda x: torch.tensor(float(x), dtype=torch.float64)
    t0T, dtT, t1T = f64(t0).to(dtype), f64(dt).to(dtype), (f64(t0) + f64(dt)).to(dtype)  # rk_common.py:63-65, 273
    sign = torch.tensor(float(ctrl.time_sign), dtype=dtype)
    times = []
    for i in range(ctrl.n_times):
        if (ctrl.alpha_is_one >> i) & 1:                                                 # rk_common.py:72-75, misc.py:193
            ti = torch.nextafter(t1T, t1T - 1)
        else:
            ti = t0T + torch.tensor(float(ctrl.alpha[i]), dtype=dtype) * dtT             # rk_common.py:77
        times.append(sign * ti)
    return torch.stack(times)
