"""Shared pieces of the `jump_dy` tests of the rowwise family (state impulses at a row's jump points): the CPU row oracle
extended by `row_impulse` and the IMPULSE variant of `row_control_points`, the device driver on it, and the problems.

Both are stated from the text of the rule, never imported from the package:

    row_impulse        for a carried row r with jumped[r] != 0: o = row_map[r] (None: r), k = dy_index[jump_hit[r], o];
                       k >= 0: y[r] += dy[k, o] (dy[k, 0] for a shared dy), one addition in the state's type; no other
                       row of y or dy is read or written
    IMPULSE controller (`pts.jump_hit` set)  the controller of `StepsMixin` with two differences: the jump table is tested
                       with t0 < p <= t0 + dt (a step with p == t0 + dt ends on p and keeps its dt), and mode 0 writes
                       jump_hit[r] = next_jump[r] as it was before the launch for the rows whose accepted step ended on
                       a jump point

The open test `t0 < p < t0 + dt` and the closed one differ for exactly one prepared step: the one with p == t0 + dt on
the step so far (after the cut at a step point).  So the variant is `StepsMixin.row_control_points` followed, for every
row with a prepared step that was not cut at a jump point, by that one comparison and the cut it asks for."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from _rowwise_steps_oracle import StepsOracle, _view, point_views

from torchdiffeq_amd import _native, rowwise

NAN = float("nan")
F64 = torch.float64


class ImpulseMixin:
    """`row_impulse` and the IMPULSE variant of `row_control_points` on top of `StepsMixin`."""

    @staticmethod
    def row_impulse(y, dy, dy_index, jump_hit, jumped, row_map=None) -> None:
        for r in range(y.shape[0]):
            if int(jumped[r]) == 0:
                continue
            o = r if row_map is None else int(row_map[r])
            k = int(dy_index[int(jump_hit[r]), o])
            if k >= 0:
                y[r] = y[r] + dy[k, o if dy.shape[1] > 1 else 0]

    def row_control_points(self, mode, part, ctrl, st, pts, dts_out, times_out, dtype) -> None:
        if not pts.jump_hit:
            return super().row_control_points(mode, part, ctrl, st, pts, dts_out, times_out, dtype)
        assert pts.jump_t and int(pts.jump_closed) == 1
        inner = self._inner
        B = int(st.n_rows)
        T = inner._np_type(dtype)
        q = point_views(pts, B, T)
        hit = _view(pts.jump_hit, ctypes.c_int32, (B,))
        before = q["next_jump"].copy()
        super().row_control_points(mode, part, ctrl, st, pts, dts_out, times_out, dtype)
        if mode == 1:
            return
        v = inner._state_views(st)
        dts, times = dts_out.numpy(), times_out.numpy().reshape(-1, B)
        sign = float(ctrl.time_sign)
        for r in range(B):
            if mode == 0 and q["jumped"][r]:
                hit[r] = before[r]
            if not v["active"][r] or q["on_point"][r] == 2 or q["jump_count"][r] < 1:
                continue
            t0, dt = float(v["t0"][r]), float(v["dt"][r])
            p = float(q["jump_t"][q["next_jump"][r], r])
            if not (t0 < p and p == t0 + dt):
                continue
            # the step lands on the point: a step onto it, ending on the point's own bits like any cut step; it keeps its
            # size (p - t0 may round above dt, hence above the row's max_step, and such a step is never accepted)
            q["on_point"][r], q["clip_t"][r] = 2, p
            with np.errstate(all="ignore"):
                dts[r] = T(dt) * T(sign)
                for i in range(int(ctrl.n_times)):
                    if (ctrl.alpha_is_one >> i) & 1:
                        tt = np.nextafter(T(p), T(p) - T(1))
                    else:
                        tt = T(t0) + T(ctrl.alpha[i]) * T(dt)
                    times[i, r] = T(sign) * tt


class ImpulseOracle(ImpulseMixin, StepsOracle):
    """`StepsOracle` plus the launches of a solve with `jump_dy`."""


@pytest.fixture()
def impulse_driver(monkeypatch, oracle_kernels):
    """Inside `with impulse_driver():` a CPU state is solved by `HipRowKernels` on the oracle's row operations, those of
    `jump_dy` included."""
    wrapped = ImpulseOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


# -- the problems -------------------------------------------------------------------------------------------------------------
def decay_problem(B, L, dtype, seed, device="cpu"):
    """Rows y' = -k_r y + c_r: elementwise, smooth, and with y0 > 0 and c > 0 a state with no zero component.  -> (y0, maker
    of the func (for the rows `rows_of`, taking `rows` when `by_rows`, for a direction of time))."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-0.5, 0.7, B, dtype=F64)[torch.randperm(B, generator=g)][:, None].to(device, dtype)
    c = (0.5 + torch.rand(B, L, generator=g, dtype=F64)).to(device, dtype)
    y0 = (0.5 + torch.rand(B, L, generator=g, dtype=F64)).to(device, dtype)

    def make(by_rows=False, rows_of=None, direction=1):
        kk, cc = (k, c) if rows_of is None else (k[rows_of], c[rows_of])
        if by_rows:
            return lambda t, y, rows: (-kk[rows] * y + cc[rows]) * direction
        return lambda t, y: (-kk * y + cc) * direction
    return y0, make


def doses(K, B, L, dtype, seed, device="cpu"):
    """[K, B, L] impulses of either sign, none zero."""
    g = torch.Generator().manual_seed(seed)
    d = 0.25 + torch.rand(K, B, L, generator=g, dtype=F64)
    s = torch.where(torch.rand(K, B, L, generator=g, dtype=F64) < 0.3, -1.0, 1.0).to(F64)
    return (d * s).to(device, dtype)


def device_impulse_problem(dtype, L, direction, device="cpu"):
    """The problem of the device-vs-host comparisons (on the oracle and on the kernels): B = 6, a per-row [2, B] table of
    dose times with a NaN entry and a dropped point, per-row doses, a step table and per-row bounds next to them.
    -> (y0, func, t, options)."""
    B = 6
    y0, make = decay_problem(B, L, dtype, 11, device)
    jump = torch.tensor([[0.5, 0.3, NAN, 0.7, 0.25, 0.65], [0.2, 0.85, 0.4, NAN, 0.75, -0.5]], dtype=F64) * direction
    step = torch.tensor([[0.6, NAN, 0.35, 0.1, NAN, 0.15]], dtype=F64) * direction
    dy = doses(2, B, L, dtype, 5, device)
    dy[0, 2] = NAN                                           # (behind a NaN time: ignored)
    t = torch.linspace(0, 1, 3, dtype=F64) * direction
    options = {"jump_t": jump, "jump_dy": dy, "step_t": step,
               "max_step": torch.tensor([0.05, 0.5, 0.1, 0.3, 0.2, 0.4], dtype=F64)}
    return y0, make(direction=direction), t.to(device), options
