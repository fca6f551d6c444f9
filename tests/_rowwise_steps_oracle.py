"""Shared pieces of the step-option tests of the rowwise family (`min_step`, `max_step`, `step_t`, `jump_t` per row): the
CPU row oracle extended by `row_control_points` and `row_select`, the device driver on it, the vectors of a
`_native.RowPoints` on either device, and the problems.

`row_control_points` is stated on the numpy views of `_state_views`, row by row, from the text of the rule
(rk_common.py:223-241, 266-361), never imported from the package:

    prepared step      dt non-finite -> min_r; clamp to [min_r, max_r]; underflow on the unclipped t0 + dt > t0; with
                       p = step[next_step]: t0 < p < t0 + dt cuts the step (t1 = p, dt = p - t0); the same test for the jump
                       table on the step so far, and it wins; the stage of abscissa 1 at prev_T(T(t1)), the others at
                       T(t0) + alpha_T T(dt)
    after the ratio    the whole-batch controller of the oracle with the row's bounds decides and gives the next step size;
                       an accepted cut step ends at the point itself and moves the index unless it is the last

Modes 1, 2 and 3 are the inner `row_control` on a one-row view of the state with the row's bounds, then the cut."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import DenseOracle
from _rowwise_event_oracle import quiet  # noqa: F401
from _rowwise_kernels import RowVectors

from torchdiffeq_amd import _native, rowwise

METHODS = ["dopri5", "tsit5", "bosh3", "fehlberg2", "adaptive_heun", "dopri8"]
POINT_I32 = ("step_count", "jump_count", "next_step", "next_jump", "on_point", "jumped")
POINT_F64 = ("clip_t", "min_step", "max_step")


def _view(ptr, ctype, shape):
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape)


def point_views(pts, n_rows, T):
    """numpy views of what a RowPoints points to (CPU addresses); None for a null pointer."""
    v = {}
    for name in POINT_I32:
        v[name] = _view(getattr(pts, name), ctypes.c_int32, (n_rows,)) if getattr(pts, name) else None
    for name in POINT_F64:
        v[name] = _view(getattr(pts, name), ctypes.c_double, (n_rows,)) if getattr(pts, name) else None
    v["step_t"] = _view(pts.step_t, ctypes.c_double, (int(pts.n_step), n_rows)) if pts.step_t else None
    v["jump_t"] = _view(pts.jump_t, ctypes.c_double, (int(pts.n_jump), n_rows)) if pts.jump_t else None
    ctype = ctypes.c_float if T is np.float32 else ctypes.c_double
    v["jump_times"] = _view(pts.jump_times, ctype, (n_rows,))
    return v


class StepsMixin:
    """`row_control_points` and `row_select` for an oracle of the `CompactOracle` family (`self._inner`)."""

    @staticmethod
    def row_select(dst, src, mask) -> None:
        rows = torch.nonzero(mask).view(-1)
        dst[rows] = src[rows]

    def _one_row_control(self, mode, part, ctrl, st, v, r, nch, dtype):
        """The inner `row_control` on row r alone: a RowState of one row that points into the vectors of `st`."""
        one = type(st)()
        for name, _ in type(st)._fields_:
            setattr(one, name, getattr(st, name))
        for name, a in v.items():
            if name not in ("tgrid", "status"):
                setattr(one, name, a[r:r + 1].ctypes.data)
        tg = np.ascontiguousarray(v["tgrid"][:, r:r + 1])
        status = np.zeros(2, dtype=np.int32)
        one.tgrid, one.status, one.n_rows = tg.ctypes.data, status.ctypes.data, 1
        B = int(st.n_rows)
        sums = part.view(-1)[:3 * B * nch].view(3, B, nch)[:, r:r + 1].contiguous()
        dts, times = torch.empty(1, dtype=dtype), torch.empty(int(ctrl.n_times), dtype=dtype)
        self._inner.row_control(mode, sums, ctrl, one, dts, times, dtype)
        return dts, times, status

    def row_control_points(self, mode, part, ctrl, st, pts, dts_out, times_out, dtype) -> None:
        inner = self._inner
        B, L = int(st.n_rows), int(st.row_len)
        T = inner._np_type(dtype)
        nch = inner.row_partials(L, dtype)
        v = inner._state_views(st)
        status = _view(st.status, ctypes.c_int32, (3,))
        q = point_views(pts, B, T)
        sums = part.view(-1)[:3 * B * nch].view(3, B, nch).numpy()
        dts, times = dts_out.numpy(), times_out.numpy().reshape(-1, B)
        n_times, sign = int(ctrl.n_times), float(ctrl.time_sign)
        n_live, n_jumped, first_err = 0, 0, 0x7FFFFFFF

        def total(k, r):
            x = sums[k, r]
            return math.fsum(x) if np.isfinite(x).all() else float(x.sum())

        def bounds(r):
            lo = float(ctrl.min_step) if q["min_step"] is None else float(q["min_step"][r])
            hi = float(ctrl.max_step) if q["max_step"] is None else float(q["max_step"][r])
            return lo, hi

        def row_ctrl(r):
            c = type(ctrl).from_buffer_copy(ctrl)
            c.min_step, c.max_step = bounds(r)
            return c

        def clamp(x, lo, hi):                               # torch.clamp on host doubles: NaN stays
            if x != x:
                return x
            m = x if x > lo else lo
            return m if m < hi else hi

        def freeze(r):
            dts[r] = T(0)
            times[:n_times, r] = T(sign) * T(v["t0"][r])

        def cut(r):
            """The prepared step of row r (dt clamped, dts / times written for it) cut at the row's next points."""
            t0, dt, on, t1 = float(v["t0"][r]), float(v["dt"][r]), 0, None
            for kind, tab, cnt, nxt in ((1, q["step_t"], q["step_count"], q["next_step"]),
                                        (2, q["jump_t"], q["jump_count"], q["next_jump"])):
                if tab is not None and cnt[r] >= 1:
                    p = float(tab[nxt[r], r])
                    if t0 < p < t0 + dt:
                        on, t1, dt = kind, p, p - t0
            q["on_point"][r] = on
            if not on:
                return
            q["clip_t"][r] = t1
            v["dt"][r] = dt
            with np.errstate(all="ignore"):
                dts[r] = T(dt) * T(sign)
                for i in range(n_times):
                    if (ctrl.alpha_is_one >> i) & 1:
                        tt = np.nextafter(T(t1), T(t1) - T(1))
                    else:
                        tt = T(t0) + T(ctrl.alpha[i]) * T(dt)
                    times[i, r] = T(sign) * tt

        def prepare(r):
            lo, hi = bounds(r)
            dtn = float(v["dt"][r])
            if not math.isfinite(dtn):
                dtn = lo
            dtn = clamp(dtn, lo, hi)
            v["dt"][r] = dtn
            t0 = float(v["t0"][r])
            with np.errstate(all="ignore"):
                dts[r] = T(dtn) * T(sign)
            times[:n_times, r] = inner._row_stage_times(ctrl, T, t0, dtn)
            code = 3 if v["bad_y"][r] else 0
            if not t0 + dtn > t0:
                code = 1
            if v["since"][r] >= st.max_num_steps:
                code = 2
            v["code"][r] = code
            cut(r)
            return code != 0

        for r in range(B):
            live = bool(v["active"][r])
            if mode != 0:
                one_dts, one_times, one_status = self._one_row_control(mode, part, row_ctrl(r), st, v, r, nch, dtype)
                n_written = 1 if mode == 1 else n_times      # (mode 1: the one time of the heuristic's own evaluation)
                dts[r] = one_dts.numpy()[0]
                times[:n_written, r] = one_times.numpy()[:n_written]
                if mode != 1:
                    if live:
                        cut(r)
                        if one_status[1] != 0x7FFFFFFF:
                            first_err = min(first_err, r)
                    else:
                        q["on_point"][r] = 0
                n_live += live
                continue
            jump = False
            tj = T(v["t0"][r])
            if not live:
                v["accepted"][r] = 0
                freeze(r)
            else:
                c = row_ctrl(r)
                c.t0, c.dt, c.n_norm_seg = float(v["t0"][r]), float(v["dt"][r]), 1
                nxt = torch.empty(n_times, dtype=dtype)
                (accept, dt_next, ratio, t_next), _ = inner.step_controller(self._plan(L), [total(0, r)], c, nxt, dtype)
                on = int(q["on_point"][r])
                if on:
                    t_next = float(q["clip_t"][r])          # a cut step ends on the point's own bits
                v["ratio"][r] = ratio
                v["since"][r] += 1
                v["accepted"][r] = 1 if accept else 0
                if accept:
                    v["tprev"][r] = v["t0"][r]
                    v["t0"][r] = t_next
                    v["n_acc"][r] += 1
                    lo = hi = int(v["next_out"][r])
                    while hi < st.n_out and v["tgrid"][hi, r] <= t_next:
                        hi += 1
                    v["out_lo"][r], v["out_hi"][r], v["next_out"][r] = lo, hi, hi
                    if hi > lo:
                        v["since"][r] = 0
                    v["bad_y"][r] = 1 if total(2, r) != 0.0 else 0
                    if on == 1 and q["next_step"][r] != q["step_count"][r] - 1:
                        q["next_step"][r] += 1
                    if on == 2:
                        if q["next_jump"][r] != q["jump_count"][r] - 1:
                            q["next_jump"][r] += 1
                        jump = True
                    tj = T(t_next)
                    if jump:
                        tj = np.nextafter(tj, tj + T(1))
                    if hi >= st.n_out:
                        live = False
                        v["active"][r] = 0
                else:
                    v["n_rej"][r] += 1
                v["dt"][r] = dt_next
                if live:
                    if prepare(r):
                        first_err = min(first_err, r)
                else:
                    freeze(r)
                    q["on_point"][r] = 0                    # the row has finished: no prepared step
            q["jumped"][r] = 1 if jump else 0
            q["jump_times"][r] = T(sign) * tj
            n_live += live
            n_jumped += jump
        status[0], status[1], status[2] = n_live, first_err, n_jumped

    def _plan(self, L):
        from oracle.kernels import OraclePlan
        return OraclePlan([(0, L, 0.0, 0.0)], L, L)


class StepsOracle(StepsMixin, DenseOracle):
    """`EventOracle` — through the dense-output oracle, which adds compaction and the dense launches to it — plus the two
    launches of the step options, so that all three entry points run on it."""


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """Inside `with device_driver():` a CPU state is solved by `HipRowKernels` on the oracle's row operations, the two of
    the step options included (all three entry points)."""
    wrapped = StepsOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


class PointVectors:
    """A `_native.RowPoints` over tensors on `device`, built from CPU values; a name not given (or None) is a null
    pointer for the optional ones and a recognisable filler for the vectors every launch takes."""

    def __init__(self, device, B, dtype, step_t=None, jump_t=None, **init):
        self.v = {}
        for name, tab in (("step_t", step_t), ("jump_t", jump_t)):
            self.v[name] = None if tab is None else torch.as_tensor(tab, dtype=torch.float64).reshape(-1, B).contiguous().to(device)
        for name in ("min_step", "max_step"):
            val = init.get(name)
            self.v[name] = None if val is None else torch.as_tensor(val, dtype=torch.float64).reshape(B).clone().to(device)
        for kind in ("step", "jump"):
            for name in (f"{kind}_count", f"next_{kind}"):
                val = init.get(name)
                assert (val is None) == (self.v[f"{kind}_t"] is None), name
                self.v[name] = None if val is None else torch.as_tensor(val, dtype=torch.int32).reshape(B).clone().to(device)
        self.v["clip_t"] = torch.as_tensor(init.get("clip_t", [-3.25] * B), dtype=torch.float64).reshape(B).clone().to(device)
        self.v["on_point"] = torch.as_tensor(init.get("on_point", [0] * B), dtype=torch.int32).reshape(B).clone().to(device)
        self.v["jumped"] = torch.full((B,), 9, dtype=torch.int32).to(device)
        self.v["jump_times"] = torch.full((B,), -77.0, dtype=dtype).to(device)
        pts = _native.RowPoints()
        for name, t in self.v.items():
            setattr(pts, name, None if t is None else t.data_ptr())
        pts.n_step = 0 if self.v["step_t"] is None else self.v["step_t"].shape[0]
        pts.n_jump = 0 if self.v["jump_t"] is None else self.v["jump_t"].shape[0]
        self.pts = pts

    def cpu(self):
        return {name: None if t is None else t.cpu() for name, t in self.v.items()}


class RowVectors3(RowVectors):
    """`RowVectors` with the three status words of `row_control_points`."""

    def __init__(self, device, *a, **kw):
        super().__init__(device, *a, **kw)
        self.v["status"] = torch.tensor([-1, -1, -1], dtype=torch.int32).to(device)
        self.st.status = self.v["status"].data_ptr()


# -- the problems -------------------------------------------------------------------------------------------------------------
def switched_problem(B, L, dtype, seed, device="cpu"):
    """Rows y' = -k_r y + s_r(t) c_r with a forcing whose sign flips at every time of the row's `switch` list (a [K, B]
    table, NaN: none): elementwise, no transcendental, discontinuous exactly at the jump points.  -> (y0, maker of the
    func of a table (taking `rows` when `by_rows`), k)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-0.5, 1.0, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].to(device, dtype)
    c = (1 + torch.rand(B, L, generator=g, dtype=torch.float64)).to(device, dtype)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64).to(device, dtype)

    def make(switch, by_rows=False, rows_of=None, direction=1):
        sw = torch.as_tensor(switch, dtype=torch.float64)
        sw = (sw[:, None].expand(-1, B) if sw.dim() == 1 else sw).to(device, dtype)
        sw = torch.where(torch.isnan(sw), torch.full_like(sw, float("inf")), sw)
        kk, cc, ss = (k, c, sw) if rows_of is None else (k[rows_of], c[rows_of], sw[:, rows_of])
        kk = kk * direction                                  # (direction = -1: rows that decay in decreasing time)

        def forcing(t, kr, cr, sr):
            flips = (t[None, :] >= sr).sum(dim=0)            # the points already behind the row, in TRUE time
            s = 1 - 2 * (flips % 2).to(t.dtype)
            return s[:, None] * cr

        if by_rows:
            return lambda t, y, rows: -kk[rows] * y + forcing(t, kk[rows], cc[rows], ss[:, rows])
        return lambda t, y: -kk * y + forcing(t, kk, cc, ss)
    return y0, make, k


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def device_problem(dtype, L, direction, device="cpu"):
    """The problem of the device-vs-host comparisons (here on the oracle, in tests/test_rowwise_steps_gpu.py on the
    kernels): B = 6, per-row tables and bounds.  -> (y0, func, t, options)."""
    B = 6
    y0, make, _ = switched_problem(B, L, dtype, 7, device)
    step = torch.tensor([[0.2, float("nan"), 0.35, 0.0, 0.6, 0.15], [0.8, float("nan"), float("nan"), 0.5, 2.0, 0.45]], dtype=torch.float64) * direction
    jump = torch.tensor([[0.5, 0.3, float("nan"), 0.7, 0.25, 0.65]], dtype=torch.float64) * direction
    t = torch.linspace(0, 1, 3, dtype=torch.float64) * direction
    options = {"step_t": step, "jump_t": jump, "min_step": torch.linspace(1e-6, 1e-4, B, dtype=torch.float64),
               "max_step": torch.tensor([0.05, 0.5, 0.1, 0.3, 0.2, 0.4], dtype=torch.float64)}
    # the rows decay in the direction of the solve: integrated against it they grow by up to e^10, and so does the
    # rounding-level difference between two summation orders that the bounds of this comparison are about
    return y0, make(jump, direction=direction), t.to(device), options


def device_tolerances(dtype):
    return dict(rtol=1e-6, atol=1e-8) if dtype == torch.float64 else dict(rtol=1e-4, atol=1e-6)


def assert_device_matches_host(dev, sd, host, sh, dtype, method):
    """fp64: equal counts and nfe, 1e-12 (dopri8 1e-7).  fp32: the rule of tests/test_rowwise_gpu.py::test_hip_shapes — a
    row with equal counts within 1e-5, a row whose counts differ by at most 1 within 1e-4, at most one such row."""
    B = dev.shape[1]
    da, dr, ha, hr = (x.cpu() for x in (sd["n_accepted"], sd["n_rejected"], sh["n_accepted"], sh["n_rejected"]))
    if dtype == torch.float64:
        assert da.tolist() == ha.tolist() and dr.tolist() == hr.tolist()
        assert sd["nfe"] == sh["nfe"]
        bound = 1e-7 if method == "dopri8" else 1e-12
        for r in range(B):
            assert _rel(dev[:, r].cpu(), host[:, r]) < bound, r
        return 0
    differ = (da != ha) | (dr != hr)
    assert int(differ.sum()) <= 1
    for r in range(B):
        if differ[r]:
            assert abs(int(da[r]) - int(ha[r])) <= 1 and abs(int(dr[r]) - int(hr[r])) <= 1, r
        assert _rel(dev[:, r].cpu(), host[:, r]) < (1e-4 if differ[r] else 1e-5), r
    return int(differ.sum())
