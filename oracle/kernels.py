"""ctypes binding of oracle/_build/librk_oracle.so with the same tensor-level interface as
torchdiffeq_amd._native.HipKernels, operating on CPU torch tensors.

TEST INFRASTRUCTURE ONLY (see rk_oracle.c).  Two uses:
  * kernel parity: tests call the same method on `HipKernels` (GPU) and `OracleKernels` (CPU) with the
    same seeded inputs and compare;
  * host-logic tests without a GPU: tests monkeypatch `torchdiffeq_amd._native.get_kernels` to return an
    `OracleKernels`, which lets the product's solver / adjoint / sharding control flow run on CPU
    tensors.  The product itself never imports this module.
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
from typing import List, Sequence, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "librk_oracle.so")

_c_void_pp = ctypes.POINTER(ctypes.c_void_p)
_c_double_p = ctypes.POINTER(ctypes.c_double)


class MultiOut(ctypes.Structure):
    _fields_ = [("out", ctypes.c_void_p), ("coef", ctypes.c_double * 14), ("mask", ctypes.c_uint32),
                ("add_y0", ctypes.c_int32)]


class Segment(ctypes.Structure):
    _fields_ = [("chunk_start", ctypes.c_int64), ("numel", ctypes.c_int64),
                ("rtol", ctypes.c_double), ("atol", ctypes.c_double)]


def build(force: bool = False) -> str:
    """Compile rk_oracle.c with gcc (seconds)."""
    src = os.path.join(_HERE, "rk_oracle.c")
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-B", "_build/librk_oracle.so"],
                              stdout=subprocess.DEVNULL)
    return _LIB_PATH


def load() -> ctypes.CDLL:
    lib = ctypes.CDLL(build())
    V, I, I64, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    sigs = {
        "oracle_abi_version": [],
        "oracle_stage_combine": [V, V, _c_void_pp, _c_double_p, I, D, I64, I],
        "oracle_error_norm": [V, V, V, _c_void_pp, _c_double_p, I, D, ctypes.POINTER(Segment), I, I64, I64,
                              V, V, I],
        "oracle_init_norms": [I, V, V, V, ctypes.POINTER(Segment), I, I64, I64, V, V, I],
        "oracle_init_scaled": [I, V, V, V, ctypes.POINTER(Segment), I, I64, I64, V, V, I],
        "oracle_dense_eval": [V, V, V, V, V, _c_void_pp, _c_double_p, I, D, D, I64, I],
        "oracle_interp_fit": [V, V, V, V, V, _c_void_pp, _c_double_p, I, D, I64, I],
        "oracle_rk4_38_stage": [I, V, V, V, V, V, V, D, I64, I],
        "oracle_lerp": [V, V, V, D, I64, I],
        "oracle_fixed_stage": [I, V, V, _c_void_pp, _c_double_p, I, D, I64, I],
        "oracle_weighted_sum": [V, _c_void_pp, _c_double_p, I, I64, I],
        "oracle_stage_combine_err": [V, V, V, _c_void_pp, _c_double_p, _c_double_p, I, D, I64, I],
        "oracle_stage_combine_multi": [ctypes.POINTER(MultiOut), I, V, V, _c_void_pp, I, D, I64, I],
        "oracle_error_norm_partial": [V, V, V, _c_void_pp, _c_double_p, I, D, ctypes.POINTER(Segment), I, I64, I64,
                                      V, V, I],
        "oracle_error_norm_partial_ctrl": [V, V, V, _c_void_pp, _c_double_p, I, D, ctypes.POINTER(Segment), I, I64, I64,
                                           V, V, V, V, V, V, I],
        "oracle_step_controller": [ctypes.POINTER(Segment), I, V, V, V, V, V, I, I],
        "oracle_error_norm_vec": [V, V, V, _c_void_pp, _c_double_p, I, D, V, D, V, D, ctypes.POINTER(Segment), I, I64,
                                  V, V, I],
        "oracle_error_norm_vec_ctrl": [V, V, V, _c_void_pp, _c_double_p, I, D, V, D, V, D, ctypes.POINTER(Segment), I, I64,
                                       V, V, V, V, V, V, V, I, I],
        "oracle_init_norms_vec": [I, V, V, V, V, D, V, D, ctypes.POINTER(Segment), I, I64, V, V, I],
        "oracle_stage_combine_sel": [V, V, V, V, V, D, V, I64, I],
        "oracle_pack_segments": [V, _c_void_pp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                 _c_double_p, I, I64, I64, I],
        "oracle_scale_many": [_c_void_pp, V, _c_double_p, I, I64, I],
        "oracle_multi_dot": [V, _c_void_pp, I, I64, V, I],
        "oracle_adams_predict": [V, V, V, V, _c_void_pp, _c_double_p, _c_double_p, I, D, I64, I],
        "oracle_adams_correct": [V, V, V, V, V, V, D, I, ctypes.POINTER(Segment), I, I64, I64, I64, V, V, I],
    }
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = argtypes
    return lib


def _code(dtype: torch.dtype) -> int:
    return {torch.float32: 0, torch.float64: 1}[dtype]


def _ok(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}")


class OraclePlan:
    def __init__(self, segments: Sequence[Tuple[int, int, float, float]], total: int, chunk: int):
        self.chunk = chunk
        self.n_seg = len(segments)
        self.numels = [int(s[1]) for s in segments]
        self.n_chunks = max(1, math.ceil(total / chunk))
        arr = (Segment * self.n_seg)()
        for i, (off, numel, rtol, atol) in enumerate(segments):
            assert off % chunk == 0
            arr[i] = Segment(off // chunk, numel, float(rtol), float(atol))
        self.segs = arr
        self.out = torch.zeros(3 * self.n_seg + 4, dtype=torch.float64)
        self.out_ptr = self.out.data_ptr()
        self.bad_ptr = self.out_ptr + 16 * self.n_seg
        self.ctrl_ptr = self.out_ptr + 24 * self.n_seg
        self.ctrl_dev = torch.zeros(2, dtype=torch.float64)
        # {accept, sign * T(dt'), t0', dt'}: the product's four device-resident controller words (NormPlan.ctrl_dev), kept
        # apart from the two-word `ctrl_dev` above, whose shape existing callers rely on.  error_norm_vec_ctrl reads its
        # trial step from here under `state_in_dev` and rewrites all four; `ctrl_dev` receives the first two.
        self.ctrl_state = torch.zeros(4, dtype=torch.float64)


class OracleKernels:
    """CPU twin of HipKernels (same method names and argument meaning)."""
    name = "oracle"

    def __init__(self):
        self.lib = load()

    @staticmethod
    def _terms(ks, coefs):
        n = len(ks)
        for k in ks:
            assert k.device.type == "cpu" and k.is_contiguous()
        return (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks]), (ctypes.c_double * n)(*coefs), n

    def make_plan(self, segments, total, chunk, device) -> OraclePlan:
        return OraclePlan(segments, total, chunk)

    def stage_combine(self, out, y0, ks, coefs, dt):
        ptrs, cf, n = self._terms(ks, coefs)
        _ok(self.lib.oracle_stage_combine(out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                          _code(y0.dtype)), "oracle_stage_combine")

    def stage_combine_fill(self, out, y0, ks, coefs, dt, fill_dst, fill_vals):
        """Host twin of tdeq_stage_combine_fill = stage_combine + fill_scalars."""
        self.stage_combine(out, y0, ks, coefs, dt)
        self.fill_scalars(fill_dst, fill_vals)

    def error_norm(self, plan, y0, y1, ks, coefs, dt, scaled_out=None):
        ptrs, cf, n = self._terms(ks, coefs)
        so = None if scaled_out is None else scaled_out.data_ptr()
        _ok(self.lib.oracle_error_norm(so, y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt, plan.segs, plan.n_seg,
                                       plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr, _code(y0.dtype)),
            "oracle_error_norm")

    def stage_combine_err(self, out, err_out, y0, ks, coefs, err_coefs, dt):
        ptrs, cf, n = self._terms(ks, coefs)
        ef = (ctypes.c_double * n)(*err_coefs)
        _ok(self.lib.oracle_stage_combine_err(out.data_ptr(), err_out.data_ptr(), y0.data_ptr(), ptrs, cf, ef, n, dt,
                                              y0.numel(), _code(y0.dtype)), "oracle_stage_combine_err")

    def stage_combine_multi(self, outs, rows, y0, acc_in, ks, dt):
        n = len(ks)
        for k in ks:
            assert k.device.type == "cpu" and k.is_contiguous()
        ptrs = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
        spec = (MultiOut * len(outs))()
        for o, (t, (coefs, mask, add_y0)) in enumerate(zip(outs, rows)):
            spec[o].out = t.data_ptr()
            for j, c in enumerate(coefs):
                spec[o].coef[j] = c
            spec[o].mask, spec[o].add_y0 = mask, 1 if add_y0 else 0
        _ok(self.lib.oracle_stage_combine_multi(spec, len(outs), y0.data_ptr(),
                                                None if acc_in is None else acc_in.data_ptr(), ptrs, n, dt, y0.numel(),
                                                _code(y0.dtype)), "oracle_stage_combine_multi")

    def error_norm_partial(self, plan, err_partial, y0, y1, ks, coefs, dt):
        n = len(ks)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        _ok(self.lib.oracle_error_norm_partial(err_partial.data_ptr(), y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt,
                                               plan.segs, plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr,
                                               plan.bad_ptr, _code(y0.dtype)), "oracle_error_norm_partial")

    def error_scaled(self, plan, out, y0, y1, ks, coefs, dt):
        self.error_norm(plan, y0, y1, ks, coefs, dt, scaled_out=out)

    def init_norms(self, plan, mode, a, b, yscale):
        _ok(self.lib.oracle_init_norms(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), plan.segs, plan.n_seg,
                                       plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr, _code(yscale.dtype)),
            "oracle_init_norms")

    def init_scaled(self, plan, mode, a, b, yscale, out0, out1=None):
        _ok(self.lib.oracle_init_scaled(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), plan.segs, plan.n_seg,
                                        plan.chunk, plan.n_chunks, out0.data_ptr(),
                                        None if out1 is None else out1.data_ptr(), _code(yscale.dtype)),
            "oracle_init_scaled")

    def read_norms(self, plan) -> Tuple[List[float], List[float], List[float]]:
        v = plan.out.tolist()
        n = plan.n_seg
        return v[:n], v[n:2 * n], v[2 * n:3 * n]

    def error_norm_partial_ctrl(self, plan, err_partial, y0, y1, ks, coefs, dt, ctrl, next_times):
        """Host twin of tdeq_error_norm_partial_ctrl; `ctrl` is a ctypes struct laid out as oracle_step_ctrl."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        _ok(self.lib.oracle_error_norm_partial_ctrl(err_partial.data_ptr(), y0.data_ptr(), y1.data_ptr(), ptrs, cf, n,
                                                    dt, plan.segs, plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr,
                                                    plan.bad_ptr, ctypes.addressof(ctrl), plan.ctrl_ptr,
                                                    plan.ctrl_dev.data_ptr(), next_times.data_ptr(), _code(y0.dtype)),
            "oracle_error_norm_partial_ctrl")

    def step_controller(self, plan, sumsq, ctrl, next_times, dtype, ratio_dtype=None):
        """The controller alone on given per-segment sums -> (out_ctrl[4], ctrl_dev[2]) as lists.  `ratio_dtype`: the type
        the error ratio is rounded to — `dtype` unless given (per-element tolerances: torch.float64 for either state type)."""
        ss = (ctypes.c_double * plan.n_seg)(*sumsq)
        _ok(self.lib.oracle_step_controller(plan.segs, plan.n_seg, ctypes.addressof(ss), ctypes.addressof(ctrl),
                                            plan.ctrl_ptr, plan.ctrl_dev.data_ptr(), next_times.data_ptr(),
                                            _code(dtype), _code(dtype if ratio_dtype is None else ratio_dtype)),
            "oracle_step_controller")
        return plan.out.tolist()[3 * plan.n_seg:], plan.ctrl_dev.tolist()

    # -- per-element tolerances (twins of HipKernels.error_norm_vec / error_norm_vec_ctrl / init_norms_vec) ---------------
    vec_partial = True          # `partial=` continues the error row of stage_combine_err
    vec_ctrl_in_graph = True    # `state_in_dev` is honoured (the trial step is read from plan.ctrl_state)

    @staticmethod
    def _tol(tol):
        """(vector pointer or None, scalar) of one tolerance: an fp64 vector over the flat padded state, or a host float."""
        if isinstance(tol, torch.Tensor):
            assert tol.device.type == "cpu" and tol.dtype == torch.float64 and tol.is_contiguous()
            return tol.data_ptr(), 0.0
        return None, float(tol)

    @staticmethod
    def _rest(ks, coefs):
        n = len(ks)
        for k in ks:
            assert k.device.type == "cpu" and k.is_contiguous()
        return (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks]), (ctypes.c_double * max(n, 1))(*coefs), n

    def error_norm_vec(self, plan, y0, y1, ks, coefs, dt, rtol, atol, partial=None):
        ptrs, cf, n = self._rest(ks, coefs)
        (rv, rs), (av, as_) = self._tol(rtol), self._tol(atol)
        _ok(self.lib.oracle_error_norm_vec(None if partial is None else partial.data_ptr(), y0.data_ptr(), y1.data_ptr(),
                                           ptrs, cf, n, dt, rv, rs, av, as_, plan.segs, plan.n_seg, plan.chunk,
                                           plan.out_ptr, plan.bad_ptr, _code(y0.dtype)), "oracle_error_norm_vec")

    def error_norm_vec_ctrl(self, plan, y0, y1, ks, coefs, dt, rtol, atol, ctrl, next_times, partial=None,
                            state_in_dev=False):
        ptrs, cf, n = self._rest(ks, coefs)
        (rv, rs), (av, as_) = self._tol(rtol), self._tol(atol)
        _ok(self.lib.oracle_error_norm_vec_ctrl(None if partial is None else partial.data_ptr(), y0.data_ptr(),
                                                y1.data_ptr(), ptrs, cf, n, dt, rv, rs, av, as_, plan.segs, plan.n_seg,
                                                plan.chunk, plan.out_ptr, plan.bad_ptr, ctypes.addressof(ctrl),
                                                plan.ctrl_ptr, plan.ctrl_dev.data_ptr(), plan.ctrl_state.data_ptr(),
                                                next_times.data_ptr(), 1 if state_in_dev else 0, _code(y0.dtype)),
            "oracle_error_norm_vec_ctrl")

    def init_norms_vec(self, plan, mode, a, b, yscale, rtol, atol):
        (rv, rs), (av, as_) = self._tol(rtol), self._tol(atol)
        _ok(self.lib.oracle_init_norms_vec(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), rv, rs, av, as_, plan.segs,
                                           plan.n_seg, plan.chunk, plan.out_ptr, plan.bad_ptr, _code(yscale.dtype)),
            "oracle_init_norms_vec")

    def read_ctrl(self, plan):
        v = plan.out.tolist()
        n = plan.n_seg
        return v[3 * n] != 0.0, v[3 * n + 1], v[3 * n + 2], v[2 * n:3 * n]

    def stage_combine_sel(self, out, y_acc, f_acc, y_rej, f_rej, coef, plan):
        _ok(self.lib.oracle_stage_combine_sel(out.data_ptr(), y_acc.data_ptr(), f_acc.data_ptr(), y_rej.data_ptr(),
                                              f_rej.data_ptr(), coef, plan.ctrl_dev.data_ptr(), out.numel(),
                                              _code(out.dtype)), "oracle_stage_combine_sel")

    def dense_eval(self, out, y0, y1, f0, f1, ks, coefs, dt, x):
        ptrs, cf, n = self._terms(ks, coefs)
        _ok(self.lib.oracle_dense_eval(out.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(), f1.data_ptr(),
                                       ptrs, cf, n, dt, x, y0.numel(), _code(y0.dtype)), "oracle_dense_eval")

    def dense_eval_multi(self, out_rows, y0, y1, f0, f1, ks, coefs, dt, xs):
        """Host twin of tdeq_dense_eval_multi: the reference evaluates one output time at a time."""
        for q, x in enumerate(xs):
            self.dense_eval(out_rows[q], y0, y1, f0, f1, ks, coefs, dt, x)

    def interp_fit(self, coeffs, y0, y1, f0, f1, ks, coefs, dt):
        ptrs, cf, n = self._terms(ks, coefs)
        _ok(self.lib.oracle_interp_fit(coeffs.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(),
                                       f1.data_ptr(), ptrs, cf, n, dt, y0.numel(), _code(y0.dtype)),
            "oracle_interp_fit")

    def rk4_stage(self, stage, out, y0, k1, k2, k3, k4, dt):
        p = lambda t: None if t is None else t.data_ptr()
        _ok(self.lib.oracle_rk4_38_stage(stage, out.data_ptr(), y0.data_ptr(), p(k1), p(k2), p(k3), p(k4), dt,
                                         y0.numel(), _code(y0.dtype)), "oracle_rk4_38_stage")

    def lerp(self, out, y0, y1, slope):
        _ok(self.lib.oracle_lerp(out.data_ptr(), y0.data_ptr(), y1.data_ptr(), slope, y0.numel(),
                                 _code(y0.dtype)), "oracle_lerp")

    def fixed_stage(self, mode, out, y0, ks, ws, dt):
        ptrs, cf, n = self._terms(ks, ws)
        _ok(self.lib.oracle_fixed_stage(mode, out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                        _code(y0.dtype)), "oracle_fixed_stage")

    def weighted_sum(self, out, xs, ws):
        ptrs, cf, n = self._terms(xs, ws)
        _ok(self.lib.oracle_weighted_sum(out.data_ptr(), ptrs, cf, n, out.numel(), _code(out.dtype)),
            "oracle_weighted_sum")

    def scale_many(self, outs, g, ws):
        ptrs, cf, n = self._terms(outs, ws)
        _ok(self.lib.oracle_scale_many(ptrs, g.data_ptr(), cf, n, g.numel(), _code(g.dtype)), "oracle_scale_many")

    def multi_dot(self, g, xs):
        """fp64 tensor [len(xs)] of <g, x_m>."""
        n = len(xs)
        ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
        out = torch.empty(n, dtype=torch.float64)
        _ok(self.lib.oracle_multi_dot(g.data_ptr(), ptrs, n, g.numel(), out.data_ptr(), _code(g.dtype)),
            "oracle_multi_dot")
        return out

    def adams_predict(self, y_out, y0, hist, cb, cm=None, dt=0.0, dy_out=None, delta_out=None):
        ptrs, cbf, n = self._terms(hist, cb)
        cmf = None if cm is None else (ctypes.c_double * n)(*cm)
        p = lambda t: None if t is None else t.data_ptr()
        _ok(self.lib.oracle_adams_predict(y_out.data_ptr(), p(dy_out), p(delta_out), y0.data_ptr(), ptrs, cbf, cmf, n,
                                          dt, y0.numel(), _code(y0.dtype)), "oracle_adams_predict")

    def adams_correct(self, plan, dy_out, dy_old, y_out=None, f=None, delta=None, y0=None, c=0.0, compute=True):
        p = lambda t: None if t is None else t.data_ptr()
        _ok(self.lib.oracle_adams_correct(p(y_out), dy_out.data_ptr(), p(f), p(delta), dy_old.data_ptr(), p(y0), c,
                                          1 if compute else 0, plan.segs, plan.n_seg, plan.chunk, plan.n_chunks,
                                          dy_out.numel(), plan.out_ptr, plan.bad_ptr, _code(dy_out.dtype)),
            "oracle_adams_correct")

    def pack_segments(self, out, srcs, chunk_starts, numels, scales, chunk):
        n = len(srcs)
        ptrs = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in srcs])
        cs = (ctypes.c_int64 * n)(*chunk_starts)
        nm = (ctypes.c_int64 * n)(*numels)
        sc = (ctypes.c_double * n)(*scales)
        _ok(self.lib.oracle_pack_segments(out.data_ptr(), ptrs, cs, nm, sc, n, chunk, out.numel() // chunk,
                                          _code(out.dtype)), "oracle_pack_segments")

    def fill_scalars(self, dst, vals):
        """Host twin of tdeq_fill_scalars: vals converted to dst's dtype."""
        import torch as _torch
        dst.copy_(_torch.tensor(list(vals), dtype=_torch.float64).to(dst.dtype))

    # -- fixed-grid captured step: the step data kept on the device (include/tdeq_hip.h, tdeq_grid_advance ...) ---------
    # Restated from the header's text in numpy scalars of the grid type G and the state type T, one rounded operation
    # at a time; pinned to the reference's own stage times by tests/test_fixed_grid_oracle.py.
    RK4_38_TIMES = ((0.0, 2), (1 / 3, 0), (2 / 3, 0), (0.0, 1 | 4))      # t0 (NEXT), t0 + dt/3, t0 + 2dt/3, t1 (PREV)

    @staticmethod
    def perturb_next(tt):
        """Perturb.NEXT of a numpy scalar: np.nextafter(tt, tt + 1) in its own type."""
        with np.errstate(all="ignore"):
            return np.nextafter(tt, tt + type(tt)(1))

    @staticmethod
    def perturb_prev(tt):
        """Perturb.PREV of a numpy scalar: np.nextafter(tt, tt - 1) in its own type."""
        with np.errstate(all="ignore"):
            return np.nextafter(tt, tt - type(tt)(1))

    def grid_advance_stages(self, grid, counter, perturb, sign, fracs, modes, times_out, dt_out) -> None:
        assert grid.device.type == "cpu" and counter.dtype == torch.int64 and dt_out.dtype == torch.float64
        assert 1 <= len(fracs) == len(modes) <= 4 and grid.numel() >= 2
        G, T = self._np_type(grid.dtype), self._np_type(times_out.dtype)
        c = int(counter) + 1
        counter.fill_(c)
        if c + 1 >= grid.numel():
            return                                          # past the last interval: nothing else is written
        g, times = grid.numpy(), times_out.numpy()
        t0, t1 = G(g[c]), G(g[c + 1])
        with np.errstate(all="ignore"):
            dt = t1 - t0
            for i, (frac, mode) in enumerate(zip(fracs, modes)):
                tg = t1 if mode & 1 else (t0 if frac == 0.0 else t0 + dt * G(frac))
                tt = T(tg)
                if perturb and mode & 2:
                    tt = self.perturb_next(tt)
                if perturb and mode & 4:
                    tt = self.perturb_prev(tt)
                times[i] = T(sign) * tt
            dt_out.numpy()[0] = np.float64(dt) * np.float64(sign)

    def grid_advance(self, grid, counter, perturb, sign, times_out, dt_out) -> None:
        fracs, modes = zip(*self.RK4_38_TIMES)
        self.grid_advance_stages(grid, counter, perturb, sign, fracs, modes, times_out, dt_out)

    def grid_commit(self, solution, y_cur, y_new, counter) -> None:
        n = y_cur.numel()
        row = int(counter) + 1
        assert 0 <= row < solution.shape[0] and solution.stride(0) >= n
        solution[row, :n].copy_(y_new)
        y_cur.copy_(y_new)

    def fixed_stage_dev(self, mode, out, y0, ks, ws, dt_dev) -> None:
        self.fixed_stage(mode, out, y0, ks, ws, float(dt_dev[0]))

    def rk4_stage_dev(self, stage, out, y0, k1, k2, k3, k4, dt_dev) -> None:
        self.rk4_stage(stage, out, y0, k1, k2, k3, k4, float(dt_dev[0]))

    # -- per-row step control: the row interface of HipKernels, row by row ------------------------------------------------
    # The contract (csrc/tdeq_kernels_rowwise.hpp): every element of row r is what the whole-batch operation gives for
    # that row alone with dt = float(dts[r]).  So each method below loops over the rows and calls the whole-batch oracle
    # on the row's slice; what has no whole-batch twin is restated in numpy scalars of T, one rounded operation at a
    # time.  Row sums are `math.fsum` of the fp64 squares of the per-element T ratios: the correctly rounded sum, which
    # any summation order of the device must be close to.  A row's sum is stored in its first partial (the others are
    # zero): the layout of `part` is [3][B * nch] as on the device, how a sum is split over the partials is not.
    @staticmethod
    def row_partials(row_len: int, dtype) -> int:
        """Partials per row, restated from the geometry rule: 16-byte elements when the row is a whole number of them,
        one partial up to 1024 elements, else one per 2048."""
        lv = {torch.float32: 4, torch.float64: 2}[dtype]
        nv = row_len // lv if row_len % lv == 0 else row_len
        return 1 if nv <= 1024 else -(-nv // 2048)

    @staticmethod
    def _np_type(dtype):
        return {torch.float32: np.float32, torch.float64: np.float64}[dtype]

    @staticmethod
    def _fsum_sq(x) -> float:
        sq = np.asarray(x, dtype=np.float64) ** 2
        return math.fsum(sq) if np.isfinite(sq).all() else float(sq.sum())

    def row_combine(self, outs, rows, y0, acc_in, ks, dts, active) -> None:
        for r in range(y0.shape[0]):
            if not int(active[r]):
                for out, (_, _, add_y0) in zip(outs, rows):
                    if add_y0:
                        out[r].copy_(y0[r])
                    else:
                        out[r].zero_()
                continue
            self.stage_combine_multi([o[r] for o in outs], rows, y0[r], None if acc_in is None else acc_in[r],
                                     [k[r] for k in ks], float(dts[r]))

    def row_reduce(self, mode: int, part, y0, y1, partial, ks, coefs, dts, active, rtol: float, atol: float) -> None:
        B, L = y0.shape
        nch = self.row_partials(L, y0.dtype)
        assert part.numel() >= 3 * B * nch and part.dtype == torch.float64
        T = self._np_type(y0.dtype)
        plan = OraclePlan([(0, L, rtol, atol)], L, L)
        out = part.view(-1)[:3 * B * nch].view(3, B, nch)
        out.zero_()
        for r in range(B):
            if mode == 0:
                if not int(active[r]):
                    continue
                dt = float(dts[r])
                if partial is None:
                    scaled = torch.empty_like(y0[r])
                    self.error_scaled(plan, scaled, y0[r], y1[r], [k[r] for k in ks], coefs, dt)
                    scaled = scaled.numpy()
                else:
                    # e = partial + sum_j fl(fl(c_j) * T(dt)) * k_j, left to right; e / (atol + rtol * max(|y0|, |y1|))
                    with np.errstate(all="ignore"):
                        e = partial[r].numpy().copy()
                        for k, c in zip(ks, coefs):
                            e = e + k[r].numpy() * (T(c) * T(dt))
                        tol = T(atol) + T(rtol) * np.fmax(np.abs(y0[r].numpy()), np.abs(y1[r].numpy()))
                        scaled = e / tol
                out[0, r, 0] = self._fsum_sq(scaled)
                out[2, r, 0] = float((~(torch.isfinite(y0[r]) & torch.isfinite(y1[r]))).sum())
            else:
                # y0 = the scale state, y1 = a, partial = b: (a / scale, b / scale) or (a - b) / scale
                s0, s1 = torch.empty_like(y0[r]), torch.empty_like(y0[r])
                self.init_scaled(plan, mode - 1, y1[r], partial[r], y0[r], s0, s1 if mode == 1 else None)
                out[0, r, 0] = self._fsum_sq(s0.numpy())
                if mode == 1:
                    out[1, r, 0] = self._fsum_sq(s1.numpy())
                out[2, r, 0] = float((~torch.isfinite(y0[r])).sum())

    @staticmethod
    def _state_views(st):
        """numpy views of the vectors a RowState points to (CPU addresses)."""
        B, n_out = int(st.n_rows), int(st.n_out)

        def view(name, ctype, shape):
            return np.ctypeslib.as_array(ctypes.cast(getattr(st, name), ctypes.POINTER(ctype)), shape=shape)
        v = {name: view(name, ctypes.c_double, (B,)) for name in ("t0", "tprev", "dt", "h0", "ratio")}
        v.update({name: view(name, ctypes.c_int32, (B,)) for name in ("active", "accepted", "out_lo", "out_hi", "next_out",
                                                                        "since", "bad_y", "code")})
        v.update({name: view(name, ctypes.c_int64, (B,)) for name in ("n_acc", "n_rej")})
        v["tgrid"] = view("tgrid", ctypes.c_double, (n_out, B))
        v["status"] = view("status", ctypes.c_int32, (2,))
        return v

    @staticmethod
    def _row_stage_times(ctrl, T, t0: float, dt: float):
        """Stage times of the trial step (t0, dt) in T: nextafter(T(t0 + dt), -inf side) where alpha_i == 1, else
        T(t0) + T(alpha_i) * T(dt); times the direction of time."""
        t0T, dtT, t1T = T(t0), T(dt), T(t0 + dt)
        out = []
        with np.errstate(all="ignore"):
            for i in range(ctrl.n_times):
                if (ctrl.alpha_is_one >> i) & 1:
                    tt = np.nextafter(t1T, t1T - T(1))
                else:
                    tt = t0T + T(ctrl.alpha[i]) * dtT
                out.append(T(ctrl.time_sign) * tt)
        return out

    def row_control(self, mode: int, part, ctrl, st, dts_out, times_out, dtype) -> None:
        B, L = int(st.n_rows), int(st.row_len)
        T = self._np_type(dtype)
        nch = self.row_partials(L, dtype)
        v = self._state_views(st)
        sums = part.view(-1)[:3 * B * nch].view(3, B, nch).numpy()
        dts, times = dts_out.numpy(), times_out.numpy().reshape(-1, B)
        n_times, sign = int(ctrl.n_times), float(ctrl.time_sign)
        plan = OraclePlan([(0, L, 0.0, 0.0)], L, L)
        n_live, first_err = 0, 0x7FFFFFFF

        def total(q, r):
            x = sums[q, r]
            return math.fsum(x) if np.isfinite(x).all() else float(x.sum())

        def norm(s):                                        # sqrt(mean) rounded to T
            with np.errstate(all="ignore"):
                return T(np.sqrt(np.float64(s) / np.float64(L)))

        def freeze(r):
            dts[r] = T(0)
            times[:n_times, r] = T(sign) * T(v["t0"][r])

        def prepare(r, expect=None):
            dtn = float(v["dt"][r])
            if not math.isfinite(dtn):
                dtn = float(ctrl.min_step)
            dtn = min(max(dtn, float(ctrl.min_step)), float(ctrl.max_step))
            v["dt"][r] = dtn
            t0 = float(v["t0"][r])
            dts[r] = T(dtn) * T(sign)
            tt = self._row_stage_times(ctrl, T, t0, dtn)
            if expect is not None:          # the next trial step of the whole-batch controller: the same step, the same bits
                assert dts[r] == T(expect[0]) and [float(x) for x in tt] == expect[1], (r, tt, expect)
            times[:n_times, r] = tt
            code = 3 if v["bad_y"][r] else 0
            if not t0 + dtn > t0:
                code = 1
            if v["since"][r] >= st.max_num_steps:
                code = 2
            v["code"][r] = code
            return code != 0

        for r in range(B):
            live = bool(v["active"][r])
            s0, s1, sb = total(0, r), total(1, r), total(2, r)
            expect = None
            if mode == 0:
                if not live:
                    v["accepted"][r] = 0
                    freeze(r)
                    continue
                c = type(ctrl).from_buffer_copy(ctrl)
                c.t0, c.dt, c.n_norm_seg = float(v["t0"][r]), float(v["dt"][r]), 1
                nxt = torch.empty(n_times, dtype=dtype)
                (accept, dt_next, ratio, t_next), (_, dts_next) = self.step_controller(plan, [s0], c, nxt, dtype)
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
                    v["bad_y"][r] = 1 if sb != 0.0 else 0
                    if hi >= st.n_out:
                        live = False
                        v["active"][r] = 0
                else:
                    v["n_rej"][r] += 1
                v["dt"][r] = dt_next
                expect = (dts_next, nxt.double().tolist())
            elif mode == 1:
                with np.errstate(all="ignore"):
                    d0, d1 = norm(s0), norm(s1)
                    h0 = T(1e-6) if (d0 < T(1e-5) or d1 < T(1e-5)) else (T(0.01) * d0) / d1
                    h0 = -h0 if h0 < T(0) else h0
                    v["h0"][r] = float(h0)
                    v["bad_y"][r] = 1 if sb != 0.0 else 0
                    dts[r] = T(float(h0) * sign)
                    times[0, r] = T(sign) * T(float(v["t0"][r]) + float(h0))
                    v["dt"][r] = float(d1)                  # parked for mode 2
                n_live += live
                continue
            elif mode == 2:
                with np.errstate(all="ignore"):
                    h0, d1 = T(v["h0"][r]), T(v["dt"][r])
                    d2 = norm(s0) / h0
                    d2 = -d2 if d2 < T(0) else d2
                    if d1 <= T(1e-15) and d2 <= T(1e-15):
                        lo_, val = T(1e-6), h0 * T(1e-3)
                        h1 = val if val > lo_ else lo_
                    else:
                        m = d2 if d2 > d1 else d1
                        q = (T(1) / m) * T(0.01)
                        e = 1.0 / float(st.order + 1)
                        h1 = np.sqrt(q) if e == 0.5 else T(math.pow(float(q), e)) if float(q) >= 0 else T(np.nan)
                    h1 = -h1 if h1 < T(0) else h1
                    big = T(100) * h0
                    v["dt"][r] = float(h1 if h1 < big else big)
            else:
                v["bad_y"][r] = 1 if sb != 0.0 else 0
            if live:
                if prepare(r, expect):
                    first_err = min(first_err, r)
            else:
                freeze(r)
            n_live += live
        v["status"][0], v["status"][1] = n_live, first_err

    def row_dense_commit(self, sol, y0, y1, f0, f1, ks, coefs, dts, st) -> None:
        v = self._state_views(st)
        T = self._np_type(y0.dtype)
        for r in range(int(st.n_rows)):
            if not v["accepted"][r]:
                continue
            ta, tb = v["tprev"][r], v["t0"][r]
            for j in range(int(v["out_lo"][r]), int(v["out_hi"][r])):
                x = T((v["tgrid"][j, r] - ta) / (tb - ta))      # the fraction in fp64, rounded to T once
                self.dense_eval(sol[j, r], y0[r], y1[r], f0[r], f1[r], [k[r] for k in ks], coefs, float(dts[r]), float(x))
            y0[r].copy_(y1[r])
            f0[r].copy_(f1[r])

    def row_scale_many(self, outs, g, w) -> None:
        for r in range(g.shape[0]):
            self.scale_many([o[r] for o in outs], g[r], [float(x) for x in w[:, r]])

    @staticmethod
    def row_multi_dot(g, xs) -> torch.Tensor:
        """fp64 [len(xs), B]: the correctly rounded sum of the fp64 products of each row."""
        out = torch.empty(len(xs), g.shape[0], dtype=torch.float64)
        g64 = g.double().numpy()
        for m, x in enumerate(xs):
            prod = g64 * x.double().numpy()
            for r in range(g.shape[0]):
                out[m, r] = math.fsum(prod[r]) if np.isfinite(prod[r]).all() else float(prod[r].sum())
        return out
