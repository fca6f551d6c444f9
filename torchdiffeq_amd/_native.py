"""ctypes binding of libtdeq_hip.so (include/tdeq_hip.h) and the tensor-level kernel interface.

`HipKernels` is the compute backend of the package: every state-sized arithmetic operation of the solvers on a
real fp32 / fp64 state on a ROCm device goes through it — `get_kernels()` raises if the library is missing, there is
no substitute on the GPU.  States the kernels do not take (not on a ROCm device, or complex) are served by the
torch-op `_fallback.HostKernels` behind the same interface.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import math
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

TDEQ_ABI_VERSION = 35
TDEQ_F32, TDEQ_F64 = 0, 1
TDEQ_C64, TDEQ_C128 = 2, 3        # interleaved complex: the norm entry points only (include/tdeq_hip.h)
TDEQ_BF16, TDEQ_F16 = 4, 5        # reduced-precision states: the entry points of the host-driven step (LowPrecisionHipKernels)
TDEQ_MAX_TERMS = 14
TDEQ_INLINE_SEGMENTS = 16
TDEQ_CHUNK_QUANTUM = 1024
TDEQ_MAX_STAGE_TIMES = 16
TDEQ_MAX_DENSE_OUTPUTS = 16
TDEQ_MAX_MULTI_OUT = 4
TDEQ_MAX_GATHER = 4

_LIB_NAME = "libtdeq_hip.so"
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)

_c_void_pp = ctypes.POINTER(ctypes.c_void_p)
_c_double_p = ctypes.POINTER(ctypes.c_double)


class Segment(ctypes.Structure):
    """`tdeq_segment` of include/tdeq_hip.h."""
    _fields_ = [("chunk_start", ctypes.c_int64), ("numel", ctypes.c_int64),
                ("rtol", ctypes.c_double), ("atol", ctypes.c_double)]


class StepCtrl(ctypes.Structure):
    """`tdeq_step_ctrl` of include/tdeq_hip.h: the scalar inputs of the device-resident step controller."""
    _fields_ = [("t0", ctypes.c_double), ("dt", ctypes.c_double), ("safety", ctypes.c_double),
                ("ifactor", ctypes.c_double), ("dfactor", ctypes.c_double), ("exponent", ctypes.c_double),
                ("min_step", ctypes.c_double), ("max_step", ctypes.c_double), ("time_sign", ctypes.c_double),
                ("alpha", ctypes.c_double * TDEQ_MAX_STAGE_TIMES), ("alpha_is_one", ctypes.c_uint32),
                ("n_times", ctypes.c_int32), ("n_norm_seg", ctypes.c_int32), ("leading_abs", ctypes.c_int32)]


def step_ctrl(alpha, alpha_is_one, order, safety, ifactor, dfactor, min_step, max_step, time_sign, n_norm_seg) -> StepCtrl:
    """A `StepCtrl` from the stage abscissae (`alpha_is_one`: which of them are exactly 1), the method's order, the
    controller's constants, the step bounds and the direction of time; t0 / dt are per step, `leading_abs` stays 0."""
    c = StepCtrl()
    c.safety, c.ifactor, c.dfactor = safety, ifactor, dfactor
    c.exponent = 1.0 / order
    c.min_step, c.max_step, c.time_sign = min_step, max_step, time_sign
    for i, a in enumerate(alpha):
        c.alpha[i] = float(a)
    c.alpha_is_one = sum(1 << i for i, one in enumerate(alpha_is_one) if one)
    c.n_times, c.n_norm_seg = len(alpha), n_norm_seg
    return c


class MultiOut(ctypes.Structure):
    """`tdeq_multi_out` of include/tdeq_hip.h: one output of tdeq_stage_combine_multi."""
    _fields_ = [("out", ctypes.c_void_p), ("coef", ctypes.c_double * TDEQ_MAX_TERMS), ("mask", ctypes.c_uint32),
                ("add_y0", ctypes.c_int32)]


class RowState(ctypes.Structure):
    """`tdeq_row_state` of include/tdeq_hip.h: the per-row device vectors of an `odeint_rowwise` solve."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("t0", "tprev", "dt", "h0", "tgrid", "active", "accepted", "out_lo",
                                                      "out_hi", "next_out", "since", "bad_y", "code", "n_acc", "n_rej",
                                                      "ratio", "status")] + \
               [("n_rows", ctypes.c_int64), ("row_len", ctypes.c_int64), ("max_num_steps", ctypes.c_int64),
                ("n_out", ctypes.c_int32), ("order", ctypes.c_int32)]


class RowPoints(ctypes.Structure):
    """`tdeq_row_points` of include/tdeq_hip.h: the per-row step bounds and the per-row `step_t` / `jump_t` tables of a
    rowwise solve, with the vectors `tdeq_row_control_points` keeps for them (a null pointer: absent)."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("step_t", "jump_t", "step_count", "jump_count", "next_step",
                                                      "next_jump", "clip_t", "on_point", "min_step", "max_step", "jumped",
                                                      "jump_times")] + \
               [("n_step", ctypes.c_int32), ("n_jump", ctypes.c_int32)] + \
               [("jump_hit", ctypes.c_void_p), ("jump_closed", ctypes.c_int32)]     # (ABI 30, `jump_dy`; zero: absent)


# name -> (restype, argtypes); the authoritative list of exported symbols (checked by the tests).
ABI_SIGNATURES = {
    "tdeq_abi_version": (ctypes.c_int, []),
    "tdeq_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "tdeq_stage_combine": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                          ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_void_p]),
    "tdeq_stage_combine_timed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                                ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tdeq_stage_combine_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                               ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_void_p, _c_double_p, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_error_norm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                       ctypes.c_int, ctypes.c_double, ctypes.POINTER(Segment),
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_error_norm_vec": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                           ctypes.c_double, ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_error_norm_vec_ctrl": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                                ctypes.c_double, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                                ctypes.c_double, ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(StepCtrl), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_init_norms_vec": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_double, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(Segment),
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_err": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                              _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_double,
                                              ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_multi": (ctypes.c_int, [ctypes.POINTER(MultiOut), ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, _c_void_pp, ctypes.c_int, ctypes.c_double,
                                                ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_multi_dev": (ctypes.c_int, [ctypes.POINTER(MultiOut), ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_void_p, _c_void_pp, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_multi_timed": (ctypes.c_int, [ctypes.POINTER(MultiOut), ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_void_p, _c_void_pp, ctypes.c_int, ctypes.c_double,
                                                      ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
    "tdeq_error_norm_partial": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                               _c_double_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(Segment),
                                               ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_error_norm_partial_ctrl": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                                    _c_double_p, ctypes.c_int, ctypes.c_double,
                                                    ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.POINTER(StepCtrl), ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                    ctypes.c_int, ctypes.c_void_p]),
    "tdeq_step_controller": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Segment), ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(StepCtrl), ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                              _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_void_p]),
    "tdeq_step_commit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int, ctypes.c_void_p]),
    "tdeq_stage_combine_sel": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_void_p]),
    "tdeq_init_norms": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_init_scaled": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_void_p]),
    "tdeq_dense_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_void_p]),
    "tdeq_dense_eval_multi": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                             ctypes.c_double, _c_double_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_void_p]),
    "tdeq_interp_fit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_rk4_38_stage": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_rk4_38_stage_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_grid_advance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p]),
    "tdeq_grid_commit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_grid_advance_stages": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_double, _c_double_p, ctypes.POINTER(ctypes.c_int),
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_void_p]),
    "tdeq_fixed_stage_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_lerp": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                 ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_fixed_stage": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p,
                                        ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_void_p]),
    "tdeq_weighted_sum": (ctypes.c_int, [ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int, ctypes.c_int64,
                                         ctypes.c_int, ctypes.c_void_p]),
    "tdeq_scale_many": (ctypes.c_int, [_c_void_pp, ctypes.c_void_p, _c_double_p, ctypes.c_int, ctypes.c_int64,
                                       ctypes.c_int, ctypes.c_void_p]),
    "tdeq_dots_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "tdeq_multi_dot": (ctypes.c_int, [ctypes.c_void_p, _c_void_pp, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_pack_segments": (ctypes.c_int, [ctypes.c_void_p, _c_void_pp, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64), _c_double_p, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_fill_scalars": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]),
    "tdeq_adams_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          _c_void_pp, _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_adams_correct": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                                          ctypes.POINTER(Segment), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    # per-row step control (ABI 22, rowwise.py)
    "tdeq_row_partials": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int]),
    "tdeq_row_combine": (ctypes.c_int, [ctypes.POINTER(MultiOut), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        _c_void_pp, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_reduce": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                       _c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_control": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(StepCtrl), ctypes.POINTER(RowState),
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_dense_commit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.POINTER(RowState), ctypes.c_int, ctypes.c_void_p]),
    # backward of the row-linear operations (ABI 23, rowwise_autodiff.py)
    "tdeq_row_scale_many": (ctypes.c_int, [_c_void_pp, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_dots_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "tdeq_row_multi_dot": (ctypes.c_int, [ctypes.c_void_p, _c_void_pp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                          ctypes.c_void_p]),
    # compaction of a rowwise batch (ABI 24, odeint_rowwise(compact=...))
    "tdeq_row_gather": (ctypes.c_int, [_c_void_pp, _c_void_pp, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_dense_commit_mapped": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                                    _c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(RowState),
                                                    ctypes.c_int, ctypes.c_void_p]),
    # per-row tolerances of the row reductions (ABI 25, odeint_rowwise(rtol=[B], atol=[B]))
    "tdeq_row_reduce_tol": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_void_pp,
                                           _c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    # per-row terminal events (ABI 26, rowwise_event.py)
    "tdeq_row_event_detect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(StepCtrl),
                                             ctypes.POINTER(RowState), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_void_p]),
    "tdeq_row_event_fit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, _c_void_pp, _c_double_p, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_event_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # compaction of an event solve (ABI 27, odeint_rowwise_event(compact=...))
    "tdeq_row_event_fit_mapped": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 _c_void_pp, _c_double_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_event_eval_mapped": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # per-row dense output (ABI 28, rowwise_dense.py)
    "tdeq_row_dense_slots": (ctypes.c_int, [ctypes.POINTER(RowState), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tdeq_row_dense_pack": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_dense_search": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_void_p]),
    # calculus on the per-row dense record (ABI 31, `RowDenseOutput.derivative` / `.antiderivative` / `.integral`)
    "tdeq_row_dense_prefix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_void_p]),
    "tdeq_row_dense_calc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # extrema of the per-row dense record over a time window (ABI 32, `RowDenseOutput.maximum` / `.minimum`)
    "tdeq_row_dense_extremum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # level crossings of the per-row dense record over a time window (ABI 33, `RowDenseOutput.crossings` / `.time_above`)
    "tdeq_row_dense_level": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                            ctypes.c_void_p]),
    # area above and below a level over a time window (ABI 34, `RowDenseOutput.exposure` / `.area_above` / `.area_below`)
    "tdeq_row_dense_exposure": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    # the times of all crossings of a level over a time window (ABI 35, `RowDenseOutput.crossing_times`)
    "tdeq_row_dense_level_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                  ctypes.c_int, ctypes.c_void_p]),
    # per-row step options (ABI 29, `min_step` / `max_step` / `step_t` / `jump_t` of the rowwise family)
    "tdeq_row_control_points": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(StepCtrl),
                                               ctypes.POINTER(RowState), ctypes.POINTER(RowPoints), ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tdeq_row_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_int, ctypes.c_void_p]),
    # state impulses at jump points (ABI 30, `jump_dy`)
    "tdeq_row_impulse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int, ctypes.c_void_p]),
}


class NativeLibraryError(RuntimeError):
    pass


def library_path() -> str:
    return _LIB_PATH


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the C-ABI library and bind every declared symbol.  Needs no GPU."""
    path = path or _LIB_PATH
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} not found: build it with `python -m torchdiffeq_amd.build` "
            "(hipcc --offload-arch=gfx950).  torchdiffeq_amd has no CPU/eager fallback.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in ABI_SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    version = lib.tdeq_abi_version()
    if version != TDEQ_ABI_VERSION:
        raise NativeLibraryError(f"{path}: ABI version {version}, expected {TDEQ_ABI_VERSION}")
    return lib


def dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return TDEQ_F32
    if dtype == torch.float64:
        return TDEQ_F64
    if dtype == torch.complex64:
        return TDEQ_C64
    if dtype == torch.complex128:
        return TDEQ_C128
    if dtype == torch.bfloat16:
        return TDEQ_BF16
    if dtype == torch.float16:
        return TDEQ_F16
    raise TypeError(f"torchdiffeq_amd supports float32 / float64 (and complex64 / complex128) states, got {dtype}")


def _check(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code} "
                           f"({'hipError_t' if code > 0 else 'argument error'})")


def pick_chunk(numel: int) -> int:
    """Elements per reduction chunk (one workgroup, one fp64 partial per chunk)."""
    env = os.environ.get("TDEQ_CHUNK")
    if env:
        return int(env)
    return 2048 if numel >= (1 << 20) else 1024


class NormPlan:
    """Segment table + workspace + read-back buffers of the norm kernels for one state layout.

    `segments` = [(element offset, numel, rtol, atol)]; offsets must be multiples of `chunk`.
    Results of the last norm launch are read with `HipKernels.read_norms(plan)`.
    """

    def __init__(self, segments: Sequence[Tuple[int, int, float, float]], total: int, chunk: int,
                 device: torch.device, pinned: bool):
        assert chunk % TDEQ_CHUNK_QUANTUM == 0
        self.chunk = chunk
        self.n_seg = len(segments)
        self.numels = [int(s[1]) for s in segments]
        self.n_chunks = max(1, math.ceil(total / chunk))
        arr = (Segment * self.n_seg)()
        for i, (off, numel, rtol, atol) in enumerate(segments):
            assert off % chunk == 0, "segment offsets must be chunk aligned"
            arr[i] = Segment(off // chunk, numel, float(rtol), float(atol))
        self.segs = arr
        self.segs_dev = None
        if self.n_seg > TDEQ_INLINE_SEGMENTS:
            raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
            self.segs_dev = torch.from_numpy(raw).to(device)
        self.workspace = torch.empty(3 * self.n_chunks, dtype=torch.float64, device=device)
        self.workspace_bytes = self.workspace.numel() * 8
        # [2*n_seg sums | n_seg non-finite counters | 4 controller words]; pinned host memory is written by
        # the finalize kernel directly (zero-copy), so a read-back is one stream sync and no memcpy.
        self.pinned = pinned
        self.expect = ()         # index ranges the pending norm launch will write (poll mode)
        if pinned:
            self.out = torch.zeros(3 * self.n_seg + 4, dtype=torch.float64, device="cpu", pin_memory=True)
            self.out_np = self.out.numpy()
            self.out_bits = self.out_np.view(np.uint64)
        else:
            self.out = torch.zeros(3 * self.n_seg + 4, dtype=torch.float64, device=device)
            self.out_np = None
        self.out_ptr = self.out.data_ptr()
        self.bad_ptr = self.out_ptr + 16 * self.n_seg
        self.ctrl_ptr = self.out_ptr + 24 * self.n_seg
        # {accept, sign * T(dt'), t0', dt'} of the device-resident controller (tdeq_stage_combine_sel, hipGraph mode)
        self.ctrl_dev = torch.zeros(4, dtype=torch.float64, device=device)


class HipKernels:
    """Tensor-level wrappers of the C-ABI.  All launches go to the current torch HIP stream."""

    name = "hip"

    # Read-back modes (TDEQ_READBACK): "poll" (default) = the finalize kernel stores into pinned host
    # memory and the host spins on those words (each entry is one aligned 8-byte store, pre-set to a
    # sentinel NaN payload) — no driver-level stream sync on the critical path of the accept/reject loop;
    # "pinned" = same zero-copy store, waited for with a stream synchronize; "copy" = device buffer + memcpy.
    _SENTINEL = np.uint64(0x7FF8DEADBEEF0001)
    _POLL_TIMEOUT_S = 5.0

    def __init__(self, lib: ctypes.CDLL):
        self.lib = lib
        mode = os.environ.get("TDEQ_READBACK", "poll")
        if mode not in ("poll", "pinned", "copy"):
            raise ValueError(f"TDEQ_READBACK={mode!r}: expected poll | pinned | copy")
        self._mode = mode
        self._pinned = mode in ("poll", "pinned")

    def _arm(self, plan: "NormPlan", n_sum: int, ctrl: bool = False) -> None:
        """Before a norm launch in poll mode: mark the entries the launch will overwrite."""
        if self._mode == "poll" and plan.pinned:
            n = plan.n_seg
            plan.out_bits[:n_sum * n] = self._SENTINEL
            plan.out_bits[2 * n:3 * n + (4 if ctrl else 0)] = self._SENTINEL
            plan.expect = ((0, n_sum * n), (2 * n, 3 * n + (4 if ctrl else 0)))

    # -- helpers ---------------------------------------------------------------------------------
    # The raw hipStream_t of the CURRENT device's current torch stream.  `torch.cuda.current_stream().cuda_stream`
    # gives the same value but costs 4–8 us of host time per call (device-index resolution, an `is_available()` probe
    # that reads os.environ, a Stream object) — seven calls per trial step, 12–17 % of the host time of a launch-bound
    # step (tools/host_profile2.py, r02); the C accessors below cost ~0.2 us.
    _raw_stream = staticmethod(getattr(torch._C, "_cuda_getCurrentRawStream", None))
    _cur_device = staticmethod(getattr(torch._C, "_cuda_getDevice", None))

    @classmethod
    def _stream(cls) -> int:
        if cls._raw_stream is not None and cls._cur_device is not None:
            return cls._raw_stream(cls._cur_device())
        return torch.cuda.current_stream().cuda_stream

    # Host-side argument marshalling is on the critical path of small / medium states.  The entry points copy the
    # host arrays into the kernel-argument block before they return, so one pointer array per term count is reused
    # (overwritten per call) and the coefficient arrays of the (immutable, few) tableau rows are built once.
    # (ctypes releases the GIL during a call: the reused pointer arrays are per thread.)
    _TLS = threading.local()
    _COEF_ARRAYS: dict = {}
    _PACK_TABLES: dict = {}

    @classmethod
    def _terms(cls, ks: Sequence[torch.Tensor], coefs: Sequence[float]):
        n = len(ks)
        if n > TDEQ_MAX_TERMS:
            ptrs = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
        else:
            arrays = getattr(cls._TLS, "ptr_arrays", None)
            if arrays is None:
                arrays = cls._TLS.ptr_arrays = [(ctypes.c_void_p * m)() for m in range(TDEQ_MAX_TERMS + 1)]
            ptrs = arrays[n]
            for j in range(n):
                ptrs[j] = ks[j].data_ptr()
        if isinstance(coefs, tuple):        # (a tableau row's RowCoefs included)
            cf = cls._COEF_ARRAYS.get(coefs)
            if cf is None:
                if len(cls._COEF_ARRAYS) > 4096:      # not a tableau row cache any more: start over
                    cls._COEF_ARRAYS.clear()
                cf = cls._COEF_ARRAYS[coefs] = (ctypes.c_double * n)(*coefs)
        else:
            cf = (ctypes.c_double * n)(*coefs)
        return ptrs, cf, n

    def make_plan(self, segments, total, chunk, device) -> NormPlan:
        return NormPlan(segments, total, chunk, device, self._pinned)

    # -- kernels ---------------------------------------------------------------------------------
    def stage_combine(self, out, y0, ks, coefs, dt: float) -> None:
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_stage_combine(out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                           dtype_code(y0.dtype), self._stream()), "tdeq_stage_combine")

    def stage_combine_timed(self, out, y0, ks, coefs, dt: float, start_event, stop_event) -> None:
        """`stage_combine` whose dispatch stamps two torch.cuda.Event(enable_timing=True) objects with its own begin /
        end times (measurement hook, see include/tdeq_hip.h).  The events must have been recorded once before (torch
        creates the underlying hipEvent_t lazily)."""
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_stage_combine_timed(out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                                 dtype_code(y0.dtype), self._stream(), start_event.cuda_event,
                                                 stop_event.cuda_event), "tdeq_stage_combine_timed")

    def stage_combine_fill(self, out, y0, ks, coefs, dt: float, fill_dst, fill_vals) -> None:
        """stage_combine of a step's first stage that also writes `fill_vals` (stage times) into `fill_dst`."""
        ptrs, cf, n = self._terms(ks, coefs)
        m = len(fill_vals)
        fv = (ctypes.c_double * m)(*fill_vals)
        _check(self.lib.tdeq_stage_combine_fill(out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                                dtype_code(y0.dtype), fill_dst.data_ptr(), fv, m, self._stream()),
               "tdeq_stage_combine_fill")

    def error_norm(self, plan: NormPlan, y0, y1, ks, coefs, dt: float, scaled_out=None) -> None:
        ptrs, cf, n = self._terms(ks, coefs)
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        so = None if scaled_out is None else scaled_out.data_ptr()
        self._arm(plan, 1)
        _check(self.lib.tdeq_error_norm(so, y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt, plan.segs, dev,
                                        plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr,
                                        plan.workspace.data_ptr(), plan.workspace_bytes,
                                        dtype_code(y0.dtype), self._stream()), "tdeq_error_norm")

    vec_partial = True      # error_norm_vec[_ctrl] continue a partial error row (`partial=`) like error_norm_partial

    vec_ctrl_in_graph = True     # tdeq_error_norm_vec_ctrl takes `state_in_dev` (ABI 21): captured steps with per-element tolerances

    def error_norm_vec(self, plan: NormPlan, y0, y1, ks, coefs, dt: float, rtol, atol, partial=None) -> None:
        """`error_norm` with per-element tolerances (tdeq_error_norm_vec): `rtol` / `atol` = an fp64 device vector over the
        flat padded state, or a host float for a 0-dim tolerance (at least one vector).  `partial`: the error row's leading
        run from `stage_combine_err`; `ks` / `coefs` are the remaining stages then."""
        ptrs, cf, n = self._terms(ks, coefs)
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        rv, rs = (rtol.data_ptr(), 0.0) if isinstance(rtol, torch.Tensor) else (None, float(rtol))
        av, as_ = (atol.data_ptr(), 0.0) if isinstance(atol, torch.Tensor) else (None, float(atol))
        self._arm(plan, 1)
        pp = None if partial is None else partial.data_ptr()
        _check(self.lib.tdeq_error_norm_vec(pp, y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt, rv, rs, av, as_, plan.segs, dev,
                                            plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr,
                                            plan.workspace.data_ptr(), plan.workspace_bytes, dtype_code(y0.dtype),
                                            self._stream()), "tdeq_error_norm_vec")

    def error_norm_vec_ctrl(self, plan: NormPlan, y0, y1, ks, coefs, dt: float, rtol, atol, ctrl: StepCtrl, next_times,
                            partial=None, state_in_dev: bool = False) -> None:
        """`error_norm_vec` whose finalize step also runs the step controller on the device (tdeq_error_norm_vec_ctrl) —
        read with `read_ctrl`.  `state_in_dev` (captured steps): the step size comes from `plan.ctrl_dev`, `dt` is ignored."""
        ptrs, cf, n = self._terms(ks, coefs)
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        rv, rs = (rtol.data_ptr(), 0.0) if isinstance(rtol, torch.Tensor) else (None, float(rtol))
        av, as_ = (atol.data_ptr(), 0.0) if isinstance(atol, torch.Tensor) else (None, float(atol))
        self._arm(plan, 1, ctrl=True)
        pp = None if partial is None else partial.data_ptr()
        _check(self.lib.tdeq_error_norm_vec_ctrl(pp, y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt, rv, rs, av, as_, plan.segs,
                                                 dev, plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr,
                                                 ctypes.byref(ctrl), plan.ctrl_ptr, plan.ctrl_dev.data_ptr(),
                                                 next_times.data_ptr(), 1 if state_in_dev else 0, plan.workspace.data_ptr(),
                                                 plan.workspace_bytes, dtype_code(y0.dtype), self._stream()),
               "tdeq_error_norm_vec_ctrl")

    def init_norms_vec(self, plan: NormPlan, mode: int, a, b, yscale, rtol, atol) -> None:
        """`init_norms` with per-element tolerances (tdeq_init_norms_vec): `rtol` / `atol` = an fp64 device vector over the
        flat padded state, or a host float for a 0-dim tolerance (at least one vector); sums in fp64, the promoted type."""
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        rv, rs = (rtol.data_ptr(), 0.0) if isinstance(rtol, torch.Tensor) else (None, float(rtol))
        av, as_ = (atol.data_ptr(), 0.0) if isinstance(atol, torch.Tensor) else (None, float(atol))
        self._arm(plan, 2 if mode == 0 else 1)
        _check(self.lib.tdeq_init_norms_vec(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), rv, rs, av, as_, plan.segs, dev,
                                            plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr,
                                            plan.workspace.data_ptr(), plan.workspace_bytes, dtype_code(yscale.dtype),
                                            self._stream()), "tdeq_init_norms_vec")

    def stage_combine_err(self, out, err_out, y0, ks, coefs, err_coefs, dt: float) -> None:
        """Last combine of a step + partial embedded error over the same stages (tdeq_stage_combine_err)."""
        ptrs, cf, n = self._terms(ks, coefs)
        ef = (ctypes.c_double * n)(*err_coefs)
        _check(self.lib.tdeq_stage_combine_err(out.data_ptr(), err_out.data_ptr(), y0.data_ptr(), ptrs, cf, ef, n, dt,
                                               y0.numel(), dtype_code(y0.dtype), self._stream()),
               "tdeq_stage_combine_err")

    _MULTI_SPECS: dict = {}

    @classmethod
    def multi_spec(cls, rows):
        """The constant part of a tdeq_stage_combine_multi call, built once per tableau row group: `rows` =
        ((coefs over the call's stage streams, mask, add_y0), ...), one entry per output.  Returns a `tdeq_multi_out`
        array whose `out` pointers are filled in per call (per thread: ctypes releases the GIL during a call)."""
        per_thread = getattr(cls._TLS, "multi_specs", None)
        if per_thread is None:
            per_thread = cls._TLS.multi_specs = {}
        arr = per_thread.get(rows)
        if arr is None:
            if len(per_thread) > 1024:
                per_thread.clear()
            arr = (MultiOut * len(rows))()
            for o, (coefs, mask, add_y0) in enumerate(rows):
                assert len(coefs) <= TDEQ_MAX_TERMS and mask
                for j, c in enumerate(coefs):
                    arr[o].coef[j] = c
                arr[o].mask = mask
                arr[o].add_y0 = 1 if add_y0 else 0
            per_thread[rows] = arr
        return arr

    def stage_combine_multi_dev(self, outs, rows, y0, acc_in, ks, plan: "NormPlan") -> None:
        """`stage_combine_multi` with the step size read on the device from the plan's controller words (hipGraph mode)."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
        spec = self.multi_spec(rows)
        for o, t in enumerate(outs):
            spec[o].out = t.data_ptr()
        _check(self.lib.tdeq_stage_combine_multi_dev(spec, len(outs), y0.data_ptr(),
                                                     None if acc_in is None else acc_in.data_ptr(), ptrs, n,
                                                     plan.ctrl_dev.data_ptr(), y0.numel(), dtype_code(y0.dtype),
                                                     self._stream()), "tdeq_stage_combine_multi_dev")

    def stage_combine_multi(self, outs, rows, y0, acc_in, ks, dt: float, events=None) -> None:
        """One pass over the stages `ks` producing len(outs) tensors (tdeq_stage_combine_multi): output o =
        [y0 +] [acc_in +] sum over the set bits j of rows[o].mask of (rows[o].coefs[j] * dt) * ks[j] — a row's own
        stage input plus carried left-to-right partial sums of later rows.  `rows` as for `multi_spec` (a tuple)."""
        n = len(ks)
        arrays = getattr(self._TLS, "ptr_arrays", None)
        if arrays is None:
            arrays = self._TLS.ptr_arrays = [(ctypes.c_void_p * m)() for m in range(TDEQ_MAX_TERMS + 1)]
        ptrs = arrays[n]
        for j in range(n):
            ptrs[j] = ks[j].data_ptr()
        spec = self.multi_spec(rows)
        for o, t in enumerate(outs):
            spec[o].out = t.data_ptr()
        if events is not None:      # measurement hook: (start, stop) torch events stamped by the dispatch itself
            _check(self.lib.tdeq_stage_combine_multi_timed(
                spec, len(outs), y0.data_ptr(), None if acc_in is None else acc_in.data_ptr(), ptrs, n, dt, y0.numel(),
                dtype_code(y0.dtype), self._stream(), events[0].cuda_event, events[1].cuda_event),
                "tdeq_stage_combine_multi_timed")
            return
        _check(self.lib.tdeq_stage_combine_multi(spec, len(outs), y0.data_ptr(),
                                                 None if acc_in is None else acc_in.data_ptr(), ptrs, n, dt,
                                                 y0.numel(), dtype_code(y0.dtype), self._stream()),
               "tdeq_stage_combine_multi")

    def error_norm_partial(self, plan: NormPlan, err_partial, y0, y1, ks, coefs, dt: float) -> None:
        """Error norm continuing `err_partial` with the remaining stages `ks` (0..2 of them)."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        self._arm(plan, 1)
        _check(self.lib.tdeq_error_norm_partial(err_partial.data_ptr(), y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt,
                                                plan.segs, dev, plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr,
                                                plan.bad_ptr, plan.workspace.data_ptr(), plan.workspace_bytes,
                                                dtype_code(y0.dtype), self._stream()), "tdeq_error_norm_partial")

    def error_scaled(self, plan: NormPlan, out, y0, y1, ks, coefs, dt: float) -> None:
        """err/tol materialised into `out` (for user norm callables); norms are produced as well."""
        self.error_norm(plan, y0, y1, ks, coefs, dt, scaled_out=out)

    def init_norms(self, plan: NormPlan, mode: int, a, b, yscale) -> None:
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        self._arm(plan, 2 if mode == 0 else 1)
        _check(self.lib.tdeq_init_norms(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), plan.segs, dev,
                                        plan.n_seg, plan.chunk, plan.n_chunks, plan.out_ptr, plan.bad_ptr,
                                        plan.workspace.data_ptr(), plan.workspace_bytes,
                                        dtype_code(yscale.dtype), self._stream()), "tdeq_init_norms")

    def init_scaled(self, plan: NormPlan, mode: int, a, b, yscale, out0, out1=None) -> None:
        """a/scale, b/scale (mode 0) or (a-b)/scale (mode 1) materialised for a user norm (tdeq_init_scaled)."""
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        _check(self.lib.tdeq_init_scaled(mode, a.data_ptr(), b.data_ptr(), yscale.data_ptr(), plan.segs, dev,
                                         plan.n_seg, plan.chunk, plan.n_chunks, out0.data_ptr(),
                                         None if out1 is None else out1.data_ptr(), dtype_code(yscale.dtype),
                                         self._stream()), "tdeq_init_scaled")

    def read_norms(self, plan: NormPlan) -> Tuple[List[float], List[float], List[float]]:
        """(sumsq[0:n_seg], sumsq[n_seg:2n_seg], nonfinite[0:n_seg]) of the last norm launch."""
        n = plan.n_seg
        v = self._read_out(plan)
        return v[:n], v[n:2 * n], v[2 * n:3 * n]

    def _read_out(self, plan: NormPlan) -> List[float]:
        """All words of the plan's result buffer once the pending norm launch has written its share."""
        if plan.pinned and self._mode == "poll" and plan.expect:
            bits, sent = plan.out_bits, self._SENTINEL
            (a0, a1), (b0, b1) = plan.expect
            spins, t_start = 0, None
            while (bits[a0:a1] == sent).any() or (bits[b0:b1] == sent).any():
                spins += 1
                if spins & 0x3FFF == 0:       # every 16k spins: bounded wait, then fall back to a real sync
                    import time
                    t_start = t_start or time.monotonic()
                    if time.monotonic() - t_start > self._POLL_TIMEOUT_S:
                        torch.cuda.current_stream().synchronize()
                        if (bits[a0:a1] == sent).any() or (bits[b0:b1] == sent).any():
                            raise RuntimeError("norm kernel did not write its results (poll timeout)")
                        break
            plan.expect = ()
            return plan.out_np.tolist()
        if plan.pinned:
            torch.cuda.current_stream().synchronize()
            return plan.out_np.tolist()
        return plan.out.tolist()

    norm_copies_last_stage = True       # tdeq_error_norm_partial_ctrl(copy_last_k=...), ABI 21

    def error_norm_partial_ctrl(self, plan: NormPlan, err_partial, y0, y1, ks, coefs, dt: float, ctrl: StepCtrl,
                                next_times, state_in_dev: bool = False, copy_last_to=None) -> None:
        """`error_norm_partial` whose finalize step also runs the step controller on the device: accept flag,
        next step size and the next trial step's stage times (`next_times`, T[n_times]) — read with `read_ctrl`.
        `copy_last_to` (captured steps): the launch also writes `ks[-1]` into this buffer."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        self._arm(plan, 1, ctrl=True)
        _check(self.lib.tdeq_error_norm_partial_ctrl(
            err_partial.data_ptr(), y0.data_ptr(), y1.data_ptr(), ptrs, cf, n, dt, plan.segs,
            plan.segs_dev.data_ptr() if plan.segs_dev is not None else None, plan.n_seg, plan.chunk,
            plan.n_chunks, plan.out_ptr, plan.bad_ptr, ctypes.byref(ctrl), plan.ctrl_ptr, plan.ctrl_dev.data_ptr(),
            next_times.data_ptr(), 1 if state_in_dev else 0, None if copy_last_to is None else copy_last_to.data_ptr(),
            plan.workspace.data_ptr(), plan.workspace_bytes, dtype_code(y0.dtype), self._stream()),
            "tdeq_error_norm_partial_ctrl")

    def step_controller(self, plan: NormPlan, sums_plan: NormPlan, numel_plan: NormPlan, ctrl: StepCtrl, next_times,
                        dtype: torch.dtype, state_in_dev: bool = False) -> None:
        """The controller alone (tdeq_step_controller) on the per-segment sums in `sums_plan.out` (DEVICE memory: a
        plan made with pinned=False, filled by a norm launch and all-reduced over the ranks of a lock-step sharded
        solve), with the element counts of `numel_plan`'s segment table (the GLOBAL counts); results land in `plan`
        like those of `error_norm_partial_ctrl` — read with `read_ctrl(plan)`."""
        assert not sums_plan.pinned and sums_plan.n_seg == plan.n_seg == numel_plan.n_seg
        self._arm(plan, 1, ctrl=True)
        _check(self.lib.tdeq_step_controller(
            sums_plan.out_ptr, sums_plan.bad_ptr, numel_plan.segs,
            numel_plan.segs_dev.data_ptr() if numel_plan.segs_dev is not None else None, plan.n_seg, plan.out_ptr,
            plan.bad_ptr, ctypes.byref(ctrl), plan.ctrl_ptr, plan.ctrl_dev.data_ptr(), next_times.data_ptr(),
            1 if state_in_dev else 0, dtype_code(dtype), self._stream()), "tdeq_step_controller")

    def read_ctrl(self, plan: NormPlan) -> Tuple[bool, float, float, List[float]]:
        """(accept, dt_next, error_ratio, nonfinite[0:n_seg]) of the last `error_norm_partial_ctrl` launch."""
        n = plan.n_seg
        v = self._read_out(plan)
        return v[3 * n] != 0.0, v[3 * n + 1], v[3 * n + 2], v[2 * n:3 * n]

    def stage_combine_dev(self, out, err_out, y0, ks, coefs, err_coefs, plan: NormPlan) -> None:
        """stage_combine / stage_combine_err (err_out given) with the step size read on the device from the plan's
        controller words (hipGraph mode)."""
        ptrs, cf, n = self._terms(ks, coefs)
        ef = None if err_coefs is None else (ctypes.c_double * n)(*err_coefs)
        _check(self.lib.tdeq_stage_combine_dev(out.data_ptr(), None if err_out is None else err_out.data_ptr(),
                                               y0.data_ptr(), ptrs, cf, ef, n, plan.ctrl_dev.data_ptr(), y0.numel(),
                                               dtype_code(y0.dtype), self._stream()), "tdeq_stage_combine_dev")

    def step_commit(self, y_prev, f_prev, y_cur, f_cur, y1, f1, plan: NormPlan) -> None:
        _check(self.lib.tdeq_step_commit(y_prev.data_ptr(), f_prev.data_ptr(), y_cur.data_ptr(), f_cur.data_ptr(),
                                         y1.data_ptr(), f1.data_ptr(), plan.ctrl_dev.data_ptr(), y_cur.numel(),
                                         dtype_code(y_cur.dtype), self._stream()), "tdeq_step_commit")

    def arm_readback(self, plan: NormPlan, n_sum: int = 1, ctrl: bool = True) -> None:
        """Mark the words a norm launch inside a replayed hipGraph is about to write (poll mode)."""
        self._arm(plan, n_sum, ctrl=ctrl)

    def stage_combine_sel(self, out, y_acc, f_acc, y_rej, f_rej, coef: float, plan: NormPlan) -> None:
        """First stage of the next trial step on the pair the device controller selected (tdeq_stage_combine_sel)."""
        _check(self.lib.tdeq_stage_combine_sel(out.data_ptr(), y_acc.data_ptr(), f_acc.data_ptr(), y_rej.data_ptr(),
                                               f_rej.data_ptr(), coef, plan.ctrl_dev.data_ptr(), out.numel(),
                                               dtype_code(out.dtype), self._stream()), "tdeq_stage_combine_sel")

    def dense_eval(self, out, y0, y1, f0, f1, ks, coefs, dt: float, x: float) -> None:
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_dense_eval(out.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(),
                                        f1.data_ptr(), ptrs, cf, n, dt, x, y0.numel(),
                                        dtype_code(y0.dtype), self._stream()), "tdeq_dense_eval")

    def dense_eval_multi(self, out_rows, y0, y1, f0, f1, ks, coefs, dt: float, xs: Sequence[float]) -> None:
        """Dense output at several points of ONE step: out_rows[q] = y(x_q) for the rows of a contiguous
        [len(xs), n] tensor (a slice of the solution)."""
        ptrs, cf, n = self._terms(ks, coefs)
        m = len(xs)
        xa = (ctypes.c_double * m)(*xs)
        _check(self.lib.tdeq_dense_eval_multi(out_rows.data_ptr(), out_rows.stride(0) if m > 1 else y0.numel(),
                                              y0.data_ptr(), y1.data_ptr(), f0.data_ptr(), f1.data_ptr(), ptrs, cf, n,
                                              dt, xa, m, y0.numel(), dtype_code(y0.dtype), self._stream()),
               "tdeq_dense_eval_multi")

    def interp_fit(self, coeffs, y0, y1, f0, f1, ks, coefs, dt: float) -> None:
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_interp_fit(coeffs.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(),
                                        f1.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                        dtype_code(y0.dtype), self._stream()), "tdeq_interp_fit")

    def rk4_stage(self, stage: int, out, y0, k1, k2, k3, k4, dt: float) -> None:
        p = lambda t: None if t is None else t.data_ptr()
        _check(self.lib.tdeq_rk4_38_stage(stage, out.data_ptr(), y0.data_ptr(), p(k1), p(k2), p(k3), p(k4),
                                          dt, y0.numel(), dtype_code(y0.dtype), self._stream()),
               "tdeq_rk4_38_stage")

    # -- hipGraph mode of the fixed-grid rk4 solver (device-resident step state) -----------------------
    def rk4_stage_dev(self, stage: int, out, y0, k1, k2, k3, k4, dt_dev) -> None:
        p = lambda t: None if t is None else t.data_ptr()
        _check(self.lib.tdeq_rk4_38_stage_dev(stage, out.data_ptr(), y0.data_ptr(), p(k1), p(k2), p(k3), p(k4),
                                              dt_dev.data_ptr(), y0.numel(), dtype_code(y0.dtype), self._stream()),
               "tdeq_rk4_38_stage_dev")

    def grid_advance(self, grid, counter, perturb: bool, sign: float, times_out, dt_out) -> None:
        _check(self.lib.tdeq_grid_advance(grid.data_ptr(), dtype_code(grid.dtype), grid.numel(), counter.data_ptr(),
                                          1 if perturb else 0, sign, times_out.data_ptr(), dt_out.data_ptr(),
                                          dtype_code(times_out.dtype), self._stream()), "tdeq_grid_advance")

    def grid_advance_stages(self, grid, counter, perturb: bool, sign: float, fracs, modes, times_out, dt_out) -> None:
        """tdeq_grid_advance_stages: the next step's dt and stage times t0 + dt*frac_i / t1 (mode bits: 1 = t1,
        2 = Perturb.NEXT, 4 = Perturb.PREV), formed on the device."""
        n = len(fracs)
        fr = (ctypes.c_double * n)(*fracs)
        md = (ctypes.c_int * n)(*modes)
        _check(self.lib.tdeq_grid_advance_stages(grid.data_ptr(), dtype_code(grid.dtype), grid.numel(),
                                                 counter.data_ptr(), 1 if perturb else 0, sign, fr, md, n,
                                                 times_out.data_ptr(), dt_out.data_ptr(), dtype_code(times_out.dtype),
                                                 self._stream()), "tdeq_grid_advance_stages")

    def fixed_stage_dev(self, mode: int, out, y0, ks, ws, dt_dev) -> None:
        """fixed_stage with the step size read from device memory (hipGraph mode)."""
        ptrs, cf, n = self._terms(ks, ws)
        _check(self.lib.tdeq_fixed_stage_dev(mode, out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt_dev.data_ptr(),
                                             y0.numel(), dtype_code(y0.dtype), self._stream()), "tdeq_fixed_stage_dev")

    def grid_commit(self, solution, y_cur, y_new, counter) -> None:
        _check(self.lib.tdeq_grid_commit(solution.data_ptr(), solution.stride(0), y_cur.data_ptr(), y_new.data_ptr(),
                                         counter.data_ptr(), y_cur.numel(), dtype_code(y_cur.dtype), self._stream()),
               "tdeq_grid_commit")

    def lerp(self, out, y0, y1, slope: float) -> None:
        _check(self.lib.tdeq_lerp(out.data_ptr(), y0.data_ptr(), y1.data_ptr(), slope, y0.numel(),
                                  dtype_code(y0.dtype), self._stream()), "tdeq_lerp")

    def fixed_stage(self, mode: int, out, y0, ks, ws, dt: float) -> None:
        """mode 0: out = y0 + dt*(sum_j k_j*w_j); mode 1: out = y0 + (dt*k_0)*w_0 (low-order fixed-grid steps)."""
        ptrs, cf, n = self._terms(ks, ws)
        _check(self.lib.tdeq_fixed_stage(mode, out.data_ptr(), y0.data_ptr(), ptrs, cf, n, dt, y0.numel(),
                                         dtype_code(y0.dtype), self._stream()), "tdeq_fixed_stage")

    def weighted_sum(self, out, xs, ws) -> None:
        """out = (x_0*w_0 + x_1*w_1) + ... (left to right)."""
        ptrs, cf, n = self._terms(xs, ws)
        _check(self.lib.tdeq_weighted_sum(out.data_ptr(), ptrs, cf, n, out.numel(), dtype_code(out.dtype),
                                          self._stream()), "tdeq_weighted_sum")

    def scale_many(self, outs, g, ws) -> None:
        """outs[m] = ws[m] * g (backward of the linear kernels: g is read once)."""
        ptrs, cf, n = self._terms(outs, ws)
        _check(self.lib.tdeq_scale_many(ptrs, g.data_ptr(), cf, n, g.numel(), dtype_code(g.dtype), self._stream()),
               "tdeq_scale_many")

    def multi_dot(self, g, xs) -> torch.Tensor:
        """fp64 device tensor [len(xs)] of <g, x_m> (no host read-back)."""
        n = len(xs)
        ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
        out = torch.empty(n, dtype=torch.float64, device=g.device)
        nbytes = self.lib.tdeq_dots_workspace_bytes(g.numel(), n)
        ws = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=g.device)
        _check(self.lib.tdeq_multi_dot(g.data_ptr(), ptrs, n, g.numel(), out.data_ptr(), ws.data_ptr(), nbytes,
                                       dtype_code(g.dtype), self._stream()), "tdeq_multi_dot")
        return out

    # -- Adams–Bashforth(–Moulton) -----------------------------------------------------------------
    def adams_predict(self, y_out, y0, hist, cb, cm=None, dt: float = 0.0, dy_out=None, delta_out=None) -> None:
        """y_out = y0 + sum_j T(cb_j) f_j [, dy_out = that sum, delta_out = T(dt) * sum_j T(cm_j) f_j] in one pass over
        the history `hist` (newest first) — tdeq_adams_predict."""
        ptrs, cbf, n = self._terms(hist, cb)
        cmf = None if cm is None else (ctypes.c_double * n)(*cm)
        p = lambda t: None if t is None else t.data_ptr()
        _check(self.lib.tdeq_adams_predict(y_out.data_ptr(), p(dy_out), p(delta_out), y0.data_ptr(), ptrs, cbf, cmf, n,
                                           dt, y0.numel(), dtype_code(y0.dtype), self._stream()), "tdeq_adams_predict")

    def adams_correct(self, plan: NormPlan, dy_out, dy_old, y_out=None, f=None, delta=None, y0=None, c: float = 0.0,
                      compute: bool = True) -> None:
        """One corrector iteration (dy_out = T(c) f + delta, y_out = y0 + dy_out) fused with its convergence census;
        compute=False: census of (dy_old, dy_out) only.  Read the per-segment counts with `read_norms(plan)`."""
        p = lambda t: None if t is None else t.data_ptr()
        dev = plan.segs_dev.data_ptr() if plan.segs_dev is not None else None
        self._arm(plan, 1)
        _check(self.lib.tdeq_adams_correct(p(y_out), dy_out.data_ptr(), p(f), p(delta), dy_old.data_ptr(), p(y0), c,
                                           1 if compute else 0, plan.segs, dev, plan.n_seg, plan.chunk, plan.n_chunks,
                                           dy_out.numel(), plan.out_ptr, plan.bad_ptr, plan.workspace.data_ptr(),
                                           plan.workspace_bytes, dtype_code(dy_out.dtype), self._stream()),
               "tdeq_adams_correct")

    def pack_segments(self, out, srcs, chunk_starts: Sequence[int], numels: Sequence[int], scales: Sequence[float],
                      chunk: int) -> None:
        """out (a whole number of chunks) <- the pieces `srcs` (contiguous tensors of out's dtype, or None = zeros) at
        their chunk-aligned segment starts, times +-1; padding zero-filled.  One launch (tdeq_pack_segments)."""
        n = len(srcs)
        ptrs = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in srcs])
        # the three constant tables of a layout are converted once (keyed by identity-stable tuples)
        key = (tuple(chunk_starts), tuple(numels), tuple(scales))
        tabs = self._PACK_TABLES.get(key)
        if tabs is None:
            if len(self._PACK_TABLES) > 1024:
                self._PACK_TABLES.clear()
            tabs = self._PACK_TABLES[key] = ((ctypes.c_int64 * n)(*chunk_starts), (ctypes.c_int64 * n)(*numels),
                                             (ctypes.c_double * n)(*scales))
        cs, nm, sc = tabs
        _check(self.lib.tdeq_pack_segments(out.data_ptr(), ptrs, cs, nm, sc, n, chunk, out.numel() // chunk,
                                           dtype_code(out.dtype), self._stream()), "tdeq_pack_segments")

    def fill_scalars(self, dst, vals: Sequence[float]) -> None:
        n = len(vals)
        arr = (ctypes.c_double * n)(*vals)
        _check(self.lib.tdeq_fill_scalars(dst.data_ptr(), arr, n, dtype_code(dst.dtype), self._stream()),
               "tdeq_fill_scalars")

    # -- per-row step control (odeint_rowwise, rowwise.py) ---------------------------------------------------------
    # States are [B, L] tensors; `dts` = sign * T(dt_r) per row, `active` int32 per row; `st` a RowState.
    def row_partials(self, row_len: int, dtype) -> int:
        """fp64 partials per row of the row reductions (a function of L and the dtype only)."""
        return int(self.lib.tdeq_row_partials(row_len, dtype_code(dtype)))

    def row_combine(self, outs, rows, y0, acc_in, ks, dts, active) -> None:
        """tdeq_row_combine: `rows` as for `multi_spec`, one entry per output; the step size of each row from `dts`."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
        spec = self.multi_spec(rows)
        for o, t in enumerate(outs):
            spec[o].out = t.data_ptr()
        _check(self.lib.tdeq_row_combine(spec, len(outs), y0.data_ptr(), None if acc_in is None else acc_in.data_ptr(),
                                         ptrs, n, dts.data_ptr(), active.data_ptr(), y0.shape[0], y0.shape[1],
                                         dtype_code(y0.dtype), self._stream()), "tdeq_row_combine")

    def row_reduce(self, mode: int, part, y0, y1, partial, ks, coefs, dts, active, rtol: float, atol: float) -> None:
        """tdeq_row_reduce into `part` (fp64, 3 * B * row_partials)."""
        n = len(ks)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        _check(self.lib.tdeq_row_reduce(mode, y0.data_ptr(), y1.data_ptr(), None if partial is None else partial.data_ptr(),
                                        ptrs, cf, n, None if dts is None else dts.data_ptr(),
                                        None if active is None else active.data_ptr(), rtol, atol, y0.shape[0],
                                        y0.shape[1], part.data_ptr(), part.numel() * 8, dtype_code(y0.dtype),
                                        self._stream()), "tdeq_row_reduce")

    def row_reduce_tol(self, mode: int, part, y0, y1, partial, ks, coefs, dts, active, rtol_rows, atol_rows) -> None:
        """tdeq_row_reduce_tol: `row_reduce` with the tolerances of each row from two contiguous [B] tensors of the
        state's dtype on its device."""
        n = len(ks)
        for v in (rtol_rows, atol_rows):
            if v.shape != (y0.shape[0],) or v.dtype != y0.dtype or v.device != y0.device or not v.is_contiguous():
                raise ValueError("row_reduce_tol: the tolerances must be contiguous [B] tensors of the state's dtype on "
                                 "its device")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[k.data_ptr() for k in ks])
        cf = (ctypes.c_double * max(n, 1))(*coefs)
        _check(self.lib.tdeq_row_reduce_tol(mode, y0.data_ptr(), y1.data_ptr(),
                                            None if partial is None else partial.data_ptr(), ptrs, cf, n,
                                            None if dts is None else dts.data_ptr(),
                                            None if active is None else active.data_ptr(), rtol_rows.data_ptr(),
                                            atol_rows.data_ptr(), y0.shape[0], y0.shape[1], part.data_ptr(),
                                            part.numel() * 8, dtype_code(y0.dtype), self._stream()), "tdeq_row_reduce_tol")

    def row_control(self, mode: int, part, ctrl: StepCtrl, st: RowState, dts_out, times_out, dtype) -> None:
        _check(self.lib.tdeq_row_control(mode, part.data_ptr(), ctypes.byref(ctrl), ctypes.byref(st), dts_out.data_ptr(),
                                         times_out.data_ptr(), dtype_code(dtype), self._stream()), "tdeq_row_control")

    def row_control_points(self, mode: int, part, ctrl: StepCtrl, st: RowState, pts: RowPoints, dts_out, times_out,
                           dtype) -> None:
        """tdeq_row_control_points: `row_control` with the per-row bounds and points of `pts`; `st.status` has 3 words."""
        _check(self.lib.tdeq_row_control_points(mode, part.data_ptr(), ctypes.byref(ctrl), ctypes.byref(st),
                                                ctypes.byref(pts), dts_out.data_ptr(), times_out.data_ptr(),
                                                dtype_code(dtype), self._stream()), "tdeq_row_control_points")

    def row_select(self, dst, src, mask) -> None:
        """tdeq_row_select: dst[r, :] = src[r, :] for the rows with mask[r] != 0 (`mask` int32 [B] on the device)."""
        if dst.shape[0] == 0:
            return
        _check(self.lib.tdeq_row_select(dst.data_ptr(), src.data_ptr(), mask.data_ptr(), dst.shape[0], dst.shape[1],
                                        dtype_code(dst.dtype), self._stream()), "tdeq_row_select")

    def row_impulse(self, y, dy, dy_index, jump_hit, jumped, row_map=None) -> None:
        """tdeq_row_impulse: y[r, :] += dy[k, o or 0, :] for the rows with jumped[r] != 0, o = row_map[r] (None: r), k =
        dy_index[jump_hit[r], o] when >= 0.  `y` [n, L], `dy` [K, B or 1, L] of y's dtype, `dy_index` int32 [K', B], the
        three row vectors int32 [n]; all on the device."""
        if y.shape[0] == 0:
            return
        _check(self.lib.tdeq_row_impulse(y.data_ptr(), dy.data_ptr(), dy.shape[1], dy_index.data_ptr(), dy_index.shape[1],
                                         jump_hit.data_ptr(), jumped.data_ptr(),
                                         None if row_map is None else row_map.data_ptr(), y.shape[0], y.shape[1],
                                         dtype_code(y.dtype), self._stream()), "tdeq_row_impulse")

    def row_dense_commit(self, sol, y0, y1, f0, f1, ks, coefs, dts, st: RowState) -> None:
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_row_dense_commit(sol.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(), f1.data_ptr(),
                                              ptrs, cf, n, dts.data_ptr(), ctypes.byref(st), dtype_code(y0.dtype),
                                              self._stream()), "tdeq_row_dense_commit")

    def row_dense_commit_mapped(self, sol, row_map, y0, y1, f0, f1, ks, coefs, dts, st: RowState) -> None:
        """tdeq_row_dense_commit_mapped: `sol` [n_out, sol_rows, L], the state tensors [st.n_rows, L], `row_map` int32
        [st.n_rows] = the solution row of each state row."""
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_row_dense_commit_mapped(sol.data_ptr(), row_map.data_ptr(), sol.shape[1], y0.data_ptr(),
                                                     y1.data_ptr(), f0.data_ptr(), f1.data_ptr(), ptrs, cf, n,
                                                     dts.data_ptr(), ctypes.byref(st), dtype_code(y0.dtype),
                                                     self._stream()), "tdeq_row_dense_commit_mapped")

    def row_gather(self, outs, srcs, idx) -> None:
        """tdeq_row_gather: outs[m][q, :] = srcs[m][idx[q], :] for up to 4 [*, L] tensors of one dtype in one launch;
        `idx` int32 on the device, `outs[m]` contiguous [len(idx), L]."""
        n = len(srcs)
        if idx.numel() == 0:                  # (nothing to gather; empty tensors have null pointers, which the ABI refuses)
            return
        dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        src = (ctypes.c_void_p * n)(*[x.data_ptr() for x in srcs])
        _check(self.lib.tdeq_row_gather(dst, src, n, idx.data_ptr(), idx.numel(), srcs[0].shape[1],
                                        dtype_code(srcs[0].dtype), self._stream()), "tdeq_row_gather")

    def row_scale_many(self, outs, g, w) -> None:
        """tdeq_row_scale_many: outs[m][r, :] = w[m, r] * g[r, :]; `w` a contiguous [len(outs), B] tensor of g's dtype."""
        n = len(outs)
        if w.shape != (n, g.shape[0]) or w.dtype != g.dtype or not w.is_contiguous():
            raise ValueError("row_scale_many: w must be a contiguous [n_out, B] tensor of g's dtype")
        ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        _check(self.lib.tdeq_row_scale_many(ptrs, n, g.data_ptr(), w.data_ptr(), g.shape[0], g.shape[1],
                                            dtype_code(g.dtype), self._stream()), "tdeq_row_scale_many")

    def row_multi_dot(self, g, xs) -> torch.Tensor:
        """tdeq_row_multi_dot: fp64 device tensor [len(xs), B] of the row dots <g[r], x_m[r]>."""
        n, (B, L) = len(xs), g.shape
        ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
        out = torch.empty(n, B, dtype=torch.float64, device=g.device)
        nbytes = self.lib.tdeq_row_dots_workspace_bytes(B, L, n, dtype_code(g.dtype))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device) if nbytes else None
        _check(self.lib.tdeq_row_multi_dot(g.data_ptr(), ptrs, n, B, L, out.data_ptr(),
                                           None if ws is None else ws.data_ptr(), nbytes, dtype_code(g.dtype),
                                           self._stream()), "tdeq_row_multi_dot")
        return out

    # -- per-row terminal events (odeint_rowwise_event, rowwise_event.py) ----------------------------------------------
    def row_event_detect(self, g1, sign0, ctrl: StepCtrl, st: RowState, dts, times, fired, fired_now, lo, hi) -> None:
        """tdeq_row_event_detect: `g1` [n] of the state dtype, `sign0` / `fired` / `fired_now` int32 [n], `lo` / `hi` fp64
        [n]; `dts` [n] and `times` [n_times, n] are the buffers the controller just wrote."""
        n = int(st.n_rows)
        if g1.shape != (n,) or g1.dtype != dts.dtype or not g1.is_contiguous():
            raise ValueError("row_event_detect: g1 must be a contiguous [n_rows] tensor of the state's dtype")
        _check(self.lib.tdeq_row_event_detect(g1.data_ptr(), sign0.data_ptr(), ctypes.byref(ctrl), ctypes.byref(st),
                                              dts.data_ptr(), times.data_ptr(), fired.data_ptr(), fired_now.data_ptr(),
                                              lo.data_ptr(), hi.data_ptr(), dtype_code(g1.dtype), self._stream()),
               "tdeq_row_event_detect")

    def row_event_fit(self, q, fired_now, y0, y1, f0, f1, ks, coefs, dts) -> None:
        """tdeq_row_event_fit: `q` a contiguous [5, n, L] tensor of the state's dtype."""
        if q.shape != (5,) + tuple(y0.shape) or q.dtype != y0.dtype or not q.is_contiguous():
            raise ValueError("row_event_fit: q must be a contiguous [5, n_rows, L] tensor of the state's dtype")
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_row_event_fit(q.data_ptr(), fired_now.data_ptr(), y0.data_ptr(), y1.data_ptr(), f0.data_ptr(),
                                           f1.data_ptr(), ptrs, cf, n, dts.data_ptr(), y0.shape[0], y0.shape[1],
                                           dtype_code(y0.dtype), self._stream()), "tdeq_row_event_fit")

    def row_event_eval(self, out, q, x, mask) -> None:
        """tdeq_row_event_eval: out[r, :] = q[:, r, :] at x[r] for the rows with mask[r] (int32 [n])."""
        if q.shape != (5,) + tuple(out.shape) or q.dtype != out.dtype or not q.is_contiguous() or not out.is_contiguous():
            raise ValueError("row_event_eval: q must be a contiguous [5, n_rows, L] tensor of out's dtype")
        if x.shape != (out.shape[0],) or x.dtype != out.dtype or not x.is_contiguous():
            raise ValueError("row_event_eval: x must be a contiguous [n_rows] tensor of out's dtype")
        _check(self.lib.tdeq_row_event_eval(out.data_ptr(), q.data_ptr(), x.data_ptr(), mask.data_ptr(), out.shape[0],
                                            out.shape[1], dtype_code(out.dtype), self._stream()), "tdeq_row_event_eval")

    def row_event_fit_mapped(self, q, row_map, fired_now, y0, y1, f0, f1, ks, coefs, dts) -> None:
        """tdeq_row_event_fit_mapped: `q` a contiguous [5, q_rows, L] tensor of the state's dtype, the state tensors [n, L],
        `row_map` int32 [n] = the row of `q` of each state row."""
        if q.dim() != 3 or q.shape[0] != 5 or q.shape[2] != y0.shape[1] or q.dtype != y0.dtype or not q.is_contiguous():
            raise ValueError("row_event_fit_mapped: q must be a contiguous [5, q_rows, L] tensor of the state's dtype")
        if row_map.shape != (y0.shape[0],) or row_map.dtype != torch.int32 or not row_map.is_contiguous():
            raise ValueError("row_event_fit_mapped: row_map must be a contiguous int32 [n_rows] tensor")
        ptrs, cf, n = self._terms(ks, coefs)
        _check(self.lib.tdeq_row_event_fit_mapped(q.data_ptr(), row_map.data_ptr(), q.shape[1], fired_now.data_ptr(),
                                                  y0.data_ptr(), y1.data_ptr(), f0.data_ptr(), f1.data_ptr(), ptrs, cf, n,
                                                  dts.data_ptr(), y0.shape[0], y0.shape[1], dtype_code(y0.dtype),
                                                  self._stream()), "tdeq_row_event_fit_mapped")

    def row_event_eval_mapped(self, out, dst_map, q, src_map, x) -> None:
        """tdeq_row_event_eval_mapped: out[dst_map[i] (None: i), :] = q[:, src_map[i], :] at x[i]; the maps int32 [n_idx] on
        the device, `x` [n_idx] of out's dtype, `q` a contiguous [5, q_rows, L] tensor, `out` [out_rows, L]."""
        n_idx = src_map.numel()
        if n_idx == 0:                        # (nothing to evaluate; empty tensors have null pointers, which the ABI refuses)
            return
        if q.dim() != 3 or q.shape[0] != 5 or q.shape[2] != out.shape[1] or q.dtype != out.dtype or not q.is_contiguous() \
                or not out.is_contiguous():
            raise ValueError("row_event_eval_mapped: q must be a contiguous [5, q_rows, L] tensor of out's dtype")
        if x.shape != (n_idx,) or x.dtype != out.dtype or not x.is_contiguous():
            raise ValueError("row_event_eval_mapped: x must be a contiguous [n_idx] tensor of out's dtype")
        for m in (src_map, dst_map):
            if m is not None and (m.shape != (n_idx,) or m.dtype != torch.int32 or not m.is_contiguous()):
                raise ValueError("row_event_eval_mapped: the maps must be contiguous int32 [n_idx] tensors")
        _check(self.lib.tdeq_row_event_eval_mapped(out.data_ptr(), None if dst_map is None else dst_map.data_ptr(),
                                                   out.shape[0], q.data_ptr(), src_map.data_ptr(), q.shape[1], x.data_ptr(),
                                                   n_idx, out.shape[1], dtype_code(out.dtype), self._stream()),
               "tdeq_row_event_eval_mapped")

    # -- per-row dense output (odeint_rowwise_dense, rowwise_dense.py) -------------------------------------------------
    def row_dense_slots(self, st: RowState, row_map, cap: int, counter, slot_row, slot_ord, slot_ta, slot_tb, slot,
                        mask) -> None:
        """tdeq_row_dense_slots: every accepted row of `st` takes a slot of a chunk of `cap` slots.  `counter` int32 [2],
        `slot_row` / `slot_ord` int32 [cap], `slot_ta` / `slot_tb` fp64 [cap], `slot` / `mask` int32 [n_rows], `row_map`
        int32 [n_rows] or None (identity)."""
        n = int(st.n_rows)
        for name, t, dtype, size in (("counter", counter, torch.int32, 2), ("slot_row", slot_row, torch.int32, cap),
                                     ("slot_ord", slot_ord, torch.int32, cap), ("slot_ta", slot_ta, torch.float64, cap),
                                     ("slot_tb", slot_tb, torch.float64, cap), ("slot", slot, torch.int32, n),
                                     ("mask", mask, torch.int32, n)):
            if t.shape != (size,) or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"row_dense_slots: {name} must be a contiguous {dtype} [{size}] tensor")
        if row_map is not None and (row_map.shape != (n,) or row_map.dtype != torch.int32 or not row_map.is_contiguous()):
            raise ValueError("row_dense_slots: row_map must be a contiguous int32 [n_rows] tensor")
        _check(self.lib.tdeq_row_dense_slots(ctypes.byref(st), None if row_map is None else row_map.data_ptr(), cap,
                                             counter.data_ptr(), slot_row.data_ptr(), slot_ord.data_ptr(),
                                             slot_ta.data_ptr(), slot_tb.data_ptr(), slot.data_ptr(), mask.data_ptr(),
                                             self._stream()), "tdeq_row_dense_slots")

    def row_dense_pack(self, dst, src, dest, n_used: int) -> None:
        """tdeq_row_dense_pack: dst[:, dest[s]] = src[:, s] for s < n_used; `dst` [5, dst_rows, L] and `src` [5, src_rows, L]
        contiguous in one dtype, `dest` int64 [n_used] on the device, its values rows of `dst`."""
        if n_used == 0:                       # (nothing to move; empty tensors have null pointers, which the ABI refuses)
            return
        for name, t in (("dst", dst), ("src", src)):
            if t.dim() != 3 or t.shape[0] != 5 or t.shape[2] != dst.shape[2] or t.dtype != dst.dtype or not t.is_contiguous():
                raise ValueError(f"row_dense_pack: {name} must be a contiguous [5, rows, L] tensor of one dtype")
        if dest.shape != (n_used,) or dest.dtype != torch.int64 or not dest.is_contiguous():
            raise ValueError("row_dense_pack: dest must be a contiguous int64 [n_used] tensor")
        _check(self.lib.tdeq_row_dense_pack(dst.data_ptr(), dst.shape[1], src.data_ptr(), src.shape[1], dest.data_ptr(),
                                            n_used, dst.shape[2], dtype_code(dst.dtype), self._stream()),
               "tdeq_row_dense_pack")

    def row_dense_search(self, tq, offsets, seg_ta, seg_tb, t0, t1, seg, x, status) -> None:
        """tdeq_row_dense_search: `tq` fp64 [Q, B] in solver time, `offsets` int64 [B + 1], `seg_ta` / `seg_tb` fp64 [n_seg],
        `t0` / `t1` fp64 [B]; writes `seg` int32 [Q * B] and `x` [Q * B] of the state's dtype and lowers `status` (int32
        [1], preset to INT32_MAX) to the smallest out-of-range query index."""
        if tq.numel() == 0:
            return
        Q, B = tq.shape
        n_seg = seg_ta.numel()
        for name, t, dtype, size in (("tq", tq.view(-1), torch.float64, Q * B), ("offsets", offsets, torch.int64, B + 1),
                                     ("seg_ta", seg_ta, torch.float64, n_seg), ("seg_tb", seg_tb, torch.float64, n_seg),
                                     ("t0", t0, torch.float64, B), ("t1", t1, torch.float64, B),
                                     ("seg", seg, torch.int32, Q * B), ("x", x, x.dtype, Q * B),
                                     ("status", status, torch.int32, 1)):
            if t.shape != (size,) or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"row_dense_search: {name} must be a contiguous {dtype} [{size}] tensor")
        if not tq.is_contiguous():
            raise ValueError("row_dense_search: tq must be contiguous")
        _check(self.lib.tdeq_row_dense_search(tq.data_ptr(), Q, offsets.data_ptr(), seg_ta.data_ptr(), seg_tb.data_ptr(),
                                              n_seg, t0.data_ptr(), t1.data_ptr(), B, seg.data_ptr(), x.data_ptr(),
                                              status.data_ptr(), dtype_code(x.dtype), self._stream()),
               "tdeq_row_dense_search")

    # -- calculus on the per-row dense record (RowDenseOutput.derivative / antiderivative / integral) --------------------
    def row_dense_prefix(self, prefix, coeffs, offsets, seg_ta, seg_tb) -> None:
        """tdeq_row_dense_prefix: `prefix` fp64 [n_seg, L] = the exclusive prefix, per row and left to right in fp64, of the
        whole-segment integrals of `coeffs` [5, n_seg, L]; `offsets` int64 [B + 1], `seg_ta` / `seg_tb` fp64 [n_seg]."""
        n_seg, B = seg_ta.numel(), offsets.numel() - 1
        if n_seg == 0 or B <= 0:              # (nothing to add up; empty tensors have null pointers, which the ABI refuses)
            return
        if coeffs.dim() != 3 or coeffs.shape[:2] != (5, n_seg) or not coeffs.is_contiguous():
            raise ValueError("row_dense_prefix: coeffs must be a contiguous [5, n_seg, L] tensor")
        L = coeffs.shape[2]
        for name, t, dtype, shape in (("prefix", prefix, torch.float64, (n_seg, L)), ("offsets", offsets, torch.int64, (B + 1,)),
                                      ("seg_ta", seg_ta, torch.float64, (n_seg,)), ("seg_tb", seg_tb, torch.float64, (n_seg,))):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"row_dense_prefix: {name} must be a contiguous {dtype} {list(shape)} tensor")
        _check(self.lib.tdeq_row_dense_prefix(prefix.data_ptr(), coeffs.data_ptr(), offsets.data_ptr(), seg_ta.data_ptr(),
                                              seg_tb.data_ptr(), n_seg, B, L, dtype_code(coeffs.dtype), self._stream()),
               "tdeq_row_dense_prefix")

    def row_dense_calc(self, out, mode: int, coeffs, seg_ta, seg_tb, prefix, sign: float, seg, x, tq=None, seg2=None,
                       x2=None, tq2=None) -> None:
        """tdeq_row_dense_calc: out[i, :] for the queries (seg[i], x[i], tq[i]) of `row_dense_search`; `mode` 0: the derivative
        (`prefix`, `tq` and the second list may be None), 1: the antiderivative, 2: the integral from the first list to the
        second (`seg2`, `x2`, `tq2`).  `out` [n_idx, L] and `x` [n_idx] of the dtype of `coeffs` [5, n_seg, L], `seg` int32
        [n_idx], `tq` fp64 with n_idx elements in solver time, `prefix` fp64 [n_seg, L], `sign` +1.0 or -1.0."""
        n_idx = seg.numel()
        if n_idx == 0:
            return
        n_seg = seg_ta.numel()
        if coeffs.dim() != 3 or coeffs.shape[:2] != (5, n_seg) or coeffs.dtype != out.dtype or not coeffs.is_contiguous():
            raise ValueError("row_dense_calc: coeffs must be a contiguous [5, n_seg, L] tensor of out's dtype")
        L = coeffs.shape[2]
        if mode not in (0, 1, 2) or (mode != 0 and (prefix is None or tq is None)) \
                or (mode == 2 and (seg2 is None or x2 is None or tq2 is None)):
            raise ValueError("row_dense_calc: mode 0 (derivative), 1 (antiderivative: prefix, tq) or 2 (integral: also seg2, "
                             "x2, tq2)")
        checks = [("out", out, out.dtype, (n_idx, L)), ("seg_ta", seg_ta, torch.float64, (n_seg,)),
                  ("seg_tb", seg_tb, torch.float64, (n_seg,)), ("seg", seg, torch.int32, (n_idx,)), ("x", x, out.dtype, (n_idx,))]
        if mode != 0:
            checks += [("prefix", prefix, torch.float64, (n_seg, L)), ("tq", tq.view(-1), torch.float64, (n_idx,))]
        if mode == 2:
            checks += [("seg2", seg2, torch.int32, (n_idx,)), ("x2", x2, out.dtype, (n_idx,)),
                       ("tq2", tq2.view(-1), torch.float64, (n_idx,))]
        for name, t, dtype, shape in checks:
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"row_dense_calc: {name} must be a contiguous {dtype} {list(shape)} tensor")
        if (mode != 0 and not tq.is_contiguous()) or (mode == 2 and not tq2.is_contiguous()):
            raise ValueError("row_dense_calc: tq and tq2 must be contiguous")

        def ptr(t, needed):
            return t.data_ptr() if needed and t is not None else None
        _check(self.lib.tdeq_row_dense_calc(out.data_ptr(), mode, coeffs.data_ptr(), n_seg, seg_ta.data_ptr(),
                                            seg_tb.data_ptr(), ptr(prefix, mode != 0), float(sign), seg.data_ptr(),
                                            x.data_ptr(), ptr(tq, mode != 0), ptr(seg2, mode == 2), ptr(x2, mode == 2),
                                            ptr(tq2, mode == 2), n_idx, L, dtype_code(out.dtype), self._stream()),
               "tdeq_row_dense_calc")

    # -- queries over a time window of the record (RowDenseOutput.maximum / crossings / exposure / crossing_times) -----------
    def _row_dense_window(self, name: str, outs, coeffs, seg_ta, seg_tb, sign: float, seg, x, tq, seg2, x2, tq2, level=None,
                          like=None, refuse=None):
        """What the bindings of the four window kernels share.  The windows lie between the queries (seg[i], x[i], tq[i]) and
        (seg2[i], x2[i], tq2[i]) of `row_dense_search`: `seg`, `seg2` int32 [n_idx], `x`, `x2` [n_idx] of the dtype of `coeffs`
        [5, n_seg, L], `tq`, `tq2` fp64 with n_idx elements in solver time, `sign` +1.0 or -1.0; with a `level` [n_rows, L] of
        that dtype query i belongs to row i % n_rows.  `outs`: the binding's outputs as (name, tensor, dtype or None for that
        of `coeffs`, leading dimensions), each [*leading, n_idx, L].  Validated in this order: `coeffs` (of the dtype of the
        tensor `like` = (name, tensor), when given), `level`, `refuse` (the binding's own complaint, or None), then every
        output, `level` and the shared tensors -> the arguments of the entry point from `level` (or `coeffs`) on, or None
        for no queries."""
        n_idx = seg.numel()
        if n_idx == 0:
            return None
        n_seg = seg_ta.numel()
        if coeffs.dim() != 3 or coeffs.shape[:2] != (5, n_seg) or not coeffs.is_contiguous() \
                or (like is not None and coeffs.dtype != like[1].dtype):
            raise ValueError(f"{name}: coeffs must be a contiguous [5, n_seg, L] tensor" +
                             (f" of {like[0]}' dtype" if like is not None else ""))
        L, T = coeffs.shape[2], coeffs.dtype
        table, head = [(n, t, dtype or T, (*lead, n_idx, L)) for n, t, dtype, lead in outs], ()
        if level is not None:
            if level.dim() != 2 or level.shape[1] != L or level.shape[0] == 0 or n_idx % level.shape[0] != 0:
                raise ValueError(f"{name}: level must be [n_rows, {L}] with n_rows dividing the {n_idx} queries")
            table.append(("level", level, T, (level.shape[0], L)))
            head = (level.data_ptr(), level.shape[0])
        if refuse is not None:
            raise ValueError(f"{name}: {refuse}")
        table += [("seg_ta", seg_ta, torch.float64, (n_seg,)), ("seg_tb", seg_tb, torch.float64, (n_seg,)),
                  ("seg", seg, torch.int32, (n_idx,)), ("x", x, T, (n_idx,)), ("tq", tq.view(-1), torch.float64, (n_idx,)),
                  ("seg2", seg2, torch.int32, (n_idx,)), ("x2", x2, T, (n_idx,)),
                  ("tq2", tq2.view(-1), torch.float64, (n_idx,))]
        for n, t, dtype, shape in table:
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"{name}: {n} must be a contiguous {dtype} {list(shape)} tensor")
        if not tq.is_contiguous() or not tq2.is_contiguous():
            raise ValueError(f"{name}: tq and tq2 must be contiguous")
        return (*head, coeffs.data_ptr(), n_seg, seg_ta.data_ptr(), seg_tb.data_ptr(), float(sign), seg.data_ptr(),
                x.data_ptr(), tq.data_ptr(), seg2.data_ptr(), x2.data_ptr(), tq2.data_ptr(), n_idx, L, dtype_code(T),
                self._stream())

    def row_dense_extremum(self, values, times, which: int, coeffs, seg_ta, seg_tb, sign: float, seg, x, tq, seg2, x2,
                           tq2) -> None:
        """tdeq_row_dense_extremum: per element the maximum (`which` 0) or minimum (1) of the record on each window, and its
        time.  `values` [n_idx, L] of the dtype of `coeffs`, `times` fp64 [n_idx, L] (true time); the record and the two query
        lists as `_row_dense_window` describes them."""
        tail = self._row_dense_window("row_dense_extremum", (("values", values, None, ()), ("times", times, torch.float64, ())),
                                      coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2, like=("values", values),
                                      refuse=None if which in (0, 1) else "which 0 (maximum) or 1 (minimum)")
        if tail is not None:
            _check(self.lib.tdeq_row_dense_extremum(values.data_ptr(), times.data_ptr(), which, *tail),
                   "tdeq_row_dense_extremum")

    def row_dense_level(self, count, first, last, time_above, level, coeffs, seg_ta, seg_tb, sign: float, seg, x, tq, seg2, x2,
                        tq2) -> None:
        """tdeq_row_dense_level: per element the crossings of `level` [n_rows, L] on each window, and the time above it.
        `count` int32, `first`, `last` (true time) and `time_above` fp64, all [n_idx, L]; the record and the two query lists as
        `_row_dense_window` describes them."""
        f64 = torch.float64
        tail = self._row_dense_window("row_dense_level", (("count", count, torch.int32, ()), ("first", first, f64, ()),
                                                          ("last", last, f64, ()), ("time_above", time_above, f64, ())),
                                      coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2, level=level)
        if tail is not None:
            _check(self.lib.tdeq_row_dense_level(count.data_ptr(), first.data_ptr(), last.data_ptr(), time_above.data_ptr(),
                                                 *tail), "tdeq_row_dense_level")

    def row_dense_exposure(self, area_above, area_below, time_above, level, coeffs, seg_ta, seg_tb, sign: float, seg, x, tq,
                           seg2, x2, tq2) -> None:
        """tdeq_row_dense_exposure: per element the area between the record and `level` [n_rows, L] above and below it on each
        window, and the time above it.  `area_above`, `area_below` [n_idx, L] of the dtype of `coeffs`, `time_above` fp64
        [n_idx, L]; the record and the two query lists as `_row_dense_window` describes them."""
        tail = self._row_dense_window("row_dense_exposure", (("area_above", area_above, None, ()),
                                                             ("area_below", area_below, None, ()),
                                                             ("time_above", time_above, torch.float64, ())),
                                      coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2, level=level)
        if tail is not None:
            _check(self.lib.tdeq_row_dense_exposure(area_above.data_ptr(), area_below.data_ptr(), time_above.data_ptr(), *tail),
                   "tdeq_row_dense_exposure")

    def row_dense_level_times(self, n_rising, n_falling, rising, falling, level, coeffs, seg_ta, seg_tb, sign: float, seg, x,
                              tq, seg2, x2, tq2) -> None:
        """tdeq_row_dense_level_times: per element the true times of the first K rising and the first K falling crossings of
        `level` [n_rows, L] on each window, and the number of crossings of each direction.  `n_rising`, `n_falling` int32
        [n_idx, L]; `rising`, `falling` fp64 [K, n_idx, L] with K = rising.shape[0]; the record and the two query lists as
        `_row_dense_window` describes them."""
        K = rising.shape[0] if rising.dim() == 3 else None
        tail = self._row_dense_window("row_dense_level_times",
                                      (("n_rising", n_rising, torch.int32, ()), ("n_falling", n_falling, torch.int32, ()),
                                       ("rising", rising, torch.float64, (K,)), ("falling", falling, torch.float64, (K,))),
                                      coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2, level=level,
                                      refuse=None if K is not None else "rising must be a [K, n_idx, L] tensor")
        if tail is not None:
            _check(self.lib.tdeq_row_dense_level_times(n_rising.data_ptr(), n_falling.data_ptr(), rising.data_ptr(),
                                                       falling.data_ptr(), K, *tail), "tdeq_row_dense_level_times")


class ComplexHipKernels:
    """complex64 / complex128 states on the HIP kernels (r04; r03 ran them as torch ops).

    Every LINEAR operation of a Runge–Kutta step has real coefficients (rk_common.py:79,89,201-205, interp.py,
    rk_common.py:110-157), and ATen itself evaluates `complex * real` per component — so those calls go to the real
    kernels on the state's interleaved (re, im) view: zero copy, 2n elements of the real type, bit-identical to the
    torch-op path.  The tolerance-scaled norms (misc.py:80-82, 50-56 with |.| the complex modulus) have kernels of their
    own (csrc/tdeq_kernels_complex.hpp, dtype codes TDEQ_C64 / TDEQ_C128): those calls pass the complex tensors through,
    with segment tables, chunks and counts in complex elements."""

    name = "hip-complex"
    _NORM_CALLS = frozenset(("error_norm", "error_norm_partial", "error_norm_partial_ctrl", "error_scaled", "init_norms",
                             "init_scaled"))
    _AS_IS = frozenset(("make_plan", "read_norms", "read_ctrl", "arm_readback", "multi_spec", "_arm", "_read_out",
                        "_stream", "_terms"))

    def __init__(self, inner: "HipKernels"):
        self._inner = inner
        self.lib = inner.lib
        self._host = None

    @staticmethod
    def _real(x):
        if isinstance(x, torch.Tensor):
            if not x.is_complex():
                return x
            r = torch.view_as_real(x)
            return r.reshape(-1) if x.dim() <= 1 else r.reshape(x.shape[0], -1)
        if isinstance(x, (list, tuple)) and any(isinstance(t, torch.Tensor) for t in x):
            return type(x)(ComplexHipKernels._real(t) for t in x)
        return x

    def __getattr__(self, name):
        attr = getattr(self._inner, name)          # AttributeError for what HipKernels does not have either
        if not callable(attr) or name in self._AS_IS or name in self._NORM_CALLS:
            return attr
        real = self._real

        def on_real_views(*args, **kwargs):
            return attr(*[real(a) for a in args], **{k: real(v) for k, v in kwargs.items()})
        on_real_views.__name__ = name
        self.__dict__[name] = on_real_views         # next lookup skips __getattr__
        return on_real_views

    # -- the calls whose COUNTS are in complex elements ------------------------------------------------------------
    def pack_segments(self, out, srcs, chunk_starts, numels, scales, chunk: int) -> None:
        self._inner.pack_segments(self._real(out), [None if t is None else self._real(t.reshape(-1)) for t in srcs],
                                  chunk_starts, [2 * int(n) for n in numels], scales, 2 * chunk)

    def step_controller(self, plan, sums_plan, numel_plan, ctrl, next_times, dtype, state_in_dev: bool = False) -> None:
        real = torch.float32 if dtype in (torch.complex64, torch.float32) else torch.float64
        self._inner.step_controller(plan, sums_plan, numel_plan, ctrl, next_times, real, state_in_dev)

    # -- Adams–Moulton corrector: its convergence census needs |.| (fixed_adams.py:189-192) and has no complex kernel;
    #    SURVEY.md §2 puts the multistep methods out of scope, so this one step stays a torch-op evaluation on the device
    def adams_correct(self, plan, dy_out, dy_old, y_out=None, f=None, delta=None, y0=None, c: float = 0.0,
                      compute: bool = True) -> None:
        from . import _fallback
        if self._host is None:
            self._host = _fallback.HostKernels()
        hp = getattr(plan, "_host_plan", None)
        if hp is None:
            segs = [(int(sg.chunk_start) * plan.chunk, int(sg.numel), float(sg.rtol), float(sg.atol)) for sg in plan.segs]
            hp = plan._host_plan = _fallback.HostPlan(segs, plan.n_chunks * plan.chunk, plan.chunk)
        self._host.adams_correct(hp, dy_out, dy_old, y_out, f, delta, y0, c, compute)
        n = plan.n_seg
        if plan.pinned:
            plan.out_np[:n] = hp.sums0
            plan.out_np[2 * n:3 * n] = hp.bad
        else:
            plan.out[:n] = torch.tensor(hp.sums0, dtype=torch.float64)
            plan.out[2 * n:3 * n] = torch.tensor(hp.bad, dtype=torch.float64)
        plan.expect = ()


class _GuardProbe:
    """Test hook for the device guard on a one-GPU box (tests/test_dist_gpu.py): `pretend_current` = the index the guard
    should take for the caller's current device — a state on cuda:0 then looks like a state on a NON-current device
    and the switching branch runs for real (to device 0); `switched` counts how often it did."""
    pretend_current = None
    switched = 0


def device_guard(device):
    """Context that makes `device` the current HIP device.  Every launch goes to `torch.cuda.current_stream()` — the
    CURRENT device's stream — and a kernel cannot be launched into another device's stream, so each entry point of the
    package runs under this guard: a state on `cuda:1` is integrated on cuda:1's stream whatever the caller's current
    device is.  Free when the device already is the current one (and for the CPU tensors of the host-logic tests)."""
    device = torch.device(device)
    if device.type != "cuda" or device.index is None:
        return contextlib.nullcontext()
    current = torch.cuda.current_device() if _GuardProbe.pretend_current is None else _GuardProbe.pretend_current
    if device.index == current:
        return contextlib.nullcontext()
    _GuardProbe.switched += 1
    return torch.cuda.device(device)


def on_state_device(method):
    """Decorator for solver entry points (`integrate*`): run under `device_guard(self.y0.device)`."""
    @functools.wraps(method)
    def guarded(self, *args, **kwargs):
        with device_guard(self.y0.device):
            return method(self, *args, **kwargs)
    return guarded


_KERNELS: Optional[HipKernels] = None
_HOST_KERNELS = None
_LOW_KERNELS = None
_LOW_HIP_KERNELS = None
_COMPLEX_KERNELS = None


def get_kernels(device: torch.device, dtype: Optional[torch.dtype] = None):
    """The compute backend for a state of `dtype` on `device`.

    A real or complex fp32 / fp64 state on a ROCm device -> the HIP kernels, and ONLY those: a missing or stale
    libtdeq_hip.so raises `NativeLibraryError` here (no silent substitute on the GPU); complex states through
    `ComplexHipKernels` (real kernels on the (re, im) view + the complex norm kernels).  A state that the kernels do
    not take — not on a ROCm device (BASELINE.json configs[0] is a CPU case; the reference runs wherever its tensors
    live, odeint.py:49-108) — -> `_fallback.HostKernels` / `LowPrecisionHostKernels`, the same interface in torch ops,
    with one `HostPathWarning` per process.  bf16 / fp16 states on a ROCm device -> `_lowp.LowPrecisionHipKernels`."""
    global _KERNELS, _HOST_KERNELS, _LOW_KERNELS, _LOW_HIP_KERNELS, _COMPLEX_KERNELS
    device = torch.device(device)
    is_complex = dtype is not None and dtype.is_complex
    if dtype in (torch.bfloat16, torch.float16):
        # states below fp32: integrated in their own precision like the reference's (misc.py:185-187), every operation
        # rounded to the storage type as ATen rounds it — on a ROCm device by the HIP kernels of csrc/tdeq_kernels_lp.hpp
        # (`_lowp.LowPrecisionHipKernels`: a missing library raises here, as for fp32), elsewhere by torch ops
        if device.type == "cuda":
            if _LOW_HIP_KERNELS is None:
                if _KERNELS is None:
                    _KERNELS = HipKernels(load_library())
                from . import _lowp
                _LOW_HIP_KERNELS = _lowp.LowPrecisionHipKernels(_KERNELS)
            return _LOW_HIP_KERNELS
        from . import _fallback
        _fallback.warn_once(f"the state is {dtype} on '{device}'")
        if _LOW_KERNELS is None:
            _LOW_KERNELS = _fallback.LowPrecisionHostKernels()
        return _LOW_KERNELS
    if device.type != "cuda":
        from . import _fallback
        _fallback.warn_once(f"the state lives on '{device}'")
        if _HOST_KERNELS is None:
            _HOST_KERNELS = _fallback.HostKernels()
        return _HOST_KERNELS
    if _KERNELS is None:
        _KERNELS = HipKernels(load_library())
    if is_complex:
        if _COMPLEX_KERNELS is None:
            _COMPLEX_KERNELS = ComplexHipKernels(_KERNELS)
        return _COMPLEX_KERNELS
    return _KERNELS
