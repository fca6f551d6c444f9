"""Every flat entry point of csrc/tdeq_abi.hip refuses bad arguments BEFORE any launch, so the refusals are checked
without a GPU: one table of calls per entry point, each with the status it must return — TDEQ_EINVAL (-1),
TDEQ_EWORKSPACE (-2), or 0 for an empty state.  The table pins the ORDER of the checks as well: every refusal is
repeated with an empty state (where the entry point has that path) and with a workspace one byte short (where it takes
one), and two faults together still give -1 — the argument checks come first, the workspace size last.

No call of the table is valid with a non-empty state: a call that passed the checks would launch on pointers into host
memory.  The statuses were recorded from the library as it stood before the launch layer was rewritten."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EINVAL, EWORKSPACE, OK = -1, -2, 0
F32, F64, C64, C128, BF16, F16 = 0, 1, 2, 3, 4, 5
REAL = (F32, F64)
LOWP = REAL + (BF16, F16)                 # the entry points of the host-driven 16-bit step
CPLX = REAL + (C64, C128)
NORM = LOWP + (C64, C128)                 # the norm entry points: real, 16-bit, interleaved complex
CODES = tuple(range(-1, 9))
MAX_SEGMENTS, INLINE_SEGMENTS = 4096, 16

_buf = (ctypes.c_double * 64)()
P = ctypes.addressof(_buf)                # a non-null pointer (host memory: never reaches a kernel)


def ptr_array(n=16, null_at=None):
    a = (ctypes.c_void_p * n)(*([P] * n))
    if null_at is not None:
        a[null_at] = None
    return a


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


class Entry:
    """One entry point with a valid call (`args`, in the order of the C signature) and what the table derives from it."""

    def __init__(self, name, args, nulls, *, arrays=(), counts=(), accepts=REAL, dtypes=("dtype",), size="n", empty=False,
                 extra=(), label=None):
        self.name, self.args, self.nulls, self.arrays, self.counts = name, args, nulls, arrays, counts
        self.accepts, self.dtypes, self.size, self.empty, self.extra = accepts, dtypes, size, empty, extra
        self.label = label or name
        self.ok = dict(args)
        if size not in self.ok:
            self.size = None

    def call(self, lib, **overrides):
        a = dict(self.ok, **overrides)
        return getattr(lib, self.name)(*[a[name] for name, _ in self.args])

    def cases(self):
        """(label, overrides, expected status)"""
        from torchdiffeq_amd import _native
        ok, out = self.ok, []

        def refuse(label, **ov):
            out.append((label, ov, EINVAL))
            # the order of the checks: an empty state or a short workspace does not change the answer
            if self.empty and self.size not in ov:
                out.append((label + " + n=0", dict(ov, **{self.size: 0}), EINVAL))
            if "workspace_bytes" in ok and "workspace_bytes" not in ov:
                out.append((label + " + short workspace", dict(ov, workspace_bytes=ok["workspace_bytes"] - 1), EINVAL))

        for name in self.nulls:
            refuse(f"null {name}", **{name: None})
        for arr, count in self.arrays:
            for at in sorted({0, ok[count] - 1}):
                refuse(f"null {arr}[{at}]", **{arr: ptr_array(16, null_at=at)})
        for count, lo, hi in self.counts:
            refuse(f"{count}={lo - 1}", **{count: lo - 1})
            if hi is not None:
                refuse(f"{count}={hi + 1}", **{count: hi + 1})
        for dt in self.dtypes:
            for code in CODES:
                if code not in self.accepts:
                    refuse(f"{dt}={code}", **{dt: code})
        if self.size:
            refuse(f"{self.size}=-1", **{self.size: -1})
        if self.empty:
            for code in self.accepts:
                out.append((f"{self.size}=0 {self.dtypes[0]}={code}", {self.size: 0, self.dtypes[0]: code}, OK))
        if "n_seg" in ok:
            refuse("n_seg=0", n_seg=0)
            refuse("n_seg above TDEQ_MAX_SEGMENTS", n_seg=MAX_SEGMENTS + 1)
            refuse("n_seg above TDEQ_INLINE_SEGMENTS without segs_dev", n_seg=INLINE_SEGMENTS + 1)
        if "chunk" in ok:
            refuse("chunk=0", chunk=0)
            refuse("chunk=1000", chunk=1000)
            refuse("n_chunks=0", n_chunks=0)
            refuse("n_chunks=2^31", n_chunks=2 ** 31)
        if "workspace_bytes" in ok:
            out.append(("workspace one byte short", dict(workspace_bytes=ok["workspace_bytes"] - 1), EWORKSPACE))
        if "ctrl" in ok:
            for field, value in (("n_times", 0), ("n_times", 17), ("n_norm_seg", -1), ("n_norm_seg", ok["n_seg"] + 1)):
                c = _native.StepCtrl()
                c.n_times, c.n_norm_seg = 2, 1
                setattr(c, field, value)
                refuse(f"ctrl.{field}={value}", ctrl=ctypes.pointer(c))
        for item in self.extra:
            label, ov, expected = item[:3]
            twins = item[3] if len(item) > 3 else True
            if expected == EINVAL and twins:
                refuse(label, **ov)
            else:
                out.append((label, ov, expected))
        return out


def _table():
    from torchdiffeq_amd import _native
    K, D = ptr_array(), _buf
    segs = (_native.Segment * (INLINE_SEGMENTS + 1))(*[_native.Segment(0, 4, 1e-3, 1e-4)] * (INLINE_SEGMENTS + 1))
    c_ok = _native.StepCtrl()
    c_ok.n_times, c_ok.n_norm_seg = 2, 1
    ctrl = ctypes.pointer(c_ok)

    def multi_outs(n_out=2, mask=0b111, null_at=None, mask_at=None):
        o = (_native.MultiOut * 4)()
        for i in range(4):
            o[i].out, o[i].mask, o[i].add_y0 = P, 0b111, 0
        if null_at is not None:
            o[null_at].out = None
        if mask_at is not None:
            o[mask_at].mask = mask
        return o

    table = [("segs", segs), ("segs_dev", None), ("n_seg", 1), ("chunk", 1024), ("n_chunks", 1)]
    sums = [("out_sumsq", P), ("out_nonfinite", P)]
    ws = [("workspace", P), ("workspace_bytes", 24)]
    ctl = [("ctrl", ctrl), ("out_ctrl", P), ("ctrl_dev", P), ("next_times", P), ("state_in_dev", 0)]
    ctl_nulls = ["ctrl", "out_ctrl", "ctrl_dev", "next_times"]
    tail = [("dtype", F32), ("stream", None)]
    terms = [("k", K), ("coef", D), ("n_terms", 3)]
    tols = [("rtol_vec", P), ("rtol_scalar", 1e-3), ("atol_vec", None), ("atol_scalar", 1e-6)]
    no_tols = ("rtol_vec and atol_vec both null", dict(rtol_vec=None, atol_vec=None), EINVAL)
    multi_extra = (("null outs[0].out", dict(outs=multi_outs(null_at=0)), EINVAL),
                   ("null outs[n_out-1].out", dict(outs=multi_outs(null_at=1)), EINVAL),
                   ("mask == 0", dict(outs=multi_outs(mask=0, mask_at=0)), EINVAL),
                   ("mask == 0 in the last output", dict(outs=multi_outs(mask=0, mask_at=1)), EINVAL),
                   ("mask bit at n_terms", dict(outs=multi_outs(mask=0b1000, mask_at=0)), EINVAL),
                   ("mask bit above n_terms", dict(outs=multi_outs(mask=1 << 20, mask_at=1)), EINVAL),
                   ("mask bit at n_terms = 14", dict(outs=multi_outs(mask=1 << 14, mask_at=0), n_terms=14), EINVAL))
    multi = [("outs", multi_outs()), ("n_out", 2), ("y0", P), ("acc_in", None), ("k", K), ("n_terms", 3)]
    dense = [("y0", P), ("y1", P), ("f0", P), ("f1", P)]
    rk4_k = [("k1", P), ("k2", P), ("k3", P), ("k4", P)]
    # a stage reads k1..k<stage>: each of them missing in turn; with an empty state the stage alone is looked at
    rk4_missing = tuple((f"stage {s} without k{j}", dict(stage=s, **{f"k{j}": None}), EINVAL, False)
                        for s in range(1, 5) for j in range(1, s + 1)) + \
        (("n=0 looks at the stage only", dict(stage=2, k1=None, n=0), OK),)
    grid = [("grid", P), ("grid_dtype", F64), ("n_grid", 4), ("counter", P), ("perturb", 1), ("sign", 1.0)]
    modes = (ctypes.c_int * 4)(0, 0, 0, 0)

    return [
        Entry("tdeq_stage_combine", [("out", P), ("y0", P)] + terms + [("dt", 0.1), ("n", 4)] + tail,
              ["out", "y0", "k", "coef"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)], accepts=LOWP, empty=True),
        Entry("tdeq_stage_combine_timed",
              [("out", P), ("y0", P)] + terms + [("dt", 0.1), ("n", 4)] + tail + [("start_event", P), ("stop_event", P)],
              ["out", "y0", "k", "coef", "start_event", "stop_event"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 14)], extra=(("n=0", dict(n=0), EINVAL),)),
        Entry("tdeq_stage_combine_fill",
              [("out", P), ("y0", P), ("k", K), ("coef", D), ("n_terms", 2), ("dt", 0.1), ("n", 4), ("dtype", F32),
               ("fill_dst", P), ("fill_vals", D), ("n_fill", 2), ("stream", None)],
              ["out", "y0", "k", "coef", "fill_dst", "fill_vals"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 2), ("n_fill", 1, 16)], accepts=LOWP, extra=(("n=0", dict(n=0), EINVAL),)),
        Entry("tdeq_error_norm",
              [("scaled_out", None), ("y0", P), ("y1", P)] + terms + [("dt", 0.1)] + table + sums + ws + tail,
              ["y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 14)], accepts=NORM),
        Entry("tdeq_error_norm_vec",
              [("err_partial", None), ("y0", P), ("y1", P)] + terms + [("dt", 0.1)] + tols + table + sums + ws + tail,
              ["y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 14)],
              extra=(no_tols, ("n_terms=-1 with err_partial", dict(err_partial=P, n_terms=-1), EINVAL),
                     ("n_terms=15 with err_partial", dict(err_partial=P, n_terms=15), EINVAL))),
        Entry("tdeq_error_norm_vec_ctrl",
              [("err_partial", None), ("y0", P), ("y1", P)] + terms + [("dt", 0.1)] + tols + table + sums + ctl + ws + tail,
              ["y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"] + ctl_nulls,
              arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)],
              extra=(no_tols, ("n_terms=-1 with err_partial", dict(err_partial=P, n_terms=-1), EINVAL),
                     ("n_terms=15 with err_partial", dict(err_partial=P, n_terms=15), EINVAL))),
        Entry("tdeq_stage_combine_err",
              [("out", P), ("err_out", P), ("y0", P), ("k", K), ("coef", D), ("err_coef", D), ("n_terms", 3), ("dt", 0.1),
               ("n", 4)] + tail,
              ["out", "err_out", "y0", "k", "coef", "err_coef"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)],
              accepts=LOWP, empty=True),
        Entry("tdeq_stage_combine_multi", multi + [("dt", 0.1), ("n", 4)] + tail, ["outs", "y0", "k"],
              arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14), ("n_out", 1, 4)], empty=True, extra=multi_extra),
        Entry("tdeq_stage_combine_multi_dev", multi + [("ctrl_dev", P), ("n", 4)] + tail, ["outs", "y0", "k", "ctrl_dev"],
              arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14), ("n_out", 1, 4)], empty=True, extra=multi_extra),
        Entry("tdeq_stage_combine_multi_timed",
              multi + [("dt", 0.1), ("n", 4)] + tail + [("start_event", P), ("stop_event", P)],
              ["outs", "y0", "k", "start_event", "stop_event"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 14), ("n_out", 1, 4)], empty=True, extra=multi_extra),
        Entry("tdeq_error_norm_partial",
              [("err_partial", P), ("y0", P), ("y1", P), ("k", K), ("coef", D), ("n_terms", 2), ("dt", 0.1)] + table + sums +
              ws + tail,
              ["err_partial", "y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"],
              arrays=[("k", "n_terms")], counts=[("n_terms", 0, 2)], accepts=CPLX),
        # fp32 / fp64 / complex: continues err_partial with 0..2 terms; the 16-bit codes are refused HERE because a 16-bit
        # row is rounded once and has no partial sum to continue
        Entry("tdeq_error_norm_partial_ctrl",
              [("err_partial", P), ("y0", P), ("y1", P), ("k", K), ("coef", D), ("n_terms", 2), ("dt", 0.1)] + table + sums +
              ctl + [("copy_last_k", None)] + ws + tail,
              ["err_partial", "y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"] + ctl_nulls,
              arrays=[("k", "n_terms")], counts=[("n_terms", 0, 2)], accepts=CPLX,
              extra=(("copy_last_k with complex64", dict(copy_last_k=P, dtype=C64), EINVAL),
                     ("copy_last_k with complex128", dict(copy_last_k=P, dtype=C128), EINVAL),
                     ("copy_last_k without a term", dict(copy_last_k=P, n_terms=0), EINVAL))),
        # bfloat16 / float16: the whole error row in one launch — err_partial must be null, 1..14 terms
        Entry("tdeq_error_norm_partial_ctrl",
              [("err_partial", None), ("y0", P), ("y1", P)] + terms + [("dt", 0.1)] + table + sums + ctl +
              [("copy_last_k", None)] + ws + [("dtype", BF16), ("stream", None)],
              ["y0", "y1", "k", "coef", "segs", "out_sumsq", "out_nonfinite", "workspace"] + ctl_nulls,
              arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)], accepts=NORM, label="tdeq_error_norm_partial_ctrl[16-bit]",
              extra=tuple((f"{what} with dtype={code}", dict(ov, dtype=code), EINVAL) for code in (BF16, F16)
                          for what, ov in (("err_partial", dict(err_partial=P)), ("copy_last_k", dict(copy_last_k=P)),
                                           ("n_terms=0", dict(n_terms=0)), ("null k[2]", dict(k=ptr_array(16, 2)))))),
        Entry("tdeq_step_controller",
              [("sums", P), ("nonfinite", P), ("segs", segs), ("segs_dev", None), ("n_seg", 1)] + sums + ctl + tail,
              ["sums", "nonfinite", "segs", "out_sumsq", "out_nonfinite"] + ctl_nulls),
        Entry("tdeq_stage_combine_dev",
              [("out", P), ("err_out", None), ("y0", P), ("k", K), ("coef", D), ("err_coef", None), ("n_terms", 3),
               ("ctrl_dev", P), ("n", 4)] + tail,
              ["out", "y0", "k", "coef", "ctrl_dev"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)], accepts=LOWP,
              empty=True,
              extra=(("err_out without err_coef", dict(err_out=P), EINVAL),
                     ("bfloat16 with err_out", dict(err_out=P, err_coef=D, dtype=BF16), EINVAL),
                     ("float16 with err_out", dict(err_out=P, err_coef=D, dtype=F16), EINVAL))),
        Entry("tdeq_step_commit",
              [(a, P) for a in ("y_prev", "f_prev", "y_cur", "f_cur", "y1", "f1", "ctrl_dev")] + [("n", 4)] + tail,
              ["y_prev", "f_prev", "y_cur", "f_cur", "y1", "f1", "ctrl_dev"], empty=True),
        Entry("tdeq_stage_combine_sel",
              [(a, P) for a in ("out", "y_acc", "f_acc", "y_rej", "f_rej")] + [("coef", 0.2), ("ctrl_dev", P), ("n", 4)] + tail,
              ["out", "y_acc", "f_acc", "y_rej", "f_rej", "ctrl_dev"], accepts=LOWP, empty=True),
        Entry("tdeq_init_norms", [("mode", 0), ("a", P), ("b", P), ("yscale", P)] + table + sums + ws + tail,
              ["a", "b", "yscale", "segs", "out_sumsq", "out_nonfinite", "workspace"], counts=[("mode", 0, 1)], accepts=NORM),
        Entry("tdeq_init_norms_vec", [("mode", 0), ("a", P), ("b", P), ("yscale", P)] + tols + table + sums + ws + tail,
              ["a", "b", "yscale", "segs", "out_sumsq", "out_nonfinite", "workspace"], counts=[("mode", 0, 1)],
              extra=(no_tols,)),
        Entry("tdeq_init_scaled", [("mode", 0), ("a", P), ("b", P), ("yscale", P)] + table + [("out0", P), ("out1", P)] + tail,
              ["a", "b", "yscale", "segs", "out0"], counts=[("mode", 0, 1)], accepts=NORM,
              extra=(("mode 0 without out1", dict(out1=None), EINVAL),)),
        Entry("tdeq_dense_eval", [("out", P)] + dense + terms + [("dt", 0.1), ("x", 0.5), ("n", 4)] + tail,
              ["out", "y0", "y1", "f0", "f1", "k", "coef"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)],
              accepts=LOWP, empty=True),
        Entry("tdeq_dense_eval_multi",
              [("out", P), ("out_stride", 4)] + dense + terms + [("dt", 0.1), ("x", D), ("n_x", 2), ("n", 4)] + tail,
              ["out", "y0", "y1", "f0", "f1", "k", "coef", "x"], arrays=[("k", "n_terms")],
              counts=[("n_terms", 1, 14), ("n_x", 1, 16)], accepts=LOWP, empty=True,
              extra=(("out_stride < n with n_x > 1", dict(out_stride=3), EINVAL, False),
                     ("out_stride < n with n_x > 1 and an empty state", dict(out_stride=-1, n=0), EINVAL, False))),
        Entry("tdeq_interp_fit", [("coeffs", P)] + dense + terms + [("dt", 0.1), ("n", 4)] + tail,
              ["coeffs", "y0", "y1", "f0", "f1", "k", "coef"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 14)],
              accepts=LOWP, empty=True),
        Entry("tdeq_rk4_38_stage", [("stage", 4), ("out", P), ("y0", P)] + rk4_k + [("dt", 0.1), ("n", 4)] + tail,
              ["out", "y0"], counts=[("stage", 1, 4)], accepts=LOWP, empty=True,
              extra=rk4_missing + tuple((label + " (bfloat16)", dict(ov, dtype=BF16), e, False)
                                        for label, ov, e, *_ in rk4_missing)),
        Entry("tdeq_rk4_38_stage_dev", [("stage", 4), ("out", P), ("y0", P)] + rk4_k + [("dt_dev", P), ("n", 4)] + tail,
              ["out", "y0", "dt_dev"], counts=[("stage", 1, 4)], empty=True, extra=rk4_missing),
        Entry("tdeq_grid_advance", grid + [("times_out", P), ("dt_out", P), ("state_dtype", F32), ("stream", None)],
              ["grid", "counter", "times_out", "dt_out"], counts=[("n_grid", 2, None)], dtypes=("grid_dtype", "state_dtype")),
        Entry("tdeq_grid_advance_stages",
              grid + [("frac", D), ("mode", modes), ("n_times", 2), ("times_out", P), ("dt_out", P), ("state_dtype", F32),
                      ("stream", None)],
              ["grid", "counter", "frac", "mode", "times_out", "dt_out"], counts=[("n_grid", 2, None), ("n_times", 1, 4)],
              dtypes=("grid_dtype", "state_dtype")),
        Entry("tdeq_grid_commit",
              [("solution", P), ("row_stride", 4), ("y_cur", P), ("y_new", P), ("counter", P), ("n", 4)] + tail,
              ["solution", "y_cur", "y_new", "counter"], empty=True,
              extra=(("row_stride < n", dict(row_stride=3), EINVAL, False),)),
        Entry("tdeq_lerp", [("out", P), ("y0", P), ("y1", P), ("slope", 0.5), ("n", 4)] + tail, ["out", "y0", "y1"],
              accepts=LOWP, empty=True),
        Entry("tdeq_fixed_stage",
              [("mode", 0), ("out", P), ("y0", P), ("k", K), ("w", D), ("n_terms", 3), ("dt", 0.1), ("n", 4)] + tail,
              ["out", "y0", "k", "w"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 4), ("mode", 0, 1)], accepts=LOWP,
              empty=True, extra=(("mode 1 with two terms", dict(mode=1, n_terms=2), EINVAL),
                                 ("mode 1, n=0", dict(mode=1, n_terms=1, n=0), OK))),
        Entry("tdeq_fixed_stage_dev",
              [("mode", 0), ("out", P), ("y0", P), ("k", K), ("w", D), ("n_terms", 3), ("dt_dev", P), ("n", 4)] + tail,
              ["out", "y0", "k", "w", "dt_dev"], arrays=[("k", "n_terms")], counts=[("n_terms", 1, 4), ("mode", 0, 1)],
              empty=True, extra=(("mode 1 with two terms", dict(mode=1, n_terms=2), EINVAL),
                                 ("mode 1, n=0", dict(mode=1, n_terms=1, n=0), OK))),
        Entry("tdeq_weighted_sum", [("out", P), ("x", K), ("w", D), ("n_terms", 3), ("n", 4)] + tail, ["out", "x", "w"],
              arrays=[("x", "n_terms")], counts=[("n_terms", 1, 8)], accepts=LOWP, empty=True),
        Entry("tdeq_scale_many", [("outs", K), ("g", P), ("w", D), ("n_out", 3), ("n", 4)] + tail, ["outs", "g", "w"],
              arrays=[("outs", "n_out")], counts=[("n_out", 1, 14)], empty=True),
        Entry("tdeq_multi_dot", [("g", P), ("x", K), ("n_x", 3), ("n", 4), ("out", P)] + ws + tail,
              ["g", "x", "out", "workspace"], arrays=[("x", "n_x")], counts=[("n_x", 1, 14)]),
        Entry("tdeq_pack_segments",
              [("out", P), ("src", K), ("chunk_start", i64(0, 1)), ("numel", i64(4, 4)), ("scale", D), ("n_seg", 2),
               ("chunk", 1024), ("n_chunks", 2)] + tail,
              ["out", "src", "chunk_start", "numel", "scale"], counts=[("n_seg", 1, 16)],
              extra=(("chunk_start[0] != 0", dict(chunk_start=i64(1, 1)), EINVAL),
                     ("numel[0] < 0", dict(numel=i64(-1, 4)), EINVAL),
                     ("numel[1] < 0", dict(numel=i64(4, -1)), EINVAL),
                     ("chunk_start not increasing", dict(chunk_start=i64(0, 0)), EINVAL),
                     ("chunk_start decreasing", dict(chunk_start=i64(0, 2, 1), numel=i64(4, 4, 4), n_seg=3, n_chunks=4), EINVAL),
                     ("chunk_start[1] == n_chunks", dict(chunk_start=i64(0, 2)), EINVAL),
                     ("numel[0] above its chunks", dict(numel=i64(1025, 4)), EINVAL),
                     ("numel[1] above its chunks", dict(numel=i64(4, 1025)), EINVAL))),
        Entry("tdeq_fill_scalars", [("dst", P), ("vals", D), ("n_vals", 2)] + tail, ["dst", "vals"],
              counts=[("n_vals", 1, 16)]),
        Entry("tdeq_adams_predict",
              [("y_out", P), ("dy_out", None), ("delta_out", None), ("y0", P), ("f_hist", K), ("cb", D), ("cm", None),
               ("n_terms", 3), ("dt", 0.1), ("n", 4)] + tail,
              ["y_out", "y0", "f_hist", "cb"], arrays=[("f_hist", "n_terms")], counts=[("n_terms", 1, 14)], empty=True,
              extra=(("dy_out without delta_out", dict(dy_out=P, cm=D), EINVAL),
                     ("delta_out without dy_out", dict(delta_out=P, cm=D), EINVAL),
                     ("implicit without cm", dict(dy_out=P, delta_out=P), EINVAL),
                     ("implicit, n=0", dict(dy_out=P, delta_out=P, cm=D, n=0), OK))),
        Entry("tdeq_adams_correct",
              [("y_out", P), ("dy_out", P), ("f", P), ("delta", P), ("dy_old", P), ("y0", P), ("c", 0.1), ("compute", 1)] +
              table + [("n", 4), ("out_count", P), ("out_nonfinite", P)] + ws + tail,
              ["y_out", "dy_out", "f", "delta", "dy_old", "y0", "segs", "out_count", "out_nonfinite", "workspace"],
              extra=(("compute=0 needs dy_old all the same", dict(compute=0, y_out=None, f=None, delta=None, y0=None,
                                                                  dy_old=None), EINVAL),)),
    ]


@pytest.fixture(scope="module")
def lib():
    from torchdiffeq_amd import _native
    return _native.load_library()


def _entries():
    return _table()


def test_every_flat_entry_point_is_in_the_table():
    text = open(os.path.join(ROOT, "torchdiffeq_amd", "csrc", "tdeq_abi.hip")).read()
    defined = set(re.findall(r"^(?:int|size_t) (tdeq_\w+)\(", text, flags=re.M))
    assert len(defined) >= 40, "parse of tdeq_abi.hip failed"
    no_refusal = {"tdeq_abi_version", "tdeq_workspace_bytes", "tdeq_dots_workspace_bytes"}     # these return no status
    assert {e.name for e in _entries()} == defined - no_refusal


@pytest.mark.parametrize("label", [e.label for e in _table()])
def test_refusals(lib, label):
    (entry,) = [e for e in _entries() if e.label == label]
    cases = entry.cases()
    assert len(cases) >= 10
    wrong = []
    for what, overrides, expected in cases:
        got = entry.call(lib, **overrides)
        assert got in (EINVAL, EWORKSPACE, OK), f"{label}: {what}: status {got} — this call got past the argument checks"
        if got != expected:
            wrong.append((what, expected, got))
    assert not wrong, f"{label}: (case, expected, returned) {wrong}"


def test_two_faults_at_once(lib):
    """Where two faults meet, the order of the checks decides the status.  (test_refusals repeats every refusal with an
    empty state and a short workspace; these are the pairs spelled out.)"""
    e = {x.label: x for x in _entries()}
    for name in ("tdeq_error_norm", "tdeq_error_norm_vec", "tdeq_error_norm_vec_ctrl", "tdeq_error_norm_partial",
                 "tdeq_error_norm_partial_ctrl", "tdeq_error_norm_partial_ctrl[16-bit]", "tdeq_init_norms",
                 "tdeq_init_norms_vec", "tdeq_adams_correct"):
        assert e[name].call(lib, workspace_bytes=23) == EWORKSPACE, name
        assert e[name].call(lib, workspace_bytes=23, chunk=1000) == EINVAL, name        # the segment table first
        assert e[name].call(lib, workspace_bytes=23, n_chunks=0) == EINVAL, name
        assert e[name].call(lib, workspace_bytes=0, n_chunks=2 ** 31) == EINVAL, name
    for name in ("tdeq_stage_combine", "tdeq_stage_combine_err", "tdeq_stage_combine_multi", "tdeq_stage_combine_multi_dev",
                 "tdeq_stage_combine_multi_timed", "tdeq_stage_combine_dev", "tdeq_dense_eval", "tdeq_dense_eval_multi",
                 "tdeq_interp_fit", "tdeq_adams_predict"):
        assert e[name].call(lib, n=0) == OK, name
        assert e[name].call(lib, n=0, n_terms=0) == EINVAL, name                        # the term count before n == 0
        assert e[name].call(lib, n=0, n_terms=15) == EINVAL, name
        arr = "f_hist" if name == "tdeq_adams_predict" else "k"
        assert e[name].call(lib, n=0, **{arr: ptr_array(16, null_at=2)}) == EINVAL, name      # and every k[j]
    for name in ("tdeq_rk4_38_stage", "tdeq_rk4_38_stage_dev"):
        for stage in (0, 5):
            assert e[name].call(lib, n=0, stage=stage) == EINVAL, name
        assert e[name].call(lib, n=0, stage=1) == OK, name
    assert e["tdeq_multi_dot"].call(lib, workspace_bytes=23) == EWORKSPACE
    assert e["tdeq_multi_dot"].call(lib, workspace_bytes=23, n_x=15) == EINVAL
