"""Shared builders of the per-element-tolerance kernel tests (tests/test_vec_tol_oracle.py on the CPU twin,
tests/test_vec_tol_kernels_gpu.py on the HIP kernels): segmented layouts that reach every segment-table path, seeded
inputs with NaN in every padding element, the reference's expressions evaluated literally by ATen on the CPU, and the
step-controller argument block."""
import math

import numpy as np
import torch

from torchdiffeq_amd import _native

CHUNK = 1024
DT = 0.0371
# 14 error-row weights (the longest row the kernels take); magnitudes of a tableau's c_error
COEFS = (0.0371, -0.211, 0.5, 1.25, -0.0625, 0.33, 0.9, -0.47, 0.018, 0.73, -1.1, 0.26, 0.061, -0.84)


def _seeded_numels(n_seg):
    g = torch.Generator().manual_seed(n_seg)
    numels = [int(v) for v in torch.randint(1, 3 * CHUNK, (n_seg,), generator=g)]
    numels[1] = 5 * CHUNK + 17                      # one segment of several chunks with a ragged end
    return numels


# name -> segment numels (each padded to a multiple of the chunk); every segment <= 6000 elements, so the 1e-12 bound the
# project uses for fp64 sums of <= 5000..6000 squares carries over
LAYOUTS = {
    "one_1": [1], "one_1031": [1031], "one_5000": [5000],   # single segment
    "three": [1, 1024, 1025],                                # inline table, fused controller (<= 4 segments)
    "four": [1023, 7, 2049, 1],                              # the last inline-controller bucket
    "five": [5, 1024, 3000, 1, 1500],                        # parallel finalize + presummed controller, inline table
    "sixteen": _seeded_numels(16),                           # the last inline table
    "seventeen": _seeded_numels(17),                         # device table
}
assert all(m <= 6000 for v in LAYOUTS.values() for m in v)


class Layout:
    def __init__(self, name, numels=None):
        self.name, self.numels = name, list(LAYOUTS[name] if numels is None else numels)
        self.offs, off = [], 0
        for m in self.numels:
            self.offs.append(off)
            off += -(-m // CHUNK) * CHUNK
        self.total, self.n_seg = off, len(self.numels)
        # the tolerances of the segment table are what the product passes with per-element tolerances: (0, 1)
        self.segs = [(o, m, 0.0, 1.0) for o, m in zip(self.offs, self.numels)]
        self.valid = torch.zeros(self.total, dtype=torch.bool)
        for o, m in zip(self.offs, self.numels):
            self.valid[o:o + m] = True

    def plan(self, kern, device=None):
        return kern.make_plan(self.segs, self.total, CHUNK, device)

    def index(self, seg, t):
        """Flat padded index of element t of segment seg."""
        assert 0 <= t < self.numels[seg]
        return self.offs[seg] + t

    def poison(self, x):
        """NaN in every padding element of x (a flat padded stream), in place."""
        x[~self.valid] = float("nan")
        return x


class Inputs:
    """Seeded streams over a layout, CPU tensors.  State-typed: y0, y1, ks[14], a, b, yscale; fp64: rtol_v, atol_v.  Every
    padding element of every stream is NaN: a kernel whose `valid` or base is off reads one and its sum turns NaN."""

    def __init__(self, layout, dtype, seed=0, err_scale=1e-4):
        g = torch.Generator().manual_seed(1000 * seed + layout.total)
        n = layout.total
        r = lambda s=1.0: layout.poison((torch.randn(n, generator=g, dtype=torch.float64) * s).to(dtype))
        self.layout, self.dtype = layout, dtype
        self.y0, self.y1 = r(), r()
        self.ks = [r(err_scale) for _ in range(14)]
        self.a, self.b, self.yscale = r(), r(), r()
        self.rtol_v = layout.poison(torch.rand(n, generator=g, dtype=torch.float64) * 1e-3 + 1e-6)
        self.atol_v = layout.poison(torch.rand(n, generator=g, dtype=torch.float64) * 1e-5 + 1e-8)

    def tolerances(self, form):
        """(rtol, atol) of the form `both` / `rtol_only` / `atol_only`: an fp64 vector, or a Python float (0-dim)."""
        return (self.rtol_v if form != "atol_only" else 3e-4), (self.atol_v if form != "rtol_only" else 2e-6)

    def streams(self):
        return [self.y0, self.y1, *self.ks, self.a, self.b, self.yscale]


def to_device(x, misalign=False):
    """x on the GPU; `misalign`: as a view that starts one element into its allocation (4 or 8 bytes off a 16-byte base)."""
    if not misalign:
        return x.cuda()
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    buf[1:].copy_(x)
    out = buf[1:]
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def _w(tol):
    """A tolerance as the reference holds it: a dimensioned fp64 tensor, or a 0-dim fp64 tensor (rk_common.py:186-187)."""
    return tol if isinstance(tol, torch.Tensor) else torch.tensor(tol, dtype=torch.float64)


def aten_error_sums(layout, y0, y1, ks, coefs, dt, rtol, atol, partial=None):
    """misc.py:80-82 evaluated literally by ATen on CPU tensors, type promotion included (a dimensioned fp64 tolerance
    promotes, a 0-dim one does not); the error row left to right with every product and sum rounded in T
    (rk_common.py:89).  Per-segment sums of squares, each segment evaluated on its own slice."""
    dtype = y0.dtype
    dtT = torch.tensor(dt, dtype=torch.float64).to(dtype)
    rtol, atol = _w(rtol), _w(atol)
    sums = []
    for o, m in zip(layout.offs, layout.numels):
        sl = slice(o, o + m)
        err = None if partial is None else partial[sl]
        for k_, c in zip(ks, coefs):
            p = k_[sl] * (torch.tensor(c, dtype=torch.float64).to(dtype) * dtT)
            err = p if err is None else err + p
        tol = (atol[sl] if atol.dim() else atol) + (rtol[sl] if rtol.dim() else rtol) * torch.max(y0[sl].abs(), y1[sl].abs())
        q = err / tol
        assert q.dtype == torch.float64
        sums.append(float(q.abs().pow(2).sum()))
    return sums


def aten_init_sums(layout, mode, a, b, y, rtol, atol):
    """misc.py:50-56, 68 the same way: scale = atol + |y| * rtol; mode 0 -> (sum (a/scale)^2, sum (b/scale)^2), mode 1 ->
    (sum ((a - b)/scale)^2, None) per segment."""
    rtol, atol = _w(rtol), _w(atol)
    s0, s1 = [], []
    for o, m in zip(layout.offs, layout.numels):
        sl = slice(o, o + m)
        scale = (atol[sl] if atol.dim() else atol) + torch.abs(y[sl]) * (rtol[sl] if rtol.dim() else rtol)   # misc.py:50
        assert scale.dtype == torch.float64
        if mode == 0:
            s0.append(float((a[sl] / scale).abs().pow(2).sum()))        # misc.py:55
            s1.append(float((b[sl] / scale).abs().pow(2).sum()))        # misc.py:56
        else:
            q = (a[sl] - b[sl]) / scale                                 # misc.py:68
            assert q.dtype == torch.float64
            s0.append(float(q.abs().pow(2).sum()))
    return s0, (s1 if mode == 0 else None)


def close(got, want, rel=1e-12):
    """Per-segment sums equal to `rel`; non-finite entries equal as such (NaN == NaN, inf == inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(got[~fin], want[~fin], equal_nan=True):
        return False
    return bool(np.all(np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin])))


def max_rel_diff(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def step_ctrl(t0, dt, order, tab, sign=1.0, min_step=0.0, max_step=math.inf, n_norm_seg=1, np_dtype=np.float64):
    """The controller's argument block for a trial step (t0, dt) of the pair `tab`: the reference's constants, the stage
    abscissae rounded to the state's type."""
    c = _native.StepCtrl()
    c.t0, c.dt = t0, dt
    c.safety, c.ifactor, c.dfactor = 0.9, 10.0, 0.2
    c.exponent = 1.0 / order
    c.min_step, c.max_step, c.time_sign = min_step, max_step, sign
    mask = 0
    for i, a in enumerate(tab.alpha):
        c.alpha[i] = float(np_dtype(a))
        if a == 1.0:
            mask |= 1 << i
    c.alpha_is_one, c.n_times, c.n_norm_seg = mask, len(tab.alpha), n_norm_seg
    return c


def ctrl_rows():
    """(tableau, order, sign, t0, dt, min_step, max_step): forward, backward, forced reject, forced accept."""
    from torchdiffeq_amd.tableaus import DOPRI5, DOPRI8
    return [(DOPRI5, 5, 1.0, 0.37, 0.0123, 0.0, math.inf),
            (DOPRI8, 8, -1.0, -2.5, 0.31, 0.0, math.inf),
            (DOPRI5, 5, 1.0, 1e3, 0.5, 0.1, 0.4),           # dt > max_step: forced reject
            (DOPRI5, 5, 1.0, 0.0, 0.05, 0.05, 1.0)]         # dt <= min_step: forced accept


# The fp32 rounding band of the error ratio: partial = 1 everywhere, no remaining stages, y0 = y1 = 0, rtol the 0-dim 0,
# atol[i] = 1 -/+ 2^-30.  err / tol = 1 / (1 -/+ 2^-30) in fp64, ratio = sqrt(mean(.^2)) = 1 +/- 9.3e-10: above (below) 1 in
# fp64, exactly 1.0 once rounded to fp32 (half an fp32 ulp at 1 is 6e-8).  A sum of n equal fp64 values and its mean carry
# at most ~n * 1.1e-16 relative error, far inside 9.3e-10 for the segment sizes used.
BAND_ATOL = {"reject": 1.0 - 2.0 ** -30, "accept": 1.0 + 2.0 ** -30}


def band_inputs(layout, dtype, which):
    n = layout.total
    z = lambda: layout.poison(torch.zeros(n, dtype=dtype))
    part = layout.poison(torch.ones(n, dtype=dtype))
    atol_v = layout.poison(torch.full((n,), BAND_ATOL[which], dtype=torch.float64))
    return z(), z(), part, atol_v
