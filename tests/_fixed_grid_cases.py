"""Shared pieces of the fixed-grid captured-step tests (tests/test_fixed_grid_oracle.py on the CPU,
tests/test_fixed_grid_kernels_gpu.py on the MI355X, tests/golden/make_golden_fixed_grid.py): the edge grids, the stage
lists, the inputs of the stage kernels, the bit-for-bit comparison and sentinel-bordered output windows.  No test in here."""
import math

import numpy as np
import torch

DT = {"f32": torch.float32, "f64": torch.float64}
NP = {"f32": np.float32, "f64": np.float64}
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
METHODS = ("euler", "midpoint", "heun2", "heun3", "rk4")

# Every entry is a float32 number, so the same list serves a float and a double grid.  Strictly increasing: a negative
# time, a step that ends on zero and one that starts there, a float32 subnormal, the smallest float32 normal, a one-ulp
# interval (1, 1 + 2^-23), a time where x + 1 == x in float32 but not in float64 (2^24), dt over 50 binades.
EDGE_GRID = (-2.5, -1.0, -2.0 ** -30, 0.0, 2.0 ** -140, 2.0 ** -126, float(np.float32(1 / 3)), 1.0, 1.0 + 2.0 ** -23,
             2.0 ** 24, 2.0 ** 24 + 2.0, 2.0 ** 40)
ONE_ULP_INTERVAL = EDGE_GRID.index(1.0)
# float64 only: none of these is a float32 number (the double-grid, float-state cast); 1e-320 is a float64 subnormal
CAST_GRID = tuple(sorted((0.1, 0.1 + 2.0 ** -40, 1e-320, 1 / 3, 1.0 - 2.0 ** -53, 1e10 + 1 / 7)))
GRIDS = {"edge": EDGE_GRID, "cast": CAST_GRID}

assert all(float(np.float32(x)) == x for x in EDGE_GRID) and all(float(np.float32(x)) != x for x in CAST_GRID)
assert all(a < b for g in GRIDS.values() for a, b in zip(g, g[1:]))


def golden_cases():
    """(key, grid name, state, grid type, perturb, reversed) of every recorded reference solve, without the method."""
    out = []
    for gname in GRIDS:
        for state in DT:
            for gtype in DT:
                if gname == "cast" and gtype == "f32":
                    continue
                for perturb in (False, True):
                    for rev in (False, True):
                        key = "{}_y{}_t{}_{}_{}".format(gname, state, gtype, "perturb" if perturb else "plain",
                                                        "rev" if rev else "fwd")
                        out.append((key, gname, state, gtype, perturb, rev))
    return out


def graph_times(method):
    """((fraction of dt, mode bits), ...) of the method's stage times: the solver class's `_graph_times`."""
    from torchdiffeq_amd.solvers import fixed
    cls = {"euler": fixed.Euler, "midpoint": fixed.Midpoint, "heun2": fixed.Heun2, "heun3": fixed.Heun3,
           "rk4": fixed.RK4}[method]
    return cls._graph_times


# stage lists no solver uses: 1 to 4 times, mode bits 1 (t1), 2 (NEXT), 4 (PREV) mixed, frac = 0 with bit 1 set, NEXT and PREV
# on the same time, a fraction that is no float32 number
SYNTHETIC_STAGES = (
    ((0.0, 1),),
    ((0.7, 4), (0.0, 1 | 2)),
    ((0.0, 4), (0.25, 2 | 4), (1.0, 2)),
    ((0.1, 0), (0.0, 1 | 4), (0.9, 2), (0.0, 2 | 4)),
)


def walk_grid(kern, grid, sign, perturb, stages, state_dtype, calls=None):
    """`grid_advance_stages` of the CPU oracle `kern` from counter = -1 over the whole grid.  One entry per call:
    (counter, times [n_times] or None, dt or None) — None where the call wrote nothing (c + 1 >= n_grid)."""
    fracs, modes = [f for f, _ in stages], [m for _, m in stages]
    counter = torch.full((), -1, dtype=torch.int64)
    times = torch.empty(len(stages), dtype=state_dtype)
    dt = torch.empty(1, dtype=torch.float64)
    out = []
    for _ in range(grid.numel() if calls is None else calls):
        times.fill_(math.nan)
        dt.fill_(math.nan)
        kern.grid_advance_stages(grid, counter, perturb, sign, fracs, modes, times, dt)
        wrote = int(counter) + 1 < grid.numel()
        if not wrote:
            assert bool(torch.isnan(times).all()) and bool(torch.isnan(dt).all())
        out.append((int(counter), times.clone() if wrote else None, dt.clone() if wrote else None))
    return out


def bits(t):
    return t.contiguous().view(INT[t.dtype])


def same_bits(got, ref, what=""):
    """Every bit: NaN payloads, the sign of a zero and subnormals count."""
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    diff = bits(got) != bits(ref)
    if bool(diff.any()):
        at = int(diff.reshape(-1).nonzero()[0])
        raise AssertionError((what, int(diff.sum()), at, got.reshape(-1)[at].item(), ref.reshape(-1)[at].item()))


def same_as_host_arithmetic(got, ref, what=""):
    """A kernel's arithmetic against the CPU oracle's: every bit where the oracle's value is a number (zeros with their
    sign, subnormals, inf); where it is NaN the kernel's must be NaN.  The payload of a NaN that an operation creates
    (inf - inf, 0 * inf) is the processor's choice — x86 sets the sign bit, the GPU does not — so it is compared only
    between two device results (`same_bits` against the host-dt entry point)."""
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nan_got, nan_ref = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_got, nan_ref), (what, "NaN at other positions", int((nan_got != nan_ref).sum()))
    diff = (bits(got) != bits(ref)) & ~nan_ref
    if bool(diff.any()):
        at = int(diff.nonzero()[0])
        raise AssertionError((what, int(diff.sum()), at, got[at].item(), ref[at].item()))


def draw(n, seed, dtype, count):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g, dtype=torch.float64).to(dtype) for _ in range(count)]


def draw_edge(n, seed, dtype, count):
    """`count` tensors of the values at which a stage kernel can differ from the oracle (the idea of
    `_lowp_kernels.draw_edge` at the ranges of float32 / float64).  The kind of value is chosen per POSITION, for all
    tensors alike, so that sums and products of them stay in that range:
      0  ordinary (randn),
      1  the type's subnormals and the 12 binades above them (products with dt and the weights fall below the normals),
      2  a quarter of the type's largest value up to that value: products and sums overflow to inf,
      3  per tensor one of +0, -0, +inf, -inf, NaN or an ordinary value."""
    g = torch.Generator().manual_seed(seed)
    kind = (torch.arange(n) + seed) % 4
    fi = torch.finfo(dtype)
    big = float(fi.max)
    lo = math.log2(fi.smallest_normal) - (23 if dtype == torch.float32 else 52)
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan], dtype=torch.float64)
    out = []
    for _ in range(count):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        sgn = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
        span = (23 if dtype == torch.float32 else 52) + 12.0
        tiny = sgn * torch.exp2(lo + span * torch.rand(n, generator=g, dtype=torch.float64))
        large = sgn * big * (0.25 + 0.75 * torch.rand(n, generator=g, dtype=torch.float64))
        pick = torch.randint(0, 8, (n,), generator=g)
        spec = torch.where(pick < 5, special[pick.clamp(max=4)], x)
        v = torch.where(kind == 1, tiny, torch.where(kind == 2, large, torch.where(kind == 3, spec, x)))
        out.append(v.to(dtype))
    return out


def dev(ts, offset=0):
    """On the GPU; offset > 0: a view that starts `offset` elements into its buffer (not 16-byte aligned)."""
    out = []
    for t in ts:
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
        buf[offset:].copy_(t)
        assert (buf[offset:].data_ptr() % 16 == 0) == (offset == 0)
        out.append(buf[offset:])
    return out


PAD = 64
SENTINEL = {torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5, torch.int64: 0x5A5A5A5A5A5A5A5A}


class Window:
    """An output tensor of `n` elements (`rows` rows `stride` apart) carved out of a larger allocation filled with a
    sentinel bit pattern — a NaN with a payload no kernel produces — starting `offset` elements past a 16-byte boundary."""

    def __init__(self, n, dtype, offset=0, rows=1, stride=None, device="cuda"):
        stride = n if stride is None else stride
        self.itype = INT.get(dtype, dtype)
        self.sentinel = SENTINEL[dtype]
        self.lo = PAD + offset
        self.hi = self.lo + (rows - 1) * stride + n
        self.raw = torch.full((self.hi + PAD,), self.sentinel, dtype=self.itype, device=device)
        self.big = self.raw.view(dtype)
        assert self.big.data_ptr() % 16 == 0
        self.t = self.big[self.lo:self.hi] if rows == 1 else self.big[self.lo:].as_strided((rows, n), (stride, 1))

    def intact(self):
        return bool((self.raw[:self.lo] == self.sentinel).all()) and bool((self.raw[self.hi:] == self.sentinel).all())

    def untouched(self):
        """The window itself still holds the sentinel everywhere."""
        return bool((self.raw == self.sentinel).all())
