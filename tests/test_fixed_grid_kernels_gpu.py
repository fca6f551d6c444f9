"""The kernels that keep a fixed-grid step's data on the device (csrc/tdeq_kernels.hpp: grid_advance_kernel,
grid_advance_stages_kernel, grid_commit_kernel, the `dt_dev` branch of fixed_stage_kernel / rk4_kernel,
fill_scalars_kernel), entry point by entry point on the MI355X against oracle/kernels.py — the rule of
include/tdeq_hip.h restated in numpy scalars and pinned to the reference by tests/test_fixed_grid_oracle.py:

  a. tdeq_grid_advance_stages / tdeq_grid_advance: counter, stage times and dt after every call of a walk over the edge
     grids (tests/_fixed_grid_cases.py), all (grid type, state type) pairs, `perturb` off and on, both signs, every
     method's stage list and synthetic ones; nothing but the counter is written past the last interval;
  b. tdeq_grid_commit: only row counter + 1, columns [0, n) and y_cur change, with padded and unaligned rows;
  c. tdeq_fixed_stage_dev / tdeq_rk4_38_stage_dev: the 16-byte body, the scalar tail and the unaligned instantiation,
     at step sizes where rounding `*dt_dev` to the state's type on the device could differ from the host's rounding;
  d. tdeq_fill_scalars against its oracle twin;
  e. one whole captured step per method from these kernels alone, and the same solve through `odeint(hip_graph=True)`.

Every comparison is of bit patterns (tests/_fixed_grid_cases.py: `same_bits`; `same_as_host_arithmetic` where the oracle's
value is a NaN that an operation created).  Every output lies in a window bordered by a sentinel pattern that is checked
after the call.  No tensor has more than 65536 + 7 elements."""
import math
import warnings

import pytest
import torch

import torchdiffeq_amd as tda
from _fixed_grid_cases import (DT, EDGE_GRID, GRIDS, INT, METHODS, ONE_ULP_INTERVAL, SYNTHETIC_STAGES, Window, bits, dev,
                               draw, draw_edge, graph_times, same_as_host_arithmetic, same_bits, walk_grid)
from torchdiffeq_amd._graph import _DtCell
from torchdiffeq_amd._native import _check, dtype_code

pytestmark = pytest.mark.gpu
TYPES = ["f32", "f64"]
GRID_CASES = [("edge", "f32"), ("edge", "f64"), ("cast", "f64")]     # the cast grid's entries are no float32 numbers


# ---------------------------------------------------------------------------------------------------------------------
# a. the next step's dt and stage times
# ---------------------------------------------------------------------------------------------------------------------
def stage_lists():
    return [(m, graph_times(m)) for m in METHODS] + [("synthetic%d" % len(s), s) for s in SYNTHETIC_STAGES]


class StepData:
    """counter, times_out[4] and dt_out of a walk, each inside its own sentinel-bordered window."""

    def __init__(self, state_dtype):
        self.counter = Window(1, torch.int64)
        self.times = Window(4, state_dtype)
        self.dt = Window(1, torch.float64)
        self.counter.t.fill_(-1)

    def reset_outputs(self):
        self.times.raw.fill_(self.times.sentinel)
        self.dt.raw.fill_(self.dt.sentinel)

    def check(self, ref, n_times, what):
        c_ref, t_ref, dt_ref = ref
        assert int(self.counter.t[0]) == c_ref, what
        assert self.counter.intact() and self.times.intact() and self.dt.intact(), what
        if t_ref is None:                                   # c + 1 >= n_grid: only the counter has changed
            assert self.times.untouched() and self.dt.untouched(), what
            return
        same_bits(self.times.t[:n_times], t_ref, what)
        same_bits(self.dt.t, dt_ref, what)
        raw = self.times.raw.cpu()
        assert bool((raw[self.times.lo + n_times:] == self.times.sentinel).all()), (what, "times_out[n_times:] written")


@pytest.mark.parametrize("state", TYPES)
@pytest.mark.parametrize("gname,gtype", GRID_CASES, ids=["-".join(c) for c in GRID_CASES])
def test_grid_advance_stages_walk(hip_kernels, oracle_kernels, gname, gtype, state):
    t = torch.tensor(GRIDS[gname], dtype=torch.float64).to(DT[gtype])
    for sign in (1.0, -1.0):
        grid = t if sign > 0 else (-t.flip(0)).contiguous()          # a decreasing t is solved as -t with sign = -1
        grid_dev = grid.cuda()
        for perturb in (False, True):
            for name, stages in stage_lists():
                fracs, modes = [f for f, _ in stages], [m for _, m in stages]
                refs = walk_grid(oracle_kernels, grid, sign, perturb, stages, DT[state])
                assert len(refs) == grid.numel() and refs[-1][1] is None and refs[-2][1] is not None
                d = StepData(DT[state])
                for call, ref in enumerate(refs):
                    d.reset_outputs()
                    hip_kernels.grid_advance_stages(grid_dev, d.counter.t[0], perturb, sign, fracs, modes, d.times.t, d.dt.t)
                    d.check(ref, len(stages), (gname, gtype, state, sign, perturb, name, call))


@pytest.mark.parametrize("state", TYPES)
@pytest.mark.parametrize("gname,gtype", GRID_CASES, ids=["-".join(c) for c in GRID_CASES])
def test_grid_advance_is_the_stage_walk_of_rk4(hip_kernels, oracle_kernels, gname, gtype, state):
    t = torch.tensor(GRIDS[gname], dtype=torch.float64).to(DT[gtype])
    stages = graph_times("rk4")
    fracs, modes = [f for f, _ in stages], [m for _, m in stages]
    for sign in (1.0, -1.0):
        grid = t if sign > 0 else (-t.flip(0)).contiguous()
        grid_dev = grid.cuda()
        for perturb in (False, True):
            counter = torch.full((), -1, dtype=torch.int64)
            times, dt = torch.empty(4, dtype=DT[state]), torch.empty(1, dtype=torch.float64)
            d, via_stages = StepData(DT[state]), StepData(DT[state])
            for call in range(grid.numel()):
                what = (gname, gtype, state, sign, perturb, call)
                times.fill_(math.nan)
                oracle_kernels.grid_advance(grid, counter, perturb, sign, times, dt)
                wrote = int(counter) + 1 < grid.numel()
                assert bool(torch.isnan(times).all()) != wrote
                d.reset_outputs()
                hip_kernels.grid_advance(grid_dev, d.counter.t[0], perturb, sign, d.times.t, d.dt.t)
                d.check((int(counter), times if wrote else None, dt if wrote else None), 4, what)
                via_stages.reset_outputs()
                hip_kernels.grid_advance_stages(grid_dev, via_stages.counter.t[0], perturb, sign, fracs, modes,
                                                via_stages.times.t, via_stages.dt.t)
                assert torch.equal(d.counter.raw, via_stages.counter.raw) and torch.equal(d.times.raw, via_stages.times.raw) \
                    and torch.equal(d.dt.raw, via_stages.dt.raw), what


# ---------------------------------------------------------------------------------------------------------------------
# b. the step's result becomes an output row and the next state
# ---------------------------------------------------------------------------------------------------------------------
def any_bits(n, seed, dtype):
    """Uniformly drawn bit patterns (NaNs with every payload, subnormals, both zeros among them) with -0.0, a quiet and a
    signalling NaN with payloads planted at the front."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64)
    if dtype == torch.float32:
        raw = lo.to(torch.int32)
    else:
        raw = (torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64) << 32) | lo
    t = raw.view(dtype).clone()
    planted = [-0.0] if n < 3 else [-0.0, math.nan, math.nan]
    t[:len(planted)] = torch.tensor(planted, dtype=dtype)
    if n >= 3:
        b = bits(t)
        b[1] |= 0x1234                                                   # a quiet NaN with a payload
        b[2] = (0x7F800000 if dtype == torch.float32 else 0x7FF0000000000000) | 0x4321     # a signalling one
    return t


COMMIT_ROWS = 4


@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 65536 + 7])
def test_grid_commit_writes_one_row_and_the_state(hip_kernels, oracle_kernels, n, name):
    dtype = DT[name]
    y_new = any_bits(n, 11 + n, dtype)
    y_new_dev = y_new.cuda()
    for layout, (stride, offset) in {"dense": (n, 0), "padded": (n + 3, 0), "unaligned": (n, 1)}.items():
        for c in (-1, 0, COMMIT_ROWS - 2):                   # row c + 1 of 4: never outside [-1, n_grid - 2]
            what = (n, name, layout, c)
            assert -1 <= c <= COMMIT_ROWS - 2
            sol = Window(n, dtype, offset, rows=COMMIT_ROWS, stride=stride)
            assert sol.t.shape == (COMMIT_ROWS, n) and (sol.t.stride(0) == stride or n == 1)
            assert (sol.t.data_ptr() % 16 == 0) == (offset == 0)
            assert sol.lo + (COMMIT_ROWS - 1) * stride + n == sol.hi <= sol.raw.numel() - 64
            y_cur = Window(n, dtype, offset)
            counter = torch.full((), c, dtype=torch.int64, device="cuda")
            # as HipKernels.grid_commit does, with the row stride given (a one-column view has no stride of its own)
            _check(hip_kernels.lib.tdeq_grid_commit(sol.t.data_ptr(), stride, y_cur.t.data_ptr(), y_new_dev.data_ptr(),
                                                    counter.data_ptr(), n, dtype_code(dtype), hip_kernels._stream()),
                   "tdeq_grid_commit")
            assert int(counter) == c
            expect = torch.full((sol.raw.numel(),), sol.sentinel, dtype=INT[dtype])
            ref_rows = expect.view(dtype)[sol.lo:].as_strided((COMMIT_ROWS, n), (stride, 1))
            ref_cur = torch.full((n,), math.nan, dtype=dtype)
            oracle_kernels.grid_commit(ref_rows, ref_cur, y_new, torch.tensor(c, dtype=torch.int64))
            same_bits(ref_cur, y_new, what)
            assert torch.equal(sol.raw.cpu(), expect), (what, "solution: something else than row c + 1, columns [0, n)")
            same_bits(y_cur.t, ref_cur, what)
            assert y_cur.intact(), what
            same_bits(y_new_dev, y_new, what)


def test_grid_commit_through_the_wrapper(hip_kernels, oracle_kernels):
    """HipKernels.grid_commit itself (it takes the row stride from the tensor) on a padded solution."""
    n, dtype = 1031, torch.float32
    y_new = any_bits(n, 5, dtype)
    sol = Window(n, dtype, 0, rows=COMMIT_ROWS, stride=n + 3)
    y_cur = Window(n, dtype)
    hip_kernels.grid_commit(sol.t, y_cur.t, y_new.cuda(), torch.full((), 1, dtype=torch.int64, device="cuda"))
    expect = torch.full((sol.raw.numel(),), sol.sentinel, dtype=torch.int32)
    ref_rows = expect.view(dtype)[sol.lo:].as_strided((COMMIT_ROWS, n), (n + 3, 1))
    oracle_kernels.grid_commit(ref_rows, torch.empty(n, dtype=dtype), y_new, torch.tensor(1, dtype=torch.int64))
    assert torch.equal(sol.raw.cpu(), expect)
    same_bits(y_cur.t, y_new)
    assert y_cur.intact()


# ---------------------------------------------------------------------------------------------------------------------
# c. stage kernels with the step size read on the device
# ---------------------------------------------------------------------------------------------------------------------
THIRD, TWO_THIRDS = 1 / 3, 2 / 3
# (mode, weights): what Heun2 / Heun3 launch — mode 1 with one term, mode 0 with one and two — and mode 0 with 3 and 4 terms
FIXED_CASES = [(1, (1.0,)), (1, (THIRD,)), (0, (TWO_THIRDS,)), (0, (0.5, 0.5)), (0, (1 / 4, 3 / 4)),
               (0, (1 / 4, THIRD, 3 / 4)), (0, (1 / 4, THIRD, TWO_THIRDS, 3 / 4))]
STAGE_SIZES = [1, 2, 3, 5, 255, 1023, 1024, 1025, 4099, 65536 + 7]


def dt_values(oracle_kernels):
    """Step sizes as double: plain ones, one that is no float32 number and rounds up, one below the float32 subnormals,
    one beyond the float32 range, a negative zero, and the dt the oracle forms for the one-ulp interval of the edge grid."""
    grid = torch.tensor(EDGE_GRID, dtype=torch.float32)
    one_ulp = float(walk_grid(oracle_kernels, grid, 1.0, False, graph_times("euler"), torch.float32)[ONE_ULP_INTERVAL][2])
    assert one_ulp == 2.0 ** -23
    return [0.1, -0.1, 1.0 + 2.0 ** -30, 1e-46, 1e39, -0.0, one_ulp]


def dt_cell(value):
    """{unused, sign * dt} as `_integrate_graph` lays it out: the kernels get a pointer to word 1."""
    cell = torch.tensor([math.nan, value], dtype=torch.float64, device="cuda")
    return cell, torch.tensor([math.nan, value], dtype=torch.float64)[1:]


def run_stage(kern, case, out, y0, ks, dt, on_device):
    kind, a, b = case
    if kind == "fixed":
        (kern.fixed_stage_dev if on_device else kern.fixed_stage)(a, out, y0, ks[:len(b)], b, dt)
    else:
        k = list(ks[:a]) + [None] * (4 - a)
        (kern.rk4_stage_dev if on_device else kern.rk4_stage)(a, out, y0, k[0], k[1], k[2], k[3], dt)


STAGE_CASES = [("fixed", m, w) for m, w in FIXED_CASES] + [("rk4", s, None) for s in (1, 2, 3, 4)]


def check_stage(hip, oracle, case, y0, ks, y0_dev, ks_dev, out_offset, dts, what):
    n, dtype = y0.numel(), y0.dtype
    for dt in dts:
        cell, dt_cpu = dt_cell(dt)
        ref = torch.empty(n, dtype=dtype)
        run_stage(oracle, case, ref, y0, ks, dt_cpu, True)
        via_dev, via_host = Window(n, dtype, out_offset), Window(n, dtype, out_offset)
        run_stage(hip, case, via_dev.t, y0_dev, ks_dev, cell[1:], True)
        run_stage(hip, case, via_host.t, y0_dev, ks_dev, float(dt_cpu[0]), False)
        assert via_dev.intact() and via_host.intact(), (what, dt)
        same_as_host_arithmetic(via_dev.t, ref, (what, dt, "device dt against the oracle"))
        same_bits(via_dev.t, via_host.t, (what, dt, "device dt against the host-dt entry point"))
        assert math.isnan(float(cell[0])) and (float(cell[1]) == dt or dt != dt)


@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("n", STAGE_SIZES)
def test_stage_kernels_with_device_dt(hip_kernels, oracle_kernels, n, name):
    dtype, dts = DT[name], dt_values(oracle_kernels)
    for kind in ("randn", "edge"):
        y0, *ks = (draw_edge if kind == "edge" else draw)(n, 40 + n, dtype, 5)
        y0_dev, *ks_dev = dev([y0] + ks)
        for case in STAGE_CASES:
            check_stage(hip_kernels, oracle_kernels, case, y0, ks, y0_dev, ks_dev, 0, dts, (n, name, kind, case))


@pytest.mark.parametrize("name", TYPES)
def test_stage_kernels_with_device_dt_unaligned(hip_kernels, oracle_kernels, name):
    """`out`, `y0` and one `k` each in turn one element off a 16-byte boundary: the scalar instantiation."""
    dtype, n, dts = DT[name], 4099, dt_values(oracle_kernels)
    y0, *ks = draw_edge(n, 77, dtype, 5)
    for case in STAGE_CASES:
        n_k = len(case[2]) if case[0] == "fixed" else case[1]
        for shifted in ("out", "y0", "k"):
            y0_dev, = dev([y0], 1 if shifted == "y0" else 0)
            ks_dev = dev(ks[:n_k - 1]) + dev(ks[n_k - 1:n_k], 1 if shifted == "k" else 0) + dev(ks[n_k:])
            check_stage(hip_kernels, oracle_kernels, case, y0, ks, y0_dev, ks_dev, 1 if shifted == "out" else 0,
                        dts, (name, case, shifted))


# ---------------------------------------------------------------------------------------------------------------------
# d. host scalars -> device words
# ---------------------------------------------------------------------------------------------------------------------
FILL_VALUES = [0.1, 1e-46, 1e39, math.inf, -math.inf, math.nan, -0.0, -0.1, 1e-320, 1.0 + 2.0 ** -30, 2.0 ** -140,
               -1e39, 3.0, 2.0 ** -149, -2.0 ** -126, 1 / 3]


@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("n_vals", [1, 4, 16])
def test_fill_scalars(hip_kernels, oracle_kernels, n_vals, name):
    dtype = DT[name]
    for start in range(0, len(FILL_VALUES), n_vals):
        vals = (FILL_VALUES[start:] + FILL_VALUES[:start])[:n_vals]
        w = Window(n_vals, dtype)
        hip_kernels.fill_scalars(w.t, vals)
        ref = torch.full((n_vals,), 7.0, dtype=dtype)
        oracle_kernels.fill_scalars(ref, vals)
        same_bits(w.t, ref, (n_vals, name, vals))
        assert w.intact(), (n_vals, name, vals)
        assert int(w.raw[w.hi]) == w.sentinel               # the element after the last one


# ---------------------------------------------------------------------------------------------------------------------
# e. one captured step, kernels only — and the same solve through the public entry point
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_N = 1031
CHAIN_GRID = EDGE_GRID[:-1]                 # without 2^40
CHAIN_SCALE = 2.0 ** -100


def field(t, y):
    return y * t


def step_chain(kern, method, perturb, y0, grid):
    """What FixedGridODESolver._integrate_graph puts on the stream for `method`, from the kernels alone:
    grid_advance_stages, then per interval the method's stage kernels, grid_commit, grid_advance_stages."""
    stages = graph_times(method)
    fracs, modes = [f for f, _ in stages], [m for _, m in stages]
    n_t, device = grid.numel(), y0.device
    solution = torch.zeros(n_t, y0.numel(), dtype=y0.dtype, device=device)
    solution[0].copy_(y0)
    y_cur = y0.clone()
    counter = torch.full((), -1, dtype=torch.int64, device=device)
    times = torch.empty(len(stages), dtype=y0.dtype, device=device)
    ctrl = _DtCell(torch.zeros(2, dtype=torch.float64, device=device))
    dt_dev = ctrl.ctrl_dev[1:]
    ts = times.unbind(0)
    new = lambda: torch.empty_like(y_cur)

    def combine(out, k, c):           # euler's and midpoint's stages: tdeq_stage_combine_dev, dt = ctrl_dev[1]
        if hasattr(kern, "stage_combine_dev"):
            kern.stage_combine_dev(out, None, y_cur, [k], (c,), None, ctrl)
        else:
            kern.stage_combine(out, y_cur, [k], (c,), float(ctrl.ctrl_dev[1]))
        return out

    def step():
        k1 = field(ts[0], y_cur)
        if method == "euler":
            return combine(new(), k1, 1.0)
        if method == "midpoint":
            return combine(new(), field(ts[1], combine(new(), k1, 0.5)), 1.0)
        if method == "heun2":
            ya, y1 = new(), new()
            kern.fixed_stage_dev(1, ya, y_cur, [k1], (1.0,), dt_dev)
            kern.fixed_stage_dev(0, y1, y_cur, [k1, field(ts[1], ya)], (0.5, 0.5), dt_dev)
            return y1
        if method == "heun3":
            ya, yb, y1 = new(), new(), new()
            kern.fixed_stage_dev(1, ya, y_cur, [k1], (THIRD,), dt_dev)
            kern.fixed_stage_dev(0, yb, y_cur, [field(ts[1], ya)], (TWO_THIRDS,), dt_dev)
            kern.fixed_stage_dev(0, y1, y_cur, [k1, field(ts[2], yb)], (1 / 4, 3 / 4), dt_dev)
            return y1
        ya, yb, yc, y1 = new(), new(), new(), new()
        kern.rk4_stage_dev(1, ya, y_cur, k1, None, None, None, dt_dev)
        k2 = field(ts[1], ya)
        kern.rk4_stage_dev(2, yb, y_cur, k1, k2, None, None, dt_dev)
        k3 = field(ts[2], yb)
        kern.rk4_stage_dev(3, yc, y_cur, k1, k2, k3, None, dt_dev)
        kern.rk4_stage_dev(4, y1, y_cur, k1, k2, k3, field(ts[3], yc), dt_dev)
        return y1

    kern.grid_advance_stages(grid, counter, perturb, 1.0, fracs, modes, times, dt_dev)
    for _ in range(n_t - 1):
        kern.grid_commit(solution, y_cur, step(), counter)
        kern.grid_advance_stages(grid, counter, perturb, 1.0, fracs, modes, times, dt_dev)
    assert int(counter) == n_t - 1
    return solution


_chain_refs = {}


def chain_reference(oracle_kernels, method, name, perturb):
    """The oracle's solve, once per case.  The state stays finite on this grid — rows of 2^-100 * randn — with one
    exception: the 3/8 rule multiplies the state by 1.4e77 over the last two intervals (dt = 2^24 - 1 at t = 1, then
    dt = 2 at t = 2^24), more than float32 holds above 2^-100, so the float32 rk4 solve ends in a row of +-inf.  That row
    stays in the comparison: the device must overflow in the same elements to the same signs."""
    key = (method, name, perturb)
    if key not in _chain_refs:
        y0 = draw(CHAIN_N, 5, DT[name], 1)[0] * CHAIN_SCALE
        grid = torch.tensor(CHAIN_GRID, dtype=DT[name])
        sol = step_chain(oracle_kernels, method, perturb, y0, grid)
        finite = torch.isfinite(sol).all(dim=1)
        if (method, name) == ("rk4", "f32"):
            assert bool(finite[:-1].all()) and bool(torch.isinf(sol[-1]).all())
        else:
            assert bool(finite.all()), (key, finite.tolist())
        assert not bool(torch.isnan(sol).any()) and bool((sol[-1] != sol[0]).all())
        _chain_refs[key] = (y0, grid, sol)
    return _chain_refs[key]


@pytest.mark.parametrize("perturb", [False, True], ids=["plain", "perturb"])
@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("method", METHODS)
def test_one_captured_step_from_the_kernels_alone(hip_kernels, oracle_kernels, method, name, perturb):
    y0, grid, ref = chain_reference(oracle_kernels, method, name, perturb)
    got = step_chain(hip_kernels, method, perturb, y0.cuda(), grid.cuda())
    for row in range(grid.numel()):
        same_bits(got[row], ref[row], (method, name, perturb, "row", row))


@pytest.mark.parametrize("perturb", [False, True], ids=["plain", "perturb"])
@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("method", METHODS)
def test_captured_solve_on_the_edge_grid_through_odeint(oracle_kernels, method, name, perturb):
    """A non-uniform grid that crosses zero, solved by replaying the captured step: the eager solve's bits and the
    oracle chain's."""
    y0, grid, ref = chain_reference(oracle_kernels, method, name, perturb)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")            # in particular: no "running the eager path" fallback warning
        y_graph = tda.odeint(field, y0.cuda(), grid.cuda(), method=method, options=dict(hip_graph=True, perturb=perturb))
        y_eager = tda.odeint(field, y0.cuda(), grid.cuda(), method=method, options=dict(hip_graph=False, perturb=perturb))
    for row in range(grid.numel()):
        same_bits(y_graph[row], y_eager[row], (method, name, perturb, "graph against eager, row", row))
        same_bits(y_graph[row], ref[row], (method, name, perturb, "graph against the oracle chain, row", row))
