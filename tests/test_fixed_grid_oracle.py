"""The CPU oracle of the fixed-grid captured step (oracle/kernels.py: grid_advance_stages, grid_advance, grid_commit,
fixed_stage_dev, rk4_stage_dev), without a GPU:

  a. pinned to the reference: walking `grid_advance_stages` over a grid with a method's `_graph_times` reproduces, bit
     for bit, the times the reference's euler / midpoint / heun2 / heun3 / rk4 handed to `func` on that grid
     (tests/golden/fixed_grid_times.npz, written by tests/golden/make_golden_fixed_grid.py) — both state types, both grid
     types, `perturb` off and on, both directions, on grids chosen for their edges (tests/_fixed_grid_cases.py);
  b. its perturbation against np.nextafter at the values where a hand-written nextafter has branches of its own;
  c. the rule for the end of the grid, `grid_commit` and the `_dev` stage twins;
  d. the argument checks of the six C entry points, which return before any launch (as tests/test_abi.py does for others).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from _fixed_grid_cases import (DT, GRIDS, METHODS, NP, ONE_ULP_INTERVAL, SYNTHETIC_STAGES, bits, draw, golden_cases,
                               graph_times, same_bits, walk_grid)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_grid_times.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def solver_grid(gname, gtype, rev):
    """The grid as the solver holds it: a decreasing `t` is solved as the increasing -t with sign = -1
    (FixedGridODESolver._integrate_graph gets it that way)."""
    t = torch.tensor(GRIDS[gname], dtype=torch.float64).to(DT[gtype])
    return ((-t.flip(0)).contiguous(), -1.0) if rev else (t, 1.0)


def test_fixture_holds_the_grids_of_the_case_file(golden):
    for gname, g in GRIDS.items():
        assert golden["grid_" + gname].dtype == np.float64 and golden["grid_" + gname].tolist() == list(g)
    assert len(golden) == len(GRIDS) + len(METHODS) * len(golden_cases())
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("case", golden_cases(), ids=[c[0] for c in golden_cases()])
def test_oracle_walk_reproduces_the_reference_stage_times(golden, oracle_kernels, case):
    key, gname, state, gtype, perturb, rev = case
    grid, sign = solver_grid(gname, gtype, rev)
    for method in METHODS:
        stages = graph_times(method)
        ref = golden["{}_{}".format(method, key)]
        assert ref.dtype == NP[state] and ref.shape == ((grid.numel() - 1) * len(stages),), (method, ref.shape)
        steps = walk_grid(oracle_kernels, grid, sign, perturb, stages, DT[state])
        assert [c for c, _, _ in steps] == list(range(grid.numel()))
        assert steps[-1][1] is None and steps[-1][2] is None           # the last call found no interval to prepare
        got = torch.cat([t for _, t, _ in steps[:-1]])
        same_bits(got, torch.from_numpy(ref), (method, key))
        g64 = grid.double()
        for c, _, dt in steps[:-1]:                                    # dt in the grid's type, times the direction
            expect = (grid[c + 1] - grid[c]).double() * sign
            same_bits(dt, expect.reshape(1), (method, key, c))
            assert float(dt) * sign > 0 and g64[c + 1] > g64[c]
        if method == "rk4":
            counter = torch.full((), -1, dtype=torch.int64)
            times, dt = torch.empty(4, dtype=DT[state]), torch.empty(1, dtype=torch.float64)
            for c, t_ref, dt_ref in steps[:-1]:
                oracle_kernels.grid_advance(grid, counter, perturb, sign, times, dt)
                assert int(counter) == c
                same_bits(times, t_ref, ("grid_advance", key, c))
                same_bits(dt, dt_ref, ("grid_advance", key, c))


def test_the_edge_grid_reaches_the_branches_it_is_there_for(oracle_kernels):
    """What the grids were chosen for, stated on the oracle's own output (so that a later edit of the lists cannot lose a
    branch silently): under `perturb` the float walk perturbs a zero to both sides, stands still at 2^24 (x + 1 == x), and
    leaves a subnormal time; the double grid's entries change when cast to a float state."""
    g32 = torch.tensor(GRIDS["edge"], dtype=torch.float32)
    steps = walk_grid(oracle_kernels, g32, 1.0, True, graph_times("rk4"), torch.float32)
    t0s = [float(t[0]) for _, t, _ in steps[:-1]]
    t1s = [float(t[3]) for _, t, _ in steps[:-1]]
    tiny = float(np.float32(2.0 ** -149))
    assert tiny in t0s and -tiny in t1s                                 # NEXT and PREV of 0.0
    assert 2.0 ** 24 in t0s and 2.0 ** 24 - 1 in t1s                    # NEXT stands still, PREV does not
    assert 2.0 ** -140 + tiny in t0s and -2.5 + 2.0 ** -22 in t0s       # a subnormal and a negative time, one ulp up
    assert float(steps[ONE_ULP_INTERVAL][2]) == 2.0 ** -23
    steps64 = walk_grid(oracle_kernels, g32.double(), 1.0, True, graph_times("rk4"), torch.float64)
    assert float(steps64[9][1][0]) == 2.0 ** 24 + 2.0 ** -28            # ... where x + 1 != x in double
    cast = torch.tensor(GRIDS["cast"], dtype=torch.float64)
    plain = walk_grid(oracle_kernels, cast, 1.0, False, graph_times("euler"), torch.float32)
    assert all(float(t[0]) != float(cast[c]) for c, t, _ in plain[:-1])
    assert float(plain[0][1][0]) == 0.0                                 # the float64 subnormal is a float zero


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_oracle_perturbation_is_nextafter(oracle_kernels, name):
    T = NP[name]
    fi = np.finfo(T)
    tiny = fi.smallest_subnormal
    values = [0.0, -0.0, tiny, -tiny, math.inf, -math.inf, math.nan, 2.0 ** 24, -2.0 ** 24, fi.max, -fi.max,
              fi.smallest_normal, -fi.smallest_normal, 1.0, -1.0]
    itype = {"f32": np.int32, "f64": np.int64}[name]
    for v in values:
        x = T(v)
        with np.errstate(all="ignore"):
            up_ref, down_ref = np.nextafter(x, x + T(1)), np.nextafter(x, x - T(1))
        up, down = oracle_kernels.perturb_next(x), oracle_kernels.perturb_prev(x)
        assert type(up) is T and type(down) is T
        assert up.view(itype) == up_ref.view(itype) and down.view(itype) == down_ref.view(itype), v
    # the values themselves, from the definition of nextafter rather than from numpy: one step of the integer pattern away
    # from zero or towards it; a zero of either sign steps to the smallest subnormal; a value with x + 1 == x stays
    step = lambda x, k: (x.view(itype) + itype(k)).view(T)
    one = T(1)
    assert oracle_kernels.perturb_next(one) == step(one, 1) and oracle_kernels.perturb_prev(one) == step(one, -1)
    assert oracle_kernels.perturb_next(-one) == step(-one, -1) and oracle_kernels.perturb_prev(-one) == step(-one, 1)
    for z in (T(0.0), T(-0.0)):
        assert oracle_kernels.perturb_next(z) == tiny and oracle_kernels.perturb_prev(z) == -tiny
    assert oracle_kernels.perturb_next(-tiny).view(itype) == T(-0.0).view(itype)
    assert oracle_kernels.perturb_prev(tiny).view(itype) == T(0.0).view(itype)
    big = T(2.0 ** 24) if name == "f32" else T(2.0 ** 53)
    assert oracle_kernels.perturb_next(big) == big and oracle_kernels.perturb_prev(big) == step(big, -1)
    assert oracle_kernels.perturb_next(T(math.inf)) == math.inf and oracle_kernels.perturb_prev(T(math.inf)) == math.inf
    assert oracle_kernels.perturb_prev(T(-math.inf)) == -math.inf and oracle_kernels.perturb_next(T(-math.inf)) == -math.inf
    assert np.isnan(oracle_kernels.perturb_next(T(math.nan))) and np.isnan(oracle_kernels.perturb_prev(T(math.nan)))


def test_oracle_writes_nothing_but_the_counter_past_the_last_interval(oracle_kernels):
    grid = torch.tensor([0.5, 0.75], dtype=torch.float64)
    for stages in SYNTHETIC_STAGES:
        steps = walk_grid(oracle_kernels, grid, 1.0, True, stages, torch.float32, calls=4)
        assert [c for c, _, _ in steps] == [0, 1, 2, 3]
        assert steps[0][1] is not None and all(t is None and dt is None for _, t, dt in steps[1:])


def test_oracle_synthetic_stage_lists(oracle_kernels):
    """Mode bit 1 wins over the fraction, NEXT then PREV on one time gives the time back (away from a power of two)."""
    grid = torch.tensor([0.5, 0.75], dtype=torch.float64)
    (_, t, dt), = walk_grid(oracle_kernels, grid, -1.0, True, SYNTHETIC_STAGES[3], torch.float64, calls=1)
    t0, h = np.float64(0.5), np.float64(0.25)
    assert float(dt) == -0.25
    assert t.tolist() == [-(t0 + h * np.float64(0.1)), -np.nextafter(np.float64(0.75), 0.0),
                          -np.nextafter(t0 + h * np.float64(0.9), 1.0), -0.5]


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_oracle_commit_and_dev_stage_twins(oracle_kernels, name):
    dtype, n = DT[name], 37
    y_new, y_cur, k1, k2 = draw(n, 3, dtype, 4)
    y_new[0], y_new[1] = -0.0, math.nan
    sol = torch.full((4, n + 3), 7.0, dtype=dtype)
    before = sol.clone()
    oracle_kernels.grid_commit(sol[:, :n], y_cur, y_new, torch.tensor(1, dtype=torch.int64))
    same_bits(sol[2, :n], y_new)
    same_bits(y_cur, y_new)
    sol[2, :n] = 7.0
    same_bits(sol, before)
    dt_dev = torch.tensor([math.nan, 0.1], dtype=torch.float64)[1:]
    a, b = torch.empty(n, dtype=dtype), torch.empty(n, dtype=dtype)
    oracle_kernels.fixed_stage_dev(0, a, y_new, [k1, k2], (0.25, 0.75), dt_dev)
    oracle_kernels.fixed_stage(0, b, y_new, [k1, k2], (0.25, 0.75), 0.1)
    same_bits(a, b)
    oracle_kernels.rk4_stage_dev(2, a, y_new, k1, k2, None, None, dt_dev)
    oracle_kernels.rk4_stage(2, b, y_new, k1, k2, None, None, 0.1)
    same_bits(a, b)
    assert bits(a).ne(0).any()


# ---------------------------------------------------------------------------------------------------------------------
# d. argument checks of the C entry points: every one of these returns before a launch, so no GPU is needed
# ---------------------------------------------------------------------------------------------------------------------
EINVAL = -1
BAD_DTYPES = (4, 5, 2, 3, 7, -1)        # bfloat16, float16, the complex codes, unknown


@pytest.fixture(scope="module")
def abi():
    from torchdiffeq_amd import _native
    lib = _native.load_library()
    buf = (ctypes.c_double * 8)()
    modes = (ctypes.c_int * 4)(0, 0, 0, 0)
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 4)(p, p, p, p)
    return lib, buf, modes, p, ptrs


def test_grid_advance_argument_errors(abi):
    lib, buf, modes, p, _ = abi
    ok = dict(grid=p, gdt=1, n_grid=4, counter=p, perturb=1, sign=1.0, times=p, dt=p, sdt=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tdeq_grid_advance(a["grid"], a["gdt"], a["n_grid"], a["counter"], a["perturb"], a["sign"], a["times"],
                                     a["dt"], a["sdt"], None)

    def call_stages(frac=buf, mode=modes, n_times=2, **kw):
        a = dict(ok, **kw)
        return lib.tdeq_grid_advance_stages(a["grid"], a["gdt"], a["n_grid"], a["counter"], a["perturb"], a["sign"], frac,
                                            mode, n_times, a["times"], a["dt"], a["sdt"], None)
    for fn in (call, call_stages):
        for name in ("grid", "counter", "times", "dt"):
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
        for n_grid in (1, 0, -3):
            assert fn(n_grid=n_grid) == EINVAL
        for code in BAD_DTYPES:
            assert fn(gdt=code) == EINVAL and fn(sdt=code) == EINVAL, code
    assert call_stages(frac=None) == EINVAL and call_stages(mode=None) == EINVAL
    for n_times in (0, 5, -1):
        assert call_stages(n_times=n_times) == EINVAL


def test_grid_commit_argument_errors(abi):
    lib, _, _, p, _ = abi
    commit = lib.tdeq_grid_commit
    assert commit(None, 4, p, p, p, 4, 1, None) == EINVAL
    assert commit(p, 4, None, p, p, 4, 1, None) == EINVAL
    assert commit(p, 4, p, None, p, 4, 1, None) == EINVAL
    assert commit(p, 4, p, p, None, 4, 1, None) == EINVAL
    assert commit(p, 3, p, p, p, 4, 1, None) == EINVAL                      # row_stride < n
    assert commit(p, 4, p, p, p, -1, 1, None) == EINVAL
    for code in BAD_DTYPES:
        assert commit(p, 4, p, p, p, 4, code, None) == EINVAL
        assert commit(p, 4, p, p, p, 0, code, None) == EINVAL
    for code in (0, 1):
        assert commit(p, 0, p, p, p, 0, code, None) == 0                    # empty state: no-op
        assert commit(p, 5, p, p, p, 0, code, None) == 0


def test_fixed_stage_dev_argument_errors(abi):
    lib, buf, _, p, ptrs = abi
    stage = lib.tdeq_fixed_stage_dev
    null_k = (ctypes.c_void_p * 4)(p, None, p, p)
    assert stage(0, None, p, ptrs, buf, 1, p, 4, 1, None) == EINVAL
    assert stage(0, p, None, ptrs, buf, 1, p, 4, 1, None) == EINVAL
    assert stage(0, p, p, None, buf, 1, p, 4, 1, None) == EINVAL
    assert stage(0, p, p, ptrs, None, 1, p, 4, 1, None) == EINVAL
    assert stage(0, p, p, ptrs, buf, 1, None, 4, 1, None) == EINVAL          # null dt_dev
    assert stage(0, p, p, null_k, buf, 2, p, 4, 1, None) == EINVAL           # a null term
    assert stage(0, p, p, ptrs, buf, 1, p, -1, 1, None) == EINVAL
    assert stage(1, p, p, ptrs, buf, 2, p, 4, 1, None) == EINVAL             # mode 1 takes one term
    assert stage(2, p, p, ptrs, buf, 1, p, 4, 1, None) == EINVAL             # mode 2 has no step size
    for n_terms in (0, 5):
        assert stage(0, p, p, ptrs, buf, n_terms, p, 4, 1, None) == EINVAL
        assert stage(0, p, p, ptrs, buf, n_terms, p, 0, 1, None) == EINVAL
    for code in BAD_DTYPES:
        assert stage(0, p, p, ptrs, buf, 1, p, 4, code, None) == EINVAL
        assert stage(0, p, p, ptrs, buf, 1, p, 0, code, None) == EINVAL
    for code in (0, 1):
        assert stage(1, p, p, ptrs, buf, 1, p, 0, code, None) == 0           # empty state: no-op
        for n_terms in (1, 2, 3, 4):
            assert stage(0, p, p, ptrs, buf, n_terms, p, 0, code, None) == 0


def test_rk4_stage_dev_argument_errors(abi):
    lib, _, _, p, _ = abi
    stage = lib.tdeq_rk4_38_stage_dev
    assert stage(1, None, p, p, p, p, p, p, 4, 1, None) == EINVAL
    assert stage(1, p, None, p, p, p, p, p, 4, 1, None) == EINVAL
    assert stage(1, p, p, p, p, p, p, None, 4, 1, None) == EINVAL            # null dt_dev
    assert stage(1, p, p, p, p, p, p, p, -1, 1, None) == EINVAL
    for code in BAD_DTYPES:
        assert stage(1, p, p, p, p, p, p, p, 4, code, None) == EINVAL
        assert stage(1, p, p, p, p, p, p, p, 0, code, None) == EINVAL
    for code in (0, 1):
        for bad in (0, 5):
            assert stage(bad, p, p, p, p, p, p, p, 0, code, None) == EINVAL
        for good in (1, 2, 3, 4):
            assert stage(good, p, p, p, p, p, p, p, 0, code, None) == 0      # empty state: no-op


def test_fill_scalars_argument_errors(abi):
    lib, buf, _, p, _ = abi
    fill = lib.tdeq_fill_scalars
    assert fill(None, buf, 1, 1, None) == EINVAL
    assert fill(p, None, 1, 1, None) == EINVAL
    for n_vals in (0, 17, -1):
        assert fill(p, buf, n_vals, 1, None) == EINVAL
        assert fill(p, buf, n_vals, 0, None) == EINVAL
    for code in (2, 3, 7, -1):
        assert fill(p, buf, 1, code, None) == EINVAL
