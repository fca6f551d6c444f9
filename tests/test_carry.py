"""Carried partial sums (tableaus.carry_plan, tdeq_stage_combine_multi): the planned launches must reproduce the
row-by-row `_runge_kutta_step` (rk_common.py:69-89) BIT FOR BIT — every stage input, the partial embedded error, and
therefore every decision of a solve — while moving fewer words."""
import os

import numpy as np
import pytest
import torch

from torchdiffeq_amd import tableaus as tb


def _rand(n, dtype, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64, device="cpu").to(dtype)
    if special and n >= 8:          # signed zeros and an exact cancellation partner: the cases a `0 + x` start would change
        x[0], x[1], x[2] = 0.0, -0.0, -0.0
    return x


@pytest.mark.parametrize("name,words,launches,before", [("dopri5", 35, 7, 37), ("dopri8", 75, 13, 98), ("tsit5", 41, 8, 46)])
def test_plan_word_counts(name, words, launches, before):
    plan = tb.carry_plan(name)
    tab = tb.ADAPTIVE_TABLEAUS[name]
    assert (plan.words, plan.launches) == (words, launches)
    assert tb.row_by_row_words(tab) == before
    rows = tab.beta_rows()
    S = len(rows) if tab.fsal_solution else len(rows) + 1          # launch rows (tsit5: + the c_sol combine)
    # structure: every row's stage input is produced exactly once; the error partial exactly once
    produced = [0]
    for op in plan.ops:
        if op is None:
            continue
        assert len(op.targets) <= tb.MAX_MULTI_OUT and op.targets[0] == op.row
        for t, (coefs, mask, done) in zip(op.targets, op.spec):
            assert mask and mask < (1 << len(op.idx)) and len(coefs) == len(op.idx)
            if done:
                produced.append(t)
    assert sorted(produced) == list(range(S))
    assert sum(1 for op in plan.ops if op is not None and S in op.targets) == 1
    assert tb.carry_plan("bosh3") is None and tb.carry_plan("fehlberg2") is None


def _run_rows(kern, tab, y0, ks, dt, planned):
    """Stage inputs y_1..y_{S-1} [+ the solution y1 of a non-FSAL pair] (given ALL stages up front — the combines are
    linear in them, so parity of the launch forms does not need a func) + the partial error and what is left to the
    norm kernel."""
    rows = tab.beta_rows()
    if not tab.fsal_solution:
        rows = rows + [tb.SparseRow.from_dense(tab.c_sol)]
    S = len(rows)
    err = tb.SparseRow.from_dense(tab.c_error)
    ys = {}
    if not planned:
        for i in range(1, S):
            r = rows[i]
            ys[i] = torch.empty_like(y0)
            if i == S - 1:
                ep = torch.empty_like(y0)
                kern.stage_combine_err(ys[i], ep, y0, [ks[j] for j in r.idx], r.coef, err.coef[:len(r.idx)], dt)
            else:
                kern.stage_combine(ys[i], y0, [ks[j] for j in r.idx], r.coef, dt)
        return ys, ep, err.idx[len(rows[-1].idx):]
    plan = tb.carry_plan(tab.name)
    held = {}
    for i in range(1, S):
        op = plan.ops[i]
        if op is None:
            ys[i] = held.pop(i)
            continue
        outs = [torch.empty_like(y0) for _ in op.targets]
        kern.stage_combine_multi(outs, op.spec, y0, held.pop(i) if op.continues else None, [ks[j] for j in op.idx], dt)
        ys[i] = outs[0]
        for t, b in zip(op.targets[1:], outs[1:]):
            held[t] = b
    ep = held.pop(S)
    assert not held
    return ys, ep, plan.err_idx


def _bits(x):
    return x.cpu().contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("name", ["dopri5", "dopri8", "tsit5"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 7, 1024, 4099])
@pytest.mark.parametrize("dt", [0.37, -0.011])
def test_planned_rows_equal_row_by_row_oracle(oracle_kernels, name, dtype, n, dt):
    tab = tb.ADAPTIVE_TABLEAUS[name]
    y0 = _rand(n, dtype, 1)
    ks = [_rand(n, dtype, 10 + j) for j in range(len(tab.beta) + 1)]
    a, ea, ra = _run_rows(oracle_kernels, tab, y0, ks, dt, planned=False)
    b, eb, rb = _run_rows(oracle_kernels, tab, y0, ks, dt, planned=True)
    for i in a:
        assert torch.equal(_bits(a[i]), _bits(b[i])), (name, i)
    # the error: (partial + remaining stages) must be the same left-to-right sum either way
    err = tb.SparseRow.from_dense(tab.c_error)
    T = np.float32 if dtype == torch.float32 else np.float64

    def finish(ep, rem):
        e = ep.numpy().copy()
        for j in rem:
            c = T(T(dict(zip(err.idx, err.coef))[j]) * T(dt))
            e = (e + ks[j].numpy() * c).astype(T)
        return e
    assert np.array_equal(finish(ea, ra).view(np.int32 if T is np.float32 else np.int64),
                          finish(eb, rb).view(np.int32 if T is np.float32 else np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dopri5", "dopri8", "tsit5"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 5, 1023, 65536 + 3, 1 << 20])
@pytest.mark.parametrize("dt", [0.37, -0.011])
def test_planned_rows_equal_row_by_row_hip_and_oracle(hip_kernels, oracle_kernels, name, dtype, n, dt):
    tab = tb.ADAPTIVE_TABLEAUS[name]
    y0 = _rand(n, dtype, 1)
    ks = [_rand(n, dtype, 10 + j) for j in range(len(tab.beta) + 1)]
    ref, eref, _ = _run_rows(oracle_kernels, tab, y0, ks, dt, planned=False)
    dev = torch.device("cuda:0")
    y0d, ksd = y0.to(dev), [k.to(dev) for k in ks]
    for planned in (False, True):
        got, ep, _ = _run_rows(hip_kernels, tab, y0d, ksd, dt, planned=planned)
        for i in ref:
            assert torch.equal(_bits(ref[i]), _bits(got[i])), (name, i, planned)
    got, ep, rem = _run_rows(hip_kernels, tab, y0d, ksd, dt, planned=True)
    o, eo, remo = _run_rows(oracle_kernels, tab, y0, ks, dt, planned=True)
    assert rem == remo and torch.equal(_bits(eo), _bits(ep))


@pytest.mark.gpu
def test_multi_unaligned_views_take_the_scalar_path(hip_kernels, oracle_kernels):
    tab = tb.DOPRI8
    n = 3001
    dev = torch.device("cuda:0")
    y0 = _rand(n + 1, torch.float32, 3)
    ks = [_rand(n + 1, torch.float32, 30 + j) for j in range(14)]
    ref, eref, _ = _run_rows(oracle_kernels, tab, y0[1:].clone(), [k[1:].clone() for k in ks], 0.1, planned=True)
    got, eg, _ = _run_rows(hip_kernels, tab, y0.to(dev)[1:], [k.to(dev)[1:] for k in ks], 0.1, planned=True)
    for i in ref:
        assert torch.equal(_bits(ref[i]), _bits(got[i]))
    assert torch.equal(_bits(eref), _bits(eg))


def test_multi_rejects_bad_arguments():
    import ctypes
    from torchdiffeq_amd import _native
    lib = _native.load_library()
    spec = (_native.MultiOut * 1)()
    spec[0].out, spec[0].mask = 16, 0            # empty mask
    k = (ctypes.c_void_p * 1)(16)
    assert lib.tdeq_stage_combine_multi(spec, 1, 16, None, k, 1, 0.1, 8, 0, None) == -1
    spec[0].mask = 0b10                          # bit outside n_terms
    assert lib.tdeq_stage_combine_multi(spec, 1, 16, None, k, 1, 0.1, 8, 0, None) == -1
    spec[0].mask = 1
    assert lib.tdeq_stage_combine_multi(spec, 5, 16, None, k, 1, 0.1, 8, 0, None) == -1     # too many outputs
    assert lib.tdeq_stage_combine_multi(spec, 1, 16, None, k, 1, 0.1, 0, 0, None) == 0      # n = 0: nothing to do


def _solve(method, dtype, device, carry, monkeypatch, rtol, atol, reverse=False):
    import torchdiffeq_amd as tda
    monkeypatch.setenv("TDEQ_CARRY", "1" if carry else "0")      # "1": every tableau with a plan (dopri5 too)
    g = torch.Generator(device="cpu").manual_seed(5)
    D = 24
    G = torch.randn(D, D, generator=g, dtype=torch.float64, device="cpu") / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64, device="cpu")).to(dtype).to(device)
    y0 = torch.randn(96, D, generator=g, dtype=torch.float64, device="cpu").to(dtype).to(device)
    t = torch.tensor([0.0, 0.3, 0.7, 1.5] if not reverse else [1.5, 0.7, 0.0], dtype=torch.float64, device=device)
    steps = []

    class F(torch.nn.Module):
        def forward(self, t_, y):
            return torch.tanh(y @ A.T) * 0.5 + y @ A.T

        def callback_accept_step(self, t0, y, dt):
            steps.append(("a", float(t0), float(dt)))

        def callback_reject_step(self, t0, y, dt):
            steps.append(("r", float(t0), float(dt)))
    with torch.no_grad():
        y = tda.odeint(F(), y0, t, method=method, rtol=rtol, atol=atol)
    return y, steps


@pytest.mark.parametrize("method,dtype,rtol,atol", [("dopri5", torch.float32, 1e-6, 1e-8), ("dopri5", torch.float64, 1e-9, 1e-11),
                                                    ("dopri8", torch.float64, 1e-10, 1e-12), ("dopri8", torch.float32, 1e-6, 1e-8),
                                                    ("tsit5", torch.float32, 1e-6, 1e-8), ("tsit5", torch.float64, 1e-9, 1e-11)])
@pytest.mark.parametrize("reverse", [False, True])
def test_solve_with_plan_is_bit_identical(dev, monkeypatch, method, dtype, rtol, atol, reverse):
    a, sa = _solve(method, dtype, dev, False, monkeypatch, rtol, atol, reverse)
    b, sb = _solve(method, dtype, dev, True, monkeypatch, rtol, atol, reverse)
    assert sa == sb and len(sa) > 3
    assert torch.equal(_bits(a), _bits(b))


def test_plan_is_used_by_the_no_grad_solve(cpu_backend, monkeypatch):
    calls = []
    orig = cpu_backend.stage_combine_multi
    monkeypatch.setattr(cpu_backend, "stage_combine_multi", lambda *a, **k: (calls.append(1), orig(*a, **k))[1], raising=False)
    _solve("dopri8", torch.float64, "cpu", True, monkeypatch, 1e-8, 1e-10)
    assert calls
    n = len(calls)
    _solve("dopri8", torch.float64, "cpu", False, monkeypatch, 1e-8, 1e-10)
    assert len(calls) == n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dopri5", "dopri8", "tsit5"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [7, 1023, (1 << 17) + 5])
def test_multi_with_the_step_size_on_the_device_equals_host_dt(hip_kernels, name, dtype, n):
    """tdeq_stage_combine_multi_dev (captured steps: dt = ctrl_dev[1], read by the kernel) against the host-dt entry
    point on every planned launch of the tableau: bit-identical outputs."""
    tab = tb.ADAPTIVE_TABLEAUS[name]
    plan = tb.carry_plan(name)
    dev = torch.device("cuda:0")
    T_ = np.float32 if dtype == torch.float32 else np.float64
    dt = -0.0371
    y0 = _rand(n, dtype, 1).to(dev)
    ks = [_rand(n, dtype, 10 + j).to(dev) for j in range(len(tab.beta) + 1)]
    nplan = hip_kernels.make_plan([(0, n, 1e-3, 1e-6)], n, 1024, dev)
    nplan.ctrl_dev.copy_(torch.tensor([1.0, float(T_(dt)), 0.0, abs(dt)], dtype=torch.float64))
    acc = _rand(n, dtype, 99).to(dev)
    checked = 0
    for op in plan.ops:
        if op is None:
            continue
        a = [torch.empty_like(y0) for _ in op.targets]
        b = [torch.empty_like(y0) for _ in op.targets]
        hip_kernels.stage_combine_multi(a, op.spec, y0, acc if op.continues else None, [ks[j] for j in op.idx], dt)
        hip_kernels.stage_combine_multi_dev(b, op.spec, y0, acc if op.continues else None, [ks[j] for j in op.idx], nplan)
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y)), (name, op.row)
        checked += 1
    assert checked >= 5


# ---- one launch plan for every tableau (tableaus.launch_plan / tableau_row_plan) ---------------------------------------
_FUSED = {tb.FUSE_ROWWISE: {"dopri5": True, "bosh3": True, "dopri8": False, "tsit5": False, "fehlberg2": False,
                            "adaptive_heun": False},
          tb.FUSE_ODEINT: {"dopri5": True, "bosh3": True, "dopri8": True, "tsit5": True, "fehlberg2": False,
                           "adaptive_heun": True}}


def _hand_written_launches(tab, left):
    """The row-by-row launches as the loops of rowwise.py / _graph.py built them before there was a plan for them,
    straight from the tableau: (launches after row 0 as (idx, spec, continues, targets), err_idx, err_coef, fused)."""
    rows = tab.beta_rows()
    if not tab.fsal_solution:
        rows = rows + [tb.SparseRow.from_dense(tab.c_sol)]
    err = tb.SparseRow.from_dense(tab.c_error)
    R, n_lead = len(rows), len(rows[-1].idx)
    fused = err.idx[:n_lead] == rows[-1].idx and left[0] <= len(err.idx) - n_lead <= left[1]
    launches = []
    for i in range(1, R):
        row = rows[i]
        spec, targets = [(tuple(row.coef), (1 << len(row.idx)) - 1, True)], [i]
        if fused and i == R - 1:
            spec.append((tuple(err.coef[:n_lead]), (1 << n_lead) - 1, False))
            targets.append(R)
        launches.append((tuple(row.idx), tuple(spec), False, tuple(targets)))
    n_lead = n_lead if fused else 0
    return launches, tuple(err.idx[n_lead:]), tuple(err.coef[n_lead:]), fused


@pytest.mark.parametrize("left", [tb.FUSE_ROWWISE, tb.FUSE_ODEINT], ids=["rowwise", "odeint"])
@pytest.mark.parametrize("name", ["dopri5", "bosh3", "tsit5", "fehlberg2", "adaptive_heun", "dopri8"])
def test_row_by_row_plan_is_the_hand_written_loop(name, left):
    tab = tb.ADAPTIVE_TABLEAUS[name]
    launches, err_idx, err_coef, fused = _hand_written_launches(tab, left)
    assert fused == _FUSED[left][name]
    plan = tb.tableau_row_plan(name, left)
    assert plan.ops[0] is None and len(plan.ops) == len(launches) + 1
    got = [(op.idx, tuple((tuple(c), m, a) for c, m, a in op.spec), op.continues, op.targets) for op in plan.ops[1:]]
    assert got == launches and [op.row for op in plan.ops[1:]] == list(range(1, len(plan.ops)))
    assert (plan.err_idx, tuple(plan.err_coef)) == (err_idx, err_coef)
    assert plan.launches == len(plan.ops) + 1
    if fused:
        assert plan.words == tb.row_by_row_words(tab)
    # what odeint_rowwise launches: the carry plan where there is one, else this plan under the rowwise rule
    if tb.carry_plan(name) is not None:
        assert tb.launch_plan(name) is tb.carry_plan(name)
    elif left == tb.FUSE_ROWWISE:
        assert tb.launch_plan(name) is plan


def test_solver_row_plan_is_built_from_its_own_rows(cpu_backend, monkeypatch):
    """The plan a captured step interprets where there is no carry plan comes from the solver's own rows and `_fuse`
    (the solver classes take any Tableau), and equals the by-name plan for the shipped ones."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd.solvers.adaptive import RKAdaptiveStepsizeODESolver
    seen = []
    orig = RKAdaptiveStepsizeODESolver.integrate
    monkeypatch.setattr(RKAdaptiveStepsizeODESolver, "integrate", lambda self, t: (seen.append(self), orig(self, t))[1])
    for name in ["dopri5", "bosh3", "tsit5", "fehlberg2", "adaptive_heun", "dopri8"]:
        with torch.no_grad():
            tda.odeint(lambda t_, y: -y, torch.ones(8, dtype=torch.float64), torch.tensor([0.0, 1.0], dtype=torch.float64),
                       method=name)
        s = seen.pop()
        assert not seen and s.tableau.name == name
        if name == "fehlberg2":
            assert s._fuse is None and s._row_plan is None
            continue
        plan, want = s._row_plan, tb.tableau_row_plan(name, tb.FUSE_ODEINT)
        assert (plan.ops, plan.err_idx, tuple(plan.err_coef)) == (want.ops, want.err_idx, tuple(want.err_coef))
        assert plan.ops[-1].spec[1][0] == s._fuse[0] and (plan.err_idx, plan.err_coef) == s._fuse[1:]


# ---- odeint_rowwise: the launches of one trial step on the HIP kernels ------------------------------------------------
class _LaunchLog:
    """Stand-in for the kernels object: logs every launch (no arithmetic), so it runs without the native library."""

    def __init__(self):
        self.log = []

    def row_partials(self, L, dtype):
        return 1

    def row_combine(self, outs, rows, y0, acc_in, ks, dts, active):
        self.log.append(["combine", len(outs), [[list(c), m, a] for c, m, a in rows], acc_in is not None, len(ks)])

    def row_reduce(self, mode, part, y0, y1, partial, ks, coefs, dts, active, rtol, atol):
        self.log.append(["reduce", mode, partial is not None, len(ks), list(coefs)])

    def row_control(self, mode, *a):
        self.log.append(["control", mode])

    def row_dense_commit(self, sol, y0, y1, f0, f1, ks, coefs, dts, st):
        self.log.append(["commit", len(ks), list(coefs)])


@pytest.mark.parametrize("method,n_launches", [("dopri5", 9), ("bosh3", 6), ("tsit5", 10), ("fehlberg2", 6),
                                               ("adaptive_heun", 5), ("dopri8", 15)])
def test_rowwise_trial_step_launches(monkeypatch, method, n_launches):
    """`HipRowKernels.trial_step` issues, launch for launch and argument for argument, what it issued when the fixture
    was recorded (golden/rowwise_launch_log.json: the log of this stand-in before the two hand-written schedules became
    one plan interpreter)."""
    import json
    from torchdiffeq_amd import _native, rowwise
    fake = _LaunchLog()
    monkeypatch.setattr(_native, "get_kernels", lambda dev, dt: fake)
    y0 = torch.ones(3, 4, dtype=torch.float64)
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    with torch.no_grad():
        p = rowwise._Problem(lambda t_, y: -y, y0, t, 1e-6, 1e-8, method, None, None)
        k = rowwise.HipRowKernels(p)
        k.dts = torch.zeros(3, dtype=torch.float64)
        k.times = torch.zeros(p.method.n_stages, 3, dtype=torch.float64)
        y = p.y0.clone()
        k.trial_step(y, -y, torch.empty(2, 3, 4, dtype=torch.float64))
    with open(os.path.join(os.path.dirname(__file__), "golden", "rowwise_launch_log.json")) as f:
        want = json.load(f)[method]
    assert len(fake.log) == n_launches == len(want)
    for got, exp in zip(fake.log, want):
        assert got == exp


def test_recorded_rowwise_backend_is_freed_by_reference_count(monkeypatch):
    """A recorded solve's backend owns the heads of the whole autograd graph (solution rows, first-step and anchor
    graphs): it must die with its last reference, not wait for the cyclic collector."""
    import gc
    import weakref
    from torchdiffeq_amd import _native, rowwise
    monkeypatch.setattr(_native, "get_kernels", lambda dev, dt: _LaunchLog())
    y0 = torch.ones(3, 4, dtype=torch.float64, requires_grad=True)
    p = rowwise._Problem(lambda t_, y: -y, y0, torch.tensor([0.0, 1.0], dtype=torch.float64), 1e-6, 1e-8, "dopri5",
                         None, None, True)
    assert p.record
    gc.collect()
    gc.disable()
    try:
        k = rowwise.HipRowKernels(p)
        assert k.rec is not None
        ref = weakref.ref(k)
        del k
        assert ref() is None
    finally:
        gc.enable()
