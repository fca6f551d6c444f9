"""Per-row tolerances of `odeint_rowwise` (rtol / atol as [B] vectors) without a GPU: the torch-op host path and, through
`device_driver`, `HipRowKernels` on the CPU row oracle (tests/_rowwise_tol_oracle.py).

What is checked is bit identity, never closeness: row r of a solve with per-row tolerances IS the one-row solve with the
row's two scalars (a row's arithmetic does not depend on the batch it sits in, and the [B] vectors are rounded to the
state's type exactly as the scalars are), and constant vectors ARE the scalar solve."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from _rowwise_compact_oracle import METHODS, assert_same_solve
from _rowwise_tol_oracle import MIXED_B, device_driver, mixed_problem, quiet, random_problem  # noqa: F401

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

BACKENDS = ["host", "oracle"]
F32, F64 = torch.float32, torch.float64


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _same(a, b):
    """(solution, stats) twice: the same bits and the same counts."""
    (sa, ta), (sb, tb) = a, b
    assert torch.equal(sa, sb)
    assert torch.equal(ta["n_accepted"], tb["n_accepted"]) and torch.equal(ta["n_rejected"], tb["n_rejected"])
    assert ta["nfe"] == tb["nfe"]


# -- 1. a constant vector is the scalar ---------------------------------------------------------------------------------------
CONSTANT = [("host", m, F32) for m in METHODS] + [(b, m, F64) for b in BACKENDS for m in ("dopri5", "tsit5", "dopri8")]


@pytest.mark.parametrize("backend,method,dtype", CONSTANT,
                         ids=[f"{b}-{m}-{'f32' if d == F32 else 'f64'}" for b, m, d in CONSTANT])
def test_constant_vector_equals_scalar(backend, method, dtype, device_driver):
    B = 12
    y0, plain, _, _ = random_problem(B, 5, dtype, 3)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    rtol, atol = (1e-6, 1e-8) if dtype == F64 else (1e-3, 1e-5)
    with torch.no_grad(), _backend(backend, device_driver):
        scalar = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, method=method, return_stats=True)
        vector = tda.odeint_rowwise(plain, y0, t, rtol=torch.full((B,), rtol, dtype=torch.float64),
                                    atol=torch.full((B,), atol, dtype=torch.float64), method=method, return_stats=True)
    _same(vector, scalar)
    assert int(scalar[1]["n_accepted"].min()) >= 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_only_rtol_is_a_vector(backend, device_driver):
    """The other tolerance is filled to [B]: rtol a constant vector and atol a number give the scalar solve, and so
    does the mirror image."""
    B = 12
    y0, plain, _, _ = random_problem(B, 5, F64, 3)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    with torch.no_grad(), _backend(backend, device_driver):
        scalar = tda.odeint_rowwise(plain, y0, t, rtol=1e-6, atol=1e-8, return_stats=True)
        only_rtol = tda.odeint_rowwise(plain, y0, t, rtol=[1e-6] * B, atol=1e-8, return_stats=True)
        only_atol = tda.odeint_rowwise(plain, y0, t, rtol=1e-6, atol=torch.full((B,), 1e-8, dtype=torch.float64),
                                       return_stats=True)
    _same(only_rtol, scalar)
    _same(only_atol, scalar)


# -- 2. mixed tolerances: every row is its one-row scalar solve ---------------------------------------------------------------
def _grid(kind, t, B):
    """(t, options) of one kind of grid / option; a per-row piece is sliced by `_row_args`."""
    if kind == "t2d":            # rows that end at different times
        return t[:, None] * torch.linspace(0.2, 1.0, B, dtype=torch.float64) + 0.05 * torch.arange(B).to(torch.float64), None
    if kind == "decreasing":
        return torch.linspace(1.5, 0, 4, dtype=torch.float64), None
    if kind == "first_step":
        return t, {"first_step": torch.linspace(1e-3, 5e-3, B, dtype=torch.float64)}
    return t, None


def _row_args(t, opts, r):
    t_r = t[:, r:r + 1] if t.dim() == 2 else t
    return t_r, None if opts is None else {"first_step": opts["first_step"][r:r + 1]}


def _assert_rows_are_one_row_solves(sol, stats, y0, t, opts, rtol, atol, subset, method="dopri5"):
    for r in range(y0.shape[0]):
        t_r, o_r = _row_args(t, opts, r)
        with torch.no_grad():
            one, st = tda.odeint_rowwise(subset(slice(r, r + 1)), y0[r:r + 1], t_r, rtol=float(rtol[r]), atol=float(atol[r]),
                                         method=method, options=o_r, return_stats=True)
        assert torch.equal(one[:, 0], sol[:, r]), r
        assert int(st["n_accepted"][0]) == int(stats["n_accepted"][r]), r
        assert int(st["n_rejected"][0]) == int(stats["n_rejected"][r]), r


@pytest.mark.parametrize("kind", ["t1d", "t2d", "decreasing", "first_step"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_mixed_rows_are_one_row_solves(backend, dtype, kind, device_driver):
    y0, t, rtol, atol, plain, _, subset = mixed_problem(dtype)
    t, opts = _grid(kind, t, MIXED_B)
    with _backend(backend, device_driver):
        with torch.no_grad():
            sol, stats = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, options=opts, return_stats=True)
            # the condition on the inputs: were the tolerances ignored (every row at the loosest pair, say), at least half
            # of the rows would take another number of trial steps, so the comparison below could not pass
            _, loose = tda.odeint_rowwise(plain, y0, t, rtol=float(rtol.max()), atol=float(atol.max()), options=opts,
                                          return_stats=True)
        trials = stats["n_accepted"] + stats["n_rejected"]
        trials_loose = loose["n_accepted"] + loose["n_rejected"]
        print(f"{backend} {dtype} {kind}: trials per row {trials.tolist()}, at the loosest pair {trials_loose.tolist()}")
        assert int((trials != trials_loose).sum()) >= MIXED_B // 2
        _assert_rows_are_one_row_solves(sol, stats, y0, t, opts, rtol, atol, subset)


# -- 3. compaction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("backend", BACKENDS)
def test_mixed_compact_equals_plain(backend, c, device_driver):
    """The tolerance vectors are re-selected with the rows at every repack: the bits and counts of the plain solve."""
    y0, t, rtol, atol, plain, by_rows, _ = mixed_problem(F64)
    with torch.no_grad(), _backend(backend, device_driver):
        a = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, return_stats=True)
        b = tda.odeint_rowwise(by_rows, y0, t, rtol=rtol, atol=atol, return_stats=True, compact=c)
    _, repacks = assert_same_solve(a, b, c, "dopri5")
    assert repacks >= 1


# -- 4. a recorded solve (host path) ------------------------------------------------------------------------------------------
def test_recorded_solve_rows_are_one_row_recorded_solves():
    y0, t, rtol, atol, plain, _, subset = mixed_problem(F64)
    with torch.no_grad():
        ref, ref_stats = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, return_stats=True)
    y = y0.clone().requires_grad_(True)
    sol, stats = tda.odeint_rowwise(plain, y, t, rtol=rtol, atol=atol, return_stats=True, differentiable=True)
    assert sol.requires_grad and torch.equal(sol, ref)
    _same((sol.detach(), stats), (ref, ref_stats))
    grad, = torch.autograd.grad(sol.pow(2).sum(), y)
    for r in range(MIXED_B):
        y_r = y0[r:r + 1].clone().requires_grad_(True)
        one = tda.odeint_rowwise(subset(slice(r, r + 1)), y_r, t, rtol=float(rtol[r]), atol=float(atol[r]),
                                 differentiable=True)
        g_r, = torch.autograd.grad(one.pow(2).sum(), y_r)
        assert torch.equal(one[:, 0], sol[:, r].detach()), r
        assert torch.equal(g_r[0], grad[r]), (r, g_r[0].tolist(), grad[r].tolist())


# -- 5. validation ------------------------------------------------------------------------------------------------------------
def test_tolerance_validation():
    B, shape = 4, (2, 3)
    y0 = torch.ones(B, *shape, dtype=F64)
    t = torch.tensor([0.0, 1.0], dtype=F64)
    f = lambda t_, y: -y                                        # noqa: E731
    bad = [torch.ones(B + 1), torch.ones(B - 1), torch.ones(B, 1), torch.ones(1, B), torch.ones(B, *shape),
           torch.ones(*shape), torch.ones(3), [1e-3] * (B + 1), (1e-3,) * (B - 1), np.ones(B + 2), np.ones((B, 2)), "1e-3",
           [1e-3, None, 1e-3, 1e-3]]
    for name in ("rtol", "atol"):
        for tol in bad:
            with pytest.raises(ValueError, match="vector"):
                tda.odeint_rowwise(f, y0, t, **{name: tol})
    # [*row_shape] whose leading length happens to be something else than B, flat
    with pytest.raises(ValueError, match="vector"):
        tda.odeint_rowwise(f, torch.ones(3, 2, dtype=F64), t, rtol=torch.ones(2))


def test_accepted_vector_forms_give_equal_results():
    y0, t, rtol, atol, plain, _, _ = mixed_problem(F64)
    # values that fp32 holds exactly, so that every form names the same numbers
    rtol, atol = rtol.to(F32).to(F64), atol.to(F32).to(F64)
    forms = [lambda v: v.tolist(), lambda v: tuple(v.tolist()), lambda v: v.numpy().copy(), lambda v: v.to(F32),
             lambda v: v.clone().requires_grad_(True)]
    with torch.no_grad():
        ref = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, return_stats=True)
    for form in forms:
        with torch.no_grad():
            got = tda.odeint_rowwise(plain, y0, t, rtol=form(rtol), atol=form(atol), return_stats=True)
        _same(got, ref)
    # with grad mode on, a tolerance that requires grad is detached: it neither raises nor receives a gradient
    r = rtol.clone().requires_grad_(True)
    y = y0.clone().requires_grad_(True)
    sol = tda.odeint_rowwise(plain, y, t, rtol=r, atol=atol, differentiable=True)
    assert torch.equal(sol.detach(), ref[0])
    assert torch.autograd.grad(sol.sum(), r, allow_unused=True)[0] is None
    # a one-element tensor stays a scalar, on the scalar path (the per-row vectors are not built)
    from torchdiffeq_amd.rowwise import _Problem
    p = _Problem(plain, y0, t, torch.tensor([1e-5]), torch.tensor(1e-7), "dopri5", None, None)
    assert (p.rtol, p.atol, p.rtol_rows, p.atol_rows) == (float(torch.tensor(1e-5)), float(torch.tensor(1e-7)), None, None)
    p = _Problem(plain, y0.to(F32), t, rtol, 1e-7, "dopri5", None, None)
    assert p.rtol is None and p.rtol_rows.dtype == p.atol_rows.dtype == F32 and p.atol_rows.shape == (MIXED_B,)
    assert torch.equal(p.rtol_rows, rtol.to(F32)) and torch.equal(p.atol_rows, torch.full((MIXED_B,), 1e-7).to(F32))


# -- 6. argument validation of the entry point (no launch is reached) ---------------------------------------------------------
EINVAL, EWORKSPACE = -1, -2
BF16 = _native.TDEQ_BF16


@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def test_row_reduce_tol_argument_errors(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 14)(*([p] * 14))
    names = ("mode", "y0", "y1", "partial", "k", "coef", "n_terms", "dts", "active", "rtol_rows", "atol_rows", "n_rows",
             "row_len", "part", "part_bytes", "dtype", "stream")
    err = dict(mode=0, y0=p, y1=p, partial=None, k=ptrs, coef=buf, n_terms=2, dts=p, active=p, rtol_rows=p, atol_rows=p,
               n_rows=2, row_len=4, part=p, part_bytes=3 * 2 * 8, dtype=_native.TDEQ_F64, stream=None)
    init = dict(err, mode=1, partial=p, n_terms=0, dts=None, active=None)
    call = lambda base, **kw: lib.tdeq_row_reduce_tol(*[kw.get(n, base[n]) for n in names])      # noqa: E731
    for base in (err, init):
        for name in ("rtol_rows", "atol_rows", "y0", "y1", "part"):
            assert call(base, **{name: None}) == EINVAL, name
        assert call(base, mode=-1) == EINVAL and call(base, mode=3) == EINVAL
        assert call(base, dtype=BF16) == EINVAL and call(base, dtype=7) == EINVAL
        assert call(base, row_len=0) == EINVAL and call(base, n_rows=-1) == EINVAL
        assert call(base, part_bytes=3 * 2 * 8 - 1) == EWORKSPACE                  # a short `part`
        assert call(base, row_len=2049 * 2, part_bytes=3 * 2 * 8) == EWORKSPACE    # (two partials per row)
        assert call(base, n_rows=0, part_bytes=0) == 0                             # no row: no launch
        assert call(base, n_rows=0, rtol_rows=None) == EINVAL                      # (the null check comes first)
    for name in ("k", "coef", "dts", "active"):
        assert call(err, **{name: None}) == EINVAL, name
    assert call(err, n_terms=0) == EINVAL and call(err, n_terms=15) == EINVAL and call(err, n_terms=-1) == EINVAL
    assert call(err, k=(ctypes.c_void_p * 14)(p, None)) == EINVAL
    assert call(init, n_terms=1) == EINVAL and call(init, partial=None) == EINVAL
    # tdeq_row_reduce answers the same calls the same way
    scalar = lambda base, **kw: lib.tdeq_row_reduce(*[                                             # noqa: E731
        1e-3 if n in ("rtol_rows", "atol_rows") else kw.get(n, base[n]) for n in names])
    for base in (err, init):
        for kw in (dict(y0=None), dict(mode=3), dict(dtype=7), dict(row_len=0), dict(part_bytes=1), dict(n_rows=0)):
            assert scalar(base, **kw) == call(base, **kw), kw
