"""`RowDenseOutput.exposure` / `.area_above` / `.area_below` without a GPU: the host path against the numpy-scalar oracle and the
device driver on the oracle, bit for bit; the exact-rational bound of tests/_rowwise_dense_exposure_oracle.py; closed forms on
the oscillators and the decays; identities with `integral`, `maximum` / `minimum`; dose times; direction, compaction, the query
forms, the level's forms and the errors; the entry point's argument checks."""
import contextlib
import copy
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import U_T
from _rowwise_dense_exposure_oracle import (ExactRecord, bound_constant, device_driver, exact_signed_area_check,  # noqa: F401
                                            oracle_exposure, same_bits, search_lists)
from _rowwise_dense_extremum_oracle import oscillator_problem
from _rowwise_dense_extremum_oracle import windows as _windows
from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native
from torchdiffeq_amd.rowwise_dense import RowDenseExposure

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, L, SEED = 5, 3, 3
OSC_B, OSC_L = 4, 5
EINVAL = -1
# the largest errors of `np_exposure` (the oracle, not the package) against the closed forms on the records of this file
# (`test_closed_forms` prints them): the areas of cos(w t) against 0.5 above and below, and of the decays above a level they
# pass once.  The tests allow 10 x these.  It is the interpolant's error, not the kernel's.
ORACLE_COS_ERR = {F64: 3.5e-7, F32: 3.8e-6}
ORACLE_DECAY_ERR = {F64: 1.3e-8, F32: 2.9e-7}


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _solve(dtype, t0=0.0, t1=None, **kw):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, per_row_t1(B) if t1 is None else t1, method="dopri5",
                                        **{**tolerances("dopri5", dtype), **kw})


def _solve_oscillator(dtype, **kw):
    y0, func, _, t1 = oscillator_problem(OSC_B, OSC_L, dtype)
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", **{**tolerances("dopri5", dtype), **kw})


@functools.lru_cache(maxsize=None)
def _solved(backend, dtype, problem="decay"):
    """One solve per (backend, dtype, problem), shared by the tests that only evaluate it; called inside the backend's context."""
    return _solve(dtype) if problem == "decay" else _solve_oscillator(dtype)


def _levels(dense, problem):
    """The five level forms of tests/test_rowwise_dense_level.py: a scalar, [L], [B, 1], and two [B, L] levels placed exactly on
    the record at the first interior breakpoint of every row (the left limit there, and the next segment's value at its start)."""
    n_rows, width = dense._shape
    first = dense.offsets[:-1]
    lo, hi = (0.1, 1.2) if problem == "decay" else (-0.9, 0.9)
    return {"scalar": 0.9 if problem == "decay" else 0.5,
            "per_element": torch.linspace(lo, hi, width, dtype=F64),
            "per_row": torch.linspace(lo, hi, n_rows, dtype=F64)[:, None],
            "on_breakpoint": dense(dense.seg_end[first][None])[0],
            "on_right_limit": dense.coeffs[0, first + 1].clone()}


def _same(got, want):
    return all(same_bits(a, b) for a, b in zip(got, want))


def _signed_tolerance(dense, level, qa, qb, terms):
    """The bound on |area_above - area_below - (integral - level (tb - ta))| per (window, element): the exact check's bound (C u
    sum S h, tests/_rowwise_dense_exposure_oracle.py) on the fp64 sums, plus one rounding to T of each of the four `terms`
    ([Q, B, L] tensors) -> fp64 [Q, B, L]."""
    found = search_lists(dense, qa, qb)
    ends = (found[0], found[2], found[3], found[5])
    Q = qa.shape[0]
    n_rows, width = dense._shape
    uT = float(U_T[dense.coeffs.dtype])
    tol = torch.zeros(Q, n_rows, width, dtype=F64)
    exact = ExactRecord(dense, level)
    for i in range(Q * n_rows):
        for k in range(width):
            _, scale, n = exact.signed_area(ends, i, k, with_area=False)
            tol[i // n_rows, i % n_rows, k] = float(bound_constant(n) * Fraction(1, 2 ** 53) * scale)
    return tol + uT * sum(t.to(F64).abs() for t in terms)


# -- 1. the bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("problem", ["decay", "oscillator"])
def test_host_oracle_and_device_driver_agree_bit_for_bit(device_driver, problem, dtype):
    host = _solved("host", dtype, problem)
    qa, qb = _windows(host)
    with device_driver():
        dev = _solved("oracle", dtype, problem)                              # (its fp64 step sequence is not the host's)
        da, db = _windows(dev)
    twin = copy.copy(host)                                                   # the device driver on the HOST's record
    twin._k = dev._k
    over = under = 0
    for name, level in _levels(host, problem).items():
        got = host.exposure(level, qa, qb)
        assert isinstance(got, RowDenseExposure) and got.area_above.dtype == got.area_below.dtype == dtype
        assert got.time_above.dtype == F64 and all(v.shape == (8, *host._shape) for v in got)
        *want, _, _, _ = oracle_exposure(host, level, qa, qb)
        assert _same(got, want), name
        assert same_bits(got.time_above, host.time_above(level, qa, qb)), name
        assert same_bits(got.area_above, host.area_above(level, qa, qb)) and same_bits(got.area_below, host.area_below(level, qa, qb))
        assert not any(bool(torch.isnan(v).any()) for v in got)
        assert bool((got.area_above >= 0).all()) and bool((got.area_below >= 0).all())
        over, under = over + int((got.area_above > 0).sum()), under + int((got.area_below > 0).sum())
        with device_driver():
            assert _same(twin.exposure(level, qa, qb), got), name
    assert over > 0 and under > 0
    with device_driver():
        for name, level in _levels(dev, problem).items():
            on_dev = dev.exposure(level, da, db)
            *want, _, _, _ = oracle_exposure(dev, level, da, db)
            assert _same(on_dev, want), name
            assert same_bits(on_dev.time_above, dev.time_above(level, da, db)), name
    assert host._prefix is None and twin._prefix is None and dev._prefix is None      # nothing is built


# -- 2. the exact-rational bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_rational_bound(dtype):
    """The unclamped A_up - A_dn of the oracle on the decay and oscillator records (the eight windows), for a scalar and a
    per-element level, against the exact integral of p - lev: within (35 + 12 n) u sum S h, derived in the oracle module's
    docstring."""
    worst, seen = Fraction(0), 0
    for problem in ("oscillator", "decay"):
        dense = _solved("host", dtype, problem)
        qa, qb = _windows(dense)
        for name in ("scalar", "per_element"):
            level = _levels(dense, problem)[name]
            *_, a_up, a_dn, ends = oracle_exposure(dense, level, qa, qb)
            ratio, pairs = exact_signed_area_check(dense, level, ends, a_up, a_dn)
            worst, seen = max(worst, ratio), seen + pairs
    print(f"{seen} (window, element) pairs, largest |A_up - A_dn - exact| / bound {float(worst):.3g}")
    assert seen >= 100


# -- 3. closed forms -----------------------------------------------------------------------------------------------------------------
def _cos_closed_form(w, lo, hi):
    """cos(w t) against 0.5 on [lo, hi] -> (the area above 0.5, the area below it): sum of [sin(w t) / w - 0.5 t] over the
    intervals between the crossing times (+-pi/3 + 2 pi m) / w, by the side the middle of each interval is on."""
    times = sorted(t for m in range(-1, int(w * hi / (2 * np.pi)) + 2) for t in ((np.pi / 3 + 2 * np.pi * m) / w,
                                                                                (-np.pi / 3 + 2 * np.pi * m) / w) if lo < t < hi)
    edges = [lo, *times, hi]
    F = lambda t: np.sin(w * t) / w - 0.5 * t                                # noqa: E731
    above = sum(F(b) - F(a) for a, b in zip(edges, edges[1:]) if np.cos(w * 0.5 * (a + b)) > 0.5)
    below = -sum(F(b) - F(a) for a, b in zip(edges, edges[1:]) if not np.cos(w * 0.5 * (a + b)) > 0.5)
    return above, below


def _decay_closed_form(y0, k, lev, hi):
    """y0 exp(-k (t + t^2 / 2)) on [0, hi] against a level below y0 that it passes once, at tz < hi -> (the area above the level,
    the area below it).  The integral of exp(-k (t + t^2 / 2)) is exp(k / 2) sqrt(pi / (2 k)) erf(sqrt(k / 2) (t + 1)); the
    difference of two erf near 1 is taken as the difference of two erfc."""
    tz = -1.0 + math.sqrt(1.0 + 2.0 * math.log(y0 / lev) / k)
    assert 0.0 < tz < hi
    r = math.sqrt(k / 2.0)
    G = lambda a, b: y0 * math.exp(k / 2.0) * math.sqrt(math.pi / (2.0 * k)) * (math.erfc(r * (a + 1.0)) - math.erfc(r * (b + 1.0)))  # noqa: E731
    return G(0.0, tz) - lev * tz, lev * (hi - tz) - G(tz, hi)


@pytest.mark.parametrize("dtype", DTYPES)
def test_closed_forms(dtype):
    """Every cos(w t) element against level 0.5 on the whole row and on [0.3 t1, 0.9 t1]: `area_above` and `area_below` are the
    sums of [sin(w t) / w - 0.5 t] over the intervals on each side.  Every decay element against the value of the exact solution
    at 0.5 t1, which it passes once: both areas from the erf closed form.  The tolerance is 10 x the largest error of the
    ORACLE `np_exposure` on these records, measured by this test (it prints the figures) with the `tolerances("dopri5", dtype)`
    of the solve: cos 3.49e-7 (fp64 record, default tolerances) and 3.73e-6 (fp32), decay 1.28e-8 and 2.81e-7 — the error of the
    interpolant, not of the quadrature."""
    errs = {"oracle": [0.0, 0.0], "package": [0.0, 0.0]}
    dense = _solved("host", dtype, "oscillator")
    _, _, w, t1 = oscillator_problem(OSC_B, OSC_L, dtype)
    qa, qb = torch.stack([dense.t0, 0.3 * t1]), torch.stack([dense.t1, 0.9 * t1])
    got = dense.exposure(0.5, qa, qb)
    want = oracle_exposure(dense, 0.5, qa, qb)
    for j in range(2):
        for r in range(OSC_B):
            for k in range(OSC_L // 2):
                exact = _cos_closed_form(float(w[r, k]), float(qa[j, r]), float(qb[j, r]))
                assert exact[0] >= 0 and exact[1] > 0                        # (a window may lie below 0.5 as a whole)
                for who, out in (("oracle", want), ("package", got)):
                    errs[who][0] = max(errs[who][0], abs(float(out[0][j, r, k]) - exact[0]), abs(float(out[1][j, r, k]) - exact[1]))
    decay = _solved("host", dtype)
    y0, _, rate = decay_problem(B, L, dtype, SEED)
    half = 0.5 * per_row_t1(B)[:, None]
    level = (y0.to(F64) * torch.exp(-rate.to(F64) * (half + 0.5 * half * half))).to(dtype)
    got = [v[0] for v in decay.exposure(level, decay.t0[None], decay.t1[None])]
    want = oracle_exposure(decay, level, decay.t0[None], decay.t1[None])
    for r in range(B):
        for k in range(L):
            exact = _decay_closed_form(float(y0[r, k]), float(rate[r, 0]), float(level[r, k]), float(decay.t1[r]))
            assert exact[0] > 0 and exact[1] > 0
            for who, out in (("oracle", [v[0] for v in want[:2]]), ("package", got)):
                errs[who][1] = max(errs[who][1], abs(float(out[0][r, k]) - exact[0]), abs(float(out[1][r, k]) - exact[1]))
    print(f"largest error of the oracle: cos areas {errs['oracle'][0]:.3g}, decay areas {errs['oracle'][1]:.3g}; of the package: "
          f"{errs['package'][0]:.3g}, {errs['package'][1]:.3g}")
    assert errs["package"][0] <= 10 * ORACLE_COS_ERR[dtype] and errs["package"][1] <= 10 * ORACLE_DECAY_ERR[dtype]


# -- 4. identities -------------------------------------------------------------------------------------------------------------------
def _windows_from_t0(dense, seed):
    """Windows [6, B] that have the row's start as one end: the whole row, the whole row reversed, t0 to a random time, a random
    time back to t0, t0 to the first breakpoint, and the point t0.  `integral(ta, tb)` is the difference of two fp64
    antiderivatives from t0, each rounded at ITS OWN size, which the tolerance of the identity below has no term for; from t0
    the lower one is exactly 0 and what is compared is one antiderivative."""
    rnd = random_queries(2, dense.t0, dense.t1, seed)
    brk = dense.seg_end[dense.offsets[:-1]]
    t0, t1 = dense.t0, dense.t1
    return torch.stack([t0, t1, t0, rnd[1], t0, t0]), torch.stack([t1, t0, rnd[0], t0, brk, t0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
@pytest.mark.parametrize("problem", ["decay", "oscillator"])
def test_identities(problem, backend, device_driver, dtype):
    """Either order of the ends; area_above - area_below == integral(ta, tb) - level (tb - ta) to the exact check's bound plus one
    rounding to T of each of the four terms; a level one ulp above the maximum (below the minimum) leaves one area 0 and the
    other equal to that right-hand side; a point window; no negative area."""
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, problem)
        qa, qb = _windows(dense, seed=5)
        for name, level in _levels(dense, problem).items():
            fwd = dense.exposure(level, qa, qb)
            assert _same(fwd, dense.exposure(level, qb, qa)), name           # the order of the ends
            assert bool((fwd.area_above >= 0).all()) and bool((fwd.area_below >= 0).all())
        qa, qb = _windows_from_t0(dense, seed=5)
        lo, hi = torch.minimum(qa, qb), torch.maximum(qa, qb)                # ascending solves: the ends in solver-time order
        area = dense.integral(lo, hi)
        worst = 0.0
        for name, level in _levels(dense, problem).items():
            got = dense.exposure(level, qa, qb)
            lev = dense._level("test", level).view(dense._shape).to(F64)
            box = lev[None] * (hi - lo)[:, :, None]
            tol = _signed_tolerance(dense, level, qa, qb, (got.area_above, got.area_below, area, box))
            miss = ((got.area_above.to(F64) - got.area_below.to(F64)) - (area.to(F64) - box)).abs()
            worst = max(worst, float((miss / tol)[tol > 0].max()))
            assert bool((miss <= tol).all()), (name, worst)
            assert all(bool((v[5] == 0).all()) for v in got)                 # exposure(level, p, p)
        for j in (0, 2, 4):                                                  # (a level does not vary per query)
            a, b = lo[j:j + 1], hi[j:j + 1]
            top, bottom = dense.maximum(a, b).values[0], dense.minimum(a, b).values[0]
            whole = area[j:j + 1].to(F64)
            for level, zero, full, flip in ((torch.nextafter(top, torch.full_like(top, np.inf)), "area_above", "area_below", -1.0),
                                            (torch.nextafter(bottom, torch.full_like(bottom, -np.inf)), "area_below", "area_above", 1.0)):
                got = dense.exposure(level, a, b)
                assert bool((getattr(got, zero) == 0).all())
                box = level.to(F64)[None] * (b - a)[:, :, None]
                tol = _signed_tolerance(dense, level, a, b, (got.area_above, got.area_below, whole, box))
                miss = (getattr(got, full).to(F64) - flip * (whole - box)).abs()
                worst = max(worst, float((miss / tol)[tol > 0].max()))
                assert bool((miss <= tol).all()), (j, zero, worst)
        print(f"largest |area_above - area_below - (integral - level (tb - ta))| / tolerance {worst:.3g}")
        dense.drop_integral_cache()                                          # (`integral` built the prefix store, not `exposure`)
        dense.exposure(0.5, qa, qb)
        assert dense._prefix is None


# -- 5. dose times ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_dose_times(backend, device_driver, dtype):
    """One positive dose per row at p = 0.4 t1 (the state decays everywhere else) and a level halfway up the dose: a window that
    ends at p has no area above; one that holds p and one that starts at p, with the same far end, have the same positive area
    above, bit for bit, which the rectangle time_above x (maximum - level) bounds."""
    t1 = per_row_t1(B)
    p = (0.4 * t1)[None]
    dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64).to(dtype)
    before, after = (0.35 * t1)[None], (0.6 * t1)[None]
    with _backend(backend, device_driver):
        dense = _solve(dtype, options={"jump_t": p, "jump_dy": dy})
        level = (dense(p) + 0.5 * dy)[0]                                     # between the left and the right limit at p
        assert bool((dense(before)[0] < level).all())                        # the window starts below the level
        inside, near = dense.exposure(level, before, after), dense.exposure(level, p, after)
        far, point = dense.exposure(level, before, p), dense.exposure(level, p, p)
        peak = dense.maximum(p, after).values
        below_before = dense.area_below(level, before, p)
    assert bool((far.area_above == 0).all()) and bool((far.time_above == 0).all()) and bool((far.area_below > 0).all())
    assert all(bool((v == 0).all()) for v in point)
    assert bool((inside.area_above > 0).all())
    assert same_bits(inside.area_above, near.area_above) and same_bits(inside.time_above, near.time_above)
    assert same_bits(below_before, far.area_below)
    # y - level <= maximum - level wherever y > level (the state decays from the dose on: the rectangle is far from tight)
    assert bool((inside.area_above.to(F64) <= inside.time_above * (peak.to(F64) - level.to(F64)[None])).all())


# -- 6. direction, compaction, the interface -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_descending_solve(device_driver, dtype):
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
    dense = _solve(dtype, t0=0.3, t1=t1)
    assert dense._sign == -1.0 and bool((dense.seg_end < dense.seg_start).all())
    qa, qb = _windows(dense, seed=3)
    level = torch.linspace(1.2, 3.0, L, dtype=F64)                           # y grows as t runs down from y0 in (1, 2)
    got = dense.exposure(level, qa, qb)
    *want, _, _, _ = oracle_exposure(dense, level, qa, qb)
    assert _same(got, want) and _same(got, dense.exposure(level, qb, qa))
    assert same_bits(got.time_above, dense.time_above(level, qa, qb))
    with device_driver():
        dev = _solve(dtype, t0=0.3, t1=t1)
        da, db = _windows(dev, seed=3)
        on_dev = dev.exposure(level, da, db)
    *want, _, _, _ = oracle_exposure(dev, level, da, db)
    assert _same(on_dev, want)
    assert bool((got.area_above >= 0).all()) and bool((got.area_below >= 0).all())
    assert int((got.area_above > 0).sum()) > 0 and int((got.area_below > 0).sum()) > 0
    # the same record walked upwards: negate the times of the wire format; every number is the same
    up = copy.copy(dense)
    up._sign = 1.0                                                           # (solver time is already ascending)
    assert _same(up.exposure(level, -qa, -qb), got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_compact_gives_the_same_bits(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        plain = _solved(backend, dtype)
        packed = _solve(dtype, compact=True)
        qa, qb = _windows(plain, seed=13)
        for name, level in _levels(plain, "decay").items():
            assert _same(packed.exposure(level, qa, qb), plain.exposure(level, qa, qb)), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_query_and_level_forms(backend, device_driver, dtype):
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)                                # inside every row's interval
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype)
        per_row = shared[:, None].expand(-1, B).contiguous()
        both = dense.exposure(0.9, shared, per_row.flip(0))                                   # [Q] against [Q, B]
        assert all(v.shape == (4, B, L) for v in both)
        assert _same(both, dense.exposure(0.9, per_row, per_row.flip(0)))
        wide = dense.exposure(0.9, 0.02, shared)                                              # a number broadcasts
        assert _same(wide, dense.exposure(0.9, shared, torch.tensor(0.02, dtype=F64)))
        one = dense.exposure(0.9, 0.02, 0.21)
        assert all(v.shape == (B, L) for v in one) and _same(one, [v[0] for v in wide])
        assert dense.area_above(0.9, 0.02, 0.21).shape == dense.area_below(0.9, 0.02, 0.21).shape == (B, L)
        none = dense.exposure(0.9, torch.empty(0, dtype=F64), 0.1)
        assert all(v.shape == (0, B, L) for v in none) and none.area_above.dtype == dtype and none.time_above.dtype == F64
        # the forms of the level: a number, 0-dim, [L], [B, 1], [B, L], an integer tensor, another float dtype
        full = torch.full((B, L), 0.9, dtype=F64)
        for level in (torch.tensor(0.9, dtype=F64), full, full[:, :1], full[0], full.to(dtype)):
            assert _same(dense.exposure(level, 0.02, shared), wide)
        assert _same(dense.exposure(1, 0.02, shared), dense.exposure(torch.ones(L, dtype=torch.int64), 0.02, shared))
        rows = torch.linspace(0.5, 1.5, B, dtype=F64)[:, None]                                # one level per row
        split = dense.exposure(rows, 0.02, shared)
        for r in range(B):
            assert _same([v[:, r] for v in split], [v[:, r] for v in dense.exposure(float(rows[r]), 0.02, shared)])
        # a NaN level: that element alone
        holed = full.clone()
        holed[1, 2] = holed[4, 0] = float("nan")
        mask = torch.isnan(holed)[None].expand(4, B, L)
        got = dense.exposure(holed, 0.02, shared)
        assert all(bool(torch.isnan(v[mask]).all()) for v in got)
        assert all(same_bits(a[~mask], b[~mask]) for a, b in zip(got, wide))
        # refusals
        with pytest.raises(ValueError, match="do not broadcast"):
            dense.exposure(0.9, shared, shared[:3])
        with pytest.raises(ValueError, match="must be a number"):
            dense.area_above(0.9, 0.1, torch.zeros(2, B + 1, dtype=F64))
        for bad in (torch.zeros(B, L, dtype=torch.complex64), torch.zeros(L, dtype=torch.bool), True, "0.9", None):
            with pytest.raises(ValueError, match="level must be"):
                dense.exposure(bad, 0.02, 0.21)
        for bad in (torch.zeros(L + 1, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(2, B, L, dtype=F64)):
            with pytest.raises(ValueError, match="does not broadcast"):
                dense.area_below(bad, 0.02, 0.21)
        t = torch.tensor(0.1, dtype=F64, requires_grad=True)
        lev = torch.tensor(0.9, dtype=F64, requires_grad=True)
        for call in (lambda: dense.exposure(0.9, t, 0.2), lambda: dense.area_above(0.9, 0.0, t),
                     lambda: dense.exposure(lev, 0.0, 0.2), lambda: dense.area_below(lev, 0.0, 0.2)):
            with pytest.raises(NotImplementedError, match="does not propagate gradients"):
                call()
        with torch.no_grad():
            assert _same(dense.exposure(lev, 0.02, shared), wide)
        assert dense._prefix is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_out_of_range(backend, device_driver, dtype, monkeypatch):
    """`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives NaN in all three fields for the
    whole row of such a query, leaves the others alone and reads nothing from the device."""
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype)
        good = random_queries(3, dense.t0, dense.t1, seed=2)
        other = good.flip(0).contiguous()
        bad = good.clone()
        bad[2, 1] = float("nan")
        bad[1, 3] = float(dense.t1[3]) + 1e-9
        bad[2, 0] = -1e-9
        mask = torch.zeros(3, B, dtype=torch.bool)
        mask[2, 1] = mask[1, 3] = mask[2, 0] = True
        with pytest.raises(ValueError, match=r"dense.exposure\(level, ta, tb\): query 1 of row 3 \(ta = .*outside the row's interval"):
            dense.exposure(0.9, bad, bad.flip(0))
        with pytest.raises(ValueError, match=r"query 0 of row 0 \(tb = "):
            dense.area_above(0.9, good, bad.flip(0))
        want = dense.exposure(0.9, good, other)
        with monkeypatch.context() as m:
            def no_read(*a, **k):
                raise AssertionError("check=False read from the device")
            if backend == "oracle":
                m.setattr(torch.Tensor, "tolist", no_read)
            first, second = dense.exposure(0.9, bad, other, check=False), dense.exposure(0.9, other, bad, check=False)
            below = dense.area_below(0.9, bad, other, check=False)
        assert same_bits(below, first.area_below)
        for got in (first, second):
            assert all(bool(torch.isnan(v[mask]).all()) and not bool(torch.isnan(v[~mask]).any()) for v in got)
            assert all(same_bits(a[~mask], b[~mask]) for a, b in zip(got, want))
        with pytest.raises(ValueError, match="query 0 of row 0"):
            dense.exposure(0.9, float("nan"), 0.1)


def test_query_count_overflow(device_driver):
    """More than 2^31 - 2 windows in one call: refused before anything is allocated, as the other methods refuse it."""
    with device_driver():
        dense = _solved("oracle", F32)
        huge = torch.empty((2 ** 31) // B + 1, B, dtype=F64, device="meta")
        twin = copy.copy(dense)
        twin._query_lists = lambda what, names, ts: ([huge, huge], False)
        for call in (lambda: twin.exposure(0.9, 0.0, 0.1), lambda: twin.area_above(0.9, 0.0, 0.1),
                     lambda: twin.area_below(0.9, 0.0, 0.1)):
            with pytest.raises(ValueError, match="the query index is a 32-bit word"):
                call()


def test_abi_34_argument_errors():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION >= 34
    assert "tdeq_row_dense_exposure" in _native.ABI_SIGNATURES and tda.RowDenseExposure is RowDenseExposure
    assert "RowDenseExposure" in tda.__all__
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(area_above=p, area_below=p, time_above=p, level=p, n_rows=1, coeffs=p, n_seg=2, seg_ta=p, seg_tb=p, sign=1.0, seg=p,
              x=p, tq=p, seg2=p, x2=p, tq2=p, n_idx=1, row_len=3, dtype=_native.dtype_code(F64))

    def call(**kw):
        a = {**ok, **kw}
        return lib.tdeq_row_dense_exposure(a["area_above"], a["area_below"], a["time_above"], a["level"], a["n_rows"], a["coeffs"],
                                           a["n_seg"], a["seg_ta"], a["seg_tb"], a["sign"], a["seg"], a["x"], a["tq"], a["seg2"],
                                           a["x2"], a["tq2"], a["n_idx"], a["row_len"], a["dtype"], None)
    for name in ("area_above", "area_below", "time_above", "level", "coeffs", "seg_ta", "seg_tb", "seg", "x", "tq", "seg2", "x2",
                 "tq2"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(sign=0.0), dict(sign=2.0), dict(sign=float("nan")), dict(n_idx=-1), dict(n_rows=0), dict(n_rows=-1),
               dict(n_rows=2, n_idx=3), dict(n_rows=4, n_idx=2), dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31),
               dict(row_len=-3), dict(dtype=7), dict(dtype=_native.TDEQ_BF16)):
        assert call(**kw) == EINVAL, kw
    assert call(n_idx=0) == 0 and call(n_idx=0, n_rows=0) == 0 and call(row_len=0, dtype=_native.dtype_code(F32)) == 0
