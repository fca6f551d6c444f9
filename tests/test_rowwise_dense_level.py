"""`RowDenseOutput.crossings` / `.time_above` without a GPU: the host path against the numpy-scalar oracle and the device driver
on the oracle, bit for bit; the exact-rational bound of tests/_rowwise_dense_level_oracle.py; the oscillators against the
closed form of cos(w t) = 0.5; dose times; identities with `maximum` / `minimum`; direction, compaction, the query forms, the
level's forms and the errors; the entry point's argument checks."""
import contextlib
import copy
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_extremum_oracle import oscillator_problem
from _rowwise_dense_extremum_oracle import windows as _windows
from _rowwise_dense_level_oracle import device_driver, exact_crossing_check, oracle_level, same_bits  # noqa: F401
from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native
from torchdiffeq_amd.rowwise_dense import RowDenseCrossings

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, L, SEED = 5, 3, 3
OSC_B, OSC_L = 4, 5
EINVAL = -1
# the largest errors of `np_level` (the oracle, not the package) against the closed form on the oscillator records of this file
# (`test_oscillator_closed_forms` prints them): crossing times and time above.  The tests allow 10 x these.
ORACLE_TIME_ERR = {F64: 7.4e-8, F32: 1.1e-6}
ORACLE_ABOVE_ERR = {F64: 2.5e-7, F32: 2.7e-6}


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
    """A scalar level, an [L] level, a [B, 1] level, and two [B, L] levels placed exactly on the record at the first interior
    breakpoint of every row: `dense(t)` there (the left limit) and the next segment's value at its start."""
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
    crossed = zeros = 0
    for name, level in _levels(host, problem).items():
        got = host.crossings(level, qa, qb)
        assert isinstance(got, RowDenseCrossings) and got.count.dtype == torch.int32
        assert got.first.dtype == got.last.dtype == got.time_above.dtype == F64
        assert all(v.shape == (8, *host._shape) for v in got)
        *want, located = oracle_level(host, level, qa, qb)
        assert _same(got, want), name
        assert bool((got.count >= 0).all()) and not bool(torch.isnan(got.time_above).any())
        assert bool((torch.isnan(got.first) == (got.count == 0)).all()) and bool((torch.isnan(got.last) == (got.count == 0)).all())
        crossed += int((got.count > 0).sum())
        if name.startswith("on_"):                                           # phi == 0 at a candidate: the value is the level
            zeros += int(((got.first == host.seg_end[host.offsets[:-1]][None, :, None]) & (got.count > 0)).sum())
        with device_driver():
            assert _same(twin.crossings(level, qa, qb), got), name
    assert crossed > 0 and zeros > 0
    with device_driver():
        for name, level in _levels(dev, problem).items():
            on_dev = dev.crossings(level, da, db)
            *want, _ = oracle_level(dev, level, da, db)
            assert _same(on_dev, want), name
    assert host._prefix is None and twin._prefix is None and dev._prefix is None      # nothing is built


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_rational_bound(dtype):
    """Every crossing that a bisection located on the decay and oscillator records (whole rows, and windows clipped at both
    ends), for a scalar and a per-element level: the exact |p(z) - lev| against 18 u S + 2^-52 G, derived in the oracle module's
    docstring."""
    worst, seen = Fraction(0), 0
    for problem in ("oscillator", "decay"):
        dense = _solved("host", dtype, problem)
        qa, qb = _windows(dense)
        for name in ("scalar", "per_element"):
            level = _levels(dense, problem)[name]
            *_, located = oracle_level(dense, level, qa, qb)
            seen += len(located)
            worst = max(worst, exact_crossing_check(dense, level, located))
    print(f"{seen} located crossings, largest |p(z) - lev| / bound {float(worst):.3g}")
    assert seen >= 100


# -- 2. the closed form ------------------------------------------------------------------------------------------------------------
def _cos_closed_form(w, lo, hi):
    """cos(w t) against 0.5 on [lo, hi] -> (the crossing times inside (lo, hi), sorted; the time above 0.5)."""
    times = sorted(t for m in range(-1, int(w * hi / (2 * np.pi)) + 2) for t in ((np.pi / 3 + 2 * np.pi * m) / w,
                                                                                (-np.pi / 3 + 2 * np.pi * m) / w) if lo < t < hi)
    edges = [lo, *times, hi]
    above = sum(b - a for a, b in zip(edges, edges[1:]) if np.cos(w * 0.5 * (a + b)) > 0.5)
    return times, above


@pytest.mark.parametrize("dtype", DTYPES)
def test_oscillator_closed_forms(dtype):
    """Every cos(w t) element against level 0.5 on the whole row and on [0.3 t1, 0.9 t1]: `count` is the number of
    (+-pi/3 + 2 pi m) / w inside the window; `first`, `last` and `time_above` match the closed form.  The tolerance is 10 x the
    largest error of the ORACLE `np_level` on these records, measured by this test (it prints the figures) with the
    `tolerances("dopri5", dtype)` of the solve: crossing times 7.39e-8 (fp64 record, default tolerances) and 1.08e-6 (fp32),
    time above 2.41e-7 and 2.63e-6 — the error of the interpolant, not of the root finding."""
    dense = _solved("host", dtype, "oscillator")
    _, _, w, t1 = oscillator_problem(OSC_B, OSC_L, dtype)
    m = OSC_L // 2
    qa, qb = torch.stack([dense.t0, 0.3 * t1]), torch.stack([dense.t1, 0.9 * t1])
    got = dense.crossings(0.5, qa, qb)
    *want, _ = oracle_level(dense, 0.5, qa, qb)
    errs = {"oracle": [0.0, 0.0], "package": [0.0, 0.0]}
    total = 0
    for j in range(2):
        for r in range(OSC_B):
            for k in range(m):
                times, above = _cos_closed_form(float(w[r, k]), float(qa[j, r]), float(qb[j, r]))
                total += len(times)
                for who, out in (("oracle", want), ("package", got)):
                    assert int(out[0][j, r, k]) == len(times), (who, j, r, k)
                    if times:
                        errs[who][0] = max(errs[who][0], abs(float(out[1][j, r, k]) - times[0]),
                                           abs(float(out[2][j, r, k]) - times[-1]))
                    errs[who][1] = max(errs[who][1], abs(float(out[3][j, r, k]) - above))
    print(f"{total} crossings; largest error of the oracle: times {errs['oracle'][0]:.3g}, time above {errs['oracle'][1]:.3g}; "
          f"of the package: {errs['package'][0]:.3g}, {errs['package'][1]:.3g}")
    assert total >= 40
    assert errs["package"][0] <= 10 * ORACLE_TIME_ERR[dtype] and errs["package"][1] <= 10 * ORACLE_ABOVE_ERR[dtype]


# -- 3. dose times ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_dose_times(backend, device_driver, dtype):
    """One positive dose per row at p = 0.4 t1 (the state decays everywhere else) and a level halfway up the dose: a window
    that holds p, or starts at p, crosses the level AT p; a window that ends at p does not see the dose."""
    t1 = per_row_t1(B)
    p = (0.4 * t1)[None]
    dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64).to(dtype)
    before, after = (0.35 * t1)[None], (0.6 * t1)[None]
    with _backend(backend, device_driver):
        dense = _solve(dtype, options={"jump_t": p, "jump_dy": dy})
        level = (dense(p) + 0.5 * dy)[0]                                     # between the left and the right limit at p
        assert bool((dense(before)[0] < level).all())                        # the window starts below the level
        inside, near = dense.crossings(level, before, after), dense.crossings(level, p, after)
        far, point = dense.crossings(level, before, p), dense.crossings(level, p, p)
        ends_above = dense(after)[0] > level
        whole = dense.crossings(level, dense.t0[None], dense.t1[None])
    at_p = p[:, :, None].expand(1, B, L)
    for got in (inside, near):
        assert torch.equal(got.first, at_p)                                  # the up-crossing at the dose, bit for bit
        assert torch.equal(got.count[0], torch.where(ends_above, 1, 2).to(torch.int32))
        assert torch.equal(got.last[0][ends_above], at_p[0][ends_above]) and bool((got.last[0][~ends_above] > at_p[0][~ends_above]).all())
        assert bool((got.time_above > 0).all()) and bool((got.time_above <= (after - p)[:, :, None]).all())
        assert torch.equal(got.time_above[0][ends_above], (after - p)[0][:, None].expand(B, L)[ends_above])
    assert _same(inside, near)
    for got in (far, point):                                                 # the far end: only the left limit at p
        assert bool((got.count == 0).all()) and bool((got.time_above == 0).all())
        assert bool(torch.isnan(got.first).all()) and bool(torch.isnan(got.last).all())
    # the whole row: y0 > level comes down through it first where the level is below y0, then the dose, then down again
    starts_above = dense(dense.t0[None])[0] > level
    want = starts_above.to(torch.int32) + 1 + (~(dense(dense.t1[None])[0] > level)).to(torch.int32)
    assert torch.equal(whole.count[0], want)
    assert torch.equal(whole.first[0][~starts_above], at_p[0][~starts_above])


# -- 4. identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
@pytest.mark.parametrize("problem", ["decay", "oscillator"])
def test_identities(problem, backend, device_driver, dtype):
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, problem)
        qa, qb = _windows(dense, seed=5)
        for level in _levels(dense, problem).values():
            fwd, rev = dense.crossings(level, qa, qb), dense.crossings(level, qb, qa)
            assert _same(fwd, rev)                                           # the order of the ends
            assert same_bits(dense.time_above(level, qa, qb), fwd.time_above)
            assert bool((fwd.time_above >= 0).all()) and bool((fwd.time_above <= (qb - qa).abs()[:, :, None] + 1e-12).all())
        for j in range(qa.shape[0]):                                         # (a level does not vary per query)
            a, b = qa[j:j + 1], qb[j:j + 1]
            span = (b - a).abs()[0, :, None].expand(dense._shape).contiguous()      # tqb - tqa in solver time (ascending)
            top, bottom = dense.maximum(a, b).values[0], dense.minimum(a, b).values[0]
            over = dense.crossings(torch.nextafter(top, torch.full_like(top, np.inf)), a, b)
            assert bool((over.count == 0).all()) and bool((over.time_above == 0).all()) and bool(torch.isnan(over.first).all())
            under = dense.crossings(torch.nextafter(bottom, torch.full_like(bottom, -np.inf)), a, b)
            assert bool((under.count == 0).all()) and bool(torch.isnan(under.last).all())
            assert same_bits(under.time_above[0], span)
            far = dense.crossings(top + 1, a, b)
            assert bool((far.count == 0).all()) and bool((far.time_above == 0).all())
            assert same_bits(dense.crossings(bottom - 1, a, b).time_above[0], span)
        assert dense._prefix is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_descending_solve(device_driver, dtype):
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
    dense = _solve(dtype, t0=0.3, t1=t1)
    assert dense._sign == -1.0 and bool((dense.seg_end < dense.seg_start).all())
    qa, qb = _windows(dense, seed=3)
    level = torch.linspace(1.2, 3.0, L, dtype=F64)                           # y grows as t runs down from y0 in (1, 2)
    got = dense.crossings(level, qa, qb)
    *want, _ = oracle_level(dense, level, qa, qb)
    assert _same(got, want)
    with device_driver():
        dev = _solve(dtype, t0=0.3, t1=t1)
        da, db = _windows(dev, seed=3)
        on_dev = dev.crossings(level, da, db)
    *want, _ = oracle_level(dev, level, da, db)
    assert _same(on_dev, want)
    assert int((got.count > 0).sum()) > 0
    assert bool((got.time_above >= 0).all()) and bool((got.time_above <= (qb - qa).abs()[:, :, None]).all())
    assert int((got.time_above > 0).sum()) > 0
    lo, hi = torch.minimum(qa, qb)[:, :, None], torch.maximum(qa, qb)[:, :, None]
    hit = got.count > 0
    assert bool(((got.first >= lo) & (got.first <= hi))[hit].all()) and bool((got.first >= got.last)[hit].all())
    # a level the record passes twice in a descending solve: an oscillator run backwards from t = 2
    y0, func, w, _ = oscillator_problem(2, 2, dtype)
    with torch.no_grad():
        osc = tda.odeint_rowwise_dense(func, y0, 2.0, 0.0, method="dopri5", **tolerances("dopri5", dtype))
    both = osc.crossings(0.0, 2.0, 0.0)
    assert bool((both.count >= 0).all()) and bool((both.first > both.last)[both.count >= 2].all())
    assert int((both.count >= 2).sum()) > 0 and bool((both.time_above > 0)[both.count >= 2].all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_compact_gives_the_same_bits(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        plain = _solved(backend, dtype)
        packed = _solve(dtype, compact=True)
        qa, qb = _windows(plain, seed=13)
        for name, level in _levels(plain, "decay").items():
            assert _same(packed.crossings(level, qa, qb), plain.crossings(level, qa, qb)), name


# -- 5. the interface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_query_and_level_forms(backend, device_driver, dtype):
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)                                # inside every row's interval
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype)
        per_row = shared[:, None].expand(-1, B).contiguous()
        both = dense.crossings(0.9, shared, per_row.flip(0))                                  # [Q] against [Q, B]
        assert all(v.shape == (4, B, L) for v in both)
        assert _same(both, dense.crossings(0.9, per_row, per_row.flip(0)))
        wide = dense.crossings(0.9, 0.02, shared)                                             # a number broadcasts
        assert _same(wide, dense.crossings(0.9, shared, torch.tensor(0.02, dtype=F64)))
        one = dense.crossings(0.9, 0.02, 0.21)
        assert all(v.shape == (B, L) for v in one) and _same(one, [v[0] for v in wide])
        assert dense.time_above(0.9, 0.02, 0.21).shape == (B, L)
        none = dense.crossings(0.9, torch.empty(0, dtype=F64), 0.1)
        assert all(v.shape == (0, B, L) for v in none) and none.count.dtype == torch.int32 and none.first.dtype == F64
        # the forms of the level: a number, 0-dim, [L], [B, 1], [B, L], an integer tensor, another float dtype
        full = torch.full((B, L), 0.9, dtype=F64)
        for level in (torch.tensor(0.9, dtype=F64), full, full[:, :1], full[0], full.to(dtype)):
            assert _same(dense.crossings(level, 0.02, shared), wide)
        assert _same(dense.crossings(1, 0.02, shared), dense.crossings(torch.ones(L, dtype=torch.int64), 0.02, shared))
        rows = torch.linspace(0.5, 1.5, B, dtype=F64)[:, None]                                # one level per row
        split = dense.crossings(rows, 0.02, shared)
        for r in range(B):
            assert _same([v[:, r] for v in split], [v[:, r] for v in dense.crossings(float(rows[r]), 0.02, shared)])
        # a NaN level: that element alone
        holed = full.clone()
        holed[1, 2] = holed[4, 0] = float("nan")
        mask = torch.isnan(holed)[None].expand(4, B, L)
        got = dense.crossings(holed, 0.02, shared)
        assert bool((got.count[mask] == -1).all()) and all(bool(torch.isnan(v[mask]).all()) for v in got[1:])
        assert all(same_bits(a[~mask], b[~mask]) for a, b in zip(got, wide))
        # refusals
        with pytest.raises(ValueError, match="do not broadcast"):
            dense.crossings(0.9, shared, shared[:3])
        with pytest.raises(ValueError, match="must be a number"):
            dense.time_above(0.9, 0.1, torch.zeros(2, B + 1, dtype=F64))
        for bad in (torch.zeros(B, L, dtype=torch.complex64), torch.zeros(L, dtype=torch.bool), True, "0.9", None):
            with pytest.raises(ValueError, match="level must be"):
                dense.crossings(bad, 0.02, 0.21)
        for bad in (torch.zeros(L + 1, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(2, B, L, dtype=F64)):
            with pytest.raises(ValueError, match="does not broadcast"):
                dense.time_above(bad, 0.02, 0.21)
        t = torch.tensor(0.1, dtype=F64, requires_grad=True)
        lev = torch.tensor(0.9, dtype=F64, requires_grad=True)
        for call in (lambda: dense.crossings(0.9, t, 0.2), lambda: dense.time_above(0.9, 0.0, t),
                     lambda: dense.crossings(lev, 0.0, 0.2), lambda: dense.time_above(lev, 0.0, 0.2)):
            with pytest.raises(NotImplementedError, match="does not propagate gradients"):
                call()
        with torch.no_grad():
            assert _same(dense.crossings(lev, 0.02, shared), wide)
        assert dense._prefix is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_out_of_range(backend, device_driver, dtype, monkeypatch):
    """`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives count -1 and NaN for the whole
    row of such a query, leaves the others alone and reads nothing from the device."""
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
        with pytest.raises(ValueError, match=r"dense.crossings\(level, ta, tb\): query 1 of row 3 \(ta = .*outside the row's interval"):
            dense.crossings(0.9, bad, bad.flip(0))
        with pytest.raises(ValueError, match=r"query 0 of row 0 \(tb = "):
            dense.time_above(0.9, good, bad.flip(0))
        want = dense.crossings(0.9, good, other)
        with monkeypatch.context() as m:
            def no_read(*a, **k):
                raise AssertionError("check=False read from the device")
            if backend == "oracle":
                m.setattr(torch.Tensor, "tolist", no_read)
            first, second = dense.crossings(0.9, bad, other, check=False), dense.crossings(0.9, other, bad, check=False)
            above = dense.time_above(0.9, bad, other, check=False)
        assert same_bits(above, first.time_above)
        for got in (first, second):
            assert bool((got.count[mask] == -1).all()) and bool((got.count[~mask] >= 0).all())
            assert all(bool(torch.isnan(v[mask]).all()) for v in got[1:])
            assert all(same_bits(a[~mask], b[~mask]) for a, b in zip(got, want))
        with pytest.raises(ValueError, match="query 0 of row 0"):
            dense.crossings(0.9, float("nan"), 0.1)


def test_query_count_overflow(device_driver):
    """More than 2^31 - 2 windows in one call: refused before anything is allocated, as the other methods refuse it."""
    with device_driver():
        dense = _solved("oracle", F32)
        huge = torch.empty((2 ** 31) // B + 1, B, dtype=F64, device="meta")
        twin = copy.copy(dense)
        twin._query_lists = lambda what, names, ts: ([huge, huge], False)
        for call in (lambda: twin.crossings(0.9, 0.0, 0.1), lambda: twin.time_above(0.9, 0.0, 0.1)):
            with pytest.raises(ValueError, match="the query index is a 32-bit word"):
                call()


# -- 6. the entry point refuses bad arguments before any launch -----------------------------------------------------------------------
def test_abi_33_argument_errors():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION >= 33
    assert "tdeq_row_dense_level" in _native.ABI_SIGNATURES and tda.RowDenseCrossings is RowDenseCrossings
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(count=p, first=p, last=p, time_above=p, level=p, n_rows=1, coeffs=p, n_seg=2, seg_ta=p, seg_tb=p, sign=1.0, seg=p,
              x=p, tq=p, seg2=p, x2=p, tq2=p, n_idx=1, row_len=3, dtype=_native.dtype_code(F64))

    def call(**kw):
        a = {**ok, **kw}
        return lib.tdeq_row_dense_level(a["count"], a["first"], a["last"], a["time_above"], a["level"], a["n_rows"], a["coeffs"],
                                        a["n_seg"], a["seg_ta"], a["seg_tb"], a["sign"], a["seg"], a["x"], a["tq"], a["seg2"],
                                        a["x2"], a["tq2"], a["n_idx"], a["row_len"], a["dtype"], None)
    for name in ("count", "first", "last", "time_above", "level", "coeffs", "seg_ta", "seg_tb", "seg", "x", "tq", "seg2", "x2",
                 "tq2"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(sign=0.0), dict(sign=2.0), dict(sign=float("nan")), dict(n_idx=-1), dict(n_rows=0), dict(n_rows=-1),
               dict(n_rows=2, n_idx=3), dict(n_rows=4, n_idx=2), dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31),
               dict(row_len=-3), dict(dtype=7), dict(dtype=_native.TDEQ_BF16)):
        assert call(**kw) == EINVAL, kw
    assert call(n_idx=0) == 0 and call(n_idx=0, n_rows=0) == 0 and call(row_len=0, dtype=_native.dtype_code(F32)) == 0
