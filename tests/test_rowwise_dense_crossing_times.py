"""`RowDenseOutput.crossing_times` without a GPU: the host path against the numpy-scalar oracle and the device driver on the
oracle, bit for bit; the identities with `crossings` on the same record; the harmonic problem against the closed form of
cos(w t) = 0.3, ascending and descending; dose times; compaction, the query forms, the level's forms, `max_count` and the
errors; the entry point's argument checks."""
import contextlib
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from _rowwise_dense_crossing_times_oracle import (HARMONIC_BOUND, HARMONIC_LEVEL, HARMONIC_TOL, check_identities,  # noqa: F401
                                                  device_driver, harmonic_distance, harmonic_problem, oracle_crossing_times,
                                                  same_bits)
from _rowwise_dense_extremum_oracle import oscillator_problem
from _rowwise_dense_extremum_oracle import windows as _windows
from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native
from torchdiffeq_amd.rowwise_dense import RowDenseCrossingTimes

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, L, SEED = 5, 3, 3
OSC_B, OSC_L = 4, 5
HARM_B, HARM_P = 5, 2
EINVAL = -1


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _solve(dtype, t0=0.0, t1=None, **kw):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, per_row_t1(B) if t1 is None else t1, method="dopri5",
                                        **{**tolerances("dopri5", dtype), **kw})


def _solve_harmonic(dtype, descending=False, tol=None):
    y0, func, _, t1 = harmonic_problem(HARM_B, HARM_P, True, dtype)
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, 0.0, -t1 if descending else t1, method="dopri5",
                                        **(HARMONIC_TOL[dtype] if tol is None else tol))


@functools.lru_cache(maxsize=None)
def _solved(backend, dtype, problem="decay"):
    """One solve per (backend, dtype, problem), shared by the tests that only evaluate it; called inside the backend's context.
    `harmonic` here is a short coarse solve (t1 / 2 at 1e-4): the tests of the bits walk it with the scalar oracle."""
    if problem == "decay":
        return _solve(dtype)
    if problem == "oscillator":
        y0, func, _, t1 = oscillator_problem(OSC_B, OSC_L, dtype)
    else:
        y0, func, _, t1 = harmonic_problem(HARM_B, HARM_P, True, dtype)
        t1 = t1 / 2
    tol = dict(rtol=1e-4, atol=1e-4) if problem == "harmonic" else tolerances("dopri5", dtype)
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", **tol)


def _levels(dense, problem):
    """A scalar level and a [B, L] level (one per row times one per element) that the elements pass."""
    n_rows, width = dense._shape
    scalar, lo, hi = {"decay": (0.9, 0.1, 1.2), "oscillator": (0.5, -0.9, 0.9), "harmonic": (HARMONIC_LEVEL, -0.9, 0.9)}[problem]
    return {"scalar": scalar,
            "per_element": torch.linspace(0.5, 1.0, n_rows, dtype=F64)[:, None] * torch.linspace(lo, hi, width, dtype=F64)}


def _same(got, want):
    return all(same_bits(a, b) for a, b in zip(got, want))


def _well_formed(got, K, shape):
    """Types, shapes, and the padding rule: slot j of a list is NaN exactly from min(n, K) on (all NaN where n = -1)."""
    assert isinstance(got, RowDenseCrossingTimes)
    assert got.n_rising.dtype == got.n_falling.dtype == torch.int32 and got.rising.dtype == got.falling.dtype == F64
    assert got.n_rising.shape == got.n_falling.shape == shape and got.rising.shape == got.falling.shape == (K, *shape)
    slot = torch.arange(K).view(K, *([1] * len(shape)))
    for n, times in ((got.n_rising, got.rising), (got.n_falling, got.falling)):
        assert torch.equal(torch.isnan(times), slot >= n.clamp(min=0, max=K)[None])
    assert torch.equal(got.n_rising == -1, got.n_falling == -1)


# -- 1. the bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("problem", ["decay", "oscillator", "harmonic"])
def test_host_oracle_and_device_driver_agree_bit_for_bit(device_driver, problem, dtype):
    host = _solved("host", dtype, problem)
    qa, qb = _windows(host)
    qa, qb = torch.cat([qa, host.t0[None]]), torch.cat([qb, host.t1[None]])
    with device_driver():
        dev = _solved("oracle", dtype, problem)                              # (its fp64 step sequence is not the host's)
        da, db = _windows(dev)
    twin = copy.copy(host)                                                   # the device driver on the HOST's record
    twin._k = dev._k
    crossed = overflowed = 0
    for name, level in _levels(host, problem).items():
        want16 = oracle_crossing_times(host, level, qa, qb, 16)
        for K in (1, 4, 16):
            got = host.crossing_times(level, qa, qb, max_count=K)
            _well_formed(got, K, (9, *host._shape))
            want = want16 if K == 16 else oracle_crossing_times(host, level, qa, qb, K)
            assert _same(got, want), (name, K)
            assert _same(got[2:], [v[:K] for v in want16[2:]]) and _same(got[:2], want16[:2])     # the first K, all counted
            assert bool((got.n_rising >= 0).all())
            crossed += int((got.n_rising > 0).sum()) + int((got.n_falling > 0).sum())
            overflowed += int((got.n_rising > K).sum()) + int((got.n_falling > K).sum())
            if K != 4:
                continue
            with device_driver():
                assert _same(twin.crossing_times(level, qa, qb, max_count=K), got), name
    assert crossed > 0 and (overflowed > 0 or problem == "decay")            # (a decaying element passes a level once)
    with device_driver():
        for name, level in _levels(dev, problem).items():
            on_dev = dev.crossing_times(level, da, db)
            _well_formed(on_dev, 4, (8, *dev._shape))
            assert _same(on_dev, oracle_crossing_times(dev, level, da, db, 4)), name
    assert host._prefix is None and twin._prefix is None and dev._prefix is None      # nothing is built


# -- 2. identities with `crossings` ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
@pytest.mark.parametrize("problem", ["decay", "oscillator", "harmonic"])
def test_identities_with_crossings(problem, backend, device_driver, dtype):
    rebuilt = 0
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, problem)
        qa, qb = _windows(dense, seed=5)
        for level in _levels(dense, problem).values():
            fwd, rev = dense.crossing_times(level, qa, qb), dense.crossing_times(level, qb, qa)
            assert _same(fwd, rev)                                           # the order of the ends
            rebuilt += check_identities(fwd, dense.crossings(level, qa, qb), qa, qb, dense._sign, 4)
        assert dense._prefix is None
    assert rebuilt > 0


# -- 3. the closed form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_harmonic_closed_forms(descending, backend, device_driver, dtype):
    """Every cos(w t) element against level 0.3 on the whole row, max_count = 4: the counts are exact, and every listed time is
    within HARMONIC_BOUND of the closed form (see the constants).  A solve from 0 to -t1 walks the mirrored times in decreasing
    true time, and what falls for increasing solver time rises in true time."""
    K = 4
    with _backend(backend, device_driver):
        dense = _solve_harmonic(dtype, descending)
        got = dense.crossing_times(HARMONIC_LEVEL, dense.t0[None], dense.t1[None], max_count=K)
        ref = dense.crossings(HARMONIC_LEVEL, dense.t0[None], dense.t1[None])
    got = RowDenseCrossingTimes(got.n_rising[0], got.n_falling[0], got.rising[:, 0], got.falling[:, 0])
    assert dense._sign == (-1.0 if descending else 1.0)
    _, _, w, t1 = harmonic_problem(HARM_B, HARM_P, True, dtype)
    _well_formed(got, K, (HARM_B, 2 * HARM_P + 1))
    assert torch.equal(got.n_rising + got.n_falling, ref.count[0])
    worst, fit, overflow = harmonic_distance(got, w, t1, descending, K)
    print(f"largest distance from the closed form {worst:.3g} (bound {HARMONIC_BOUND[dtype]:.3g}); {fit} lists fit, "
          f"{overflow} overflow")
    assert fit > 0 and overflow > 0
    assert worst <= HARMONIC_BOUND[dtype]


# -- 4. dose times ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_dose_times(backend, device_driver, dtype):
    """One positive dose per row at p = 0.4 t1 (the state decays everywhere else) and a level halfway up the dose: a window
    that holds p, or starts at p, has the dose in `rising` AT p, bit for bit; a window that ends at p does not see it."""
    t1 = per_row_t1(B)
    p = (0.4 * t1)[None]
    dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64).to(dtype)
    before, after = (0.35 * t1)[None], (0.6 * t1)[None]
    with _backend(backend, device_driver):
        dense = _solve(dtype, options={"jump_t": p, "jump_dy": dy})
        level = (dense(p) + 0.5 * dy)[0]                                     # between the left and the right limit at p
        assert bool((dense(before)[0] < level).all())                        # the window starts below the level
        inside, near = dense.crossing_times(level, before, after), dense.crossing_times(level, p, after)
        far, point = dense.crossing_times(level, before, p), dense.crossing_times(level, p, p)
        ends_above = dense(after)[0] > level
    at_p = p[:, :, None].expand(1, B, L)
    for got in (inside, near):
        _well_formed(got, 4, (1, B, L))
        assert bool((got.n_rising == 1).all()) and torch.equal(got.rising[0], at_p)      # the stored dose time
        assert torch.equal(got.n_falling[0], (~ends_above).to(torch.int32))
        assert bool((got.falling[0, 0][~ends_above] > at_p[0][~ends_above]).all())
    assert _same(inside, near)
    for got in (far, point):                                                 # the far end: only the left limit at p
        assert bool((got.n_rising == 0).all()) and bool((got.n_falling == 0).all())
        assert bool(torch.isnan(got.rising).all()) and bool(torch.isnan(got.falling).all())


# -- 5. compaction -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_compact_gives_the_same_bits(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        plain = _solved(backend, dtype)
        packed = _solve(dtype, compact=True)
        qa, qb = _windows(plain, seed=13)
        for name, level in _levels(plain, "decay").items():
            assert _same(packed.crossing_times(level, qa, qb), plain.crossing_times(level, qa, qb)), name


# -- 6. the interface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_query_and_level_forms(backend, device_driver, dtype):
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)                                # inside every row's interval
    K = 4
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype)
        per_row = shared[:, None].expand(-1, B).contiguous()
        both = dense.crossing_times(0.9, shared, per_row.flip(0))                             # [Q] against [Q, B]
        _well_formed(both, K, (4, B, L))
        assert _same(both, dense.crossing_times(0.9, per_row, per_row.flip(0)))
        wide = dense.crossing_times(0.9, 0.02, shared)                                        # a number broadcasts
        assert _same(wide, dense.crossing_times(0.9, shared, torch.tensor(0.02, dtype=F64)))
        one = dense.crossing_times(0.9, 0.02, 0.21)
        _well_formed(one, K, (B, L))
        assert _same(one, [wide[0][0], wide[1][0], wide[2][:, 0], wide[3][:, 0]])
        assert dense.crossing_times(0.9, 0.02, 0.21, max_count=2).rising.shape == (2, B, L)
        none = dense.crossing_times(0.9, torch.empty(0, dtype=F64), 0.1)
        _well_formed(none, K, (0, B, L))
        # the forms of the level: a number, 0-dim, [L], [B, 1], [B, L], an integer tensor, another float dtype
        full = torch.full((B, L), 0.9, dtype=F64)
        for level in (torch.tensor(0.9, dtype=F64), full, full[:, :1], full[0], full.to(dtype)):
            assert _same(dense.crossing_times(level, 0.02, shared), wide)
        assert _same(dense.crossing_times(1, 0.02, shared), dense.crossing_times(torch.ones(L, dtype=torch.int64), 0.02, shared))
        rows = torch.linspace(0.5, 1.5, B, dtype=F64)[:, None]                                # one level per row
        split = dense.crossing_times(rows, 0.02, shared)
        for r in range(B):
            assert _same([v[..., r, :] for v in split], [v[..., r, :] for v in dense.crossing_times(float(rows[r]), 0.02, shared)])
        # a NaN level: that element alone
        holed = full.clone()
        holed[1, 2] = holed[4, 0] = float("nan")
        mask = torch.isnan(holed)[None].expand(4, B, L)
        got = dense.crossing_times(holed, 0.02, shared)
        _well_formed(got, K, (4, B, L))
        assert bool((got.n_rising[mask] == -1).all()) and bool((got.n_falling[mask] == -1).all())
        assert bool(torch.isnan(got.rising[:, mask]).all()) and bool(torch.isnan(got.falling[:, mask]).all())
        assert all(same_bits(a[..., ~mask], b[..., ~mask]) for a, b in zip(got, wide))
        # refusals
        with pytest.raises(ValueError, match="do not broadcast"):
            dense.crossing_times(0.9, shared, shared[:3])
        with pytest.raises(ValueError, match="must be a number"):
            dense.crossing_times(0.9, 0.1, torch.zeros(2, B + 1, dtype=F64))
        for bad in (torch.zeros(B, L, dtype=torch.complex64), torch.zeros(L, dtype=torch.bool), True, "0.9", None):
            with pytest.raises(ValueError, match="level must be"):
                dense.crossing_times(bad, 0.02, 0.21)
        for bad in (torch.zeros(L + 1, dtype=F64), torch.zeros(B, dtype=F64), torch.zeros(2, B, L, dtype=F64)):
            with pytest.raises(ValueError, match="does not broadcast"):
                dense.crossing_times(bad, 0.02, 0.21)
        t = torch.tensor(0.1, dtype=F64, requires_grad=True)
        lev = torch.tensor(0.9, dtype=F64, requires_grad=True)
        for call in (lambda: dense.crossing_times(0.9, t, 0.2), lambda: dense.crossing_times(0.9, 0.0, t),
                     lambda: dense.crossing_times(lev, 0.0, 0.2)):
            with pytest.raises(NotImplementedError, match="does not propagate gradients"):
                call()
        with torch.no_grad():
            assert _same(dense.crossing_times(lev, 0.02, shared), wide)
        assert dense._prefix is None


# -- 7. max_count ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_max_count_validation(backend, device_driver):
    with _backend(backend, device_driver):
        dense = _solved(backend, F64)
        for bad in (0, -1, 65536, True, False, 4.0, "4", None, torch.tensor(4), np.int64(4)):
            with pytest.raises(ValueError, match=r"max_count must be an int in \[1, 65535\]"):
                dense.crossing_times(0.9, 0.02, 0.21, max_count=bad)
        assert dense.crossing_times(0.9, 0.02, 0.21, max_count=1).falling.shape == (1, B, L)
    assert _solved("host", F64).crossing_times(0.9, torch.empty(0, dtype=F64), 0.1, max_count=65535).rising.shape == (65535, 0, B, L)


# -- 8. out-of-range ends ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_out_of_range(backend, device_driver, dtype, monkeypatch):
    """`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives -1 and NaN for the whole row of
    such a query, leaves the others alone and reads nothing from the device."""
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
        with pytest.raises(ValueError,
                           match=r"dense.crossing_times\(level, ta, tb\): query 1 of row 3 \(ta = .*outside the row's interval"):
            dense.crossing_times(0.9, bad, bad.flip(0))
        with pytest.raises(ValueError, match=r"query 0 of row 0 \(tb = "):
            dense.crossing_times(0.9, good, bad.flip(0))
        want = dense.crossing_times(0.9, good, other)
        with monkeypatch.context() as m:
            def no_read(*a, **k):
                raise AssertionError("check=False read from the device")
            if backend == "oracle":
                m.setattr(torch.Tensor, "tolist", no_read)
            first = dense.crossing_times(0.9, bad, other, check=False)
            second = dense.crossing_times(0.9, other, bad, check=False)
        for got in (first, second):
            _well_formed(got, 4, (3, B, L))
            for n in got[:2]:
                assert bool((n[mask] == -1).all()) and bool((n[~mask] >= 0).all())
            for times in got[2:]:
                assert bool(torch.isnan(times[:, mask]).all())
            assert all(same_bits(a[..., ~mask, :], b[..., ~mask, :]) for a, b in zip(got, want))
        with pytest.raises(ValueError, match="query 0 of row 0"):
            dense.crossing_times(0.9, float("nan"), 0.1)


# -- 9. the 32-bit query index ------------------------------------------------------------------------------------------------------------
def test_query_count_overflow(device_driver):
    """More than 2^31 - 2 windows in one call: refused before anything is allocated, as the other methods refuse it."""
    with device_driver():
        dense = _solved("oracle", F32)
        huge = torch.empty((2 ** 31) // B + 1, B, dtype=F64, device="meta")
        twin = copy.copy(dense)
        twin._query_lists = lambda what, names, ts: ([huge, huge], False)
        with pytest.raises(ValueError, match="the query index is a 32-bit word"):
            twin.crossing_times(0.9, 0.0, 0.1)


# -- 10. the entry point refuses bad arguments before any launch -----------------------------------------------------------------------
def test_abi_35_argument_errors():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION >= 35
    assert "tdeq_row_dense_level_times" in _native.ABI_SIGNATURES and tda.RowDenseCrossingTimes is RowDenseCrossingTimes
    assert "RowDenseCrossingTimes" in tda.__all__
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(n_rising=p, n_falling=p, rising=p, falling=p, max_count=4, level=p, n_rows=1, coeffs=p, n_seg=2, seg_ta=p, seg_tb=p,
              sign=1.0, seg=p, x=p, tq=p, seg2=p, x2=p, tq2=p, n_idx=1, row_len=3, dtype=_native.dtype_code(F64))

    def call(**kw):
        a = {**ok, **kw}
        return lib.tdeq_row_dense_level_times(a["n_rising"], a["n_falling"], a["rising"], a["falling"], a["max_count"], a["level"],
                                              a["n_rows"], a["coeffs"], a["n_seg"], a["seg_ta"], a["seg_tb"], a["sign"], a["seg"],
                                              a["x"], a["tq"], a["seg2"], a["x2"], a["tq2"], a["n_idx"], a["row_len"], a["dtype"],
                                              None)
    for name in ("n_rising", "n_falling", "rising", "falling", "level", "coeffs", "seg_ta", "seg_tb", "seg", "x", "tq", "seg2",
                 "x2", "tq2"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(max_count=0), dict(max_count=65536), dict(max_count=-4), dict(max_count=2 ** 40),
               dict(sign=0.0), dict(sign=2.0), dict(sign=float("nan")), dict(n_idx=-1), dict(n_rows=0), dict(n_rows=-1),
               dict(n_rows=2, n_idx=3), dict(n_rows=4, n_idx=2), dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31),
               dict(row_len=-3), dict(dtype=7), dict(dtype=_native.TDEQ_BF16)):
        assert call(**kw) == EINVAL, kw
    assert call(n_idx=0) == 0 and call(n_idx=0, n_rows=0) == 0 and call(row_len=0, dtype=_native.dtype_code(F32)) == 0
    assert call(n_idx=0, max_count=0) == EINVAL and call(row_len=0, max_count=65536) == EINVAL      # refusals come first
