"""`RowDenseOutput.maximum` / `.minimum` without a GPU: the host path against the numpy-scalar oracle and the device driver on the
oracle, bit for bit; the exact-rational bound of tests/_rowwise_dense_extremum_oracle.py; interior extrema of oscillators
against cos(w t); dose times; direction, compaction, the query forms and the errors; the entry point's argument checks."""
import contextlib
import copy
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_extremum_oracle import (MAXIMUM, MINIMUM, NP_T, U_T, device_driver, exact_window_check,  # noqa: F401
                                            oracle_extremum, oscillator_problem, same_bits)
from _rowwise_dense_extremum_oracle import windows as _windows
from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native
from torchdiffeq_amd.rowwise_dense import RowDenseExtremum

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
WHICH = [pytest.param(MAXIMUM, id="max"), pytest.param(MINIMUM, id="min")]
B, L, SEED = 5, 3, 3
OSC_B, OSC_L = 4, 6
EINVAL = -1


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


def _fn(dense, which):
    return dense.maximum if which == MAXIMUM else dense.minimum


# -- 1. the bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("problem", ["decay", "oscillator"])
def test_host_oracle_and_device_driver_agree_bit_for_bit(device_driver, problem, which, dtype):
    host = _solved("host", dtype, problem)
    qa, qb = _windows(host)
    got = _fn(host, which)(qa, qb)
    assert isinstance(got, RowDenseExtremum) and got.values.dtype == dtype and got.times.dtype == F64
    assert got.values.shape == got.times.shape == (8, *host._shape)
    want_v, want_t, _, _ = oracle_extremum(host, which, qa, qb)
    assert same_bits(got.values, want_v) and same_bits(got.times, want_t)
    assert not bool(torch.isnan(got.values).any()) and not bool(torch.isnan(got.times).any())
    with device_driver():
        dev = _solved("oracle", dtype, problem)                              # (its fp64 step sequence is not the host's)
        da, db = _windows(dev)
        on_dev = _fn(dev, which)(da, db)
    dev_v, dev_t, _, _ = oracle_extremum(dev, which, da, db)
    assert same_bits(on_dev.values, dev_v) and same_bits(on_dev.times, dev_t)
    twin = copy.copy(host)                                                   # the device driver on the HOST's record
    twin._k = dev._k
    again = _fn(twin, which)(qa, qb)
    assert same_bits(again.values, got.values) and same_bits(again.times, got.times)
    assert host._prefix is None and twin._prefix is None                     # the prefix store is not touched


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_rational_bound(dtype):
    """Windows over three to four steps of every oscillator row (clipped at both ends), and the whole of the shortest row of
    the decay problem: the exact p at 257 points of every segment against the exact p(x*), the bound derived in the oracle
    module's docstring."""
    worst = [Fraction(0), Fraction(0)]
    for problem in ("oscillator", "decay"):
        dense = _solved("host", dtype, problem)
        off = dense.offsets.tolist()
        n_rows = dense.t0.numel()
        mid = lambda s, u: dense.seg_start[s] + u * (dense.seg_end[s] - dense.seg_start[s])  # noqa: E731
        pick = [off[r] + (off[r + 1] - off[r]) // 2 for r in range(n_rows)]
        qa = torch.stack([mid(s, 0.3) for s in pick])[None]
        qb = torch.stack([mid(min(s + 3, off[r + 1] - 1), 0.6) for r, s in enumerate(pick)])[None]
        qb = torch.minimum(qb, dense.t1[None])                               # (a row's last step may end beyond t1)
        if problem == "decay":
            qa, qb = torch.cat([qa, dense.t0[None]]), torch.cat([qb, dense.t1[None]])
        for which in (MAXIMUM, MINIMUM):
            got = _fn(dense, which)(qa, qb)
            _, _, where, xs = oracle_extremum(dense, which, qa, qb)
            for j in range(qa.shape[0]):
                for r in range(n_rows if j == 0 else 1):
                    w = exact_window_check(dense, which, r, qa[j, r], qb[j, r], got.values[j, r], where[j, r], xs[j, r])
                    worst = [max(a, b) for a, b in zip(worst, w)]
    print("largest excess / bound {:.3g}, largest value error / bound {:.3g}".format(*map(float, worst)))


# -- 2. interior extrema ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_oscillator_interior_extrema_and_closed_form(dtype):
    dense = _solved("host", dtype, "oscillator")
    _, _, w, t1 = oscillator_problem(OSC_B, OSC_L, dtype)
    m = OSC_L // 2
    peak, trough = ((v[0], t[0]) for v, t in (dense.maximum(dense.t0[None], dense.t1[None]),
                                              dense.minimum(dense.t0[None], dense.t1[None])))
    peak, trough = RowDenseExtremum(*peak), RowDenseExtremum(*trough)
    interior = 0
    for which in (MAXIMUM, MINIMUM):
        _, _, where, xs = oracle_extremum(dense, which, dense.t0[None], dense.t1[None])
        interior += int(where[0, ..., 1].sum())
        assert bool(((xs[0] > 0) & (xs[0] < 1))[where[0, ..., 1] == 1].all())
    print(f"reported extrema of whole-row windows inside a segment: {interior} of {2 * OSC_B * OSC_L}")
    assert interior >= 20
    # the record's own error against cos(w t) on 2049 points per row is the margin
    grid = torch.linspace(0, 1, 2049, dtype=F64)[:, None] * t1[None]
    eps = (dense(grid)[:, :, :m].double() - torch.cos(w[None] * grid[:, :, None])).abs().amax(dim=0)      # [B, m]
    full = w * t1[:, None] >= 2 * np.pi                                      # the window holds a full period
    assert int(full.sum()) >= OSC_B * m // 2
    up, down = (peak.values[:, :m].double() - 1).abs(), (trough.values[:, :m].double() + 1).abs()
    print("largest |max - 1| / eps {:.3g}, |min + 1| / eps {:.3g}".format(float((up / eps)[full].max()),
                                                                         float((down / eps)[full].max())))
    assert bool((up <= eps)[full].all()) and bool((down <= eps)[full].all())
    # the times are the multiples of pi / w: to the interpolant's accuracy (|q''| = w^2 at a peak turns eps into sqrt-sized time
    # errors, hence the loose figure — a sanity check of the time, not of its rounding)
    odd = (trough.times[:, :m] * w / np.pi - 1) % 2                          # 0 (or 2) at an odd multiple of pi / w
    assert float(torch.minimum(odd, 2 - odd)[full].max()) < 1e-2


# -- 3. dose times ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_dose_times(backend, device_driver, dtype):
    """One positive dose per row at p = 0.4 t1 (the state decays everywhere else): p inside the window or at its near end
    contributes the RIGHT limit at time p; at the far end it does not; `maximum(p, p)` is the left limit."""
    t1 = per_row_t1(B)
    p = (0.4 * t1)[None]
    dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64).to(dtype)
    before, after = (0.35 * t1)[None], (0.6 * t1)[None]
    with _backend(backend, device_driver):
        dense = _solve(dtype, options={"jump_t": p, "jump_dy": dy})
        at_p = dense(p)
        inside, near = dense.maximum(before, after), dense.maximum(p, after)
        far_max, far_min, point = dense.maximum(before, p), dense.minimum(before, p), dense.maximum(p, p)
        low = dense.minimum(before, after)
        start = dense(before)
    off = dense.offsets.tolist()
    for got in (inside, near):
        assert bool((got.values > at_p).all()) and torch.equal(got.times, p[:, :, None].expand(1, B, L))
        assert float((got.values - at_p - dy).abs().max()) < (1e-4 if dtype == F32 else 1e-10)      # the state with the impulse
    assert same_bits(inside.values, near.values)
    # the far end: the window is the decaying branch before the dose, whose largest value is at its start
    assert torch.equal(far_max.times, before[:, :, None].expand(1, B, L)) and bool((far_max.values < at_p + 0.5 * dy).all())
    assert torch.equal(far_min.times, p[:, :, None].expand(1, B, L))
    assert same_bits(far_min.values, point.values) and torch.equal(point.times, far_min.times)
    assert float((far_max.values - start).abs().max()) <= (1e-5 if dtype == F32 else 1e-13)
    # the trough of the window that holds the dose is the left limit at p or the window's far end, never the right limit
    assert bool((low.values <= point.values).all())
    # maximum(p, p): the fp64 Horner form of the EARLIER segment at x = 1 rounded once — e + 1 * (d + 1 * (c + 1 * (b + 1 * a)))
    # — against dense(p), the T form e + d + c + b + a (4 additions in T): within 5 u_T (|e| + |d| + |c| + |b| + |a|)
    q = dense.coeffs.numpy()
    for r in range(B):
        s = next(s for s in range(off[r], off[r + 1]) if float(dense.seg_end[s]) == float(p[0, r]))
        e, d, c, b, a = (q[k, s].astype(np.float64) for k in range(5))
        want = (e + 1.0 * (d + 1.0 * (c + 1.0 * (b + 1.0 * a)))).astype(NP_T[dtype])
        assert same_bits(point.values[0, r], torch.from_numpy(want))
        slack = 5 * float(U_T[dtype]) * np.abs(q[:, s].astype(np.float64)).sum(axis=0)
        assert bool((np.abs(point.values[0, r].double().numpy() - at_p[0, r].double().numpy()) <= slack).all())
        assert float(dense.seg_start[s + 1]) == float(p[0, r])


# -- 4. the interface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_query_forms_and_order(backend, device_driver, dtype):
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)                                # inside every row's interval
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype)
        per_row = shared[:, None].expand(-1, B).contiguous()
        for fn in (dense.maximum, dense.minimum):
            both = fn(shared, per_row.flip(0))                                                # [Q] against [Q, B]
            assert both.values.shape == both.times.shape == (4, B, L)
            for a, b in zip(both, fn(per_row, per_row.flip(0))):
                assert same_bits(a, b)
            for a, b in zip(both, fn(per_row.flip(0), shared)):                               # the order of the ends
                assert same_bits(a, b)
            wide = fn(0.02, shared)                                                           # a number broadcasts
            assert wide.values.shape == (4, B, L) and same_bits(wide.values[1], wide.values[3])
            for a, b in zip(wide, fn(shared, torch.tensor(0.02, dtype=F64))):
                assert same_bits(a, b)
            one = fn(0.02, 0.21)
            assert one.values.shape == one.times.shape == (B, L)
            assert same_bits(one.values, wide.values[0]) and same_bits(one.times, wide.times[0])
            none = fn(torch.empty(0, dtype=F64), 0.1)
            assert none.values.shape == none.times.shape == (0, B, L) and none.times.dtype == F64
            assert bool((fn(0.1, 0.1).times == 0.1).all()) and same_bits(fn(0.1, 0.1).values, dense.maximum(0.1, 0.1).values)
        assert bool((dense.maximum(0.02, shared).values >= dense.minimum(0.02, shared).values).all())
        # y decays: the peak of a window is at its earlier end, the trough at its later end
        assert bool((dense.maximum(0.29, 0.05).times == 0.05).all()) and bool((dense.minimum(0.29, 0.05).times == 0.29).all())
        with pytest.raises(ValueError, match="do not broadcast"):
            dense.maximum(shared, shared[:3])
        with pytest.raises(ValueError, match="must be a number"):
            dense.minimum(0.1, torch.zeros(2, B + 1, dtype=F64))
        t = torch.tensor(0.1, dtype=F64, requires_grad=True)
        for call in (lambda: dense.maximum(t, 0.2), lambda: dense.minimum(0.0, t)):
            with pytest.raises(NotImplementedError, match="does not propagate gradients"):
                call()
        assert dense._prefix is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("problem", ["decay", "oscillator"])
def test_minimum_is_minus_maximum_of_the_negated_record(problem, dtype):
    """Bit for bit, but for the sign of a zero VALUE: e + x * (...) of a zero e at x = 0 is +0 unless both terms are -0, in
    the record and in its negation alike (the oscillators' velocities start at exactly 0) — hence the `+ 0.0`."""
    dense = _solved("host", dtype, problem)
    qa, qb = _windows(dense, seed=5)
    mirror = copy.copy(dense)
    mirror.coeffs = -dense.coeffs
    for lo, hi in ((dense.minimum(qa, qb), mirror.maximum(qa, qb)), (mirror.minimum(qa, qb), dense.maximum(qa, qb))):
        assert same_bits(lo.values + 0.0, -hi.values + 0.0) and same_bits(lo.times, hi.times)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", WHICH)
def test_descending_solve(device_driver, which, dtype):
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
    dense = _solve(dtype, t0=0.3, t1=t1)
    assert dense._sign == -1.0 and bool((dense.seg_end < dense.seg_start).all())
    qa, qb = _windows(dense, seed=3)
    got = _fn(dense, which)(qa, qb)
    want_v, want_t, _, _ = oracle_extremum(dense, which, qa, qb)
    assert same_bits(got.values, want_v) and same_bits(got.times, want_t)
    with device_driver():
        dev = _solve(dtype, t0=0.3, t1=t1)
        da, db = _windows(dev, seed=3)
        on_dev = _fn(dev, which)(da, db)
    dev_v, dev_t, _, _ = oracle_extremum(dev, which, da, db)
    assert same_bits(on_dev.values, dev_v) and same_bits(on_dev.times, dev_t)
    # y grows as t runs down: over the whole row the peak is at t1 (the smaller time), the trough at t0, in TRUE time
    whole = _fn(dense, which)(dense.t0[None], dense.t1[None])
    end = (dense.t1 if which == MAXIMUM else dense.t0)[None, :, None].expand(1, B, L)
    assert torch.equal(whole.times, end)
    lo, hi = torch.minimum(qa, qb)[:, :, None], torch.maximum(qa, qb)[:, :, None]
    assert bool(((got.times >= lo) & (got.times <= hi)).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_compact_gives_the_same_bits(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        plain = _solved(backend, dtype)
        packed = _solve(dtype, compact=True)
        qa, qb = _windows(plain, seed=13)
        for name in ("maximum", "minimum"):
            for a, b in zip(getattr(packed, name)(qa, qb), getattr(plain, name)(qa, qb)):
                assert same_bits(a, b), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_out_of_range(backend, device_driver, dtype, monkeypatch):
    """`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives NaN rows in both outputs, leaves
    the others alone and reads nothing from the device."""
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
        for name in ("maximum", "minimum"):
            fn = getattr(dense, name)
            with pytest.raises(ValueError, match=rf"dense.{name}\(ta, tb\): query 1 of row 3 \(ta = .*outside the row's interval"):
                fn(bad, bad.flip(0))
            with pytest.raises(ValueError, match=r"query 0 of row 0 \(tb = "):
                fn(good, bad.flip(0))
            want = fn(good, other)
            with monkeypatch.context() as m:
                def no_read(*a, **k):
                    raise AssertionError("check=False read from the device")
                if backend == "oracle":
                    m.setattr(torch.Tensor, "tolist", no_read)
                first, second = fn(bad, other, check=False), fn(other, bad, check=False)
            for got in (first, second):
                for a, b in zip(got, want):
                    assert bool(torch.isnan(a[mask]).all()) and same_bits(a[~mask], b[~mask])
        with pytest.raises(ValueError, match="query 0 of row 0"):
            dense.maximum(float("nan"), 0.1)


def test_query_count_overflow(device_driver):
    """More than 2^31 - 2 windows in one call: refused before anything is allocated, as the other methods refuse it."""
    with device_driver():
        dense = _solved("oracle", F32)
        huge = torch.empty((2 ** 31) // B + 1, B, dtype=F64, device="meta")
        twin = copy.copy(dense)
        twin._query_lists = lambda what, names, ts: ([huge, huge], False)
        for fn in (twin.maximum, twin.minimum):
            with pytest.raises(ValueError, match="the query index is a 32-bit word"):
                fn(0.0, 0.1)


# -- 5. the entry point refuses bad arguments before any launch -----------------------------------------------------------------------
def test_abi_32_argument_errors():
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION >= 32
    assert "tdeq_row_dense_extremum" in _native.ABI_SIGNATURES
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(values=p, times=p, which=0, coeffs=p, n_seg=2, seg_ta=p, seg_tb=p, sign=1.0, seg=p, x=p, tq=p, seg2=p, x2=p,
              tq2=p, n_idx=1, row_len=3, dtype=_native.dtype_code(F64))

    def call(**kw):
        a = {**ok, **kw}
        return lib.tdeq_row_dense_extremum(a["values"], a["times"], a["which"], a["coeffs"], a["n_seg"], a["seg_ta"],
                                           a["seg_tb"], a["sign"], a["seg"], a["x"], a["tq"], a["seg2"], a["x2"], a["tq2"],
                                           a["n_idx"], a["row_len"], a["dtype"], None)
    for name in ("values", "times", "coeffs", "seg_ta", "seg_tb", "seg", "x", "tq", "seg2", "x2", "tq2"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(which=2), dict(which=-1), dict(sign=0.0), dict(sign=2.0), dict(sign=float("nan")), dict(n_idx=-1),
               dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31), dict(row_len=-3), dict(dtype=7),
               dict(dtype=_native.TDEQ_BF16)):
        assert call(**kw) == EINVAL, kw
    for which in (0, 1):
        assert call(n_idx=0, which=which) == 0 and call(row_len=0, which=which, dtype=_native.dtype_code(F32)) == 0
