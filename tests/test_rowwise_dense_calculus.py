"""`RowDenseOutput.derivative` / `.antiderivative` / `.integral` without a GPU: the host path against the numpy oracle and the
device driver on the oracle, bit for bit; the exact-rational bounds of tests/_rowwise_dense_calculus_oracle.py; breakpoints,
dose times, direction, compaction, row independence, the query forms, the errors and the prefix cache."""
import contextlib
import copy
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import (ANTIDERIVATIVE, DERIVATIVE, INTEGRAL, NP_T, antiderivative_bound,  # noqa: F401
                                            device_driver, exact_antiderivative, exact_derivative, np_calc, np_prefix,
                                            same_bits)
from _rowwise_dense_oracle import NONE, DenseOracle, decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
METHODS = ["dopri5", "bosh3"]                                # dopri5 plus one low-order method
B, L, SEED, Q = 5, 3, 3, 6
EINVAL = -1


def _backend(name, device_driver):
    return device_driver() if name == "oracle" else contextlib.nullcontext()


def _solve(dtype, method, t0=0.0, t1=None, B=B, rows=None, **kw):
    y0, func, _ = decay_problem(B, L, dtype, SEED)
    t1 = per_row_t1(B) if t1 is None else t1
    if rows is not None:                                                     # the one-row problems of the same batch
        full = func
        y0, t1 = y0[rows], (t1[rows] if isinstance(t1, torch.Tensor) else t1)
        t0 = t0[rows] if isinstance(t0, torch.Tensor) else t0
        func = lambda t, y, sub=None: full(t, y, torch.tensor(rows) if sub is None else torch.tensor(rows)[sub])  # noqa: E731
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, t1, method=method, **{**tolerances(method, dtype), **kw})


@functools.lru_cache(maxsize=None)
def _solved(backend, dtype, method):
    """One solve per (backend, dtype, method), shared by the tests that only evaluate it; called inside the backend's
    context (the object keeps the backend it was solved on)."""
    return _solve(dtype, method)


def _wire(dense):
    """The record as numpy arrays in SOLVER time, for the numpy oracle."""
    sign = dense._sign
    return (dense.coeffs.numpy(), dense.offsets.numpy(), (dense.seg_start * sign).numpy(), (dense.seg_end * sign).numpy(), sign)


def _oracle_all(dense, qa, qb):
    """The three operations from the numpy oracle for [Q, B] true-time queries `qa` (and `qb`, the integral's upper ends);
    the search is the torch oracle of tests/_rowwise_dense_oracle.py."""
    coeffs, off, ta, tb, sign = _wire(dense)
    P = np_prefix(coeffs, off, ta, tb)
    found = []
    for q in (qa, qb):
        n = q.numel()
        seg, x = torch.empty(n, dtype=torch.int32), torch.empty(n, dtype=dense.coeffs.dtype)
        status = torch.tensor([NONE], dtype=torch.int32)
        DenseOracle.row_dense_search((q * sign).contiguous(), dense.offsets, torch.from_numpy(ta), torch.from_numpy(tb),
                                     dense.t0 * sign, dense.t1 * sign, seg, x, status)
        found += [seg.numpy(), x.numpy(), (q * sign).numpy().reshape(-1)]
    shape = (qa.shape[0], *dense._shape)
    return tuple(torch.from_numpy(np_calc(mode, coeffs, P, ta, tb, sign, *found[:3 if mode != INTEGRAL else 6])).view(shape)
                 for mode in (DERIVATIVE, ANTIDERIVATIVE, INTEGRAL)) + (P,)


def _queries(dense, seed=11):
    """[Q + 3, B] true-time queries: random interior points (unsorted), t0, t1 and an interior breakpoint per row."""
    off = dense.offsets.tolist()
    rows = range(dense.t0.numel())
    brk = torch.stack([dense.seg_end[off[r] + (off[r + 1] - off[r]) // 2 - 1] if off[r + 1] - off[r] > 1 else dense.t1[r]
                       for r in rows])
    sign = dense._sign
    q = random_queries(Q, dense.t0 * sign, dense.t1 * sign, seed) * sign
    return torch.cat([q, dense.t0[None], dense.t1[None], brk[None]])


# -- 1. the bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_host_oracle_and_device_driver_agree_bit_for_bit(device_driver, method, dtype):
    host = _solved("host", dtype, method)
    qa = _queries(host)
    qb = qa[torch.randperm(qa.shape[0], generator=torch.Generator().manual_seed(4))]
    want_d, want_F, want_I, P = _oracle_all(host, qa, qb)
    got = host.derivative(qa), host.antiderivative(qa), host.integral(qa, qb)
    assert same_bits(host._prefix, torch.from_numpy(P))
    assert same_bits(got[0], want_d) and same_bits(got[1], want_F) and same_bits(got[2], want_I)
    with device_driver():
        dev = _solved("oracle", dtype, method)                               # (its fp64 step sequence is not the host's)
        da = _queries(dev)
        db = da.flip(0)
        on_dev = dev.derivative(da), dev.antiderivative(da), dev.integral(da, db)
    for a, b in zip(on_dev, _oracle_all(dev, da, db)[:3]):
        assert same_bits(a, b)
    assert same_bits(dev._prefix, torch.from_numpy(_oracle_all(dev, da, db)[3]))
    # the device driver on the HOST's record: the same bits as the host path
    twin = copy.copy(host)
    twin._k, twin._prefix = dev._k, None
    for a, b in zip((twin.derivative(qa), twin.antiderivative(qa), twin.integral(qa, qb)), got):
        assert same_bits(a, b)
    assert not bool(torch.isnan(torch.stack(got)).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_exact_rational_bounds(method, dtype):
    """Every element of the three results against `fractions.Fraction` from the wire format; the bounds are derived in the
    oracle module's docstring."""
    dense = _solved("host", dtype, method)
    q = _queries(dense, seed=5)
    qb = q.flip(0)
    dv, F, I = dense.derivative(q), dense.antiderivative(q), dense.integral(q, qb)
    seg, x, _ = dense._search_host((q * dense._sign).contiguous())
    worst = [Fraction(0)] * 3
    for j in range(q.shape[0]):
        for r in range(B):
            ex, A, n = exact_antiderivative(dense, r, q[j, r])
            ex_b, A_b, n_b = exact_antiderivative(dense, r, qb[j, r])
            dex, dbound = exact_derivative(dense, int(seg[j * B + r]), x[j * B + r])
            for k in range(L):
                bound = antiderivative_bound(dense, A[k], n, F[j, r, k])
                err = abs(Fraction(float(F[j, r, k])) - ex[k])
                assert err <= bound, (j, r, k, float(err), float(bound))
                # the integral: the two end bounds added (each with the end's own computed F)
                bound_i = bound + antiderivative_bound(dense, A_b[k], n_b, dense.antiderivative(qb[j:j + 1])[0, r, k])
                err_i = abs(Fraction(float(I[j, r, k])) - (ex_b[k] - ex[k]))
                assert err_i <= bound_i, (j, r, k, float(err_i), float(bound_i))
                err_d = abs(Fraction(float(dv[j, r, k])) - dex[k])
                assert err_d <= dbound[k], (j, r, k, float(err_d), float(dbound[k]))
                for i, (e, b) in enumerate(((err, bound), (err_i, bound_i), (err_d, dbound[k]))):
                    if b:
                        worst[i] = max(worst[i], e / b)
    print("largest error / bound: antiderivative {:.3g}, integral {:.3g}, derivative {:.3g}".format(*map(float, worst)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_closed_form(dtype):
    """Against the exact solution y0 exp(-k (t + t^2 / 2)): the derivative is -k (1 + t) y; the integrand of the
    antiderivative is checked through its own derivative, d/dt F = y (a central difference of F against dense(t))."""
    y0, _, k = decay_problem(B, L, dtype, SEED)
    dense = _solved("host", dtype, "dopri5")
    q = random_queries(4, dense.t0, dense.t1, seed=9)
    y = y0[None].double() * torch.exp(-k[None].double() * (q + q * q / 2)[:, :, None])
    want = -k[None].double() * (1 + q)[:, :, None] * y
    # a sanity check of the formula, not of its rounding: the interpolant's derivative is one order below the solution, whose
    # error the solve's mixed tolerance bounds relative to |y| + atol / rtol — hence the error relative to |want| + 1
    tol = 2e-3 if dtype == F32 else 1e-5
    assert float(((dense.derivative(q).double() - want).abs() / (want.abs() + 1)).max()) < tol
    if dtype == F64:
        h = 1e-5
        slope = (dense.antiderivative(q + h) - dense.antiderivative(q - h)) / (2 * h)
        assert float(((slope - dense(q)).abs() / (dense(q).abs() + 1)).max()) < 1e-6


# -- 2. breakpoints, ends, identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_ends_and_breakpoints(backend, device_driver, method, dtype):
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, method)
        off = dense.offsets.tolist()
        assert bool((dense.antiderivative(dense.t0[None]) == 0).all())                        # F(t0) == 0 exactly
        at_t1 = dense.antiderivative(dense.t1[None])                                          # t1 is valid
        assert not bool(torch.isnan(at_t1).any()) and not bool(torch.isnan(dense.derivative(dense.t1[None])).any())
        assert min(off[r + 1] - off[r] for r in range(B)) >= 3
        first_end = torch.stack([dense.seg_end[off[r]] for r in range(B)])[None]              # an interior seg_end per row
        d, F = dense.derivative(first_end)[0], dense.antiderivative(first_end)[0]
        P = dense._prefix
    T = NP_T[dtype]
    coeffs = dense.coeffs.numpy()
    for r in range(B):
        s = off[r]                                                                            # the EARLIER segment, x = 1
        one = np.ones(1, dtype=T)
        w = np_calc(DERIVATIVE, coeffs, None, dense.seg_start.numpy(), dense.seg_end.numpy(), 1.0, np.array([s]), one)
        later = np_calc(DERIVATIVE, coeffs, None, dense.seg_start.numpy(), dense.seg_end.numpy(), 1.0, np.array([s + 1]),
                        np.zeros(1, dtype=T))
        assert same_bits(d[r], torch.from_numpy(w[0]))
        assert not torch.equal(d[r], torch.from_numpy(later[0]))                              # (the right derivative differs)
        assert same_bits(F[r], (dense._sign * P[s + 1]).to(dtype))                            # T(sign * P[s + 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_integral_identities(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, "dopri5")
        a, b = _queries(dense, seed=21), _queries(dense, seed=22)
        ab, ba = dense.integral(a, b), dense.integral(b, a)
        assert same_bits(ab[:Q], -ba[:Q]) and bool((ab[:Q] != 0).all())                       # (distinct ends)
        assert torch.equal(ab, -ba) and bool((ab[Q:] == 0).all())                             # (the same ends: 0 both ways)
        assert bool((dense.integral(a, a) == 0).all())
        # (== : F64(t0) is a zero, whose sign the subtraction may change where F64(t) is a zero itself)
        assert torch.equal(dense.integral(dense.t0[None], a), dense.antiderivative(a))
        assert torch.equal(dense.integral(0.0, a), dense.antiderivative(a))                   # a number broadcasts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_row_independence(method, dtype):
    """Row r of the B-row object equals the one-row solve's object, bit for bit: the prefix is added in the same order."""
    dense = _solved("host", dtype, method)
    q = _queries(dense, seed=8)
    full = dense.derivative(q), dense.antiderivative(q), dense.integral(q, q.flip(0))
    for r in (0, B - 1):
        one = _solve(dtype, method, rows=[r])
        qr = q[:, r:r + 1]
        alone = one.derivative(qr), one.antiderivative(qr), one.integral(qr, qr.flip(0))
        for a, b in zip(alone, full):
            assert same_bits(a[:, 0], b[:, r])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_compact_gives_the_same_bits(backend, device_driver, dtype):
    with _backend(backend, device_driver):
        plain = _solved(backend, dtype, "dopri5")
        packed = _solve(dtype, "dopri5", compact=True)
        q = _queries(plain, seed=13)
        for name in ("derivative", "antiderivative"):
            assert same_bits(getattr(packed, name)(q), getattr(plain, name)(q)), name
        assert same_bits(packed.integral(q, q.flip(0)), plain.integral(q, q.flip(0)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_descending_solve(device_driver, method, dtype):
    """t1 < t0: the oracle's sign handling; the derivative and the integrals are with respect to TRUE time."""
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
    dense = _solve(dtype, method, t0=0.3, t1=t1)
    assert dense._sign == -1.0 and bool((dense.seg_end < dense.seg_start).all())
    qa = _queries(dense, seed=3)
    qb = qa.flip(0)
    want_d, want_F, want_I, _ = _oracle_all(dense, qa, qb)
    got = dense.derivative(qa), dense.antiderivative(qa), dense.integral(qa, qb)
    assert same_bits(got[0], want_d) and same_bits(got[1], want_F) and same_bits(got[2], want_I)
    with device_driver():
        dev = _solve(dtype, method, t0=0.3, t1=t1)                           # (its fp64 step sequence is not the host's)
        da = _queries(dev, seed=3)
        on_dev = dev.derivative(da), dev.antiderivative(da), dev.integral(da, da.flip(0))
    for a, b in zip(on_dev, _oracle_all(dev, da, da.flip(0))[:3]):
        assert same_bits(a, b)
    twin = copy.copy(dense)                                                  # the device driver on the host's record
    twin._k, twin._prefix = dev._k, None
    for a, b in zip((twin.derivative(qa), twin.antiderivative(qa), twin.integral(qa, qb)), got):
        assert same_bits(a, b)
    # y > 0 and t runs down: F(t) = integral from t0 to t < t0 is negative; y decays with t, so dy/dt < 0 in true time
    assert bool((got[1][:Q] < 0).all()) and bool((got[0] < 0).all())
    assert bool((dense.antiderivative(dense.t0[None]) == 0).all())
    ex, A, n = exact_antiderivative(dense, 2, qa[1, 2])
    assert abs(Fraction(float(got[1][1, 2, 0])) - ex[0]) <= antiderivative_bound(dense, A[0], n, got[1][1, 2, 0])


# -- 3. dose times ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_dose_times(backend, device_driver, dtype):
    """One dose per row inside the interval: the dose time is a breakpoint and belongs to the earlier segment."""
    t1 = per_row_t1(B)
    jump = (0.4 * t1)[None]                                                                   # [1, B]
    dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64).to(dtype)
    with _backend(backend, device_driver):
        dense = _solve(dtype, "dopri5", options={"jump_t": jump, "jump_dy": dy})
        off = dense.offsets.tolist()
        s_of = [next(s for s in range(off[r], off[r + 1]) if float(dense.seg_end[s]) == float(jump[0, r])) for r in range(B)]
        before, behind = torch.nextafter(jump, torch.zeros_like(jump)), torch.nextafter(jump, t1[None])
        d_at, F_before, F_at, F_behind = (dense.derivative(jump)[0], dense.antiderivative(before)[0],
                                          dense.antiderivative(jump)[0], dense.antiderivative(behind)[0])
        d_behind, y_at, y_behind = dense.derivative(behind)[0], dense(jump)[0], dense(behind)[0]
        P = dense._prefix
    coeffs, _, ta, tb, sign = _wire(dense)
    T = NP_T[dtype]
    for r, s in enumerate(s_of):
        assert s + 1 < off[r + 1] and float(dense.seg_start[s + 1]) == float(jump[0, r])
        one = lambda seg, x: torch.from_numpy(np_calc(DERIVATIVE, coeffs, None, ta, tb, sign, np.array([seg]),  # noqa: E731
                                                      np.array([x], dtype=T))[0])
        assert same_bits(d_at[r], one(s, 1.0))                                                # the LEFT derivative
        x_behind = T((float(behind[0, r]) - ta[s + 1]) / (tb[s + 1] - ta[s + 1]))
        assert same_bits(d_behind[r], one(s + 1, x_behind))                                   # the later segment
        for tq, got in ((before, F_before), (jump, F_at)):                                    # the earlier segment
            want = np_calc(ANTIDERIVATIVE, coeffs, P.numpy(), ta, tb, sign, np.array([s]), np.array([0.5], dtype=T),
                           np.array([float(tq[0, r])]))
            assert same_bits(got[r], torch.from_numpy(want[0]))
        assert same_bits(F_at[r], P[s + 1].to(dtype))                                         # x = 1: the whole segment
        want = np_calc(ANTIDERIVATIVE, coeffs, P.numpy(), ta, tb, sign, np.array([s + 1]), np.array([0.5], dtype=T),
                       np.array([float(behind[0, r])]))
        assert same_bits(F_behind[r], torch.from_numpy(want[0]))
    # the state jumps by the dose, its integral does not
    assert float((y_behind - y_at - dy[0]).abs().max()) < (1e-4 if dtype == F32 else 1e-10)
    assert float((F_behind - F_at).abs().max()) < 1e-6


# -- 4. forms, errors, cache --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_query_forms(backend, device_driver, dtype):
    shared = torch.tensor([0.21, 0.05, 0.29, 0.05], dtype=F64)                                # inside every row's interval
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, "dopri5")
        per_row = shared[:, None].expand(-1, B).contiguous()
        for fn in (dense.derivative, dense.antiderivative, lambda t: dense.integral(0.02, t), lambda t: dense.integral(t, 0.25)):
            by_list = fn(shared)
            assert by_list.shape == (4, B, L) and same_bits(by_list, fn(per_row))
            assert same_bits(by_list[1], by_list[3])                                          # repeats
            one = fn(0.21)
            assert one.shape == (B, L) and same_bits(one, by_list[0]) and same_bits(fn(torch.tensor(0.21, dtype=F64)), one)
            assert same_bits(fn(shared.to(F32)), fn(shared.to(F32).to(F64)))
            assert fn(torch.empty(0, dtype=F64)).shape == (0, B, L)
        both = dense.integral(shared, per_row.flip(0))                                        # [Q] against [Q, B]
        assert both.shape == (4, B, L) and same_bits(both, dense.integral(per_row, per_row.flip(0)))
        assert dense.integral(0.1, 0.2).shape == (B, L)
        with pytest.raises(ValueError, match="do not broadcast"):
            dense.integral(shared, shared[:3])
        with pytest.raises(ValueError, match="must be a number"):
            dense.derivative(torch.zeros(2, B + 1, dtype=F64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_out_of_range(backend, device_driver, dtype):
    """Below t0, beyond t1 and NaN: `check=True` names the smallest flat query (j, r) — for the integral of `ta` first, then
    of `tb`; `check=False` gives NaN rows and leaves the others alone."""
    with _backend(backend, device_driver):
        dense = _solved(backend, dtype, "dopri5")
        good = random_queries(3, dense.t0, dense.t1, seed=2)
        bad = good.clone()
        bad[2, 1] = float("nan")
        bad[1, 3] = float(dense.t1[3]) + 1e-9
        bad[2, 0] = -1e-9
        for fn in (dense.derivative, dense.antiderivative):
            with pytest.raises(ValueError, match=r"query 1 of row 3 \(t = .*outside the row's interval"):
                fn(bad)
            got = fn(bad, check=False)
            mask = torch.zeros(3, B, dtype=torch.bool)
            mask[2, 1] = mask[1, 3] = mask[2, 0] = True
            assert bool(torch.isnan(got[mask]).all()) and same_bits(got[~mask], fn(good)[~mask])
        with pytest.raises(ValueError, match=r"dense.integral\(ta, tb\): query 1 of row 3 \(ta = "):
            dense.integral(bad, bad.flip(0))
        with pytest.raises(ValueError, match=r"query 0 of row 0 \(tb = "):
            dense.integral(good, bad.flip(0))
        got = dense.integral(good, bad, check=False)
        assert bool(torch.isnan(got[mask]).all()) and same_bits(got[~mask], dense.integral(good, good)[~mask])
        got = dense.integral(bad, good, check=False)
        assert bool(torch.isnan(got[mask]).all()) and not bool(torch.isnan(got[~mask]).any())
        with pytest.raises(ValueError, match="query 0 of row 0"):
            dense.antiderivative(float("nan"))


def test_gradients_are_refused():
    dense = _solved("host", F64, "dopri5")
    t = torch.tensor(0.1, dtype=F64, requires_grad=True)
    for call in (lambda: dense.derivative(t), lambda: dense.antiderivative(t), lambda: dense.integral(0.0, t),
                 lambda: dense.integral(t, 0.2)):
        with pytest.raises(NotImplementedError, match="does not propagate gradients"):
            call()
    with torch.no_grad():
        assert dense.derivative(t).shape == (B, L)


@pytest.mark.parametrize("backend", ["host", "oracle"])
def test_prefix_cache(backend, device_driver):
    """Built by the first antiderivative / integral only, kept, dropped on request and rebuilt with the same bits."""
    with _backend(backend, device_driver):
        dense = _solve(F32, "dopri5")
        q = _queries(dense)
        assert dense._prefix is None
        dense(q), dense.derivative(q)
        assert dense._prefix is None                                                          # never built by these
        first = dense.antiderivative(q)
        P = dense._prefix
        assert P.dtype == F64 and tuple(P.shape) == (dense.n_segments, L)
        dense.integral(q, q.flip(0))
        assert dense._prefix is P                                                             # kept
        dense.drop_integral_cache()
        assert dense._prefix is None
        fresh = _solve(F32, "dopri5")
        again = fresh.integral(q, q.flip(0)), dense.antiderivative(q)
        assert same_bits(again[1], first) and same_bits(dense._prefix, P) and dense._prefix is not P
        assert same_bits(again[0], dense.integral(q, q.flip(0)))


# -- 5. the entry points refuse bad arguments before any launch ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _native.load_library()


def test_abi_31_argument_errors(lib):
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION >= 31
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok_prefix = dict(prefix=p, coeffs=p, offsets=p, seg_ta=p, seg_tb=p, n_seg=2, n_rows=1, row_len=3, dtype=_native.dtype_code(F32))

    def prefix(**kw):
        a = {**ok_prefix, **kw}
        return lib.tdeq_row_dense_prefix(a["prefix"], a["coeffs"], a["offsets"], a["seg_ta"], a["seg_tb"], a["n_seg"],
                                         a["n_rows"], a["row_len"], a["dtype"], None)
    for name in ("prefix", "coeffs", "offsets", "seg_ta", "seg_tb"):
        assert prefix(**{name: None}) == EINVAL, name
    for kw in (dict(n_seg=-1), dict(n_rows=-1), dict(row_len=0), dict(dtype=7), dict(n_seg=2 ** 31)):
        assert prefix(**kw) == EINVAL, kw
    assert prefix(n_rows=0) == 0 and prefix(n_seg=0) == 0                                     # no-ops, no launch

    ok_calc = dict(out=p, mode=2, coeffs=p, n_seg=2, seg_ta=p, seg_tb=p, prefix=p, sign=1.0, seg=p, x=p, tq=p, seg2=p, x2=p,
                   tq2=p, n_idx=1, row_len=3, dtype=_native.dtype_code(F64))

    def calc(**kw):
        a = {**ok_calc, **kw}
        return lib.tdeq_row_dense_calc(a["out"], a["mode"], a["coeffs"], a["n_seg"], a["seg_ta"], a["seg_tb"], a["prefix"],
                                       a["sign"], a["seg"], a["x"], a["tq"], a["seg2"], a["x2"], a["tq2"], a["n_idx"],
                                       a["row_len"], a["dtype"], None)
    for name in ("out", "coeffs", "seg_ta", "seg_tb", "prefix", "seg", "x", "tq", "seg2", "x2", "tq2"):
        assert calc(**{name: None}) == EINVAL, name
    assert calc(mode=1, prefix=None) == EINVAL and calc(mode=1, tq=None) == EINVAL
    for kw in (dict(mode=3), dict(mode=-1), dict(sign=0.0), dict(sign=2.0), dict(sign=float("nan")), dict(n_idx=-1),
               dict(n_seg=-1), dict(n_seg=0), dict(n_seg=2 ** 31), dict(row_len=0), dict(dtype=7)):
        assert calc(**kw) == EINVAL, kw
    assert calc(n_idx=0) == 0
    assert calc(n_idx=0, mode=0, prefix=None, tq=None, seg2=None, x2=None, tq2=None) == 0     # the derivative needs none of them
