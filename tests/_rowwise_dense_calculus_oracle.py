"""Shared pieces of the tests of `RowDenseOutput.derivative` / `.antiderivative` / `.integral`, written from the text of
include/tdeq_hip.h (ABI 31).  Two independent statements of the three operations:

1. `np_prefix`, `np_derivative`, `np_antiderivative64`: numpy scalars (`np.float32` / `np.float64`) and the L elements of one
   segment at a time, in explicit Python loops over segments and queries, in the exact operation order of the header (an
   elementwise numpy operation rounds every element once, as the scalar does).  They define the bits.  `CalculusOracle`
   puts them behind the kernels interface (`row_dense_prefix`, `row_dense_calc`), so that the `device_driver` pattern runs
   `HipRowKernels` and the three methods on them with CPU states.
2. `exact_antiderivative`, `exact_derivative`: `fractions.Fraction` from the wire format of the dense object (`offsets`,
   `seg_start`, `seg_end`, `coeffs`, the query in true time), with the bounds below.  They catch a formula that is wrong in
   every backend at once.

The bounds (derived, not measured).  u = 2^-53, u_T the unit roundoff of the state's type T.

Antiderivative.  F = T(sign * (P[s] + J_s(x64))).  J_s is a Horner form whose deepest path — the coefficient a — sees 12
roundings: the constant 0.2 (1), a * 0.2 (1), four times (* x, + next) (8), * x (1), * h (1).  x64 = (tq - ta) / h carries two
roundings and h = tb - ta one; with 0 <= x64 <= 1, |dJ/dx| <= h (|e| + |d| + |c| + |b| + |a|), so each of them moves J by at most
u times that sum.  Every term of J is bounded by h_s |coefficient|, hence |J - J_exact| <= 15 u h_s (|e| + ... + |a|) to first
order, and 16 covers the second-order terms.  The prefix is one fp64 addition per earlier segment, each with a relative error
u on a partial sum bounded by A_r = sum_s h_s (|e| + |d| + |c| + |b| + |a|) over the row's segments up to and including the
query's (the whole-segment integrals I_s = J_s(1.0) have the error of J); the multiplication by sign is exact; the rounding
to T adds u_T |F|.  With n the number of those segments:
    |F - F_exact| <= (n + 16) u A_r + u_T |F|.
Integral: T(F64(b) - F64(a)); the two end bounds added (the fp64 subtraction and the one rounding to T are inside the u_T
terms of the ends, |F(b) - F(a)| <= |F(b)| + |F(a)|).

Derivative, with the segment and the T-rounded x of the search taken as exact inputs:
    out = (d + (c + c) x + (3 b) x^2 + (4 a) x^3) / w.
c + c and 4 a are exact.  The deepest path is b's: 3 b (1), xp = x x (1), the product (1), two sums (2), the division (1) and
w = T(fp64 difference) (2): 8 roundings, each relative to a quantity bounded by (|d| + 2 |c| + 3 |b| + 4 |a|) / |w| since
0 <= x <= 1.  The header's constant 12 covers that count and the second-order terms:
    |out - exact| <= 12 u_T (|d| + 2 |c| + 3 |b| + 4 |a|) / |w|.
"""
import contextlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import DenseOracle
from _rowwise_impulse_oracle import ImpulseOracle

from torchdiffeq_amd import _native, rowwise

DERIVATIVE, ANTIDERIVATIVE, INTEGRAL = 0, 1, 2
U64 = Fraction(1, 2 ** 53)
U_T = {torch.float32: Fraction(1, 2 ** 24), torch.float64: Fraction(1, 2 ** 53)}
NP_T = {torch.float32: np.float32, torch.float64: np.float64}


# -- 1. the bits: numpy scalars and rows of L elements, explicit loops over segments and queries ---------------------------
def _J(e, d, c, b, a, x, h):
    """J_s(x) on np.float64 values (the L elements of a segment at once; x and h scalars): every product and sum is one
    rounded numpy operation per element."""
    f = np.float64
    return (((((a * f(0.2)) * x + b * f(0.25)) * x + c * (f(1.0) / f(3.0))) * x + d * f(0.5)) * x + e) * x * h


def np_prefix(coeffs, offsets, ta, tb):
    """`coeffs` [5, n_seg, L] (any real numpy dtype), `offsets` [B + 1], `ta` / `tb` fp64 [n_seg] in solver time ->
    fp64 [n_seg, L]: P[offsets[r]] = 0, P[s + 1] = P[s] + I_s, left to right."""
    f = np.float64
    _, n_seg, L = coeffs.shape
    P = np.zeros((n_seg, L), dtype=np.float64)
    for r in range(len(offsets) - 1):
        acc = np.zeros(L, dtype=np.float64)
        for s in range(int(offsets[r]), int(offsets[r + 1])):
            P[s] = acc
            e, d, c, b, a = (coeffs[p, s].astype(np.float64) for p in range(5))
            acc = acc + _J(e, d, c, b, a, f(1.0), f(tb[s]) - f(ta[s]))
    return P


def np_derivative(coeffs, ta, tb, sign, seg, x):
    """-> [n, L] in the dtype of `coeffs`; `seg` [n], `x` [n] of that dtype (NaN marks an out-of-range query)."""
    T = coeffs.dtype.type
    n, L = len(seg), coeffs.shape[2]
    out = np.empty((n, L), dtype=coeffs.dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            s, xi = int(seg[i]), T(x[i])
            w = T(np.float64(sign) * (np.float64(tb[s]) - np.float64(ta[s])))
            d, c, b, a = (coeffs[p, s] for p in range(1, 5))
            tot = d + (c + c) * xi
            xp = xi * xi
            tot = tot + (T(3) * b) * xp
            xp = xp * xi
            tot = tot + (T(4) * a) * xp
            out[i] = tot / w
            assert tot.dtype == coeffs.dtype and type(xp) is T
    return out


def np_antiderivative64(coeffs, P, ta, tb, sign, seg, x, tq):
    """sign * (P[s] + J_s(x64)) -> fp64 [n, L], not rounded to T; `tq` fp64 [n] in solver time."""
    f = np.float64
    n, L = len(seg), coeffs.shape[2]
    out = np.empty((n, L), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = int(seg[i])
            h = f(tb[s]) - f(ta[s])
            x64 = f(np.nan) if np.isnan(x[i]) else (f(tq[i]) - f(ta[s])) / h
            e, d, c, b, a = (coeffs[p, s].astype(np.float64) for p in range(5))
            out[i] = f(sign) * (P[s] + _J(e, d, c, b, a, x64, h))
    return out


def np_calc(mode, coeffs, P, ta, tb, sign, seg, x, tq=None, seg2=None, x2=None, tq2=None):
    """`tdeq_row_dense_calc` on numpy arrays -> [n, L] in the dtype of `coeffs`."""
    if mode == DERIVATIVE:
        return np_derivative(coeffs, ta, tb, sign, seg, x)
    F = np_antiderivative64(coeffs, P, ta, tb, sign, seg, x, tq)
    if mode == ANTIDERIVATIVE:
        return F.astype(coeffs.dtype)
    with np.errstate(all="ignore"):
        return (np_antiderivative64(coeffs, P, ta, tb, sign, seg2, x2, tq2) - F).astype(coeffs.dtype)


class CalculusOracle(ImpulseOracle):
    """`DenseOracle` — through `ImpulseOracle`, its subclass with the launches of a solve with `jump_t` / `jump_dy` — plus
    `row_dense_prefix` and `row_dense_calc`, on CPU tensors."""

    @staticmethod
    def row_dense_prefix(prefix, coeffs, offsets, seg_ta, seg_tb) -> None:
        assert prefix.dtype == torch.float64 and tuple(prefix.shape) == tuple(coeffs.shape[1:])
        prefix.copy_(torch.from_numpy(np_prefix(coeffs.numpy(), offsets.numpy(), seg_ta.numpy(), seg_tb.numpy())))

    @staticmethod
    def row_dense_calc(out, mode, coeffs, seg_ta, seg_tb, prefix, sign, seg, x, tq=None, seg2=None, x2=None, tq2=None) -> None:
        flat = lambda t: None if t is None else t.numpy().reshape(-1)      # noqa: E731
        out.copy_(torch.from_numpy(np_calc(mode, coeffs.numpy(), None if prefix is None else prefix.numpy(), seg_ta.numpy(),
                                           seg_tb.numpy(), sign, flat(seg), flat(x), flat(tq), flat(seg2), flat(x2),
                                           flat(tq2))))


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_dense_oracle.py's fixture with the extended oracle."""
    assert issubclass(CalculusOracle, DenseOracle)
    wrapped = CalculusOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


# -- 2. exact rationals from the wire format -----------------------------------------------------------------------------------
def _wire(dense):
    off = dense.offsets.cpu().tolist()
    start = [Fraction(v) for v in dense.seg_start.cpu().tolist()]
    end = [Fraction(v) for v in dense.seg_end.cpu().tolist()]
    return off, start, end, dense.coeffs.cpu().to(torch.float64)


def _segment_of(off, end, r, t, descending):
    """The first segment of row r whose end is not before t (in the direction of the solve), the last one if none."""
    for s in range(off[r], off[r + 1]):
        if (t >= end[s]) if descending else (t <= end[s]):
            return s
    return off[r + 1] - 1


def exact_antiderivative(dense, r, t):
    """Row r at true time `t` (a float inside the row's interval) -> (exact integral from t0[r] per element [L] of Fraction,
    A_r per element, n = the number of the row's segments up to and including the query's)."""
    off, start, end, q = _wire(dense)
    t = Fraction(float(t))
    descending = float(dense.t1[r]) < float(dense.t0[r])
    last = _segment_of(off, end, r, t, descending)
    L = q.shape[2]
    total, A = [Fraction(0)] * L, [Fraction(0)] * L
    for s in range(off[r], last + 1):
        h = end[s] - start[s]                                                 # true time: negative for a descending solve
        x = (t - start[s]) / h if s == last else Fraction(1)
        for k in range(L):
            e, d, c, b, a = (Fraction(float(q[p, s, k])) for p in range(5))
            total[k] += h * (e * x + d * x ** 2 / 2 + c * x ** 3 / 3 + b * x ** 4 / 4 + a * x ** 5 / 5)
            A[k] += abs(h) * (abs(e) + abs(d) + abs(c) + abs(b) + abs(a))
    return total, A, last + 1 - off[r]


def antiderivative_bound(dense, A, n, F):
    """(n + 16) u A_r + u_T |F| for one element; `F` the computed value."""
    return (n + 16) * U64 * A + U_T[dense.coeffs.dtype] * abs(Fraction(float(F)))


def exact_derivative(dense, s, x):
    """Segment `s` at the fraction `x` (the T value of the search, taken as exact) -> (exact dy/dt in true time per element
    [L] of Fraction, the bound 12 u_T (|d| + 2|c| + 3|b| + 4|a|) / |w| per element)."""
    _, start, end, q = _wire(dense)
    x = Fraction(float(x))
    w = end[s] - start[s]
    values, bounds = [], []
    for k in range(q.shape[2]):
        d, c, b, a = (Fraction(float(q[p, s, k])) for p in range(1, 5))
        values.append((d + 2 * c * x + 3 * b * x ** 2 + 4 * a * x ** 3) / w)
        bounds.append(12 * U_T[dense.coeffs.dtype] * (abs(d) + 2 * abs(c) + 3 * abs(b) + 4 * abs(a)) / abs(w))
    return values, bounds


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as bit patterns (a NaN equals the same NaN, -0.0 differs from 0.0), after moving both to the CPU."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if torch.equal(a.view(torch.uint8), b.view(torch.uint8)):
        return True
    # (NaN payloads may differ between backends: compare the NaN masks, and the bits of everything else)
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros_like(a)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a).view(torch.uint8), torch.where(nb, zero, b).view(torch.uint8))
