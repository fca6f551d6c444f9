"""Shared pieces of the tests of `RowDenseOutput.exposure` / `.area_above` / `.area_below`, written from the text of
include/tdeq_hip.h (ABI 34).

1. `np_exposure`: numpy scalars (`np.float64`), explicit Python loops over queries, elements, segments and candidates, the
   candidates in LISTS from `_segment_candidates` and the roots from `_bisect` of tests/_rowwise_dense_extremum_oracle.py, the
   walk and state machine of `np_level`.  It defines the bits.  `ExposureOracle` puts it behind the kernels interface
   (`row_dense_exposure`), so that the `device_driver` pattern runs the device path of the methods with CPU states.
2. `exact_signed_area_check`: `fractions.Fraction` from the wire format: the exact integral of p - lev over the window, with
   the exact rational ends of every segment, against the unclamped A_up - A_dn, with the bound below.

The bound (derived, not measured).  u = 2^-53.  On a segment s with coefficients e, d, c, b, a, the level lev and the exact
h = tb - ta write S = |e - lev| + |d| + |c| + |b| + |a| (the exact difference), so |phi(x)| <= S on 0 <= x <= 1, and M_s = S h.
The exact area of the segment is K(xhi) - K(xlo) with K(x) = h x (a/5 x^4 + b/4 x^3 + c/3 x^2 + d/2 x + (e - lev)) and the
exact ends; |K(v) - K(u)| = h |integral of phi over [u, v]| <= M_s (v - u).
  * One evaluation of K.  The term of `a` passes the most roundings: the constant 0.2 (not a double: 1), a*0.2, four
    multiplications by x and four additions of the Horner form, `* x`, `* h`, and h = fl(tb - ta) itself: 13.  (b*0.25 and
    d*0.5 are exact, 1/3 is one more constant, el = fl(e - lev) one rounding on the shortest path.)  The terms sum to at most
    M_s in modulus, so |fl K(x) - K(x)| <= gamma_13 M_s <= 14 u M_s; the u M_s to spare (13 u^2-level terms aside) covers every
    second-order term below.
  * Telescoping.  The pieces of a segment are differences of neighbouring computed K values — K(z) of a crossing is computed
    once and used on both sides, K(u) is carried — so their exact sum is fl K(xhi) - fl K(xlo) whatever the splits: two
    evaluations, 28 u M_s.  (A_up - A_dn is the sum of ALL pieces: a piece below enters A_dn negated.)
  * The piece subtractions.  Each is rounded once, an error of at most u |piece|.  The candidates are visited in increasing x
    and z lies between its neighbours, so the pieces do not overlap: sum |piece| <= M_s (xhi - xlo) <= M_s to first order, and
    all of the segment's subtractions together cost u M_s — not one u M_s each.
  * The rounded ends.  Only xlo of the first and xhi of the last segment are computed: fl(fl(tq - ta) / fl(h)), three
    roundings, |x^ - x| <= 3 u x <= 3 u (fl(tq - ta) <= fl(tb - ta), so x^ <= 1), and K moves by at most M_s |x^ - x|:
    3 u M_s per end, at most 6 u sum M_s for the window (also when both ends lie in one segment).  Interior ends are 0.0 and 1.0.
  * The accumulators.  A segment adds at most 12 pieces (7 candidates, 6 gaps, each split at most once), a window of n segments
    at most 12 n, each into A_up or A_dn, whose partial sums are bounded by sum |piece| <= sum M_s: 12 n u sum M_s.
Together  |(A_up - A_dn) - exact| <= (28 + 1 + 6 + 12 n) u sum_s M_s = (35 + 12 n) u sum_s S_s h_s,  n the segments of the window.
"""
import contextlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import U64, same_bits  # noqa: F401
from _rowwise_dense_extremum_oracle import _bisect, _segment_candidates
from _rowwise_dense_level_oracle import LevelOracle, broadcast_level
from _rowwise_dense_oracle import NONE, DenseOracle

from torchdiffeq_amd import _native, rowwise

f64 = np.float64


def bound_constant(n_segments):
    """C of the module's docstring for a window of `n_segments` segments."""
    return 35 + 12 * n_segments


# -- 1. the bits ---------------------------------------------------------------------------------------------------------------
def np_exposure(coeffs, level, ta, tb, seg, x, tq, seg2, x2, tq2):
    """`tdeq_row_dense_exposure` on numpy arrays, `level` [n_rows, L] -> (area_above, area_below [n, L] in the dtype of
    `coeffs`, time_above fp64 [n, L], A_up, A_dn fp64 [n, L]: the two sums before the clamp and the rounding)."""
    n, L = len(seg), coeffs.shape[2]
    n_rows = level.shape[0]
    T = coeffs.dtype.type
    area_above, area_below = (np.full((n, L), np.nan, dtype=coeffs.dtype) for _ in range(2))
    above_for, sum_up, sum_dn = (np.full((n, L), np.nan) for _ in range(3))
    with np.errstate(all="ignore"):
        for i in range(n):
            if np.isnan(x[i]) or np.isnan(x2[i]):
                continue
            (sA, tqa), (sB, tqb) = (int(seg[i]), f64(tq[i])), (int(seg2[i]), f64(tq2[i]))
            if tqb < tqa:
                (sA, tqa), (sB, tqb) = (sB, tqb), (sA, tqa)
            for k in range(L):
                lev = f64(level[i % n_rows, k])
                state = t_up = None
                total, nan = f64(0.0), False
                A = {True: f64(0.0), False: f64(0.0)}                            # A_up, A_dn

                def add(q, st):
                    A[st] = A[st] + q if st else A[st] - q

                for s in range(sA, sB + 1):
                    t_a, t_b = f64(ta[s]), f64(tb[s])
                    h = t_b - t_a
                    xlo = (tqa - t_a) / h if s == sA else f64(0.0)
                    xhi = (tqb - t_a) / h if s == sB else f64(1.0)
                    e, d, c, b, a = (f64(coeffs[p, s, k]) for p in range(5))
                    phi = lambda v: (e + v * (d + v * (c + v * (b + v * a)))) - lev          # noqa: E731
                    el = e - lev
                    K = lambda v: (((((a * f64(0.2)) * v + b * f64(0.25)) * v + c * (f64(1.0) / f64(3.0))) * v   # noqa: E731
                                    + d * f64(0.5)) * v + el) * v * h
                    u = None
                    for v in _segment_candidates(e, d, c, b, a, xlo, xhi):
                        nan = nan or bool(np.isnan(phi(v)))
                        above = bool(phi(v) > 0)
                        if state is None:                                    # the first candidate of the window
                            state = above
                            if above:
                                t_up = tqa
                        elif above != state:
                            if u is None:                                    # the first candidate of a later segment
                                z = v
                            elif phi(u) == 0:
                                z = u
                            elif phi(v) == 0:
                                z = v
                            else:
                                z = _bisect(phi, u, v)
                                if z is None:                                # (only with a NaN phi: the answer is NaN)
                                    assert nan
                                    z = v
                            if u is not None:
                                add(K(z) - K(u), state)
                                add(K(v) - K(z), above)
                            if s == sA and z == xlo:
                                tz = tqa
                            elif s == sB and z == xhi:
                                tz = tqb
                            elif z == 0:
                                tz = t_a
                            elif z == 1:
                                tz = t_b
                            else:
                                tz = t_a + z * h
                            if above:
                                t_up = tz
                            else:
                                total = total + (tz - t_up)
                            state = above
                        elif u is not None:
                            add(K(v) - K(u), state)
                        u = v
                if state:
                    total = total + (tqb - t_up)
                if not nan:
                    sum_up[i, k], sum_dn[i, k] = A[True], A[False]
                    area_above[i, k] = T(f64(0.0) if A[True] < 0 else A[True])
                    area_below[i, k] = T(f64(0.0) if A[False] < 0 else A[False])
                    above_for[i, k] = total
    return area_above, area_below, above_for, sum_up, sum_dn


class ExposureOracle(LevelOracle):
    """`LevelOracle` plus `row_dense_exposure`, on CPU tensors."""

    @staticmethod
    def row_dense_exposure(area_above, area_below, time_above, level, coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2,
                           tq2) -> None:
        assert level.dtype == coeffs.dtype == area_above.dtype == area_below.dtype and level.shape[1] == coeffs.shape[2]
        assert time_above.dtype == torch.float64 and sign in (1.0, -1.0)
        assert area_above.shape == area_below.shape == time_above.shape and seg.numel() % level.shape[0] == 0
        flat = lambda t: t.numpy().reshape(-1)                                  # noqa: E731
        outs = np_exposure(coeffs.numpy(), level.numpy(), seg_ta.numpy(), seg_tb.numpy(), flat(seg), flat(x), flat(tq),
                           flat(seg2), flat(x2), flat(tq2))
        for dst, src in zip((area_above, area_below, time_above), outs):
            dst.copy_(torch.from_numpy(src))


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_dense_oracle.py's fixture with the extended oracle."""
    assert issubclass(ExposureOracle, DenseOracle)
    wrapped = ExposureOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def search_lists(dense, qa, qb):
    """The two searches of a CPU record for [Q, B] true-time windows (qa, qb), by the torch oracle of
    tests/_rowwise_dense_oracle.py -> [seg, x, tq, seg2, x2, tq2] as numpy arrays, the times in solver time."""
    sign = dense._sign
    ta, tb = (dense.seg_start * sign).contiguous(), (dense.seg_end * sign).contiguous()
    found = []
    for q in (qa, qb):
        n = q.numel()
        seg, x = torch.empty(n, dtype=torch.int32), torch.empty(n, dtype=dense.coeffs.dtype)
        status = torch.tensor([NONE], dtype=torch.int32)
        DenseOracle.row_dense_search((q * sign).contiguous(), dense.offsets, ta, tb, dense.t0 * sign, dense.t1 * sign, seg, x,
                                     status)
        found += [seg.numpy(), x.numpy(), (q * sign).numpy().reshape(-1)]
    return found


def oracle_exposure(dense, level, qa, qb):
    """`exposure` of a CPU record from the numpy oracle, for [Q, B] true-time windows (qa, qb) -> (area_above, area_below,
    time_above as tensors [Q, B, L], A_up, A_dn fp64 arrays [Q * B, L], ends = (seg, tq, seg2, tq2) of the two searches)."""
    sign = dense._sign
    found = search_lists(dense, qa, qb)
    *outs, a_up, a_dn = np_exposure(dense.coeffs.numpy(), broadcast_level(dense, level).numpy(), (dense.seg_start * sign).numpy(),
                                    (dense.seg_end * sign).numpy(), *found)
    shape = (qa.shape[0], *dense._shape)
    return (*(torch.from_numpy(v).view(shape) for v in outs), a_up, a_dn, (found[0], found[2], found[3], found[5]))


# -- 2. exact rationals from the wire format -------------------------------------------------------------------------------------
class ExactRecord:
    """The wire format of a CPU record and a level as exact rationals, converted once: segment ends in solver time, and per
    call the five coefficients of (segment, element) and the level of (window, element)."""

    def __init__(self, dense, level):
        sign = int(dense._sign)
        self.start = [Fraction(v) * sign for v in dense.seg_start.tolist()]
        self.end = [Fraction(v) * sign for v in dense.seg_end.tolist()]
        self.q = dense.coeffs.to(torch.float64).numpy()
        self.lev = broadcast_level(dense, level).to(torch.float64).numpy()

    def signed_area(self, ends, i, k, with_area=True):
        """Window i, element k: the exact integral of p - lev over the window in solver time (the ends of every segment as
        exact rationals; None without `with_area`), sum_s S_s h_s of the bound, and the number of segments -> (area, scale,
        n), all exact."""
        seg, tq, seg2, tq2 = ends
        lev = Fraction(float(self.lev[i % self.lev.shape[0], k]))
        (sA, tqa), (sB, tqb) = (int(seg[i]), Fraction(float(tq[i]))), (int(seg2[i]), Fraction(float(tq2[i])))
        if tqb < tqa:
            (sA, tqa), (sB, tqb) = (sB, tqb), (sA, tqa)
        area, scale = Fraction(0) if with_area else None, Fraction(0)
        for s in range(sA, sB + 1):
            t_a = self.start[s]
            h = self.end[s] - t_a
            e, d, c, b, a = (Fraction(float(self.q[p, s, k])) for p in range(5))
            if with_area:
                xlo = (tqa - t_a) / h if s == sA else Fraction(0)
                xhi = (tqb - t_a) / h if s == sB else Fraction(1)
                K = lambda v: h * v * (a / 5 * v ** 4 + b / 4 * v ** 3 + c / 3 * v ** 2 + d / 2 * v + (e - lev))    # noqa: E731
                area += K(xhi) - K(xlo)
            scale += (abs(e - lev) + abs(d) + abs(c) + abs(b) + abs(a)) * h
        return area, scale, sB - sA + 1


def exact_signed_area_check(dense, level, ends, a_up, a_dn):
    """Every (window, element) of `np_exposure`'s unclamped sums: |(A_up - A_dn) - exact| against (35 + 12 n) u sum S h of the
    module's docstring -> (the largest ratio seen, asserted <= 1; the pairs checked)."""
    exact = ExactRecord(dense, level)
    worst, seen = Fraction(0), 0
    for i in range(a_up.shape[0]):
        for k in range(a_up.shape[1]):
            if np.isnan(a_up[i, k]):
                continue
            area, scale, n = exact.signed_area(ends, i, k)
            miss = abs(Fraction(float(a_up[i, k])) - Fraction(float(a_dn[i, k])) - area)
            bound = bound_constant(n) * U64 * scale
            assert miss <= bound, (i, k, n, float(miss), float(bound))
            seen += 1
            if bound:
                worst = max(worst, miss / bound)
    return worst, seen
