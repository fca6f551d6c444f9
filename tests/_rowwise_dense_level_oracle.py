"""Shared pieces of the tests of `RowDenseOutput.crossings` / `.time_above`, written from the text of include/tdeq_hip.h (ABI 33).

1. `np_level`: numpy scalars (`np.float64`), explicit Python loops over queries, elements, segments and candidates, the
   candidates in LISTS from `_segment_candidates` and the roots from `_bisect` of tests/_rowwise_dense_extremum_oracle.py.  It
   defines the bits.  `LevelOracle` puts it behind the kernels interface (`row_dense_level`), so that the `device_driver`
   pattern runs the device path of the two methods with CPU states.
2. `exact_crossing_check`: `fractions.Fraction` from the wire format, for every reported crossing that a bisection located
   (strictly inside a piece), with the bound below.

The bound (derived, not measured).  u = 2^-53; on a segment with coefficients e, d, c, b, a and 0 <= x <= 1 write
S = |e| + |d| + |c| + |b| + |a| and G = |d| + 2 |c| + 3 |b| + 4 |a| (as in the extremum oracle; |p'| <= G on the segment).
  * The computed phi(x) is fl(fl(p(x)) - lev).  The subtraction is rounded correctly, so the computed sign (and an exact
    zero) is that of fl(p(x)) - lev, and fl(p(x)), a Horner form of 8 operations, is within gamma_8 S <= 9 u S of p(x):
    wherever the computed sign of phi is wrong, or the computed phi is 0, |p(x) - lev| <= 9 u S.
  * A bisection that returns `mid` for a computed zero therefore reports a z with |p(z) - lev| <= 9 u S.
  * Otherwise it ends on lo < hi with opposite computed signs that are neighbouring doubles of [0, 1] (hi - lo <= 2^-53) or,
    after 64 halvings of a piece of length at most 1, hi - lo <= 2^-64.  Across [lo, hi] the exact p moves by at most
    (hi - lo) G <= 2^-53 G.  If the exact signs at lo and hi differ (or one is zero) |p(z) - lev| <= 2^-53 G at either end;
    if they agree, the computed sign is wrong at one end, where |p - lev| <= 9 u S, and at the other end it is at most that
    plus 2^-53 G.
Hence |p(z) - lev| <= 9 u S + 2^-53 G for every z a bisection reports.  The test asserts twice that, 18 u S + 2^-52 G: both
evaluations of the last pair may carry their 9 u S, and the piece's ends are themselves rounded.
"""
import contextlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import U64, same_bits  # noqa: F401
from _rowwise_dense_extremum_oracle import ExtremumOracle, _bisect, _segment_candidates
from _rowwise_dense_oracle import NONE, DenseOracle

from torchdiffeq_amd import _native, rowwise

f64 = np.float64


# -- 1. the bits ---------------------------------------------------------------------------------------------------------------
def np_level(coeffs, level, ta, tb, sign, seg, x, tq, seg2, x2, tq2):
    """`tdeq_row_dense_level` on numpy arrays, `level` [n_rows, L] -> (count int32 [n, L], first, last, time_above fp64 [n, L],
    located: the list of (i, k, s, z) of the crossings of query i, element k that a bisection found at x = z of segment s)."""
    n, L = len(seg), coeffs.shape[2]
    n_rows = level.shape[0]
    count = np.full((n, L), -1, dtype=np.int32)
    first, last, above_for = (np.full((n, L), np.nan) for _ in range(3))
    located = []
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
                total, times, nan, found = f64(0.0), [], False, []
                for s in range(sA, sB + 1):
                    t_a, t_b = f64(ta[s]), f64(tb[s])
                    h = t_b - t_a
                    xlo = (tqa - t_a) / h if s == sA else f64(0.0)
                    xhi = (tqb - t_a) / h if s == sB else f64(1.0)
                    e, d, c, b, a = (f64(coeffs[p, s, k]) for p in range(5))
                    phi = lambda v: (e + v * (d + v * (c + v * (b + v * a)))) - lev          # noqa: E731
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
                                else:
                                    found.append((i, k, s, z))
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
                            times.append(tz)
                            if above:
                                t_up = tz
                            else:
                                total = total + (tz - t_up)
                            state = above
                        u = v
                if state:
                    total = total + (tqb - t_up)
                if not nan:
                    count[i, k] = len(times)
                    above_for[i, k] = total
                    if times:
                        first[i, k], last[i, k] = f64(sign) * times[0], f64(sign) * times[-1]
                    located += found
    return count, first, last, above_for, located


class LevelOracle(ExtremumOracle):
    """`ExtremumOracle` plus `row_dense_level`, on CPU tensors."""

    @staticmethod
    def row_dense_level(count, first, last, time_above, level, coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2) -> None:
        assert count.dtype == torch.int32 and level.dtype == coeffs.dtype and level.shape[1] == coeffs.shape[2]
        assert first.dtype == last.dtype == time_above.dtype == torch.float64
        assert count.shape == first.shape == last.shape == time_above.shape and seg.numel() % level.shape[0] == 0
        flat = lambda t: t.numpy().reshape(-1)                                  # noqa: E731
        outs = np_level(coeffs.numpy(), level.numpy(), seg_ta.numpy(), seg_tb.numpy(), sign, flat(seg), flat(x), flat(tq),
                        flat(seg2), flat(x2), flat(tq2))
        for dst, src in zip((count, first, last, time_above), outs):
            dst.copy_(torch.from_numpy(src))


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_dense_oracle.py's fixture with the extended oracle."""
    assert issubclass(LevelOracle, DenseOracle)
    wrapped = LevelOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def broadcast_level(dense, level):
    """The level as the entry point takes it: [B, L] in the state's dtype (a number, or a tensor that broadcasts)."""
    lev = level if isinstance(level, torch.Tensor) else torch.tensor(float(level), dtype=torch.float64)
    lev = lev.to(dense.coeffs.dtype).expand(dense._shape)
    return lev.reshape(dense._shape[0], -1).contiguous()


def oracle_level(dense, level, qa, qb):
    """`crossings` of a CPU record from the numpy oracle, for [Q, B] true-time windows (qa, qb); the search is the torch oracle
    of tests/_rowwise_dense_oracle.py -> (count, first, last, time_above as tensors [Q, B, L], located)."""
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
    *outs, located = np_level(dense.coeffs.numpy(), broadcast_level(dense, level).numpy(), ta.numpy(), tb.numpy(), sign, *found)
    shape = (qa.shape[0], *dense._shape)
    return (*(torch.from_numpy(v).view(shape) for v in outs), located)


# -- 2. exact rationals from the wire format -------------------------------------------------------------------------------------
def exact_crossing_check(dense, level, located):
    """Every crossing of `located` (`np_level`): the exact |p(z) - lev| from the wire format against 18 u S + 2^-52 G of its
    segment -> the largest ratio seen (asserted <= 1), 0 for an empty list."""
    q = dense.coeffs.to(torch.float64)
    lev = broadcast_level(dense, level).to(torch.float64)
    B = lev.shape[0]
    worst = Fraction(0)
    for i, k, s, z in located:
        e, d, c, b, a = (Fraction(float(q[p, s, k])) for p in range(5))
        zz = Fraction(float(z))
        assert 0 <= zz <= 1
        miss = abs(e + zz * (d + zz * (c + zz * (b + zz * a))) - Fraction(float(lev[i % B, k])))
        S = abs(e) + abs(d) + abs(c) + abs(b) + abs(a)
        G = abs(d) + 2 * abs(c) + 3 * abs(b) + 4 * abs(a)
        bound = 18 * U64 * S + Fraction(1, 2 ** 52) * G
        assert miss <= bound, (i, k, s, float(z), float(miss), float(bound))
        if bound:
            worst = max(worst, miss / bound)
    return worst
