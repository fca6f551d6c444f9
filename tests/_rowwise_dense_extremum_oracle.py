"""Shared pieces of the tests of `RowDenseOutput.maximum` / `.minimum`, written from the text of include/tdeq_hip.h (ABI 32).

1. `np_extremum`: numpy scalars (`np.float64`), explicit Python loops over queries, elements, segments, pieces and bisection
   rounds, with the pieces and candidates kept in LISTS as the header words them (the host model and the kernel use a fixed
   structure with repeats instead).  It defines the bits.  `ExtremumOracle` puts it behind the kernels interface
   (`row_dense_extremum`), so that the `device_driver` pattern runs the device path of the two methods with CPU states.
2. `exact_window_check`: `fractions.Fraction` from the wire format, with the bound below.
3. `oscillator_problem`: rows of harmonic oscillators, whose components have interior extrema on most steps.

The bound (derived, not measured).  u = 2^-53.  On a segment with coefficients e, d, c, b, a and 0 <= x <= 1 write
S = |e| + |d| + |c| + |b| + |a| and G = |d| + 2 |c| + 3 |b| + 4 |a|.
  * p is a Horner form of degree 4: 8 operations, so |fl(p(x)) - p(x)| <= gamma_8 S <= 9 u S.
  * g is a Horner form of degree 3 whose coefficients carry at most one rounding (3 b; c + c and 4 a are exact): 7 roundings
    on the deepest path, |fl(g(x)) - g(x)| <= 8 u G.  The computed g can have the wrong sign only where |g(x)| <= 8 u G.
  * Between two neighbouring candidates of a segment the exact p can rise above both only if a sign change of g in between
    went unseen.  The pieces of g are bounded by the computed roots of g1, so g is monotone on a piece up to what the
    isolation of those roots leaves (|g1| within its own rounding error there, a second-order term), and a bisection that
    was not started, or that ended next to a point where the computed sign is wrong, leaves |g| <= 8 u G between the
    candidate and the true stationary point.  The 64-round cap leaves an interval of at most 2^-64, across which g moves by
    at most 2^-64 * (2 |c| + 6 |b| + 12 |a|) < u G.  The rise is the integral of g over at most the piece, whose length is
    at most 1: p(y) <= max over the segment's candidates of p + 2 * 8 u G, the factor 2 for the second-order terms and the cap.
  * The best candidate is chosen by COMPUTED values: exact p(x*) >= exact p(candidate) - 9 u (S + S*), S* of x*'s segment.
Hence for every y of the window in a segment with S, G, and the reported x* in a segment with S*:
    p(y) - p(x*) <= 16 u G + 9 u (S + S*)
and the reported value, the computed p(x*) rounded once to T, satisfies |values - p(x*)| <= 9 u S* + u_T |values|.
For the minimum the same with the signs reversed.
"""
import contextlib
from fractions import Fraction

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import NP_T, U64, U_T, CalculusOracle, same_bits  # noqa: F401
from _rowwise_dense_oracle import NONE, DenseOracle, random_queries

from torchdiffeq_amd import _native, rowwise

MAXIMUM, MINIMUM = 0, 1
f64 = np.float64


# -- 1. the bits ---------------------------------------------------------------------------------------------------------------
def _bisect(phi, lo, hi):
    """-> the root, or None."""
    nlo = phi(lo) < 0
    if phi(lo) == 0 or phi(hi) == 0 or nlo == (phi(hi) < 0):
        return None
    for _ in range(64):
        mid = f64(0.5) * (lo + hi)
        if mid == lo or mid == hi:
            break
        if phi(mid) == 0:
            return mid
        if (phi(mid) < 0) == nlo:
            lo = mid
        else:
            hi = mid
    return lo if abs(phi(lo)) <= abs(phi(hi)) else hi


def _segment_candidates(e, d, c, b, a, xlo, xhi):
    """The candidates of one element on one segment, in increasing x (repeats kept)."""
    g = lambda x: d + x * ((c + c) + x * (f64(3) * b + x * (f64(4) * a)))      # noqa: E731
    g1 = lambda x: (c + c) + x * (f64(6) * b + x * (f64(12) * a))             # noqa: E731
    bounds1 = [xlo, xhi]
    if a != 0:
        x1 = (-b) / (f64(4) * a)
        if xlo < x1 < xhi:
            bounds1 = [xlo, x1, xhi]
    roots1 = [r for lo, hi in zip(bounds1, bounds1[1:]) for r in [_bisect(g1, lo, hi)] if r is not None]
    bounds = [xlo] + roots1 + [xhi]
    out = [bounds[0]]
    for lo, hi in zip(bounds, bounds[1:]):
        z = _bisect(g, lo, hi)
        out += ([z] if z is not None else []) + [hi]
    assert len(out) <= 7 and all(type(v) is f64 for v in out)
    return out


def np_extremum(which, coeffs, ta, tb, sign, seg, x, tq, seg2, x2, tq2):
    """`tdeq_row_dense_extremum` on numpy arrays -> (values [n, L] in the dtype of `coeffs`, times fp64 [n, L], where: int64
    [n, L, 2] = the segment and the index of the winning candidate's kind — 0 a window end or a segment end, 1 inside a
    segment —, xs fp64 [n, L] the winning x)."""
    n, L = len(seg), coeffs.shape[2]
    values = np.full((n, L), np.nan, dtype=coeffs.dtype)
    times = np.full((n, L), np.nan)
    where = np.full((n, L, 2), -1, dtype=np.int64)
    xs = np.full((n, L), np.nan)
    better = (lambda v, best: v > best) if which == MAXIMUM else (lambda v, best: v < best)
    with np.errstate(all="ignore"):
        for i in range(n):
            if np.isnan(x[i]) or np.isnan(x2[i]):
                continue
            (sA, tqa), (sB, tqb) = (int(seg[i]), f64(tq[i])), (int(seg2[i]), f64(tq2[i]))
            if tqb < tqa:
                (sA, tqa), (sB, tqb) = (sB, tqb), (sA, tqa)
            for k in range(L):
                best = when = None
                nan = False
                for s in range(sA, sB + 1):
                    t_a, t_b = f64(ta[s]), f64(tb[s])
                    h = t_b - t_a
                    xlo = (tqa - t_a) / h if s == sA else f64(0.0)
                    xhi = (tqb - t_a) / h if s == sB else f64(1.0)
                    e, d, c, b, a = (f64(coeffs[p, s, k]) for p in range(5))
                    for v in _segment_candidates(e, d, c, b, a, xlo, xhi):
                        p = e + v * (d + v * (c + v * (b + v * a)))
                        nan = nan or bool(np.isnan(p))
                        if best is None or better(p, best):
                            best = p
                            if s == sA and v == xlo:
                                when = tqa
                            elif s == sB and v == xhi:
                                when = tqb
                            elif v == 0:
                                when = t_a
                            elif v == 1:
                                when = t_b
                            else:
                                when = t_a + v * h
                            where[i, k] = (s, int(0 < v < 1 and v != xlo and v != xhi))
                            xs[i, k] = v
                if not nan:
                    values[i, k] = coeffs.dtype.type(best)
                    times[i, k] = f64(sign) * when
    return values, times, where, xs


class ExtremumOracle(CalculusOracle):
    """`CalculusOracle` plus `row_dense_extremum`, on CPU tensors."""

    @staticmethod
    def row_dense_extremum(values, times, which, coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2, tq2) -> None:
        assert times.dtype == torch.float64 and values.dtype == coeffs.dtype and values.shape == times.shape
        flat = lambda t: t.numpy().reshape(-1)                                  # noqa: E731
        v, t, _, _ = np_extremum(which, coeffs.numpy(), seg_ta.numpy(), seg_tb.numpy(), sign, flat(seg), flat(x), flat(tq),
                                 flat(seg2), flat(x2), flat(tq2))
        values.copy_(torch.from_numpy(v))
        times.copy_(torch.from_numpy(t))


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_dense_oracle.py's fixture with the extended oracle."""
    assert issubclass(ExtremumOracle, DenseOracle)
    wrapped = ExtremumOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def oracle_extremum(dense, which, qa, qb):
    """`maximum` / `minimum` of a CPU record from the numpy oracle, for [Q, B] true-time windows (qa, qb); the search is the
    torch oracle of tests/_rowwise_dense_oracle.py -> (values, times as tensors [Q, B, L], where, xs)."""
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
    v, t, where, xs = np_extremum(which, dense.coeffs.numpy(), ta.numpy(), tb.numpy(), sign, *found)
    shape = (qa.shape[0], *dense._shape)
    return torch.from_numpy(v).view(shape), torch.from_numpy(t).view(shape), where.reshape(*shape, 2), xs.reshape(shape)


# -- 2. exact rationals from the wire format -------------------------------------------------------------------------------------
SAMPLES = 257


def _poly(q, s, k):
    return [Fraction(float(q[p, s, k])) for p in range(5)]


def _exact_p(co, x):
    e, d, c, b, a = co
    return e + x * (d + x * (c + x * (b + x * a)))


def exact_window_check(dense, which, r, t_a, t_b, values, where, xs):
    """Row r on the window between the true times `t_a` and `t_b`: the exact p at SAMPLES points of every segment of the window
    (the clipped ends included) against the exact p at the reported x* (`where`, `xs` of `np_extremum`, per element), and the
    reported `values` against the same -> the largest (excess / bound, value error / bound) seen, both asserted <= 1."""
    sign = dense._sign
    off = dense.offsets.tolist()
    start = [Fraction(v) * int(sign) for v in dense.seg_start.tolist()]        # solver time
    end = [Fraction(v) * int(sign) for v in dense.seg_end.tolist()]
    q = dense.coeffs.to(torch.float64)
    lo, hi = sorted((Fraction(float(t_a)) * int(sign), Fraction(float(t_b)) * int(sign)))
    first = next((s for s in range(off[r], off[r + 1]) if lo <= end[s]), off[r + 1] - 1)
    last = next((s for s in range(off[r], off[r + 1]) if hi <= end[s]), off[r + 1] - 1)
    flip = 1 if which == MAXIMUM else -1
    worst = [Fraction(0), Fraction(0)]
    for k in range(q.shape[2]):
        s_star, x_star = int(where[k, 0]), Fraction(float(xs[k]))
        assert first <= s_star <= last
        co_star = _poly(q, s_star, k)
        p_star, S_star = _exact_p(co_star, x_star), sum(abs(v) for v in co_star)
        got = Fraction(float(values[k]))
        bound_v = 9 * U64 * S_star + U_T[dense.coeffs.dtype] * abs(got)
        assert abs(got - p_star) <= bound_v, (r, k, float(abs(got - p_star)), float(bound_v))
        if bound_v:
            worst[1] = max(worst[1], abs(got - p_star) / bound_v)
        for s in range(first, last + 1):
            h = end[s] - start[s]
            xlo = (lo - start[s]) / h if s == first else Fraction(0)
            xhi = (hi - start[s]) / h if s == last else Fraction(1)
            co = _poly(q, s, k)
            e, d, c, b, a = (abs(v) for v in co)
            bound = 16 * U64 * (d + 2 * c + 3 * b + 4 * a) + 9 * U64 * (e + d + c + b + a + S_star)
            for j in range(SAMPLES):
                y = xlo + (xhi - xlo) * Fraction(j, SAMPLES - 1)
                excess = flip * (_exact_p(co, y) - p_star)
                assert excess <= bound, (r, k, s, j, float(excess), float(bound))
                if bound:
                    worst[0] = max(worst[0], excess / bound)
    return worst


# -- 3. the oscillator problem -----------------------------------------------------------------------------------------------------
def oscillator_problem(B, L, dtype, device="cpu"):
    """Per row L // 2 oscillators q'' = -w^2 q with distinct w in [1, 9], q(0) = 1, q'(0) = 0: the state is [q_0 .., v_0 ..]
    (an odd L adds one element y' = -y, y(0) = 1), q_i = cos(w_i t), v_i = -w_i sin(w_i t).  Elementwise, no transcendental
    (the same func bits on every backend); `func(t, y, rows=None)` serves the calls with and without `compact`.
    -> (y0, func, w [B, L // 2] fp64, t1 [B] in [2, 3])."""
    m = L // 2
    w = torch.linspace(1.0, 9.0, B * m, dtype=torch.float64).view(m, B).t().contiguous()
    y0 = torch.cat([torch.ones(B, m), torch.zeros(B, m), torch.ones(B, L - 2 * m)], dim=1).to(device, dtype)
    w2 = (w * w).to(device, dtype)

    def func(t, y, rows=None):
        k = w2 if rows is None else w2[rows]
        return torch.cat([y[:, m:2 * m], -k * y[:, :m], -y[:, 2 * m:]], dim=1)
    return y0, func, w, torch.linspace(2.0, 3.0, B, dtype=torch.float64, device=device)


def windows(dense, seed=11):
    """True-time windows (qa, qb) [8, B] on the CPU for a record on any device: two random pairs (unordered), the whole row, the
    whole row reversed, inside the first segment, across the first interior breakpoint, from that breakpoint into the next
    segment, and a single point (the breakpoint).  Every row needs two segments."""
    off = dense.offsets.tolist()
    sign = dense._sign
    t0, t1, start, end = dense.t0.cpu(), dense.t1.cpu(), dense.seg_start.cpu(), dense.seg_end.cpu()
    rows = range(t0.numel())
    assert all(off[r + 1] - off[r] >= 2 for r in rows)
    rnd = random_queries(4, t0 * sign, t1 * sign, seed) * sign
    mid = lambda s, u: start[s] + u * (end[s] - start[s])                      # noqa: E731
    in_a, in_b = (torch.stack([mid(off[r], u) for r in rows]) for u in (0.25, 0.75))
    brk = torch.stack([end[off[r]] for r in rows])
    nxt = torch.stack([mid(off[r] + 1, 0.5) for r in rows])
    if sign == 1.0:
        nxt = torch.minimum(nxt, t1)                                           # (a row's last step may end beyond t1)
    else:
        nxt = torch.maximum(nxt, t1)
    qa = torch.stack([rnd[0], rnd[1], t0, t1, in_a, in_b, brk, brk])
    qb = torch.stack([rnd[2], rnd[3], t1, t0, in_b, nxt, nxt, brk])
    return qa, qb
