"""Shared pieces of the tests of `RowDenseOutput.crossing_times`, written from the text of include/tdeq_hip.h (ABI 35).

1. `np_crossing_times`: numpy scalars (`np.float64`), explicit Python loops over queries, elements, segments and candidates,
   the candidates in LISTS from `_segment_candidates` and the roots from `_bisect` of tests/_rowwise_dense_extremum_oracle.py,
   the walk, state machine, location and time rule of `np_level`.  Every crossing goes to a Python list of its direction; the
   first `max_count` of each list are the answer.  It defines the bits.  `CrossingTimesOracle` puts it behind the kernels
   interface (`row_dense_level_times`), so that the `device_driver` pattern runs the device path of the method with CPU states.
2. `harmonic_problem` and its closed form: pairs u' = w v, v' = -w u from (1, 0), so u = cos(w t) and v = -sin(w t), with
   several crossings of a level per direction and row; `harmonic_closed_form` lists the crossings of u with a level inside
   (0, t_end) in the order a solve from 0 to t_end meets them.
"""
import contextlib

import numpy as np
import pytest
import torch

from _rowwise_dense_calculus_oracle import same_bits  # noqa: F401
from _rowwise_dense_extremum_oracle import _bisect, _segment_candidates
from _rowwise_dense_level_oracle import LevelOracle, broadcast_level
from _rowwise_dense_oracle import NONE, DenseOracle

from torchdiffeq_amd import _native, rowwise

f64 = np.float64
HARMONIC_LEVEL = 0.3
# the solve of the closed-form test and the bound on a crossing time: 20 x the largest distance of the host path from the closed
# form measured when the method was specified (1.07e-9 with rtol = atol = 1e-9 in fp64, 2.47e-5 with 1e-5 in fp32) — the error
# of the solve; the margin is for a backend that takes another valid step sequence under the same tolerance
HARMONIC_TOL = {torch.float64: dict(rtol=1e-9, atol=1e-9), torch.float32: dict(rtol=1e-5, atol=1e-5)}
HARMONIC_BOUND = {torch.float64: 2e-8, torch.float32: 5e-4}


# -- 1. the bits ---------------------------------------------------------------------------------------------------------------
def np_crossing_times(coeffs, level, ta, tb, sign, max_count, seg, x, tq, seg2, x2, tq2):
    """`tdeq_row_dense_level_times` on numpy arrays, `level` [n_rows, L] -> (n_rising, n_falling int32 [n, L], rising, falling
    fp64 [max_count, n, L])."""
    n, L = len(seg), coeffs.shape[2]
    n_rows = level.shape[0]
    counts = {True: np.full((n, L), -1, dtype=np.int32), False: np.full((n, L), -1, dtype=np.int32)}      # rising, falling
    lists = {True: np.full((max_count, n, L), np.nan), False: np.full((max_count, n, L), np.nan)}
    with np.errstate(all="ignore"):
        for i in range(n):
            if np.isnan(x[i]) or np.isnan(x2[i]):
                continue
            (sA, tqa), (sB, tqb) = (int(seg[i]), f64(tq[i])), (int(seg2[i]), f64(tq2[i]))
            if tqb < tqa:
                (sA, tqa), (sB, tqb) = (sB, tqb), (sA, tqa)
            for k in range(L):
                lev = f64(level[i % n_rows, k])
                state = None
                nan = False
                times = {True: [], False: []}                                # rising, falling: every crossing, in walk order
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
                            times[above == (sign > 0)].append(f64(sign) * tz)
                            state = above
                        u = v
                if not nan:
                    for rising in (True, False):
                        counts[rising][i, k] = len(times[rising])
                        for j, t in enumerate(times[rising][:max_count]):
                            lists[rising][j, i, k] = t
    return counts[True], counts[False], lists[True], lists[False]


class CrossingTimesOracle(LevelOracle):
    """`LevelOracle` plus `row_dense_level_times`, on CPU tensors."""

    @staticmethod
    def row_dense_level_times(n_rising, n_falling, rising, falling, level, coeffs, seg_ta, seg_tb, sign, seg, x, tq, seg2, x2,
                              tq2) -> None:
        assert n_rising.dtype == n_falling.dtype == torch.int32 and rising.dtype == falling.dtype == torch.float64
        assert level.dtype == coeffs.dtype and level.shape[1] == coeffs.shape[2] and sign in (1.0, -1.0)
        assert n_rising.shape == n_falling.shape == rising.shape[1:] and rising.shape == falling.shape
        assert seg.numel() % level.shape[0] == 0 and 1 <= rising.shape[0] <= 65535
        flat = lambda t: t.numpy().reshape(-1)                                  # noqa: E731
        outs = np_crossing_times(coeffs.numpy(), level.numpy(), seg_ta.numpy(), seg_tb.numpy(), sign, rising.shape[0], flat(seg),
                                 flat(x), flat(tq), flat(seg2), flat(x2), flat(tq2))
        for dst, src in zip((n_rising, n_falling, rising, falling), outs):
            dst.copy_(torch.from_numpy(src))


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_dense_oracle.py's fixture with the extended oracle."""
    assert issubclass(CrossingTimesOracle, DenseOracle)
    wrapped = CrossingTimesOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def oracle_crossing_times(dense, level, qa, qb, max_count):
    """`crossing_times` of a CPU record from the numpy oracle, for [Q, B] true-time windows (qa, qb); the search is the torch
    oracle of tests/_rowwise_dense_oracle.py -> (n_rising, n_falling [Q, B, L], rising, falling [max_count, Q, B, L])."""
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
    outs = np_crossing_times(dense.coeffs.numpy(), broadcast_level(dense, level).numpy(), ta.numpy(), tb.numpy(), sign, max_count,
                             *found)
    shape = (qa.shape[0], *dense._shape)
    return tuple(torch.from_numpy(v).view(*v.shape[:-2], *shape) for v in outs)


# -- 2. the harmonic problem -------------------------------------------------------------------------------------------------------
def harmonic_problem(B, P, tail, dtype, device="cpu"):
    """Per row P pairs u' = w v, v' = -w u from (u, v) = (1, 0), so u = cos(w t) and v = -sin(w t), with w[r, j] =
    2 pi (1 + 0.5 (r P + j) / (B P)): the state is [u_0 .., v_0 .., (exp(-t) with `tail`)], L = 2 P + tail.  Elementwise, no
    transcendental (the same func bits on every backend); `func(t, y, rows=None)` serves the calls with and without `compact`.
    u is even in t: a solve from 0 to -t1 walks the same values in decreasing true time.
    -> (y0, func, w [B, P] fp64, t1 [B] = 3 + 0.25 r)."""
    idx = torch.arange(B * P, dtype=torch.float64).view(B, P)
    w = 2 * np.pi * (1 + 0.5 * idx / (B * P))
    y0 = torch.cat([torch.ones(B, P), torch.zeros(B, P), torch.ones(B, int(bool(tail)))], dim=1).to(device, dtype)
    wd = w.to(device, dtype)

    def func(t, y, rows=None):
        k = wd if rows is None else wd[rows]
        return torch.cat([k * y[:, P:2 * P], -k * y[:, :P], -y[:, 2 * P:]], dim=1)
    return y0, func, w, 3.0 + 0.25 * torch.arange(B, dtype=torch.float64, device=device)


def harmonic_closed_form(w, t_end, level=HARMONIC_LEVEL):
    """cos(w t) against `level` in (0, 1) strictly inside (0, t_end), t_end > 0 -> (falling, rising): with a = acos(level)
    the times (a + 2 pi m) / w, m >= 0, and (-a + 2 pi m) / w, m >= 1, each increasing.  A solve from 0 to -t_end meets the
    mirrored times -t in the same order, with the two directions swapped (cos is even)."""
    a = float(np.arccos(level))
    top = int(w * t_end / (2 * np.pi)) + 2
    falling = [(a + 2 * np.pi * m) / w for m in range(top) if (a + 2 * np.pi * m) / w < t_end]
    rising = [(-a + 2 * np.pi * m) / w for m in range(1, top) if (-a + 2 * np.pi * m) / w < t_end]
    return falling, rising


def harmonic_distance(got, w, t1, descending, K):
    """`got` = crossing_times(HARMONIC_LEVEL, whole rows, max_count=K) of a harmonic solve as [B, L] counters and [K, B, L]
    lists (CPU), for a solve from 0 to t1 or, `descending`, from 0 to -t1 (mirrored times, directions swapped).  Asserts that
    the counts are exact -> (the largest distance of a listed time from the closed form — an overflowing list holds the FIRST
    K —, the number of cos lists that fit, of those that overflow).  The tail element exp(-t) passes 0.3 once, falling, at
    log(1 / 0.3) on the way up in t and never on the way down from 1."""
    B, P = w.shape
    worst, fit, overflow = 0.0, 0, 0
    for r in range(B):
        for j in range(P):
            falling, rising = harmonic_closed_form(float(w[r, j]), float(t1[r]))
            if descending:
                falling, rising = [-t for t in rising], [-t for t in falling]
            for n, times, want in ((got.n_falling, got.falling, falling), (got.n_rising, got.rising, rising)):
                assert int(n[r, j]) == len(want), (r, j, int(n[r, j]), len(want))
                fit, overflow = fit + (len(want) <= K), overflow + (len(want) > K)
                for slot, t in enumerate(want[:K]):
                    worst = max(worst, abs(float(times[slot, r, j]) - t))
    if got.n_rising.shape[1] > 2 * P:
        tail = 2 * P
        assert bool((got.n_rising[:, tail] == 0).all())
        assert bool((got.n_falling[:, tail] == (0 if descending else 1)).all())
        if not descending:
            worst = max(worst, float((got.falling[0, :, tail] - np.log(1 / HARMONIC_LEVEL)).abs().max()))
    return worst, fit, overflow


# -- 3. identities with `crossings` on the same record ---------------------------------------------------------------------------
def _walk_order(ups, downs):
    """The crossings of one element alternate: up, down, up, ... or down, up, down, ...  From the two lists in SOLVER time (all
    of them) -> True if an up-crossing comes first, False if a down-crossing, None where the lists cannot tell (equal counts
    and equal times throughout: pairs at one instant)."""
    if len(ups) != len(downs):
        return len(ups) > len(downs)
    for u, d in zip(ups, downs):
        if u != d:
            return u < d
    return None


def _time_above_from_lists(ups, downs, tqa, tqb, up_first):
    """`total` of the level walk from the crossing times in solver time, left to right: an up-crossing sets t_up, a
    down-crossing adds tz - t_up, the window's end closes an open interval (fp64 scalars, the operation order of the header)."""
    total, t_up = np.float64(0.0), (None if up_first else tqa)
    merged = [t for pair in (zip(ups, downs) if up_first else zip(downs, ups)) for t in pair]
    longer = ups if len(ups) > len(downs) else downs
    merged += [longer[-1]] if len(ups) != len(downs) else []
    goes_up = up_first
    for tz in merged:
        if goes_up:
            t_up = tz
        else:
            total = total + (tz - t_up)
            t_up = None
        goes_up = not goes_up
    if t_up is not None:
        total = total + (tqb - t_up)
    return total


def check_identities(got, ref, qa, qb, sign, K):
    """`got` = crossing_times and `ref` = crossings of the same record, level and [Q, B] windows (CPU tensors) -> the number
    of elements whose `time_above` was rebuilt from the two lists."""
    count = got.n_rising + got.n_falling
    assert torch.equal(torch.where(got.n_rising < 0, -1, count).to(torch.int32), ref.count)
    assert torch.equal(got.n_rising < 0, ref.count < 0) and torch.equal(got.n_falling < 0, ref.count < 0)
    assert bool(((got.n_rising - got.n_falling).abs() <= 1).all())
    # the earlier of rising[0], falling[0] in the direction of the solve is `first`
    r0, f0 = sign * got.rising[0], sign * got.falling[0]                     # solver time; NaN = none
    inf = torch.full_like(r0, float("inf"))
    earliest = sign * torch.minimum(torch.where(torch.isnan(r0), inf, r0), torch.where(torch.isnan(f0), inf, f0))
    some = ref.count > 0
    assert same_bits(earliest[some], ref.first[some]) and bool(torch.isnan(ref.first[~some]).all())
    # each list is monotone in the direction of the solve
    for times in (got.rising, got.falling):
        step = sign * (times[1:] - times[:-1])
        assert bool((step[~torch.isnan(step)] >= 0).all())
    fits = (got.n_rising >= 0) & (got.n_rising <= K) & (got.n_falling <= K)
    ups, downs = (got.rising, got.falling) if sign > 0 else (got.falling, got.rising)
    n_up, n_dn = (got.n_rising, got.n_falling) if sign > 0 else (got.n_falling, got.n_rising)
    rebuilt = 0
    for j, r, k in fits.nonzero().tolist():
        u = [np.float64(sign) * np.float64(v) for v in ups[:int(n_up[j, r, k]), j, r, k].tolist()]
        d = [np.float64(sign) * np.float64(v) for v in downs[:int(n_dn[j, r, k]), j, r, k].tolist()]
        tqa, tqb = sorted((np.float64(sign) * np.float64(qa[j, r]), np.float64(sign) * np.float64(qb[j, r])))
        want = np.float64(ref.time_above[j, r, k])
        if u or d:                                                           # where both lists fit, the later last entry is `last`
            assert np.float64(sign) * max(u[-1:] + d[-1:]) == np.float64(ref.last[j, r, k])
        order = _walk_order(u, d)
        if order is None:                                                    # no crossing, or pairs at one instant: the state at
            options = [_time_above_from_lists(u, d, tqa, tqb, first) for first in (True, False)]      # the start is not in the lists
            assert any(v.tobytes() == want.tobytes() for v in options), (j, r, k)
        else:
            assert _time_above_from_lists(u, d, tqa, tqb, order).tobytes() == want.tobytes(), (j, r, k)
            rebuilt += 1
    return rebuilt
