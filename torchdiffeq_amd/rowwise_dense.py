"""`odeint_rowwise_dense`: a batch of independent IVPs whose solution can be evaluated AFTER the solve, per row.

`odeint_rowwise` needs every output time up front; `odeint_dense` treats the batch as one system.  Here row r of
`y0[B, *row_shape]` is integrated from `t0[r]` to `t1[r]` by the per-row controller of `odeint_rowwise` — the solve on the
grid `[t0, t1]`: the same driver (`rowwise._solve`), launches and controller — and the quartic of EVERY accepted step of
every row is kept.  The result evaluates `y_r(t)` at any time inside the row's interval with the bits `odeint_rowwise`
gives for that time as an output time (an interior output time does not change a row's step sequence).

Rows accept very different numbers of steps, so the store is ragged (`RowDenseStore`): during the solve the quartics go to
CHUNKS of `cap` slots (`[5, cap, L]` plus per-slot metadata: original row, index of the step within its row, the step's
ends), filled in arrival order; after it the chunks are packed once into `coeffs [5, n_seg, L]`, row r's segments
contiguous and in step order at `offsets[r] : offsets[r + 1]`.  The store is the solve's step hook (rowwise.py): what it
adds to a trial step sits between the controller and the commit, because the commit overwrites y and f0:
`tdeq_row_dense_slots` gives every accepted row a slot, `tdeq_row_event_fit_mapped` writes its quartic there.  The
host keeps an upper bound of the slots taken (a step accepts at most `n_active` rows) and reads the chunk's true counter —
one word — only when that bound leaves no room.  An evaluation is `tdeq_row_dense_search` (per query: the row's segment
and the fraction of the step) followed by `tdeq_row_event_eval_mapped`.  The derivative, antiderivative and integral of the
record are the same search followed by `tdeq_row_dense_calc`; the two integrals read a per-row prefix of whole-step
integrals that `tdeq_row_dense_prefix` builds on first use.  The maximum and minimum over a time window are the search of both ends followed
by `tdeq_row_dense_extremum`, which walks the window's segments and builds nothing; the crossings of a level and the time
above it are the same two searches followed by `tdeq_row_dense_level`, the same walk with a state machine; the area between
the record and a level, above and below it, is the same again with `tdeq_row_dense_exposure`, which integrates `y - level`
piece by piece while it walks; the times of ALL crossings, by direction, are the same walk with `tdeq_row_dense_level_times`,
which stores every located time at once; the mean, variance and covariance ALONG TIME inside a row are the same two searches
followed by `tdeq_row_dense_time_moments`, two walks over the Gauss-Legendre nodes of the window's steps, and for the
covariance `tdeq_row_dense_time_gram`, a weighted Gram matrix of the node values on the fp64 matrix instructions; the LAGGED
covariance along time is those, a third search per lag and `tdeq_row_dense_time_lagged`, one walk with two cursors over the
merged breakpoints of `t` and `t + lag`, or `tdeq_row_dense_time_lagged_gram`, its non-symmetric Gram product; the order
statistics across rows are one search followed by
`tdeq_row_dense_quantiles`, a radix select that evaluates the record in every pass; the mean, variance and covariance across
rows are one search followed by `tdeq_row_dense_moments`, two passes of fp64 sums over slabs of rows merged in a fixed order,
the covariance as a Gram matrix of deviations on the fp64 matrix instructions; the covariance with per-row covariates is one
search followed by `tdeq_row_dense_cross`, the same mean pass and a rectangular Gram kernel; the population ranks of given
values, the inverse of the order statistics, are one search followed by `tdeq_row_dense_ranks`, one counting pass with the
counters in registers.  CPU states run the same steps as torch / numpy ops.
"""
from __future__ import annotations

import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from . import rowwise
from ._native import TDEQ_ROW_CROSS_MAX_BLOCKS, TDEQ_ROW_MOMENTS_MAX_COV_LEN, TDEQ_ROW_QUANTILES_MAX_RANKS, \
    TDEQ_ROW_RANKS_MAX_VALUES, TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN, device_guard
from .rowwise import _Problem

__all__ = ["odeint_rowwise_dense", "RowDenseOutput", "RowDenseExtremum", "RowDenseCrossings", "RowDenseCrossingTimes",
           "RowDenseExposure", "RowDenseMoments", "RowDenseRanks", "RowDenseTimeMoments", "RowDenseAutocovariance"]

# the default chunk: CHUNK_ROWS_PER_ROW slots per row of the batch, at most CHUNK_BYTES of coefficients, never fewer than B
CHUNK_ROWS_PER_ROW = 4
CHUNK_BYTES = 256 << 20
QUANTILES_WORKSPACE_BYTES = 256 << 20                        # `quantiles` slices its query times to keep its workspace below
MOMENTS_WORKSPACE_BYTES = 256 << 20                          # and so does `moments`
_NONE = 0x7FFFFFFF                                          # the search's status word: no query out of range


def _dense_time(name: str, v, B: int) -> torch.Tensor:
    """`t0` / `t1` -> fp64 CPU tensor [B]."""
    if isinstance(v, torch.Tensor) and v.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"odeint_rowwise_dense does not propagate gradients ({name} requires grad); detach "
                                  "it or call it under torch.no_grad()")
    return rowwise._row_times("odeint_rowwise_dense", name, v, B)


def _dense_grid(t0, t1, B: int) -> torch.Tensor:
    """The [2, B] fp64 grid [t0, t1] of the solve."""
    start, end = _dense_time("t0", t0, B), _dense_time("t1", t1, B)
    if not (bool(torch.isfinite(start).all()) and bool(torch.isfinite(end).all())):
        raise ValueError("odeint_rowwise_dense: t0 and t1 must be finite")
    return rowwise._row_grid("odeint_rowwise_dense", start, "t1", end)


def _chunk_rows(options: dict, p_B: int, L: int, itemsize: int) -> int:
    """The slots of a chunk: `options['dense_chunk_rows']` (>= 1) or the default policy, raised to at least B — a trial
    step can accept every row, and `tdeq_row_event_fit_mapped` wants no fewer rows in `q` than in the batch."""
    rows = options.pop("dense_chunk_rows", None)
    if rows is None:
        rows = min(CHUNK_ROWS_PER_ROW * p_B, CHUNK_BYTES // (5 * max(L, 1) * itemsize))
    elif isinstance(rows, bool) or not isinstance(rows, int) or rows < 1:
        raise ValueError(f"odeint_rowwise_dense: dense_chunk_rows must be an integer >= 1, got {rows!r}")
    return max(int(rows), p_B)


class _Chunk:
    def __init__(self, cap: int, L: int, dtype, device):
        self.q = torch.empty(5, cap, L, dtype=dtype, device=device)
        self.row = torch.empty(cap, dtype=torch.int32, device=device)
        self.ord = torch.empty(cap, dtype=torch.int32, device=device)
        self.ta = torch.empty(cap, dtype=torch.float64, device=device)
        self.tb = torch.empty(cap, dtype=torch.float64, device=device)
        self.counter = torch.zeros(2, dtype=torch.int32, device=device)     # {used, overflow}


class RowDenseStore:
    """The quartics of one dense solve while it runs: chunks of `cap` slots, the step hook (rowwise.py) and the pack into
    the result."""

    stopped_now = None                                       # a dense solve stops no row

    def __init__(self, p: _Problem, cap: int):
        self.p, self.cap = p, cap
        self.chunks = []                                     # in the order they were opened; the last one is being filled
        self.bound = 0                                       # an upper bound of the slots taken in it
        self.n_chunks = 0
        self.slot = torch.empty(p.B, dtype=torch.int32, device=p.device)
        self.mask = torch.empty(p.B, dtype=torch.int32, device=p.device)

    def keep_rows(self, keep: torch.Tensor) -> None:
        pass                                                 # (a slot names its row by original index: a repack moves nothing)

    def before_step(self, n_active: int) -> None:
        """Before a trial step with `n_active` active rows (it accepts at most that many): make sure the current chunk has
        room for them.  The chunk's counter is read only when the bound leaves none."""
        if self.chunks and self.cap - self.bound < n_active:
            self.bound = int(self.chunks[-1].counter[0])     # the one word
        if not self.chunks or self.cap - self.bound < n_active:
            p = self.p
            self.chunks.append(_Chunk(self.cap, p.L, p.dtype, p.device))
            self.n_chunks += 1
            self.bound = 0
        self.bound += n_active

    def device_step(self, kern, y, y1, f0, f1, mid, coefs, dts) -> None:
        ch, n = self.chunks[-1], kern.n
        slot, mask = self.slot[:n], self.mask[:n]
        kern.k.row_dense_slots(kern.st, kern.row_map, self.cap, ch.counter, ch.row, ch.ord, ch.ta, ch.tb, slot, mask)
        kern.k.row_event_fit_mapped(ch.q, slot, mask, y, y1, f0, f1, mid, coefs, dts)

    def host_step(self, kern, accepted, y, y1, f0, f1, ks, dts) -> None:
        """The same as torch / numpy ops: slots in row order."""
        rows = [r for r, _, _ in accepted]
        if not rows:
            return
        ch = self.chunks[-1]
        used = int(ch.counter[0])
        ch.counter[0] = used + len(rows)
        if used + len(rows) > self.cap:
            ch.counter[1] = 1
            return
        at = slice(used, used + len(rows))
        ch.q[:, at] = kern.step_quartic(torch.tensor(rows), y, y1, f0, f1, ks, dts)
        ch.row[at] = torch.from_numpy((np.asarray(rows) if kern.row_map is None else kern.row_map[rows]).astype(np.int32))
        ch.ord[at] = torch.from_numpy((kern.n_acc[rows] - 1).astype(np.int32))
        ch.ta[at] = torch.from_numpy(kern.tprev[rows])
        ch.tb[at] = torch.from_numpy(kern.t0[rows])

    # -- after the loop --------------------------------------------------------------------------------------------------
    def finalize(self, kern, n_acc: torch.Tensor):
        """Pack the chunks: -> (offsets [B + 1] int64, seg_ta, seg_tb [n_seg] fp64 in solver time, coeffs [5, n_seg, L]),
        all on the state's device.  `n_acc`: the accepted steps by original row (int64, CPU).  Every chunk is released
        before the next one is packed."""
        p, dev = self.p, self.p.device
        offsets = torch.zeros(p.B + 1, dtype=torch.int64)
        torch.cumsum(n_acc, 0, out=offsets[1:])
        n_seg = int(offsets[-1])
        if n_seg > _NONE:
            raise RuntimeError(f"odeint_rowwise_dense: {n_seg} segments; the segment index is a 32-bit word")
        offsets = offsets.to(dev)
        coeffs = torch.empty(5, n_seg, p.L, dtype=p.dtype, device=dev)
        seg_ta = torch.empty(n_seg, dtype=torch.float64, device=dev)
        seg_tb = torch.empty(n_seg, dtype=torch.float64, device=dev)
        packed = 0
        self.chunks.reverse()
        while self.chunks:
            ch = self.chunks.pop()
            used, overflow = ch.counter.tolist()
            if overflow or used > self.cap:
                raise RuntimeError(f"odeint_rowwise_dense: internal error: a chunk of {self.cap} slots overflowed ({used} taken)")
            dest = offsets[ch.row[:used].to(torch.int64)] + ch.ord[:used].to(torch.int64)
            kern.pack_quartics(coeffs, ch.q, dest, used)
            seg_ta[dest] = ch.ta[:used]
            seg_tb[dest] = ch.tb[:used]
            packed += used
            del ch
        if packed != n_seg:
            raise RuntimeError(f"odeint_rowwise_dense: internal error: {packed} quartics kept for {n_seg} accepted steps")
        return offsets, seg_ta, seg_tb, coeffs


class RowDenseExtremum(NamedTuple):
    """`RowDenseOutput.maximum` / `.minimum`: per element the extreme value (the state's dtype) and the true time (fp64) at
    which that element attains it."""
    values: torch.Tensor
    times: torch.Tensor


class RowDenseCrossings(NamedTuple):
    """`RowDenseOutput.crossings`: per element the number of crossings of the level inside the window (int32; -1 where the
    answer is NaN), the fp64 true times of the first and the last crossing met in the direction of the solve (NaN if `count
    <= 0`) and the total true-time duration (fp64, >= 0) with `y > level` inside the window."""
    count: torch.Tensor
    first: torch.Tensor
    last: torch.Tensor
    time_above: torch.Tensor


class RowDenseCrossingTimes(NamedTuple):
    """`RowDenseOutput.crossing_times`: per element the number of rising and of falling crossings of the level inside the
    window (int32, ALL of them; -1 where the answer is NaN) and the fp64 true times of the first `max_count` crossings of each
    direction in the order the walk meets them — the direction of the solve — as `[max_count, ...]` lists padded with NaN from
    index `min(n, max_count)` on.  Rising is meant in true time: `y` goes from `<= level` to `> level` as true time increases."""
    n_rising: torch.Tensor
    n_falling: torch.Tensor
    rising: torch.Tensor
    falling: torch.Tensor


class RowDenseExposure(NamedTuple):
    """`RowDenseOutput.exposure`: per element the integral of `max(y - level, 0)` and of `max(level - y, 0)` over the window (the
    state's dtype, >= 0, true-time durations times state units) and the total true-time duration (fp64, >= 0) with `y >
    level` inside the window, which is `RowDenseCrossings.time_above` bit for bit."""
    area_above: torch.Tensor
    area_below: torch.Tensor
    time_above: torch.Tensor


class RowDenseMoments(NamedTuple):
    """`RowDenseOutput.moments`: per time the number of rows that took part (int64 `[Q]`), per element their mean and their
    variance (fp64 `[Q, *row_shape]`) and, with `covariance=True`, the covariance between the elements of the row (fp64 `[Q,
    L, L]`, exactly symmetric, its diagonal is `variance`), else None."""
    count: torch.Tensor
    mean: torch.Tensor
    variance: torch.Tensor
    covariance: torch.Tensor | None


class RowDenseRanks(NamedTuple):
    """`RowDenseOutput.ranks`: per threshold, time and element the number of rows of the population whose value sorts below
    the threshold and the number that equal it (int64 `[V, Q, *row_shape]`), and per time the size of the population (int64
    `[Q]`); under `weights=` all three count the fixed-point units of the weights."""
    below: torch.Tensor
    equal: torch.Tensor
    total: torch.Tensor


class RowDenseTimeMoments(NamedTuple):
    """`RowDenseOutput.time_moments`: per window its true-time duration `T` (fp64 `[Q, B]`), per element the time mean `(1/T)
    int y dt` and the variance `(1/T) int (y - mean)^2 dt` around it (fp64 `[Q, B, *row_shape]`) and, with `covariance=True`,
    the covariance along time between the elements of the row (fp64 `[Q, B, L, L]`, exactly symmetric, its diagonal is
    `variance`), else None."""
    duration: torch.Tensor
    mean: torch.Tensor
    variance: torch.Tensor
    covariance: torch.Tensor | None


class RowDenseAutocovariance(NamedTuple):
    """`RowDenseOutput.autocovariance`: per window its true-time duration `T` and per element the time mean (fp64 `[Q, B]` and
    `[Q, B, *row_shape]`: those of `time_moments`, bit for bit), per lag and element the autocovariance `C_ii(tau)` around that
    mean (fp64 `[K, Q, B, *row_shape]`) and, with `covariance=True`, the lagged covariance `C_ij(tau)` between the elements of
    the row (fp64 `[K, Q, B, L, L]`, `i` at `t` and `j` at `t + tau`, not symmetric; its diagonal is `autocovariance`), else
    None."""
    duration: torch.Tensor
    mean: torch.Tensor
    autocovariance: torch.Tensor
    covariance: torch.Tensor | None


class RowDenseOutput:
    """The piecewise quartic of a rowwise solve; `dense(t)` evaluates it, `derivative(t)`, `antiderivative(t)` and
    `integral(ta, tb)` give its time derivative and its integrals in closed form, `maximum(ta, tb)` and `minimum(ta, tb)` its
    extrema over a time window and their times, `crossings(level, ta, tb)` and `time_above(level, ta, tb)` its crossings of a
    level and the time spent above it, `crossing_times(level, ta, tb, max_count)` the times of all its crossings by direction,
    `exposure(level, ta, tb)`, `area_above(level, ta, tb)` and `area_below(level, ta, tb)` the area between it and a level,
    `time_moments(ta, tb)` its mean, variance and covariance along time inside each row,
    `quantiles(t, probs)` its order statistics across the rows, `moments(t)` their mean, variance and covariance,
    `cross_covariance(t, other)` their covariance with per-row covariates, `ranks(t, values)` and `cdf(t, values)` where given
    values stand among the rows (see `odeint_rowwise_dense`).

    Attributes (the wire format, all on the state's device): `t0`, `t1` `[B]` fp64 in true time; `offsets` `[B + 1]` int64;
    `seg_start`, `seg_end` `[n_seg]` fp64 in true time, row r's segments — its accepted steps — contiguous and in step
    order at `offsets[r] : offsets[r + 1]`; `coeffs` `[5, n_seg, L]` in the state's dtype, planes e, d, c, b, a of
    `y(x) = e + d x + c x^2 + b x^3 + a x^4` with x the fraction of the step; `n_segments` = `n_seg` =
    `n_accepted.sum()`.  Within a row `seg_start[s + 1] == seg_end[s]`, the first start is `t0[r]`, and the last end may lie
    beyond `t1[r]`."""

    def __init__(self, p: _Problem, kernels, offsets, seg_ta, seg_tb, coeffs):
        self._sign, self._shape, self._k = p.sign, tuple(p.shape), kernels
        self._t0, self._t1 = p.tgrid[0].to(p.device), p.tgrid[1].to(p.device)      # solver time, as the search takes them
        self._ta, self._tb = seg_ta, seg_tb
        self.offsets, self.coeffs = offsets, coeffs
        self.n_segments = int(seg_ta.numel())
        self._prefix = None                                  # fp64 [n_seg, L], built by the first antiderivative / integral
        if p.sign == 1.0:
            self.t0, self.t1, self.seg_start, self.seg_end = self._t0, self._t1, seg_ta, seg_tb
        else:
            self.t0, self.t1, self.seg_start, self.seg_end = (v * p.sign for v in (self._t0, self._t1, seg_ta, seg_tb))

    def _queries(self, t):
        """t -> (fp64 [Q, B] in solver time on the state's device, t was a single time)."""
        B, dev = self._shape[0], self.coeffs.device
        if isinstance(t, torch.Tensor):
            if t.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (t requires "
                                          "grad); detach it or evaluate under torch.no_grad()")
            if t.is_complex() or t.dtype == torch.bool or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != B):
                raise ValueError(f"dense(t): t must be a number, a 0-dim tensor, [Q] or [Q, B] = [Q, {B}], got a {t.dtype} "
                                 f"tensor of shape {tuple(t.shape)}")
            tq = t.detach().to(device=dev, dtype=torch.float64)
        elif isinstance(t, (int, float)) and not isinstance(t, bool):
            tq = torch.tensor(float(t), dtype=torch.float64, device=dev)
        else:
            raise ValueError(f"dense(t): t must be a number or a tensor, got {type(t).__name__}")
        single = tq.dim() == 0
        if tq.dim() < 2:
            tq = tq.reshape(-1, 1).expand(-1, B)
        return (tq * self._sign).contiguous(), single

    def _search_host(self, tq):
        """The search as numpy ops -> (seg int32 [Q * B], x [Q * B] in the state's dtype, first out-of-range index)."""
        Q, B = tq.shape
        T = np.float32 if self.coeffs.dtype == torch.float32 else np.float64
        q, off = tq.numpy(), self.offsets.numpy()
        ta, tb, t0, t1 = self._ta.numpy(), self._tb.numpy(), self._t0.numpy(), self._t1.numpy()
        ok = (q >= t0) & (q <= t1)                           # (a NaN fails both)
        seg = np.empty((Q, B), dtype=np.int64)
        for r in range(B):
            ends = tb[off[r]:off[r + 1]]
            # the first s with tq <= seg_tb[s]; the last segment ends at or beyond t1, so it is the answer if none before is
            seg[:, r] = off[r] + np.minimum(np.searchsorted(ends, np.where(ok[:, r], q[:, r], t0[r]), side="left"),
                                            len(ends) - 1)
        seg = np.where(ok, seg, off[:-1][None, :])
        with np.errstate(all="ignore"):
            x = np.where(ok, ((q - ta[seg]) / (tb[seg] - ta[seg])).astype(T), T(np.nan))
        bad = np.flatnonzero(~ok.reshape(-1))
        first = int(bad[0]) if bad.size else _NONE
        return torch.from_numpy(seg.reshape(-1).astype(np.int32)), torch.from_numpy(x.reshape(-1).astype(T)), first

    def _search_device(self, tq: torch.Tensor, status: torch.Tensor):
        """`search` with the status word given: int32 [1], preset to 0x7FFFFFFF -> (seg, x)."""
        dev = self.coeffs.device
        n = tq.numel()
        seg = torch.empty(n, dtype=torch.int32, device=dev)
        x = torch.empty(n, dtype=self.coeffs.dtype, device=dev)
        self._k.row_dense_search(tq, self.offsets, self._ta, self._tb, self._t0, self._t1, seg, x, status)
        return seg, x

    def search(self, tq: torch.Tensor):
        """The segment lookup alone, on the device kernels: `tq` fp64 `[Q, B]` in SOLVER time, contiguous, on the state's
        device -> (seg int32 [Q * B], x [Q * B] in the state's dtype, status int32 [1]: the smallest out-of-range query
        index, 0x7FFFFFFF for none — still on the device, not read)."""
        status = torch.full((1,), _NONE, dtype=torch.int32, device=self.coeffs.device)
        return (*self._search_device(tq, status), status)

    def _ask(self, what: str, names, ts, check: bool, spec, host, device, prefix: bool = False, flags: list | None = None):
        """The steps every query method shares.  The query lists `ts` (called `names` in messages) are parsed and broadcast
        against each other; the outputs are allocated from `spec`, one (dtype, leading dimensions) each, as `[*leading, Q * B,
        L]`; every list is searched; then the one evaluation: for a CPU state `host(lists)` gives the outputs' values, else
        `device(outs, lists)` launches into them, with `lists` = [seg, x, tq] of every list in turn, `tq` in solver time, and
        with `prefix` the prefix store as one more argument.  With `check` the status words of the searches are read once and
        the first out-of-range query raises -> the outputs as `[*leading, Q, B, *row_shape]`, without the Q of single times.
        `flags`: a list of further status words of the caller's own; `device` gets them as one more int32 tensor to fill, and
        with `check` their values come back in the list from the same read (`host` fills the list itself)."""
        tqs, single = self._query_lists(what, names, ts)
        Q, B = tqs[0].shape
        if self._k is not None and Q * B >= _NONE:
            raise ValueError(f"{what}: {Q * B} queries in one call; the query index is a 32-bit word")
        L, dev = self.coeffs.shape[2], self.coeffs.device
        outs = [torch.empty(*lead, Q * B, L, dtype=dtype, device=dev) for dtype, lead in spec]
        firsts = [_NONE] * len(tqs)
        if Q > 0:
            with torch.no_grad(), device_guard(dev):
                more = (self._integral_prefix(),) if prefix else ()
                if self._k is None:
                    found = [self._search_host(tq) for tq in tqs]
                    firsts = [first for _, _, first in found]
                    lists = [v for (seg, x, _), tq in zip(found, tqs) for v in (seg, x, tq)]
                    for dst, src in zip(outs, host(lists, *more)):
                        dst.copy_(src)
                else:
                    status = torch.full((len(tqs) + len(flags or ()),), _NONE, dtype=torch.int32, device=dev)
                    lists = [v for i, tq in enumerate(tqs) for v in (*self._search_device(tq, status[i:i + 1]), tq)]
                    device(outs, lists, *more, *((status[len(tqs):],) if flags else ()))
                    if check:
                        firsts = status.tolist()                          # the one read
                        if flags:
                            firsts, flags[:] = firsts[:len(tqs)], firsts[len(tqs):]
        if check:
            self._raise_out_of_range(what, names, tqs, firsts)
        outs = [v.view(*v.shape[:-2], Q, *self._shape) for v in outs]
        return [v.select(len(lead), 0) for v, (_, lead) in zip(outs, spec)] if single else outs

    def __call__(self, t, check: bool = True) -> torch.Tensor:
        """Row r at `t`: a number or 0-dim tensor -> `[B, *row_shape]`; `[Q]` (the same times for every row) or `[Q, B]` (times
        per row) -> `[Q, B, *row_shape]`.  A query outside `[t0[r], t1[r]]` (a NaN included) raises ValueError naming the
        first such query — or, with `check=False`, gives an all-NaN row without any host read."""
        return self._ask("dense(t)", ("t",), (t,), check, [(self.coeffs.dtype, ())],
                         lambda lists: [rowwise.HostRowKernels.eval_quartics(self.coeffs, *lists[:2])],
                         lambda outs, lists: self._k.row_event_eval_mapped(outs[0], None, self.coeffs, *lists[:2]))[0]

    # -- calculus on the record: closed forms of every segment's quartic ---------------------------------------------------
    def _integral_prefix(self) -> torch.Tensor:
        """The prefix store `P` fp64 `[n_seg, L]` (8 * L * n_seg bytes), built on first use and kept: per row the exclusive
        prefix of the whole-segment integrals in solver time, added left to right in fp64."""
        if self._prefix is None:
            if self._k is None:
                self._prefix = rowwise.HostRowKernels.quartic_prefix(self.coeffs, self.offsets, self._ta, self._tb)
            else:
                P = torch.empty(self.n_segments, self.coeffs.shape[2], dtype=torch.float64, device=self.coeffs.device)
                self._k.row_dense_prefix(P, self.coeffs, self.offsets, self._ta, self._tb)
                self._prefix = P
        return self._prefix

    def drop_integral_cache(self) -> None:
        """Release the prefix store of `antiderivative` / `integral`; the next such call rebuilds it (the same bits)."""
        self._prefix = None

    def _calculus(self, what: str, mode: int, names, ts, check: bool) -> torch.Tensor:
        """`derivative` (mode 0), `antiderivative` (1), `integral` (2) of the query lists `ts`, in the steps of `dense(t)`."""
        def host(lists, prefix=None):
            H = rowwise.HostRowKernels
            if mode == 0:
                seg, x, _ = lists
                s = seg.numpy().astype(np.int64)
                w = (self._sign * (self._tb.numpy()[s] - self._ta.numpy()[s])).astype(x.numpy().dtype)
                return [H.quartic_derivatives(self.coeffs, seg, x, torch.from_numpy(w))]
            F = [H.quartic_antiderivatives(self.coeffs, prefix, self._ta, self._tb, self._sign, *lists[i:i + 3])
                 for i in range(0, len(lists), 3)]
            return [(F[0] if mode == 1 else F[1] - F[0]).to(self.coeffs.dtype)]

        def device(outs, lists, prefix=None):
            self._k.row_dense_calc(outs[0], mode, self.coeffs, self._ta, self._tb, prefix, self._sign, *lists)
        return self._ask(what, names, ts, check, [(self.coeffs.dtype, ())], host, device, prefix=mode != 0)[0]

    def _query_lists(self, what: str, names, ts):
        """One or two query lists -> ([fp64 [Q, B] in solver time, ...] broadcast against each other, all were single)."""
        parsed = [self._queries(t) for t in ts]
        single = all(one for _, one in parsed)
        tqs = [tq for tq, _ in parsed]
        if len(tqs) == 2 and tqs[0].shape[0] != tqs[1].shape[0]:
            Qa, Qb = tqs[0].shape[0], tqs[1].shape[0]
            if 1 not in (Qa, Qb):
                raise ValueError(f"{what}: {names[0]} and {names[1]} hold {Qa} and {Qb} times; they do not broadcast")
            tqs = [tq.expand(Qa * Qb, self._shape[0]).contiguous() for tq in tqs]      # (one of them is 1: Qa * Qb is the other)
        return tqs, single

    def _raise_out_of_range(self, what: str, names, tqs, firsts) -> None:
        """ValueError for the first list that has an out-of-range query (`firsts`: the status word of each list)."""
        B = self._shape[0]
        for name, tq, first in zip(names, tqs, firsts):
            if first != _NONE:
                j, r = divmod(first, B)
                raise ValueError("{}: query {} of row {} ({} = {}) is outside the row's interval [t0, t1] = [{}, {}]".format(
                    what, j, r, name, float(tq[j, r]) * self._sign, float(self.t0[r]), float(self.t1[r])))

    def derivative(self, t, check: bool = True) -> torch.Tensor:
        """`dy_r/dt` of the interpolant at `t`, with respect to TRUE time (also for a descending solve), in the query forms
        and with the `check` of `dense(t)`.  Inside a step that is the quartic's derivative `(d + 2 c x + 3 b x^2 + 4 a x^3) /
        (tb - ta)` in the state's type; a breakpoint belongs to the earlier step, so at a breakpoint — a dose time of
        `jump_dy` included — the value is the LEFT derivative.  Never builds the prefix store."""
        return self._calculus("dense.derivative(t)", 0, ("t",), (t,), check)

    def antiderivative(self, t, check: bool = True) -> torch.Tensor:
        """`F_r(t)` = the integral of `y_r` from `t0[r]` to `t` in true time (`F_r(t0[r]) == 0` exactly), computed in fp64 —
        the prefix of the whole-step integrals before the query's step, added left to right, plus the closed-form integral
        of its quartic up to `t` — and rounded once to the state's type.  Query forms and `check` as `dense(t)`; the first
        call builds the prefix store (fp64 `[n_seg, L]`), see `drop_integral_cache`."""
        return self._calculus("dense.antiderivative(t)", 1, ("t",), (t,), check)

    def integral(self, ta, tb, check: bool = True) -> torch.Tensor:
        """The integral of `y_r` from `ta` to `tb` in true time: `T(F64(tb) - F64(ta))`, the difference of the two fp64
        antiderivatives rounded once, so `integral(a, b) == -integral(b, a)` bit for bit and `integral(a, a) == 0`.  `ta` and
        `tb` each take the query forms of `dense(t)` and broadcast against each other; both must lie inside `[t0[r], t1[r]]`
        (`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives NaN rows)."""
        return self._calculus("dense.integral(ta, tb)", 2, ("ta", "tb"), (ta, tb), check)

    # -- extrema over a time window: every segment's quartic between the window's ends -------------------------------------
    def _extremum(self, what: str, which: int, ta, tb, check: bool) -> RowDenseExtremum:
        """`maximum` (which 0) / `minimum` (1) in the steps of `integral`.  Nothing is built or kept."""
        record = (self.coeffs, self._ta, self._tb, self._sign)
        return RowDenseExtremum(*self._ask(
            what, ("ta", "tb"), (ta, tb), check, [(self.coeffs.dtype, ()), (torch.float64, ())],
            lambda lists: rowwise.HostRowKernels.quartic_extrema(*record, *lists, which == 0),
            lambda outs, lists: self._k.row_dense_extremum(*outs, which, *record, *lists)))

    def maximum(self, ta, tb, check: bool = True) -> RowDenseExtremum:
        """The largest value every ELEMENT of `y_r` takes on the closed window between `ta` and `tb` (true time, in either
        order: `maximum(a, b)` and `maximum(b, a)` have the same bits) and the time at which it takes it -> `RowDenseExtremum(
        values, times)`: `values` in the state's dtype, `times` fp64, both `[Q, B, *row_shape]` (`[B, *row_shape]` for two
        single times); elements of a row peak at different times.  `ta` and `tb` take the query forms of `integral` and
        broadcast against each other; both must lie inside `[t0[r], t1[r]]` (`check=True` names the offending query of `ta`
        first, then of `tb`; `check=False` gives NaN rows in both outputs and reads nothing).  Exact on the record: per step the
        quartic's stationary points are isolated by bisection (see `odeint_rowwise_dense`).  The window holds the
        left-continuous `dense(t)` and the RIGHT limits at the breakpoints `p` with `lo <= p < hi` (`lo`, `hi` the window's
        ends in the direction of the solve): a `jump_dy` dose at `p` inside the window or at its near end counts with the
        impulse, reported at time `p`; one at its far end does not.  Ties go to the earlier candidate in the direction of the
        solve.  Builds and caches nothing."""
        return self._extremum("dense.maximum(ta, tb)", 0, ta, tb, check)

    def minimum(self, ta, tb, check: bool = True) -> RowDenseExtremum:
        """The smallest value of every element on the window and its time: `maximum` with the comparison reversed."""
        return self._extremum("dense.minimum(ta, tb)", 1, ta, tb, check)

    # -- crossings of a level over a time window: the walk of the extrema with a state machine ------------------------------
    def _level(self, what: str, level) -> torch.Tensor:
        """level -> a contiguous `[B, L]` tensor of the state's dtype on the state's device."""
        B, L = self._shape[0], self.coeffs.shape[2]
        dev, dtype = self.coeffs.device, self.coeffs.dtype
        if isinstance(level, torch.Tensor):
            if level.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (level "
                                          "requires grad); detach it or evaluate under torch.no_grad()")
            if level.is_complex() or level.dtype == torch.bool:
                raise ValueError(f"{what}: level must be a real number or tensor, got a {level.dtype} tensor")
            lev = level.detach().to(device=dev, dtype=dtype)
        elif isinstance(level, (int, float)) and not isinstance(level, bool):
            lev = torch.tensor(float(level), dtype=dtype, device=dev)
        else:
            raise ValueError(f"{what}: level must be a number or a tensor, got {type(level).__name__}")
        try:
            lev = lev.expand(self._shape)
        except RuntimeError:
            raise ValueError(f"{what}: level of shape {tuple(lev.shape)} does not broadcast to [B, *row_shape] = "
                             f"{list(self._shape)}") from None
        return lev.reshape(B, L).contiguous()

    def _level_walk(self, what: str, level, ta, tb, check: bool, host: str, launch: str, spec, *count):
        """The steps of `crossings`, `exposure` and `crossing_times`: the level, then those of `maximum` with `launch` of the
        device kernels, or `host` of `HostRowKernels` for a CPU state (it takes `count`, the `max_count` of the lists, after
        the sign), filling outputs of `spec` (see `_ask`).  Nothing is built or kept."""
        lev = self._level(what, level)
        record = (self.coeffs, self._ta, self._tb, self._sign)
        return self._ask(
            what, ("ta", "tb"), (ta, tb), check, spec,
            lambda lists: getattr(rowwise.HostRowKernels, host)(self.coeffs, lev, *record[1:], *count, *lists),
            lambda outs, lists: getattr(self._k, launch)(*outs, lev, *record, *lists))

    def crossings(self, level, ta, tb, check: bool = True) -> RowDenseCrossings:
        """Where every ELEMENT of `y_r` crosses `level` on the window between `ta` and `tb` (true time, in either order: the
        same bits) and for how long it is above it -> `RowDenseCrossings(count, first, last, time_above)`, all `[Q, B,
        *row_shape]` (`[B, *row_shape]` for two single times): `count` int32, the crossings inside the window; `first` and
        `last` fp64, the true times of the first and the last crossing met in the direction of the solve (NaN without one);
        `time_above` fp64, the total duration (>= 0) with `y > level`, strictly.  `level` is a number or a real tensor that
        broadcasts to `[B, *row_shape]` (one for all, one per element, or one per row as `[B, 1, ...]`), rounded once to
        the state's dtype; it does not vary per query, and a NaN level gives `count = -1` and NaN for that element alone.
        `ta` and `tb` take the query forms of `integral` and broadcast against each other; both must lie inside `[t0[r],
        t1[r]]` (`check=True` names the offending query of `ta` first, then of `tb`; `check=False` gives `count = -1` and NaN
        for the whole row of such a query and reads nothing).  Exact on the record: between two neighbouring candidates of
        the walk of `maximum` the quartic is monotone, and a crossing there is found by bisection (see
        `odeint_rowwise_dense`).  The segment that starts at a breakpoint `p` is entered at its start: a `jump_dy` dose at `p`
        inside the window or at its near end that lifts the element over the level is a crossing at time `p`; one at the far
        end is not seen.  Builds and caches nothing."""
        f64 = torch.float64
        return RowDenseCrossings(*self._level_walk("dense.crossings(level, ta, tb)", level, ta, tb, check, "quartic_levels",
                                                   "row_dense_level", [(torch.int32, ()), (f64, ()), (f64, ()), (f64, ())]))

    def time_above(self, level, ta, tb, check: bool = True) -> torch.Tensor:
        """The total true-time duration every element spends strictly above `level` on the window: `crossings(level, ta, tb,
        check).time_above`, the same launch."""
        return self.crossings(level, ta, tb, check).time_above

    def crossing_times(self, level, ta, tb, max_count: int = 4, check: bool = True) -> RowDenseCrossingTimes:
        """EVERY crossing of `level` by every ELEMENT of `y_r` on the window between `ta` and `tb` (true time, in either order:
        the same bits), by direction -> `RowDenseCrossingTimes(n_rising, n_falling, rising, falling)`: `n_rising` and
        `n_falling` int32 `[Q, B, *row_shape]` (`[B, *row_shape]` for two single times), ALL the crossings of each direction
        inside the window, those beyond `max_count` included; `rising` and `falling` fp64 `[max_count, Q, B, *row_shape]`
        (`[max_count, B, *row_shape]`), the true times of the first `max_count` crossings of each direction in the order the
        walk meets them — the direction of the solve, as for `first` and `last` of `crossings`: decreasing true time for a
        descending solve — padded with NaN from index `min(n, max_count)` on.  Rising is meant in TRUE time: `y` goes from
        `<= level` to `> level` as true time increases (above is strict), so an up-crossing of a descending solve's walk is a
        falling crossing.  `n_rising + n_falling` is the `count` of `crossings`, and the earlier of `rising[0]`, `falling[0]`
        its `first`.  `level`, `ta`, `tb` and `check` are those of `crossings`: both counters are -1 and both lists all NaN
        where `count` is -1 (a NaN level for that element alone; an out-of-range query with `check=False` for its whole row,
        and nothing is read).  `max_count` is an `int` in `[1, 65535]`.  Memory: `16 * max_count` bytes per element and
        window, 537 MB for one whole-row window at 65536 x 128 with the default.  Everything `crossings` says about the
        record holds here: a `jump_dy` dose at a breakpoint inside the window or at its near end is a crossing at the stored
        dose time, the rounding-level gap at a step boundary can add a pair of crossings, a value that touches the level
        exactly and turns back is two crossings at the same time, and nothing is built or cached."""
        what = "dense.crossing_times(level, ta, tb)"
        if not isinstance(max_count, int) or isinstance(max_count, bool) or not 1 <= max_count <= 65535:
            raise ValueError(f"{what}: max_count must be an int in [1, 65535], got {max_count!r}")
        counts, times = (torch.int32, ()), (torch.float64, (max_count,))
        return RowDenseCrossingTimes(*self._level_walk(what, level, ta, tb, check, "quartic_crossing_times",
                                                       "row_dense_level_times", [counts, counts, times, times], max_count))

    # -- area above and below a level over a time window: the walk of the crossings, integrating as it goes --------------------
    def exposure(self, level, ta, tb, check: bool = True) -> RowDenseExposure:
        """The area between every ELEMENT of `y_r` and `level` on the window between `ta` and `tb` (true time, in either order:
        the same bits) -> `RowDenseExposure(area_above, area_below, time_above)`, all `[Q, B, *row_shape]` (`[B, *row_shape]`
        for two single times): `area_above` = the integral of `max(y - level, 0)` and `area_below` = the integral of
        `max(level - y, 0)`, both >= 0 and in the state's dtype (AUC above a threshold, the deficit below a target);
        `time_above` fp64, the `time_above` of `crossings`, bit for bit.  `level`, `ta`, `tb` and `check` are those of
        `crossings`: a NaN level gives NaN for that element alone, an out-of-range query with `check=False` NaN in all three
        fields for its whole row, and nothing is read.  Exact on the record: the walk of `crossings` splits the window at every
        crossing it finds and adds the closed-form integral of `y - level` over each piece, in fp64, left to right in solver
        time (see `odeint_rowwise_dense`); `area_above - area_below` is `integral(ta, tb) - level * (tb - ta)` for ascending
        ends, up to rounding.  A `jump_dy` dose at `p` switches sides at `p` with zero width, for `lo <= p < hi`; a window that
        ends at `p` does not see it, and `exposure(level, p, p)` is all zeros.  Builds and caches nothing."""
        T = self.coeffs.dtype
        return RowDenseExposure(*self._level_walk("dense.exposure(level, ta, tb)", level, ta, tb, check, "quartic_exposure",
                                                  "row_dense_exposure", [(T, ()), (T, ()), (torch.float64, ())]))

    def area_above(self, level, ta, tb, check: bool = True) -> torch.Tensor:
        """The integral of `max(y - level, 0)` over the window, per element: `exposure(level, ta, tb, check).area_above`, the
        same launch."""
        return self.exposure(level, ta, tb, check).area_above

    def area_below(self, level, ta, tb, check: bool = True) -> torch.Tensor:
        """The integral of `max(level - y, 0)` over the window, per element: `exposure(level, ta, tb, check).area_below`, the
        same launch."""
        return self.exposure(level, ta, tb, check).area_below

    # -- second moments along time: two walks over the Gauss-Legendre nodes of the window's segments -----------------------------
    def time_moments(self, ta, tb, *, covariance: bool = False, check: bool = True) -> RowDenseTimeMoments:
        """Mean, variance and covariance ALONG TIME, inside each row, over the window between `ta` and `tb` (true time, in
        either order: the same bits) -> `RowDenseTimeMoments(duration, mean, variance, covariance)`, all fp64 for both state
        dtypes, without the `Q` dimension for two single times — time-averaged second moments of a long or chaotic solve, the
        RMS amplitude of an oscillation (`sqrt(variance + mean^2)`), the L2 distance to a set point.  `duration` `[Q, B]`: `T =
        |tb - ta|`.  `mean` `[Q, B, *row_shape]`: `(1/T) int y dt`.  `variance` `[Q, B, *row_shape]`: `(1/T) int (y - mean)^2
        dt`, centred on that fp64 mean in a second walk — never `E[y^2] - E[y]^2`, and a sum of non-negative terms, so it is
        never negative.  `covariance=True` also gives `covariance` `[Q, B, L, L]`, `L = prod(row_shape) <= 256`: `(1/T) int
        (y_i - mean_i) (y_j - mean_j) dt`, exactly symmetric (the lower triangle is a copy of the upper), and `variance` is
        then its diagonal bit for bit, the rule of `moments`; that output holds `8 * Q * B * L^2` bytes (1 GiB for 65536 rows
        of 45 elements and one window), so reduce the rows or the windows of a call to what fits.  `ta` and `tb` take the
        query forms of `integral` and broadcast against each other; both must lie inside `[t0[r], t1[r]]` (`check=True` names
        the offending query of `ta` first, then of `tb`; `check=False` gives NaN in every field for the row of such a query
        and reads nothing).  Exact on the record up to rounding: every step is a quartic in the step fraction, a product of
        two deviations has degree 8, and the 5-point Gauss-Legendre rule on each step clipped to the window integrates that
        exactly (see `odeint_rowwise_dense`).  `mean * duration` is `integral(ta, tb)` for ascending ends, up to rounding.  A
        zero-length window gives `duration = 0`, `mean` = the record's value at that time in fp64 and exact zeros for the
        variance and covariance.  Breakpoints and `jump_dy` impulses have measure zero and add nothing; a non-finite
        coefficient propagates by IEEE rules.  A ROCm state runs HIP kernels: `tdeq_row_dense_time_moments`, one lane per
        window and element walking the steps twice with the mean in registers, and for the covariance
        `tdeq_row_dense_time_gram`, a weighted Gram matrix of the node values on the fp64 matrix instructions, one workgroup
        per window and pair of 64-element blocks (four windows per workgroup for `L <= 16`) walking the steps serially — no
        workspace, no atomics, the same bits from run to run; the windows of a call are launched in slices whose covariance
        stays under 256 MiB, and the result does not depend on the slicing.  A CPU state runs the same definition as numpy
        ops in fp64: the same bits for `duration`, `mean` and the variance without a covariance; for the covariance the same
        error bound, not the same last bits.  Builds and caches nothing.  Correlation matrices (divide by the SDs), moments
        pooled over rows and time, weights in time, higher moments and gradients are out of scope."""
        what = "dense.time_moments(ta, tb)"
        if not isinstance(covariance, bool):
            raise ValueError(f"{what}: covariance must be a bool, got {covariance!r}")
        B, L, dev, f64 = self._shape[0], self.coeffs.shape[2], self.coeffs.device, torch.float64
        if covariance and L > TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN:
            raise ValueError(f"{what}: covariance=True takes rows of at most {TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN} elements, "
                             f"this row has {L}")
        record = (self.coeffs, self._ta, self._tb, self._sign)
        duration, cov = torch.empty(0, dtype=f64, device=dev), torch.empty(0, L, L, dtype=f64, device=dev)

        def host(lists):
            nonlocal duration, cov
            duration, mean, var, cov = rowwise.HostRowKernels.quartic_time_moments(*record, covariance, *lists)
            return mean, var

        def device(outs, lists):
            nonlocal duration, cov
            n = lists[0].numel()
            duration = torch.empty(n, dtype=f64, device=dev)
            self._k.row_dense_time_moments(duration, *outs, *record, *lists)
            if covariance:
                cov = torch.empty(n, L, L, dtype=f64, device=dev)
                step = B * max(1, MOMENTS_WORKSPACE_BYTES // max(8 * B * L * L, 1))       # whole query times per launch
                for i in range(0, n, step):
                    self._k.row_dense_time_gram(cov[i:i + step], outs[1][i:i + step], *record,
                                                *(v.view(-1)[i:i + step] for v in lists))

        mean, var = self._ask(what, ("ta", "tb"), (ta, tb), check, [(f64, ()), (f64, ())], host, device)
        single = mean.dim() == len(self._shape)
        duration = duration.view(B) if single else duration.view(-1, B)
        if not covariance:
            return RowDenseTimeMoments(duration, mean, var, None)
        return RowDenseTimeMoments(duration, mean, var, cov.view(B, L, L) if single else cov.view(-1, B, L, L))

    # -- lagged second moments along time: one walk with two cursors over the merged breakpoints of t and t + lag ---------------
    def _lags(self, what: str, lags):
        """lags -> (fp64 `[K, B]` on the state's device, lags was a single number).  Lags that live on the host are checked
        here; those on a device by the flag of `autocovariance`."""
        B, dev = self._shape[0], self.coeffs.device
        if isinstance(lags, torch.Tensor):
            if lags.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (lags requires "
                                          "grad); detach it or evaluate under torch.no_grad()")
            if lags.is_complex() or lags.dtype == torch.bool or lags.dim() > 2 or (lags.dim() == 2 and lags.shape[1] != B) \
                    or (lags.dim() > 0 and lags.shape[0] == 0):
                raise ValueError(f"{what}: lags must be a number, a 0-dim tensor, [K] or [K, B] = [K, {B}] with K >= 1, got a "
                                 f"{lags.dtype} tensor of shape {tuple(lags.shape)}")
            lag = lags.detach().to(torch.float64)
        elif isinstance(lags, (int, float)) and not isinstance(lags, bool):
            lag = torch.tensor(float(lags), dtype=torch.float64)
        else:
            raise ValueError(f"{what}: lags must be a number or a tensor, got {type(lags).__name__}")
        if lag.device.type == "cpu" and not bool((lag >= 0).all()):
            raise ValueError(f"{what}: lags must be >= 0 and not NaN (C(-lag) is the transpose of C(lag)), got "
                             f"{lag[~(lag >= 0)].reshape(-1)[0].item()}")
        single = lag.dim() == 0
        if lag.dim() < 2:
            lag = lag.reshape(-1, 1).expand(-1, B)
        return lag.to(dev).contiguous(), single

    def autocovariance(self, ta, tb, lags, *, covariance: bool = False, check: bool = True) -> RowDenseAutocovariance:
        """The lagged second moment ALONG TIME, inside each row, over the window `[a, b]` between `ta` and `tb` (true time, in
        either order: the same bits), `T = b - a` -> `RowDenseAutocovariance(duration, mean, autocovariance, covariance)`, all
        fp64, without the `Q` dimension for two single times and without the `K` dimension for a single lag — the
        autocorrelation function of a long, oscillatory or chaotic solve and what is built on it: decorrelation times, the
        period of a limit cycle (the first maximum of `C_ii`), phase lags between components (the peak of `C_ij`), Green-Kubo
        integrals, the power spectrum.  `autocovariance` `[K, Q, B, *row_shape]`: `C_ii(tau) = 1 / (T - tau) int_a^(b - tau)
        (y_i(t) - m_i) (y_i(t + tau) - m_i) dt`, centred on the WHOLE-window mean `m` and divided by the overlap length.
        `covariance=True` also gives `covariance` `[K, Q, B, L, L]`, `L = prod(row_shape) <= 256`, entry `[i, j] = C_ij(tau)`
        with `i` at `t` and `j` at `t + tau`: not symmetric for `tau > 0`, and `autocovariance` is then its diagonal bit for
        bit; it holds `8 * K * Q * B * L^2` bytes.  `duration` `[Q, B]` and `mean` `[Q, B, *row_shape]` are those of
        `time_moments(ta, tb)` bit for bit: the same kernel runs first and its mean is an input of the lagged kernels.
        `lags`: a number, `[K]` (the same lags for every row) or `[K, B]` (lags per row), real, on any device, taken as fp64,
        `K >= 1`; a lag is a true-time offset `tau >= 0`.  Negative lags are refused: `C(-tau)` is the transpose of `C(tau)`.
        A lag is valid for a window if `tau == 0` or `0 < tau < T`; `tau == 0` on a zero-length window gives exact zeros, as
        `time_moments` does.  `check=True` raises ValueError naming the first invalid (lag, query, row) — after the
        out-of-range queries of `ta`, then `tb`, which behave as in `time_moments` — from the one read of the search's status
        words; `check=False` gives NaN for that (lag, window) alone and reads nothing.  Exact on the record up to rounding:
        the overlap is cut at the union of the breakpoints of the steps under `t` and of the steps under `t + tau` shifted by
        `-tau`; on every piece both factors are quartics in `t`, and the 5-point Gauss-Legendre rule of `time_moments`
        integrates their product exactly (include/tdeq_hip.h states the pieces, the nodes and the order of the sums).  At
        `tau = 0` `covariance` equals `time_moments(...).covariance` within the error bound, not in its last bits: another
        kernel, which stores no mirror.  A `jump_dy` impulse has measure zero.  A descending solve is handled in true time:
        in solver time the factor at `t + tau` is the EARLIER one, so the two factors swap roles; the matrix kernel does that
        once in its prologue (the per-element kernel has nothing to swap).  A ROCm state runs HIP kernels:
        `tdeq_row_dense_time_lagged`, one lane per lag, window and 16-byte element on a walk with two cursors, and for the
        matrix `tdeq_row_dense_time_lagged_gram`, a non-symmetric weighted Gram product on the fp64 matrix instructions, one
        workgroup per lag, window and ordered pair of 64-element blocks (four (lag, window) per workgroup for `L <= 16`) — no
        workspace, no atomics, the same bits from run to run; the matrix is launched in slices that stay under 256 MiB and
        does not depend on the slicing.  A CPU state runs the same definition as numpy ops in fp64: the same bits for
        `autocovariance` without a covariance, the same error bound for the covariance.  Builds and caches nothing.
        Gradients, normalisation to correlations (divide by `C_ii(0)`) and lags pooled over rows are out of scope."""
        what = "dense.autocovariance(ta, tb, lags)"
        if not isinstance(covariance, bool):
            raise ValueError(f"{what}: covariance must be a bool, got {covariance!r}")
        B, L, dev, f64 = self._shape[0], self.coeffs.shape[2], self.coeffs.device, torch.float64
        if covariance and L > TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN:
            raise ValueError(f"{what}: covariance=True takes rows of at most {TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN} elements, "
                             f"this row has {L}")
        lag, one_lag = self._lags(what, lags)
        K = lag.shape[0]
        record = (self.coeffs, self._ta, self._tb, self._sign)
        duration, cov = torch.empty(0, dtype=f64, device=dev), torch.empty(K, 0, L, L, dtype=f64, device=dev)
        flags, ends = [_NONE], []

        def third_list(lists):
            """-> (tau [K, Q * B], the first invalid (lag, query, row) as a 0-dim tensor, the lead cursor's queries [K * Q, B])."""
            tq, tq2 = lists[2], lists[5]
            ends[:] = [tq, tq2]
            Q = tq.shape[0]
            if K * Q * B >= _NONE:
                raise ValueError(f"{what}: {K * Q * B} (lag, query, row) in one call; their index is a 32-bit word")
            lo, hi = torch.minimum(tq, tq2), torch.maximum(tq, tq2)
            tau = lag[:, None, :].expand(K, Q, B).contiguous()
            valid = (tau == 0) | ((tau > 0) & (tau < hi - lo))
            invalid = ~valid.view(-1)
            first = torch.where(invalid.any(), invalid.to(torch.uint8).argmax(), _NONE)
            t3 = torch.where(valid, torch.minimum(lo + tau, hi), lo.expand(K, Q, B))
            return tau.view(K, Q * B), first, t3.view(K * Q, B).contiguous()

        def host(lists):
            nonlocal duration, cov
            H = rowwise.HostRowKernels
            tau, first, t3 = third_list(lists)
            flags[0] = int(first)
            duration, mean, _, _ = H.quartic_time_moments(*record, False, *lists)
            seg3 = self._search_host(t3)[0].view(K, -1)
            auto, cov = H.quartic_time_lagged(*record, covariance, mean, tau, seg3, *lists)
            return mean, auto

        def device(outs, lists, status):
            nonlocal duration, cov
            n = lists[0].numel()
            mean, auto = outs
            duration = torch.empty(n, dtype=f64, device=dev)
            self._k.row_dense_time_moments(duration, mean, torch.empty(n, L, dtype=f64, device=dev), *record, *lists)
            tau, first, t3 = third_list(lists)
            if check:
                status.copy_(first)
            # (a valid lag's query lies inside the window and an invalid one's at its start: this status word says nothing new)
            seg3 = self._search_device(t3, torch.full((1,), _NONE, dtype=torch.int32, device=dev))[0].view(K, n)
            if not covariance:
                self._k.row_dense_time_lagged(auto, mean, tau, seg3, *record, *lists)
                return
            cov = torch.empty(K, n, L, L, dtype=f64, device=dev)
            per = max(1, MOMENTS_WORKSPACE_BYTES // max(8 * B * L * L, 1))        # whole query times per launch
            if K * (n // B) <= per:
                self._k.row_dense_time_lagged_gram(cov, auto, mean, tau, seg3, *record, *lists)
                return
            for k in range(K):
                for i in range(0, n, B * per):
                    j = i + B * per
                    self._k.row_dense_time_lagged_gram(cov[k:k + 1, i:j], auto[k:k + 1, i:j], mean[i:j], tau[k:k + 1, i:j],
                                                       seg3[k:k + 1, i:j], *record, *(v.view(-1)[i:j] for v in lists))

        mean, auto = self._ask(what, ("ta", "tb"), (ta, tb), check, [(f64, ()), (f64, (K,))], host, device, flags=flags)
        if check and flags[0] != _NONE:
            Q = ends[0].shape[0]
            k, j, r = flags[0] // (Q * B), flags[0] // B % Q, flags[0] % B
            raise ValueError("{}: lag {} of query {} of row {} (lag = {}) is neither 0 nor inside (0, T) of its window, T = {}"
                             .format(what, k, j, r, float(lag[k, r]), abs(float(ends[1][j, r]) - float(ends[0][j, r]))))
        single = mean.dim() == len(self._shape)
        duration = duration.view(B) if single else duration.view(-1, B)
        cov = (cov.view(K, B, L, L) if single else cov.view(K, -1, B, L, L)) if covariance else None
        if one_lag:
            auto, cov = auto[0], None if cov is None else cov[0]
        return RowDenseAutocovariance(duration, mean, auto, cov)

    # -- order statistics across rows: a radix select on the record, nothing of size [Q, B, L] is built ----------------------
    def _quantile_ranks(self, what: str, probs, ranks, as_probs: bool = False) -> list:
        """`probs` or `ranks` -> the P ranks as Python ints in [0, B - 1]; `as_probs`: the checked probs as Python floats."""
        B = self._shape[0]
        if (probs is None) == (ranks is None):
            raise ValueError(f"{what}: give exactly one of probs and ranks")
        name, given = ("probs", probs) if ranks is None else ("ranks", ranks)
        if isinstance(given, (str, bytes)) or not hasattr(given, "__iter__"):
            raise ValueError(f"{what}: {name} must be a sequence of numbers, got {type(given).__name__}")
        given = given.tolist() if isinstance(given, (torch.Tensor, np.ndarray)) else list(given)
        if not 1 <= len(given) <= TDEQ_ROW_QUANTILES_MAX_RANKS:
            raise ValueError(f"{what}: {name} must hold 1 to {TDEQ_ROW_QUANTILES_MAX_RANKS} entries, got {len(given)}")
        out = []
        for v in given:
            if ranks is None:
                if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= v <= 1.0:      # (a NaN fails both)
                    raise ValueError(f"{what}: probs must be numbers in [0, 1], got {v!r}")
                out.append(float(v) if as_probs else int(math.floor(float(v) * (B - 1))))            # the "lower" rule
            else:
                if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= B - 1:
                    raise ValueError(f"{what}: ranks must be integers in [0, B - 1] = [0, {B - 1}], got {v!r}")
                out.append(int(v))
        return out

    def quantiles(self, t, probs=None, *, ranks=None, weights=None, check: bool = True) -> torch.Tensor:
        """Order statistics ACROSS the B rows: per time and per ELEMENT of the row, the value of rank `k_p` (0 = the smallest)
        among the B values `dense(t)[q, :, ...]` -> `[P, Q, *row_shape]` in the state's dtype (`[P, *row_shape]` for a single
        time) — the 5 % / 50 % / 95 % bands of a population of simulated patients, the envelope of an ensemble.  `t` takes the
        query forms of `dense(t)`.  Exactly one of `ranks`, a sequence of P integers in `[0, B - 1]`, and `probs`, a sequence of
        P numbers in `[0, 1]` mapped in Python doubles to `k = floor(p * (B - 1))` (the "lower" rule: `p = 1` is the largest
        value), with `1 <= P <= 16`; duplicates are allowed; anything else is a ValueError.  There is no interpolation between
        ranks: ask for two and combine them.  Every returned value is one of the B evaluated values with the bits `dense(t)`
        gives that row, except that among equal values `-0.0` sorts before `+0.0`; a NaN sorts last and comes back as the
        canonical quiet NaN.  `check=True` raises for the first out-of-range query like `dense(t)`, after one read of the
        status word; with `check=False` nothing is read and an out-of-range row counts as a NaN of that time's population, so
        it takes a top rank.  A ROCm state runs a radix select on HIP kernels (`tdeq_row_dense_quantiles`, ABI 36) that
        evaluates the record again in each of its `sizeof(dtype)` passes and never builds the `[Q, B, *row_shape]` values: next
        to the outputs the call allocates the search's `[Q, B]` lists and a workspace of at most 256 MiB (or that of one
        query time), and runs the times in slices that fit it.  A CPU state sorts the same integer keys with torch ops: the
        same bits.  Counts are integers, so the result does not depend on the order of the rows.  Means, variances and
        covariances across the rows are `moments(t)`; gradients are out of scope.

        `weights`: None, or the `[B]` / `[Q, B]` weights of `moments(t, weights=...)`, taken the same way (a real tensor of a
        floating or integer dtype on any device, as contiguous fp64; a single time takes `[B]` or `[1, B]`): WEIGHTED order
        statistics, the credible band of weighted particles, the band of a 0/1 subgroup.  `probs` is then required and
        `ranks=` is a ValueError (an integer rank has no meaning under real weights).  The definition is exact, independent
        of the order of the rows, and the same bits on both paths.  Population: the rows whose query is in range; with
        `check=False` an out-of-range row has LEFT the population and its weight counts as 0, as in `moments` — its weight
        may be NaN without effect — which differs from the unweighted call, where such a row counts as a NaN value.
        Validity: every weight of a row in range must be finite and `>= 0` (`-0.0` is 0); if one is not, or the population
        is empty, or its largest weight is 0, every output of that time is NaN, the other times are unaffected, and nothing
        is read or raised.  Fixed-point weights: with `wmax = f * 2^E`, `0.5 <= f < 1`, the largest weight of the population
        and `S = 62 - B.bit_length()`, `m_r = rint(ldexp(w_r, S - E))` (ties to even) as an integer, so `W = sum_r m_r <
        2^62` is exact in any order; the weight resolution is `2^-S` of the largest weight, 2^-45 at B = 65536.  Target: `K_p
        = min(max(ceil(p * float(W)), 1), W)` in IEEE fp64.  Answer, per element: the smallest value `v` whose cumulative
        weight `sum of m_r over the rows with value <= v` reaches `K_p`, in the order and with the bits of the unweighted
        call — `numpy.quantile(dense(t), p, axis=..., weights=w, method="inverted_cdf")` wherever the weights are dyadic.
        Three identities follow.  Weights that are all 1.0, or all the same power of two, give rank `max(ceil(p * n) - 1,
        0)` of the `n` rows in range (`p * n` a Python double product): NOT the `floor(p * (B - 1))` of the unweighted
        `probs`; the unweighted call that matches is `quantiles(t, ranks=[...])`.  Other equal weights, such as 3.7, can
        differ from that by one rank where `p * n` is an integer: a rounding of `p * W`, not a defect.  A weight of exactly
        0 gives the bits of the same record without that row.  Scaling all weights by a power of two changes no bit.  A
        ROCm state runs kernels of its own (`tdeq_row_dense_quantiles_weighted`): the largest weight by integer `atomicMax`
        on the weights' bit images, the units `m` as uint64 `[Q, B]` in the workspace, then the radix select with 64-bit
        counters, which skips a row of weight 0 before it loads its coefficients, so a subgroup costs what the subgroup
        costs.  Integer atomics only; the times are sliced as above."""
        what = "dense.quantiles(t)"
        if weights is not None and ranks is not None:
            raise ValueError(f"{what}: ranks has no meaning under weights; give probs")
        ks = self._quantile_ranks(what, probs, ranks, as_probs=weights is not None)
        tqs, single = self._query_lists(what, ("t",), (t,))
        tq = tqs[0]
        Q, B = tq.shape
        if self._k is not None and Q * B >= _NONE:
            raise ValueError(f"{what}: {Q * B} queries in one call; the query index is a 32-bit word")
        w = None if weights is None else self._weights_arg(what, weights, Q)
        P, L, dev, T = len(ks), self.coeffs.shape[2], self.coeffs.device, self.coeffs.dtype
        out = torch.empty(P, Q, L, dtype=T, device=dev)
        first = _NONE
        if Q > 0:
            with torch.no_grad(), device_guard(dev):
                if self._k is None:
                    seg, x, first = self._search_host(tq)
                    if w is None:
                        out.copy_(rowwise.HostRowKernels.quartic_quantiles(self.coeffs, seg, x, ks, Q, B))
                    else:
                        out.copy_(rowwise.HostRowKernels.quartic_quantiles_weighted(self.coeffs, seg, x, ks, w, Q, B))
                else:
                    status = torch.full((1,), _NONE, dtype=torch.int32, device=dev)
                    seg, x = self._search_device(tq, status)
                    on_dev = torch.tensor(ks, dtype=torch.int32 if w is None else torch.float64, device=dev)
                    per_time = self._k.row_dense_quantiles_workspace_bytes(P, 1, L, T) if w is None \
                        else self._k.row_dense_quantiles_weighted_workspace_bytes(P, 1, B, L, T)  # (linear in the times)
                    step = min(Q, max(1, QUANTILES_WORKSPACE_BYTES // max(per_time, 1)))
                    work = torch.empty(step * per_time, dtype=torch.uint8, device=dev)
                    for q0 in range(0, Q, step):
                        q1 = min(q0 + step, Q)
                        part = out if q1 - q0 == Q else torch.empty(P, q1 - q0, L, dtype=T, device=dev)
                        if w is None:
                            self._k.row_dense_quantiles(part, on_dev, self.coeffs, seg[q0 * B:q1 * B], x[q0 * B:q1 * B], work)
                        else:
                            self._k.row_dense_quantiles_weighted(part, on_dev, self.coeffs, seg[q0 * B:q1 * B], x[q0 * B:q1 * B],
                                                                 work, w if w.dim() == 1 else w[q0:q1])
                        if part is not out:
                            out[:, q0:q1] = part
                    if check:
                        first = int(status)                                                    # the one read
        if check:
            self._raise_out_of_range(what, ("t",), tqs, [first])
        out = out.view(P, Q, *self._shape[1:])
        return out.select(1, 0) if single else out

    # -- population ranks of given values: one counting pass over the record, the inverse of `quantiles` ---------------------
    def _rank_values(self, what: str, values, Q: int) -> torch.Tensor:
        """`values` of `ranks` -> the thresholds as a contiguous `[V, Q, L]` tensor of the state's dtype on its device."""
        row_shape, dev, T = self._shape[1:], self.coeffs.device, self.coeffs.dtype
        if isinstance(values, torch.Tensor):
            if values.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (values requires "
                                          "grad); detach it or evaluate under torch.no_grad()")
            if values.is_complex() or values.dtype == torch.bool:
                raise ValueError(f"{what}: values must be a real number or tensor, got a {values.dtype} tensor")
            vals = values.detach().to(device=dev, dtype=T)                                # rounded once to the state's dtype
        elif isinstance(values, (int, float)) and not isinstance(values, bool):
            vals = torch.tensor(float(values), dtype=T, device=dev)
        else:
            raise ValueError(f"{what}: values must be a number or a tensor, got {type(values).__name__}")
        shape, n = tuple(vals.shape), len(row_shape)
        if vals.dim() <= 1:
            vals = vals.reshape(-1, 1, *([1] * n))                                        # a number or [V]
        elif vals.dim() == 1 + n:
            vals = vals.unsqueeze(1)                                                      # [V, *row_shape]
        V = vals.shape[0]
        try:
            if vals.dim() != 2 + n:
                raise RuntimeError
            vals = vals.expand(V, Q, *row_shape)
        except RuntimeError:
            raise ValueError(f"{what}: values of shape {shape} is none of [V], [V, *row_shape] and [V, Q, *row_shape] with Q = "
                             f"{Q}, row_shape = {list(row_shape)}") from None
        if not 1 <= V <= TDEQ_ROW_RANKS_MAX_VALUES:
            raise ValueError(f"{what}: values must hold 1 to {TDEQ_ROW_RANKS_MAX_VALUES} thresholds, got {V}")
        return vals.reshape(V, Q, self.coeffs.shape[2]).contiguous()

    def ranks(self, t, values, *, weights=None, check: bool = True) -> RowDenseRanks:
        """Where given values stand in the population of the B rows, per time and per ELEMENT of the row: the inverse of
        `quantiles` -> `RowDenseRanks(below, equal, total)`.  `below` and `equal`, int64 `[V, Q, *row_shape]` (`[V, *row_shape]`
        for a single time), count the rows whose `dense(t)` value sorts below threshold v, and equals it; `total`, int64 `[Q]`,
        is the size of the population — the empirical CDF of an observation among simulated patients (NPDE, PIT), the fraction
        of them above a target, the rank of an observation in an ensemble.  `t` takes the query forms of `quantiles(t, ...)`.
        `values`: a number or a real tensor on any device (floating or integer; not bool, not complex, not requiring grad),
        rounded once to the state's dtype; a number or `[V]` gives the same thresholds to every time and element, `[V,
        *row_shape]` one set per element, `[V, Q, *row_shape]` one per time and element; size-1 dimensions broadcast inside
        each form and `1 <= V <= 16`; anything else is a ValueError.  The order is that of `quantiles`, on the ordered integer
        image of the bits `dense(t)` gives: `-0.0` sorts before `+0.0` (so `-0.0` does not EQUAL `+0.0`), every NaN is the one
        largest value, and a threshold may be NaN or infinite.  The population is all B rows, `total == B`; `check` as for
        `quantiles`: with `check=False` an out-of-range row is a NaN value of its time.  Hence for every rank `k` and `v =
        quantiles(t, ranks=[k])`: `below(v) <= k < below(v) + equal(v)`, element by element.

        `weights`: the `[B]` / `[Q, B]` weights of `quantiles(t, probs, weights=...)`, with its population (a row out of
        range has left; its weight is not inspected), validity rule and fixed-point units `m_r = rint(ldexp(w_r, S - E))`, `S =
        62 - B.bit_length()`, `E` from the largest weight in range.  `below` and `equal` are then sums of `m_r` and `total` is
        `W = sum_r m_r`; a time with a negative or non-finite weight in range, an empty population or a largest weight of 0
        has `below = equal = 0` and `total = 0`, and nothing is read or raised.  Scaling all weights by a power of two changes
        no bit.  All results are integer sums: exact, and independent of the order of the rows.  A ROCm state runs one
        counting pass on a HIP kernel (`tdeq_row_dense_ranks`, `tdeq_row_dense_ranks_weighted`) that keeps the thresholds' keys
        and its counters in registers and never builds `[Q, B, *row_shape]`; the weighted call keeps the units `[Q, B]` in a
        workspace and runs the times in slices that hold it under 256 MiB.  A CPU state compares the same keys with torch ops:
        the same bits.  The mid-rank PIT, histograms over bin edges (differences of `cdf`), thresholds per row and gradients
        are out of scope."""
        what = "dense.ranks(t)"
        tqs, single = self._query_lists(what, ("t",), (t,))
        tq = tqs[0]
        Q, B = tq.shape
        if self._k is not None and Q * B >= _NONE:
            raise ValueError(f"{what}: {Q * B} queries in one call; the query index is a 32-bit word")
        w = None if weights is None else self._weights_arg(what, weights, Q)
        vals = self._rank_values(what, values, Q)
        V, L, dev = vals.shape[0], self.coeffs.shape[2], self.coeffs.device
        below, equal = (torch.empty(V, Q, L, dtype=torch.int64, device=dev) for _ in range(2))
        total = torch.full((Q,), B, dtype=torch.int64, device=dev)
        first = _NONE
        if Q > 0:
            with torch.no_grad(), device_guard(dev):
                if self._k is None:
                    seg, x, first = self._search_host(tq)
                    if w is None:
                        got = rowwise.HostRowKernels.quartic_ranks(self.coeffs, seg, x, vals, Q, B)
                    else:
                        got = rowwise.HostRowKernels.quartic_ranks_weighted(self.coeffs, seg, x, vals, w, Q, B)
                    for dst, src in zip((below, equal, total), got):
                        dst.copy_(src)
                else:
                    status = torch.full((1,), _NONE, dtype=torch.int32, device=dev)
                    seg, x = self._search_device(tq, status)
                    if w is None:
                        self._k.row_dense_ranks(below, equal, vals, self.coeffs, seg, x)
                    else:
                        per_time = self._k.row_dense_ranks_weighted_workspace_bytes(1, B)     # (linear in the times)
                        step = min(Q, max(1, QUANTILES_WORKSPACE_BYTES // max(per_time, 1)))
                        work = torch.empty(step * per_time, dtype=torch.uint8, device=dev)
                        for q0 in range(0, Q, step):
                            q1 = min(q0 + step, Q)
                            whole = q1 - q0 == Q
                            part = (below, equal) if whole else tuple(torch.empty(V, q1 - q0, L, dtype=torch.int64, device=dev)
                                                                      for _ in range(2))
                            self._k.row_dense_ranks_weighted(*part, total[q0:q1], vals if whole else vals[:, q0:q1].contiguous(),
                                                             self.coeffs, seg[q0 * B:q1 * B], x[q0 * B:q1 * B], work,
                                                             w if w.dim() == 1 else w[q0:q1])
                            if not whole:
                                below[:, q0:q1], equal[:, q0:q1] = part
                    if check:
                        first = int(status)                                                    # the one read
        if check:
            self._raise_out_of_range(what, ("t",), tqs, [first])
        below, equal = (v.view(V, Q, *self._shape[1:]) for v in (below, equal))
        return RowDenseRanks(below.select(1, 0), equal.select(1, 0), total) if single else RowDenseRanks(below, equal, total)

    def cdf(self, t, values, *, weights=None, check: bool = True) -> torch.Tensor:
        """The empirical `P(Y <= v)` of the population at time `t`: `(below + equal) / total` of `ranks(t, values, ...)`, fp64
        `[V, Q, *row_shape]` (`[V, *row_shape]` for a single time), formed with torch ops from the integer counts on either
        device: the same bits.  `0 / 0`, a time without a valid population under `weights=`, is NaN.  `1 - cdf` is the
        fraction above a target; differences of `cdf` at bin edges give a histogram."""
        r = self.ranks(t, values, weights=weights, check=check)
        total = r.total.double()
        if r.below.dim() == len(self._shape) + 1:                                           # [V, Q, *row_shape]
            return (r.below + r.equal).double() / total.view(-1, *([1] * (len(self._shape) - 1)))
        return (r.below + r.equal).double() / total[0]

    def _weights_arg(self, what: str, weights, Q: int) -> torch.Tensor:
        """`weights=` of `moments` / `cross_covariance` -> contiguous fp64 `[B]` or `[Q, B]` on the record's device.  The
        values are not inspected."""
        B = self._shape[0]
        if not isinstance(weights, torch.Tensor):
            raise ValueError(f"{what}: weights must be a tensor, got {type(weights).__name__}")
        if weights.is_complex() or weights.dtype == torch.bool or tuple(weights.shape) not in ((B,), (Q, B)):
            raise ValueError(f"{what}: weights must be a real tensor [B] or [Q, B] with Q = {Q}, B = {B}, got a "
                             f"{weights.dtype} tensor of shape {tuple(weights.shape)}")
        if weights.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (weights requires "
                                      "grad); detach it or evaluate under torch.no_grad()")
        return weights.detach().to(device=self.coeffs.device, dtype=torch.float64).contiguous()

    # -- moments across rows: two passes over the record in fp64, nothing of size [Q, B, L] is built ---------------------------
    def moments(self, t, *, covariance: bool = False, correction: int = 1, weights=None, check: bool = True) -> RowDenseMoments:
        """Mean, variance and covariance ACROSS the rows, per time: the ensemble mean ± SD of a population of solves and the
        covariance between its state components -> `RowDenseMoments(count, mean, variance, covariance)`, all fp64 for both
        state dtypes (`count` int64), without the `Q` dimension for a single time.  `t` takes the query forms of `dense(t)`.
        The POPULATION of a time is the set of rows whose query is in range: `check=True` raises for the first out-of-range
        query like `dense(t)`, after one read of the status word; with `check=False` nothing is read and an out-of-range row
        has left that time's population.  `count` `[Q]`: the rows that took part.  `mean` `[Q, *row_shape]`: the fp64 sum of
        their `dense(t)` values over `count` (NaN for `count == 0`).  `variance` `[Q, *row_shape]`: the fp64 sum of `(y -
        mean)^2`, with that fp64 mean, over `count - correction` (`correction` is the int 0 or 1) — two passes, never `E[x^2] -
        E[x]^2`; a divisor that is not positive counts as zero, so a population too small gives NaN (or inf) by IEEE
        division.  `covariance=True` also gives `covariance` `[Q, L, L]`, `L = prod(row_shape) <= 1024`: the sum of `(y_i -
        mean_i) (y_j - mean_j)` over the same divisor, exactly symmetric (the lower triangle is a copy of the upper), and
        `variance` is then its diagonal bit for bit; otherwise `covariance` is None.  A non-finite value inside the record
        propagates by IEEE rules.  A ROCm state runs HIP kernels (`tdeq_row_dense_moments`, ABI 37) that evaluate the record
        again in each pass and never build the `[Q, B, *row_shape]` values; the covariance is a Gram matrix of deviations on
        the fp64 matrix instructions.  Next to the outputs the call allocates the search's `[Q, B]` lists and a workspace of
        at most 256 MiB (or that of one query time), and runs the times in slices that fit it; the rows are split by a rule of
        `(B, L)` alone and merged in a fixed order without atomics, so the result is the same from run to run and does not
        depend on the slicing.  A CPU state runs the same definition as plain torch ops in fp64: the same error bound, not the
        same last bits (another order of the sums).  The covariance with a second per-row quantity — sampled parameters, or
        the state at another time (cross-time covariance) — is `cross_covariance(t, other)`.  `weights`: None, or a real
        tensor `[B]` (one set for all times) or `[Q, B]` (one set per time: the importance weights of a particle filter; a
        single time takes `[B]` or `[1, B]`) of a floating or integer dtype on any device, taken as contiguous fp64 on the
        record's device — the reliability weights of `numpy.cov(aweights=weights, ddof=correction)`.  With `W1 = sum_r w_r`
        and `W2 = sum_r w_r^2` over the population, `mean_i = sum_r w_r y_ri / W1` and the centred sums `sum_r w_r (y_ri -
        mean_i) (y_rj - mean_j)` are divided by `D = W1 - correction * W2 / W1` (a `D` that is not positive or is NaN counts
        as zero); `count` still counts the rows in range, whatever their weights.  A row out of range contributes selected
        zeros to every sum, `W1` and `W2` included, so a NaN in its weight does not leak; 0/1 weights select a subgroup.  The
        weights' values are not inspected and the call makes no extra device read: a negative or non-finite weight of a row
        in range propagates by IEEE arithmetic.  On a ROCm state the weighted call runs kernels of its own
        (`tdeq_row_dense_moments_weighted`); with every weight 1.0 they give the bits of the unweighted call, and a weight
        of exactly 0 gives every field but `count` the bits it has when that row is out of range.  Higher moments,
        correlation matrices (divide by the SDs), the effective sample size and gradients are out of scope; weighted
        quantiles are `quantiles(t, probs, weights=...)`."""
        what = "dense.moments(t)"
        if isinstance(correction, bool) or not isinstance(correction, int) or correction not in (0, 1):
            raise ValueError(f"{what}: correction must be the int 0 or 1, got {correction!r}")
        if not isinstance(covariance, bool):
            raise ValueError(f"{what}: covariance must be a bool, got {covariance!r}")
        L, dev, T = self.coeffs.shape[2], self.coeffs.device, self.coeffs.dtype
        if covariance and L > TDEQ_ROW_MOMENTS_MAX_COV_LEN:
            raise ValueError(f"{what}: covariance=True takes rows of at most {TDEQ_ROW_MOMENTS_MAX_COV_LEN} elements, this "
                             f"row has {L}")
        tqs, single = self._query_lists(what, ("t",), (t,))
        tq = tqs[0]
        Q, B = tq.shape
        if self._k is not None and Q * B >= _NONE:
            raise ValueError(f"{what}: {Q * B} queries in one call; the query index is a 32-bit word")
        w = None if weights is None else self._weights_arg(what, weights, Q)
        count = torch.empty(Q, dtype=torch.int64, device=dev)
        mean, var = (torch.empty(Q, L, dtype=torch.float64, device=dev) for _ in range(2))
        cov = torch.empty(Q, L, L, dtype=torch.float64, device=dev) if covariance else None
        first = _NONE
        if Q > 0:
            with torch.no_grad(), device_guard(dev):
                if self._k is None:
                    seg, x, first = self._search_host(tq)
                    if w is None:
                        got = rowwise.HostRowKernels.quartic_moments(self.coeffs, seg, x, Q, B, covariance, correction)
                    else:
                        got = rowwise.HostRowKernels.quartic_moments_weighted(self.coeffs, seg, x, w, Q, B, covariance,
                                                                              correction)
                    for dst, src in zip((count, mean, var, cov), got):
                        if dst is not None:
                            dst.copy_(src)
                else:
                    status = torch.full((1,), _NONE, dtype=torch.int32, device=dev)
                    seg, x = self._search_device(tq, status)
                    space = self._k.row_dense_moments_workspace_bytes if w is None \
                        else self._k.row_dense_moments_weighted_workspace_bytes
                    per_time = space(covariance, 1, B, L, T)                                        # (linear in the times)
                    step = min(Q, max(1, MOMENTS_WORKSPACE_BYTES // max(per_time, 1)))
                    work = torch.empty(space(covariance, step, B, L, T), dtype=torch.uint8, device=dev)
                    for q0 in range(0, Q, step):
                        q1 = min(q0 + step, Q)
                        outs = (count[q0:q1], mean[q0:q1], var[q0:q1], None if cov is None else cov[q0:q1])
                        if w is None:
                            self._k.row_dense_moments(*outs, correction, self.coeffs, seg[q0 * B:q1 * B], x[q0 * B:q1 * B], work)
                        else:
                            self._k.row_dense_moments_weighted(*outs, correction, self.coeffs, seg[q0 * B:q1 * B],
                                                               x[q0 * B:q1 * B], work, w if w.dim() == 1 else w[q0:q1])
                    if check:
                        first = int(status)                                                    # the one read
        if check:
            self._raise_out_of_range(what, ("t",), tqs, [first])
        mean, var = (v.view(Q, *self._shape[1:]) for v in (mean, var))
        if single:
            return RowDenseMoments(count[0], mean[0], var[0], None if cov is None else cov[0])
        return RowDenseMoments(count, mean, var, cov)

    # -- covariance with a second per-row quantity: the mean pass of `moments`, then a rectangular Gram matrix -----------------
    def cross_covariance(self, t, other, *, correction: int = 1, weights=None, check: bool = True) -> torch.Tensor:
        """Covariance ACROSS the rows between the state and per-row covariates, per time: `C_y,theta(t)` of an ensemble Kalman
        or smoother update, the regression-based sensitivity of every component to every sampled input (divide by the SDs),
        the covariate-effect screen of a population run -> fp64 `[Q, L, M]`, `L = prod(row_shape)`; `[L, M]` for a single
        time.  `t` and `check` as for `moments(t)`: the population of a time is the set of rows whose query is in range.
        `other`: a real tensor `[B]` (`M = 1`) or `[B, M]`, `M >= 1`, of a floating or integer dtype on any device, taken as
        contiguous fp64 on the record's device.  With `n` the population's size, `ybar` the mean of `moments` and `zbar_m =
        sum_r other_rm / n` over the same population, `out[q, i, m] = sum_r (y_ri - ybar_i) (other_rm - zbar_m) / max(n -
        correction, 0)` in fp64 (`correction` is the int 0 or 1; a zero divisor: IEEE division) — two passes, never `E[yz] -
        E[y] E[z]`.  A row outside the population contributes exact zeros, so a NaN in its `other` entries does not leak; a
        non-finite entry of a row inside it propagates by IEEE rules.  Cross-time covariance is the same call: `other =
        dense(t_ref).reshape(B, L)` gives `cov(y(t), y(t_ref))` for all `t`.  A ROCm state runs HIP kernels
        (`tdeq_row_dense_cross`, ABI 38): the mean and count kernels of `moments` (the same bits), the column sums of `other`,
        and a rectangular Gram kernel on the fp64 matrix instructions with blocks of 64 elements by 16 covariates for `M <=
        16` and 64 by 64 otherwise; `ceil(L / 64) * ceil(M / W)` must be at most 1024 blocks.  No atomics, the split is a
        rule of `(B, L, M)` alone: the same bits from run to run and for any slicing of the times; the workspace stays under
        256 MiB (or that of one time).  A CPU state runs the definition as plain fp64 torch ops: the same error bound, not
        the same last bits.  `weights`: None, or the `[B]` / `[Q, B]` reliability weights of `moments(t, weights=...)`, taken
        the same way: `ybar` is the weighted mean of `moments`, `zbar_m = sum_r w_r other_rm / W1`, and `out[q, i, m] = sum_r
        w_r (y_ri - ybar_i) (other_rm - zbar_m) / D` with `D = W1 - correction * W2 / W1` (not positive or NaN: zero).  A row
        out of range contributes selected zeros, its weight included; the weights' values are not inspected, so a negative
        or non-finite weight of a row in range propagates by IEEE arithmetic.  On a ROCm state the weighted call runs
        kernels of its own (`tdeq_row_dense_cross_weighted`), which give the bits of the unweighted call for weights of
        1.0.  Weighted quantiles are `quantiles(t, probs, weights=...)`; gradients are out of scope."""
        what = "dense.cross_covariance(t, other)"
        if isinstance(correction, bool) or not isinstance(correction, int) or correction not in (0, 1):
            raise ValueError(f"{what}: correction must be the int 0 or 1, got {correction!r}")
        L, dev, T = self.coeffs.shape[2], self.coeffs.device, self.coeffs.dtype
        B = self._shape[0]
        if not isinstance(other, torch.Tensor):
            raise ValueError(f"{what}: other must be a tensor, got {type(other).__name__}")
        if other.is_complex() or other.dtype == torch.bool or other.dim() not in (1, 2) or other.shape[0] != B \
                or (other.dim() == 2 and other.shape[1] == 0):
            raise ValueError(f"{what}: other must be a real tensor [B] or [B, M >= 1] with B = {B}, got a {other.dtype} "
                             f"tensor of shape {tuple(other.shape)}")
        if other.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("odeint_rowwise_dense: the dense output does not propagate gradients (other requires "
                                      "grad); detach it or evaluate under torch.no_grad()")
        M = 1 if other.dim() == 1 else other.shape[1]
        W = 16 if M <= 16 else 64
        if -(-L // 64) * -(-M // W) > TDEQ_ROW_CROSS_MAX_BLOCKS:
            raise ValueError(f"{what}: {-(-L // 64)} x {-(-M // W)} blocks of 64 elements x {W} covariates; at most "
                             f"{TDEQ_ROW_CROSS_MAX_BLOCKS} are taken")
        tqs, single = self._query_lists(what, ("t",), (t,))
        tq = tqs[0]
        Q = tq.shape[0]
        if self._k is not None and Q * B >= _NONE:
            raise ValueError(f"{what}: {Q * B} queries in one call; the query index is a 32-bit word")
        w = None if weights is None else self._weights_arg(what, weights, Q)
        out = torch.empty(Q, L, M, dtype=torch.float64, device=dev)
        first = _NONE
        if Q > 0:
            with torch.no_grad(), device_guard(dev):
                z = other.detach().to(device=dev, dtype=torch.float64).reshape(B, M).contiguous()
                if self._k is None:
                    seg, x, first = self._search_host(tq)
                    if w is None:
                        out.copy_(rowwise.HostRowKernels.quartic_cross_covariance(self.coeffs, seg, x, z, Q, B, correction))
                    else:
                        out.copy_(rowwise.HostRowKernels.quartic_cross_covariance_weighted(self.coeffs, seg, x, z, w, Q, B,
                                                                                           correction))
                else:
                    status = torch.full((1,), _NONE, dtype=torch.int32, device=dev)
                    seg, x = self._search_device(tq, status)
                    space = self._k.row_dense_cross_workspace_bytes if w is None \
                        else self._k.row_dense_cross_weighted_workspace_bytes
                    per_time = space(1, B, L, M, T)                                                 # (linear in the times)
                    step = min(Q, max(1, MOMENTS_WORKSPACE_BYTES // max(per_time, 1)))
                    work = torch.empty(space(step, B, L, M, T), dtype=torch.uint8, device=dev)
                    count = torch.empty(Q, dtype=torch.int64, device=dev)
                    ybar = torch.empty(Q, L, dtype=torch.float64, device=dev)
                    for q0 in range(0, Q, step):
                        q1 = min(q0 + step, Q)
                        args = (out[q0:q1], count[q0:q1], ybar[q0:q1], z, correction, self.coeffs, seg[q0 * B:q1 * B],
                                x[q0 * B:q1 * B], work)
                        if w is None:
                            self._k.row_dense_cross(*args)
                        else:
                            self._k.row_dense_cross_weighted(*args, w if w.dim() == 1 else w[q0:q1])
                    if check:
                        first = int(status)                                                    # the one read
        if check:
            self._raise_out_of_range(what, ("t",), tqs, [first])
        return out[0] if single else out


def odeint_rowwise_dense(func, y0, t0, t1, *, rtol=1e-7, atol=1e-9, method="dopri5", options=None, compact=None,
                         return_stats=False):
    """Integrate B independent IVPs `dy_r/dt = func(t, y)[r]` from `t0[r]` to `t1[r]` and return the solution as a function:
    `dense = odeint_rowwise_dense(...)`, then `dense(t)` for times that need not be known before the solve.

    `y0`, `func`, `rtol`, `atol` (numbers or `[B]` vectors), `method` (dopri5, bosh3, tsit5, fehlberg2, adaptive_heun,
    dopri8), `options` and `compact` are those of `odeint_rowwise`; with `compact` set `func` is called as
    `func(t_rows, y, rows)`.  `t0` and `t1` are each a number, a 0-dim tensor or a `[B]` tensor: finite, `t1 != t0` in every
    row, in the same direction for all rows (`t1 < t0`: decreasing time), else ValueError.  One more option,
    `dense_chunk_rows` (an integer >= 1, raised to at least B), sets the slots of a chunk of the store.

    The solve is the `odeint_rowwise` solve on the grid `[t0, t1]`: the same step sequence, counters and errors per row (a
    failing row — max_num_steps, dt underflow, a non-finite state — raises and names the original row).  The quartic of
    every accepted step is kept (see `RowDenseOutput` for the layout).  With `options["jump_dy"]` (state impulses at the
    jump points, see `odeint_rowwise`) a dose time `p` is a breakpoint: `dense(p)` is the left limit, the state before the
    impulse, because a breakpoint belongs to the earlier step, and the segment that starts at `p` starts from the state
    with the impulse; `stats` gains `n_impulses`.

    `dense(t)`: `t` a number or 0-dim tensor -> `[B, *row_shape]`; `[Q]` (shared) or `[Q, B]` (per row) -> `[Q, B,
    *row_shape]`, in any order, repeats allowed.  Row r's segments are its accepted steps `[ta_s, tb_s]` in solver time; a
    query `tq` belongs to the FIRST segment with `tq <= tb_s` (a breakpoint belongs to the earlier step, x = 1; `tq == t0[r]`
    to the first, x = 0), and the value is that segment's quartic at `x = T((tq - ta) / (tb - ta))`, the quotient formed in
    fp64.  For a query inside `[t0[r], t1[r]]` that is bit for bit row r of `odeint_rowwise(func, y0, grid)` at that time,
    for the per-row grid `[t0, the queries sorted, t1]`.  The valid interval is `[t0[r], t1[r]]` in the direction of the
    solve, `t1[r]` included (the reference's `odeint_dense` closure raises IndexError at `t == t1`); anything else, a NaN
    included, is out of range, also where the row's last step reaches beyond `t1[r]`: with `check=True` (default) a
    ValueError that names the smallest flat query index `(j, r)` (one word read from the device), with `check=False` an
    all-NaN row and no host read.

    Calculus on the record: `dense.derivative(t)`, `dense.antiderivative(t)` and `dense.integral(ta, tb)` take the query
    forms, the valid interval and `check` of `dense(t)`, with respect to TRUE time (also for `t1 < t0`).  The derivative is the
    quartic's, in the state's dtype: `(d + (c + c) x + (3 b) x^2 + (4 a) x^3) / T(tb - ta)`; a breakpoint belongs to the
    earlier step, so at a breakpoint — a dose time of `jump_dy` included — it is the LEFT derivative.  The antiderivative
    `F_r(t)`, the integral of `y_r` from `t0[r]`, is formed in fp64 and rounded once: per row the whole-step integrals of
    the steps before the query's, added left to right (that order is part of the contract: a row's bits depend neither on B
    nor on the backend), plus the closed-form integral of the query's quartic up to `x64 = (tq - ta) / (tb - ta)`, the fraction
    NOT rounded to the state's dtype; `F_r(t0[r]) == 0`.  `integral(ta, tb) = T(F64(tb) - F64(ta))`, the difference in fp64:
    `integral(a, b) == -integral(b, a)` bit for bit, `integral(a, a) == 0`; `ta` and `tb` broadcast against each other, both
    must be in range (`check=True` names the offending query of `ta` first, then of `tb`).  A ROCm state runs them on HIP
    kernels (`tdeq_row_dense_prefix`, `tdeq_row_dense_calc`, ABI 31), a CPU state as numpy / torch ops with the same bits.

    Extrema on the record: `dense.maximum(ta, tb)` and `dense.minimum(ta, tb)` -> `RowDenseExtremum(values, times)`, per
    ELEMENT the extreme value over the closed window between the two times (either order, the query forms and `check` of
    `integral`) and the fp64 true time at which the element attains it — Cmax / Tmax and Cmin of a dosing solve.  The window
    is walked step by step in fp64: on each step the candidates are the ends (clipped to the window) and the stationary
    points of the quartic, isolated by nested bisection (the roots of y'' bound the pieces on which y' is monotone; only
    `+ - * /`, comparisons and `fabs`, at most 64 rounds per root) — the exact operation order is stated in
    include/tdeq_hip.h and is the contract: the HIP kernel (`tdeq_row_dense_extremum`, ABI 32) and the numpy path of a CPU
    state have the same bits.  `values` is the best candidate rounded once to the state's dtype.  The segment that starts at a
    breakpoint `p` is entered at its start, so the RIGHT limit at `p` counts for `lo <= p < hi`: a `jump_dy` dose inside the
    window or at its near end contributes the state with the impulse at time `p`, one at the far end does not; `maximum(p, p)`
    is `dense(p)` (the fp64 Horner form rounded once).  Ties go to the earlier candidate in the direction of the solve.  One
    launch after the two searches; cost grows with the steps inside the window (one lane per element walks them); nothing is
    built or cached.

    Level crossings on the record: `dense.crossings(level, ta, tb)` -> `RowDenseCrossings(count, first, last, time_above)`
    and `dense.time_above(level, ta, tb)` (the last field alone, the same launch) answer, per ELEMENT and over the window
    between the two times (either order, the query forms and `check` of `integral`): how often the element crosses `level`
    (int32), the fp64 true times of the first and the last crossing met in the direction of the solve (NaN without one), and
    the total true-time duration with `y > level`, strictly — T > MIC, onset and offset of a dosing solve.  `level` is a
    number or a real tensor that broadcasts to `[B, *row_shape]` (one for all, one per element, one per row as `[B, 1, ...]`),
    rounded once to the state's dtype; it does not vary per query; a NaN level gives `count = -1` and NaN for that element,
    an out-of-range query with `check=False` for its whole row.  The walk is that of `maximum`: between two neighbouring
    candidates of a step (its clipped ends, the roots of y'' that bound pieces, the stationary points) the quartic is
    monotone, so `y - level` has at most one root there, which one more bisection in fp64 finds (`+ - * /`, comparisons and
    `fabs` only).  A state machine over the candidates in solver-time order counts the crossings and adds the durations left
    to right; include/tdeq_hip.h states the operation order, which is the contract: the HIP kernel (`tdeq_row_dense_level`,
    ABI 33) and the numpy path of a CPU state have the same bits, and a window gives the same bits in either order of its
    ends.  The first candidate of every later step is the RIGHT limit at the breakpoint: a `jump_dy` dose at `p` that lifts an
    element over the level is a crossing at time `p` exactly, for `lo <= p < hi`; a window that ends at `p` does not see
    it, and `time_above(level, p, p)` is 0.  The answer is exact ON THE RECORD, and the record is discontinuous at
    rounding level at every breakpoint (the end of one step's quartic and the start of the next may differ in their last
    bits): a level inside such a gap is crossed there once more than the continuous solution would be.  A value that only
    touches the level from below is no crossing.  One launch after the two searches; nothing is built or cached.

    Every crossing of a level: `dense.crossing_times(level, ta, tb, max_count=4)` -> `RowDenseCrossingTimes(n_rising,
    n_falling, rising, falling)`, with the `level`, the query forms and the `check` of `crossings`: per ELEMENT the number of
    rising and of falling crossings inside the window (int32, all of them) and the fp64 true times of the first `max_count` of
    each direction as `[max_count, ...]` lists in the order the walk meets them (the direction of the solve), padded with NaN —
    onset and offset of every dosing interval, spike times, periods, Poincare sections.  Rising is meant in TRUE time (`y` goes
    from `<= level` to `> level` as true time increases), so the two directions of the walk swap for a descending solve.  The
    walk, the state machine, the root location and the time rule are those of `crossings`, so `n_rising + n_falling` is its
    `count` and the lists hold its `first` and, where they fit, its `last`; the HIP kernel (`tdeq_row_dense_level_times`, ABI
    35) stores each located time at once and keeps only the state and two counters per element, and the numpy path of a CPU
    state has the same bits.  `16 * max_count` bytes per element and window.  One launch after the two searches; nothing is
    built or cached.

    Exposure against a level: `dense.exposure(level, ta, tb)` -> `RowDenseExposure(area_above, area_below, time_above)`, and
    `dense.area_above(level, ta, tb)` / `dense.area_below(level, ta, tb)` (one field each, the same launch), with the `level`,
    the query forms and the `check` of `crossings`: per ELEMENT the integral of `max(y - level, 0)` and of `max(level - y, 0)`
    over the window, in the state's dtype and >= 0 — AUC above MIC, exposure above a toxic level, the deficit below a target
    trough — and the `time_above` of `crossings`, bit for bit.  No `relu(y - level)` quadrature variable is needed in the
    state, so `y` keeps its bits, and no sampling grid has to hit the dose times.  The walk, the state machine and the root
    location are those of `crossings`; between two neighbouring candidates of a step the element stays on one side of the
    level, so the piece's area is the difference of the closed-form fp64 antiderivative `K` of `y - level` (the `J_s` of
    `integral` with `e - level` in place of `e`) at its ends, and a piece that holds a crossing is split at the located root.
    The pieces above are added to one fp64 sum and the pieces below subtracted from another, left to right in solver time;
    each sum is clamped at 0 and rounded once.  include/tdeq_hip.h states the operation order, which is the contract: the HIP
    kernel (`tdeq_row_dense_exposure`, ABI 34) and the numpy path of a CPU state have the same bits, a window gives the same
    bits in either order of its ends, and an ascending and a descending solve of the same record give the same numbers.  A
    `jump_dy` dose at `p` flips the side at `p` with zero width for `lo <= p < hi`; `exposure(level, p, p)` is all zeros.  One
    launch after the two searches; nothing is built or cached.

    Second moments along time: `dense.time_moments(ta, tb, covariance=False)` -> `RowDenseTimeMoments(duration, mean,
    variance, covariance)`, with the query forms and the `check` of `integral`: per window its duration `T`, per ELEMENT the
    time mean `(1/T) int y dt` and the variance `(1/T) int (y - mean)^2 dt` and, on request, the `[L, L]` covariance along time
    between the elements of the row (`L <= 256`; `8 * Q * B * L^2` bytes) — the RMS and the variance of a component of a long
    or chaotic solve, oscillation amplitudes, the correlation of two components along one trajectory; all fp64.  Exact on
    the record up to rounding without sampling: a product of two deviations is a polynomial of degree 8 in the step fraction,
    which the 5-point Gauss-Legendre rule on each step clipped to the window integrates exactly.  Two walks in fp64, the
    second centred on the mean of the first; the quadrature weights are non-negative, so no variance is negative.
    include/tdeq_hip.h states the nodes and the order of the sums: the walk kernel (`tdeq_row_dense_time_moments`, one lane
    per window and element, the mean in registers between the walks) and the numpy path of a CPU state have the same bits;
    the covariance (`tdeq_row_dense_time_gram`) is a weighted Gram matrix of the `[5 * steps, L]` node deviations on
    `v_mfma_f64_16x16x4_f64`, one workgroup per window and pair of 64-element blocks (four windows per workgroup for `L <=
    16`) that walks the steps serially in stages of 4 steps = 20 nodes through LDS: no workspace, no atomics, the same bits
    from run to run, an error bound against the CPU path; `variance` is then its diagonal.  A zero-length window gives the
    record's value and exact zeros; breakpoints and `jump_dy` impulses add nothing.  Nothing is built or cached.

    Lagged second moments along time: `dense.autocovariance(ta, tb, lags, covariance=False)` -> `RowDenseAutocovariance(
    duration, mean, autocovariance, covariance)`: per lag `tau >= 0` (a number, `[K]` or `[K, B]`) and ELEMENT `C_ii(tau) = 1 /
    (T - tau) int_a^(b - tau) (y_i(t) - m_i)(y_i(t + tau) - m_i) dt` around the whole-window mean of `time_moments` and, on
    request, the `[L, L]` matrix `C_ij(tau)` with `i` at `t` and `j` at `t + tau` — the autocorrelation function of a long or
    chaotic solve, the period of a limit cycle, phase lags between components; all fp64.  Exact on the record up to rounding,
    across step boundaries too: the overlap is cut at the breakpoints of the steps under `t` and of the steps under `t + tau`
    shifted back, both factors are quartics on every piece, and the rule of `time_moments` integrates their product exactly.
    `tdeq_row_dense_time_moments` runs first and its mean is an input; a third search per lag places the second cursor;
    `tdeq_row_dense_time_lagged` (one lane per lag, window and element on a walk with two cursors) and the numpy path of a CPU
    state have the same bits; the matrix (`tdeq_row_dense_time_lagged_gram`) is a non-symmetric Gram product on
    `v_mfma_f64_16x16x4_f64` over all ordered pairs of 64-element blocks: no workspace, no atomics, an error bound against the
    CPU path.  Nothing is built or cached.

    Order statistics across rows: `dense.quantiles(t, probs)` or `dense.quantiles(t, ranks=...)` -> `[P, Q, *row_shape]`, per
    time and ELEMENT the value of rank `k_p` among the B rows' `dense(t)` (`probs` by the "lower" rule `k = floor(p * (B - 1))`,
    at most 16 ranks) — the percentile bands of a population, the envelope of an ensemble.  A most-significant-byte-first radix
    select on the ordered integer image of the value (`-0.0` before `+0.0`, NaN last and canonical): the HIP kernels
    (`tdeq_row_dense_quantiles`, ABI 36) evaluate the record again in each of `sizeof(dtype)` counting passes, with the
    histograms in LDS, and never build `[Q, B, *row_shape]`; the counts are integers, so the answer depends neither on the grid
    nor on the order of the rows, and the torch path of a CPU state has the same bits.  `check` as for `dense(t)`; with
    `check=False` an out-of-range row is a NaN of its time's population.  A workspace of at most 256 MiB; nothing is cached.
    `dense.quantiles(t, probs, weights=w)` gives WEIGHTED order statistics for `[B]` or `[Q, B]` weights: the weights become
    integers of a fixed-point scale set by the largest one, and the same select runs with 64-bit counters
    (`tdeq_row_dense_quantiles_weighted`); a row out of range has then left the population.
    `dense.ranks(t, values, weights=None)` -> `RowDenseRanks(below, equal, total)` is the inverse: per threshold, time and
    element the number of rows below a given value and equal to it in the same order, in ONE counting pass with the counters in
    registers (`tdeq_row_dense_ranks`); `dense.cdf(t, values)` is `(below + equal) / total`.

    Moments across rows: `dense.moments(t, covariance=False, correction=1)` -> `RowDenseMoments(count, mean, variance,
    covariance)`, per time the number of rows in range, per element their mean and variance and, on request, the `[L, L]`
    covariance between the elements (`L <= 1024`) — mean ± SD of a population, the forecast covariance of an ensemble; all
    fp64.  Two passes in fp64, the mean and then sums centred on it, divided by `count - correction`; with `check=False` an
    out-of-range row has left its time's population.  The HIP kernels (`tdeq_row_dense_moments`, ABI 37) evaluate the record
    again in each pass and never build `[Q, B, *row_shape]`: slabs of 1024 rows are added in a fixed order through LDS and merged
    in slab order, the covariance is a Gram matrix of deviations on `v_mfma_f64_16x16x4_f64` (64 x 64 blocks per pair of
    element tiles, the upper triangle mirrored; `variance` is then its diagonal).  No atomics: the same bits from run to run and
    for any slicing of the times; the torch path of a CPU state has the same error bound, not the same last bits.  A workspace
    of at most 256 MiB; nothing is cached.

    Covariance with per-row covariates: `dense.cross_covariance(t, other, correction=1)` -> fp64 `[Q, L, M]`, per time the
    covariance across the rows in range between each of the `L` elements and each of the `M` columns of `other` (`[B]` or `[B,
    M]`: the sampled parameters of the ensemble members, or `dense(t_ref).reshape(B, L)` for a cross-time covariance) — the
    `C_y,theta(t)` of an ensemble Kalman or smoother update and, divided by the SDs, a regression-based global sensitivity.  Two
    passes in fp64 over the same population and divisor as `moments`; a row out of range contributes exact zeros.  The HIP
    kernels (`tdeq_row_dense_cross`, ABI 38) reuse the mean and count kernels of `moments`, add the columns of `other` in slabs
    of 1024 rows, and compute a rectangular Gram matrix on `v_mfma_f64_16x16x4_f64` in blocks of 64 elements by 16 covariates
    (`M <= 16`) or 64 by 64, at most 1024 blocks.  No atomics: the same bits from run to run and for any slicing of the times.

    Returns `dense`; with `return_stats=True`, `(dense, stats)`: the stats of `odeint_rowwise` (`n_accepted`,
    `n_rejected`, `nfe`; with `compact` also `row_evals`, `n_repacks`) plus `n_segments` and `n_chunks`.

    Memory: the result holds `5 * L * n_seg` elements of the state's dtype (`n_seg = n_accepted.sum()`) and two fp64 words
    per segment.  During the solve the quartics sit in chunks of `cap` slots (`5 * L * cap` elements each, by default
    `cap = max(B, min(4 B, 256 MiB of coefficients))`): every chunk but the last is full to within one trial step's accepted
    rows.  Every chunk lives until the solve ends; the pack then allocates the result and releases the chunks one by one, so
    the PEAK is the result plus all chunks — about twice the result.  `antiderivative` and `integral` add a prefix store of
    `8 * L * n_seg` bytes (fp64 `[n_seg, L]`: 40 % on top of an fp32 record), built by the first such call, kept on the object
    and released by `dense.drop_integral_cache()`; `dense(t)` and `derivative` never build it.

    Out of scope (raises or is not offered): gradients through the solve, through `dense(t)` or through the methods
    above (with grad mode on and
    `y0`, `t0`, `t1`, a query tensor or a parameter of `func` requiring grad: NotImplementedError; there is no
    `differentiable` argument), events combined with dense output, 16-bit / complex / tuple states (ValueError), captured
    (hipGraph) steps, extrapolation outside `[t0[r], t1[r]]`, and the per-row adjoint this record is meant to serve.
    `odeint_dense` is unchanged.
    """
    options = dict(options or {})
    B = rowwise._batch_rows(y0)
    t, cap = None, 1
    if B is not None:
        t = _dense_grid(t0, t1, B)
        cap = _chunk_rows(options, B, int(np.prod(y0.shape[1:])), y0.element_size())
        if torch.is_grad_enabled() and (y0.requires_grad or rowwise._func_parameters_require_grad(func)):
            raise NotImplementedError("odeint_rowwise_dense does not propagate gradients (y0 or a parameter of func requires "
                                      "grad); call it under torch.no_grad()")
    options.pop("dense_chunk_rows", None)
    p = _Problem(func, y0, t, rtol, atol, method, options, None, False, compact)
    f0 = p.first_call(p.y0)
    with torch.no_grad(), device_guard(p.device):
        store = RowDenseStore(p, cap)
        sol = torch.empty(2, p.B, p.L, dtype=p.dtype, device=p.device)      # (the commit writes y(t1) here; not returned)
        sol[0].copy_(p.y0)
        kern, n_acc, n_rej = rowwise._solve(p, p.y0, f0, sol, store)
        stats = rowwise._stats(p, n_acc, n_rej)
        dense = RowDenseOutput(p, kern.k, *store.finalize(kern, stats["n_accepted"]))
    if not return_stats:
        return dense
    stats["n_segments"], stats["n_chunks"] = dense.n_segments, store.n_chunks
    return dense, stats
