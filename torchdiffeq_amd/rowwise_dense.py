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
which stores every located time at once.  CPU states run the same steps as torch / numpy ops.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import rowwise
from ._native import device_guard
from .rowwise import _Problem

__all__ = ["odeint_rowwise_dense", "RowDenseOutput", "RowDenseExtremum", "RowDenseCrossings", "RowDenseCrossingTimes",
           "RowDenseExposure"]

# the default chunk: CHUNK_ROWS_PER_ROW slots per row of the batch, at most CHUNK_BYTES of coefficients, never fewer than B
CHUNK_ROWS_PER_ROW = 4
CHUNK_BYTES = 256 << 20
_NONE = 0x7FFFFFFF                                           # the search's status word: no query out of range


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


class RowDenseOutput:
    """The piecewise quartic of a rowwise solve; `dense(t)` evaluates it, `derivative(t)`, `antiderivative(t)` and
    `integral(ta, tb)` give its time derivative and its integrals in closed form, `maximum(ta, tb)` and `minimum(ta, tb)` its
    extrema over a time window and their times, `crossings(level, ta, tb)` and `time_above(level, ta, tb)` its crossings of a
    level and the time spent above it, `crossing_times(level, ta, tb, max_count)` the times of all its crossings by direction,
    `exposure(level, ta, tb)`, `area_above(level, ta, tb)` and `area_below(level, ta, tb)` the area between it and a level (see
    `odeint_rowwise_dense`).

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

    def _ask(self, what: str, names, ts, check: bool, spec, host, device, prefix: bool = False):
        """The steps every query method shares.  The query lists `ts` (called `names` in messages) are parsed and broadcast
        against each other; the outputs are allocated from `spec`, one (dtype, leading dimensions) each, as `[*leading, Q * B,
        L]`; every list is searched; then the one evaluation: for a CPU state `host(lists)` gives the outputs' values, else
        `device(outs, lists)` launches into them, with `lists` = [seg, x, tq] of every list in turn, `tq` in solver time, and
        with `prefix` the prefix store as one more argument.  With `check` the status words of the searches are read once and
        the first out-of-range query raises -> the outputs as `[*leading, Q, B, *row_shape]`, without the Q of single times."""
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
                    status = torch.full((len(tqs),), _NONE, dtype=torch.int32, device=dev)
                    lists = [v for i, tq in enumerate(tqs) for v in (*self._search_device(tq, status[i:i + 1]), tq)]
                    device(outs, lists, *more)
                    if check:
                        firsts = status.tolist()                          # the one read
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
