"""odeint_rowwise cost against odeint's eager whole-batch step, bytes of its streaming launches, and per-row step counts
on a mixed-stiffness batch.

    python tools/rowwise_bench.py [--out profiles/rowwise_bench.json] [--reps 3] [--rowtol]
    python tools/rowwise_bench.py --stats <rocprofv3 kernel_stats.csv> --bench <that json>   (adds in-situ bandwidth)
    python tools/rowwise_bench.py --grad [--out profiles/rowwise_grad_bench.json] [--parity profiles/rowwise_grad_parity.json]
    python tools/rowwise_bench.py --grad --stats <kernel_stats.csv>[,<second>,...] --bench <that json>
                                                                 (row_scale_many bandwidth, one csv per traced repeat)
    python tools/rowwise_bench.py --compact [--out profiles/rowwise_compact_bench.json] [--reps 5]
    python tools/rowwise_bench.py --event [--reps 5]          (one JSON line: plain and event solve of one fresh process)
    python tools/rowwise_bench.py --event --plain-only        (the plain solve alone: also runs on a tree without events)
    python tools/rowwise_bench.py --event-summary parent.jsonl,new_plain.jsonl,new_event.jsonl --out profiles/rowwise_event_bench.json
    python tools/rowwise_bench.py --event --compact [--setting plain|0.5|1.0] [--reps 5]    (one JSON line of one fresh process)
    python tools/rowwise_bench.py --event-compact-summary lines.jsonl[,parent_event.jsonl,new_event.jsonl]
                                  --out profiles/rowwise_event_compact_bench.json
    python tools/rowwise_bench.py --dense [--reps 5] [--out dense.json]
    python tools/rowwise_bench.py --dense-calculus [--reps 5] [--out calculus.json]
    python tools/rowwise_bench.py --dense-calculus-summary calculus.json,parent_dense.jsonl,new_dense.jsonl,parent_bench.jsonl,
                                  new_bench.jsonl --out profiles/rowwise_dense_calculus_bench.json
    python tools/rowwise_bench.py --impulse [--reps 3] [--out profiles/rowwise_impulse_bench.json]
    python tools/rowwise_bench.py --impulse-summary impulse.json,parent_event.jsonl,new_event.jsonl,parent_dense.jsonl,
                                  new_dense.jsonl,parent_bench.jsonl,new_bench.jsonl --out profiles/rowwise_impulse_bench.json
    python tools/rowwise_bench.py --dense-summary dense.json,parent_event.jsonl,new_event.jsonl,parent_bench.jsonl,new_bench.jsonl
                                  --out profiles/rowwise_dense_bench.json

`--compact`: wall time of one solve at the headline shape with a per-row rate spread over logspace(-1, 1.5) (so that the
rows' trial counts differ), plain against `compact=0.5` and `compact=1.0`: `row_evals` against `nfe x B` (the bound on
any speed-up), the number of repacks and the time spent inside `repack`.

`--event`: the headline's plain rowwise solve and `odeint_rowwise_event` of the same func (event: y[:, 0] falls 0.25 below
its start, t_end = 0.5, so that some rows fire and the others reach t_end), each the median of `--reps` solves after a
warm-up, then one instrumented event solve with the time inside `event_fn` during the trial steps and inside the final
bisection measured between synchronisations.  One fresh process per figure; `--event-summary` folds the lines of
alternated processes (parent tree plain, this tree plain, this tree event) into the medians and spreads of
profiles/rowwise_event_bench.json.

`--event --compact`: the event solve with the rate-spread func of `--compact` (k_r * (y @ A.T), k_r over logspace(-1, 1.5),
so that the rows stop after different numbers of trial steps; the same event and t_end), one setting per fresh process —
plain, `compact=0.5` or `compact=1.0`: the median of `--reps` solves after a warm-up, `row_evals`, `event_row_evals`,
`n_repacks`, the bound nfe x B / row_evals, whether every output is bit for bit the plain solve's of the same process, and
one instrumented solve with the final bisection timed between synchronisations.  `--event-compact-summary` folds the lines
of alternated processes (the first round warms up) and, given the `--event` lines of the parent tree and of this tree,
whether the plain event solve (func y @ A.T) stayed inside the parent's spread.

`--dense`: `odeint_rowwise_dense` at the rate-spread shape of `--compact` (k_r * (y @ A.T), k_r over logspace(-1, 1.5),
t1 = 0.5) against `odeint_rowwise` on [t0, t1] in the same process — the median of `--reps` solves each after a warm-up,
`n_segments`, `n_chunks`, the bytes the result holds — and the evaluation `dense(t)` for Q = 16 random times per row:
ms per call without the host read (`check=False`), the achieved bytes/s counting 5 coefficient reads and 1 write per output
element, and the search launch alone.

`--dense-summary` folds that file with the lines of alternated fresh processes of the parent tree and of this tree — `--event`
(the plain rowwise solve and the plain event solve; the first line of each file is the warm-up round) and `bench.py --gpus 1
--steps 200 --warmup 20` — and says whether this tree's medians lie inside the parent's observed spread.

`--steps`: the headline shape with one jump point per row at a per-row time (func y @ A.T plus a forcing that changes sign
at the row's point): the solve with `jump_t` against the same func without it (whose controller grinds through the kink),
ms per trial step, the refresh calls and — from one instrumented solve, synchronised on both sides — ms per refresh; and the
achieved rate of `tdeq_row_select` on the whole state (every row selected: 1 read + 1 write per element) against the HBM
peak.

`--impulse`: the `--steps` shape with one bolus per row (`jump_dy`, func y @ A.T): the solve against the same solve with
`jump_t` alone, trial steps and refresh calls, and `tdeq_row_impulse` alone — every row selected and 1 row in 64 — next to
`tdeq_row_select` on the same state (3 words per touched element against 2).

`--grad`: forward + backward of a `differentiable=True` solve per trial step at the headline, next to plain `odeint`
backprop of the same state, and (`--parity`) the per-row deviations of the rowwise gradients from the reference's
(tests/golden/rowwise_grad.npz) on the host path and on the device.

`--rowtol`: the headline's rowwise solve with `rtol` / `atol` as constant `[B]` vectors (tdeq_row_reduce_tol): the step
sequence of the scalar solve, so the two figures compare launch for launch.

Headline workload of bench.py: dopri5, func y @ A.T, 65536 x 128 fp32, rtol 1e-7, atol 1e-9.  A trial step of
odeint_rowwise is one pass of its loop (S evaluations); odeint's is one call of its adaptive step; both are timed over
the same interval, alternated in one process, `odeint` with hip_graph=False (the eager launch sequence).
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0


def _headline(reps: int, rowtol: bool = False):
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)
    calls = [0]
    tol = dict(rtol=1e-7, atol=1e-9)
    if rowtol:
        tol = {k: torch.full((B,), v, dtype=torch.float64) for k, v in tol.items()}

    def f(t_, y):
        calls[0] += 1
        return y @ A.T
    res = {"rowwise_ms_per_trial": [], "odeint_ms_per_trial": [], "rowwise_tolerances": "[B] vectors" if rowtol else "scalars"}
    with torch.no_grad():
        for _ in range(reps + 1):
            for which in ("rowwise", "odeint"):
                calls[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if which == "rowwise":
                    _, st = tda.odeint_rowwise(f, y0, t, return_stats=True, **tol)
                else:
                    tda.odeint(f, y0, t, rtol=1e-7, atol=1e-9, options={"hip_graph": False})
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                trials = (calls[0] - 2) / 6
                res[which + "_ms_per_trial"].append(ms / trials)
                res[which + "_trials"] = trials
    for k in ("rowwise_ms_per_trial", "odeint_ms_per_trial"):
        res[k] = res[k][1:]          # the first pair warms up
    res["ratio_rowwise_over_odeint"] = min(res["rowwise_ms_per_trial"]) / min(res["odeint_ms_per_trial"])
    return res


def _steps(reps: int):
    import torchdiffeq_amd as tda
    from torchdiffeq_amd import _native, rowwise
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    tj = (0.1 + 0.3 * torch.rand(B, generator=g, dtype=torch.float64))
    tj_dev = tj.float().to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)

    def f(t_, y):
        return y @ A.T + torch.where(t_ >= tj_dev, 0.5, -0.5)[:, None]
    settings = (("without_jump_t", None), ("with_jump_t", {"jump_t": tj[None, :]}))
    res = {name: {"ms_per_solve": []} for name, _ in settings}
    with torch.no_grad():
        for rep in range(reps + 1):
            for name, options in settings:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, st = tda.odeint_rowwise(f, y0, t, rtol=1e-7, atol=1e-9, options=options, return_stats=True)
                torch.cuda.synchronize()
                if rep:                       # the first round warms up
                    res[name]["ms_per_solve"].append((time.perf_counter() - t0) * 1e3)
                trials = st["n_accepted"] + st["n_rejected"]
                res[name].update(nfe=st["nfe"], trial_steps=int(trials.max()), trials_median=float(trials.median()),
                                 refresh_calls=st["nfe"] - 2 - 6 * int(trials.max()))
        for name, _ in settings:
            res[name]["ms_per_trial_step"] = sorted(res[name]["ms_per_solve"])[len(res[name]["ms_per_solve"]) // 2] \
                / res[name]["trial_steps"]
        # one instrumented solve: the refresh (one func call + tdeq_row_select) between synchronisations
        spent = []
        orig = rowwise.HipRowKernels.refresh_after_jump

        def timed(self, y, f0):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = orig(self, y, f0)
            torch.cuda.synchronize()
            spent.append((time.perf_counter() - t0) * 1e3)
            return out
        rowwise.HipRowKernels.refresh_after_jump = timed
        try:
            tda.odeint_rowwise(f, y0, t, rtol=1e-7, atol=1e-9, options=settings[1][1])
        finally:
            rowwise.HipRowKernels.refresh_after_jump = orig
        res["refresh"] = {"calls": len(spent), "ms_per_refresh_median": sorted(spent)[len(spent) // 2] if spent else None,
                          "ms_total": sum(spent)}
        # tdeq_row_select on the whole state, every row selected
        kern = _native.get_kernels(dev, torch.float32)
        dst, src = torch.zeros_like(y0), y0.clone()
        mask = torch.ones(B, dtype=torch.int32, device=dev)
        for _ in range(3):
            kern.row_select(dst, src, mask)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        n = 20
        ev[0].record()
        for _ in range(n):
            kern.row_select(dst, src, mask)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / n
        tbs = 2 * B * D * 4 / (ms * 1e-3) / 1e12
        res["row_select"] = {"shape": [B, D], "ms": ms, "TB_per_s": tbs, "fraction_of_peak": tbs / PEAK_TBS,
                             "note": "2 x 33.5 MB per launch: the state fits the 256 MB last-level cache, so the rate is not "
                                     "bounded by HBM alone"}
    res["shape"] = [B, D]
    return res


def _impulse(reps: int):
    """The `--steps` problem with one bolus per row at the row's own time: ms per solve with `jump_dy` against `jump_t`
    alone, trial steps and refresh calls, and `tdeq_row_impulse` alone (every row, and 1 row in 64) next to
    `tdeq_row_select` on the same state."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd import _native
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    tj = (0.1 + 0.3 * torch.rand(B, generator=g, dtype=torch.float64))
    dose = torch.randn(1, B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)

    def f(t_, y):
        return y @ A.T
    settings = (("jump_t_alone", {"jump_t": tj[None, :]}), ("with_jump_dy", {"jump_t": tj[None, :], "jump_dy": dose}))
    res = {name: {"ms_per_solve": []} for name, _ in settings}
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    from torchdiffeq_amd import rowwise
    refreshes = [0]
    plain_refresh = rowwise.HipRowKernels.refresh_after_jump

    def counted(self, y, f0):                     # (counts only: no synchronisation is added to the timed solves)
        refreshes[0] += 1
        return plain_refresh(self, y, f0)
    rowwise.HipRowKernels.refresh_after_jump = counted
    with torch.no_grad():
        for rep in range(reps + 1):
            for name, options in settings:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                refreshes[0] = 0
                _, st = tda.odeint_rowwise(f, y0, t, rtol=1e-7, atol=1e-9, options=options, return_stats=True)
                torch.cuda.synchronize()
                if rep:                       # the first round warms up
                    res[name]["ms_per_solve"].append((time.perf_counter() - t0) * 1e3)
                trials = st["n_accepted"] + st["n_rejected"]
                res[name].update(nfe=st["nfe"], trial_steps=int(trials.max()), trials_median=float(trials.median()),
                                 refresh_calls=refreshes[0])
                if "n_impulses" in st:
                    res[name]["n_impulses_total"] = int(st["n_impulses"].sum())
        rowwise.HipRowKernels.refresh_after_jump = plain_refresh
        for name, _ in settings:
            res[name]["ms_per_solve_median"] = med(res[name]["ms_per_solve"])
        # the two kernels alone on the whole state
        kern = _native.get_kernels(dev, torch.float32)
        index = torch.zeros(1, B, dtype=torch.int32, device=dev)
        hit = torch.zeros(B, dtype=torch.int32, device=dev)
        every = torch.ones(B, dtype=torch.int32, device=dev)
        sparse = (torch.arange(B, device=dev) % 64 == 0).to(torch.int32)
        y, src = y0.clone(), y0.clone()

        def rate(launch, words, rows):
            for _ in range(3):
                launch()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            n = 20
            ev[0].record()
            for _ in range(n):
                launch()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / n
            tbs = words * rows * D * 4 / (ms * 1e-3) / 1e12
            return {"ms": ms, "rows_touched": rows, "words_per_touched_element": words, "TB_per_s": tbs,
                    "fraction_of_peak": tbs / PEAK_TBS}
        res["row_impulse_all_rows"] = rate(lambda: kern.row_impulse(y, dose, index, hit, every), 3, B)
        res["row_impulse_1_in_64"] = rate(lambda: kern.row_impulse(y, dose, index, hit, sparse), 3, B // 64)
        res["row_select_all_rows"] = rate(lambda: kern.row_select(y, src, every), 2, B)
        res["row_impulse_over_row_select_ms"] = res["row_impulse_all_rows"]["ms"] / res["row_select_all_rows"]["ms"]
        res["note"] = ("3 x 33.5 MB per launch with every row selected: the state fits the 256 MB last-level cache, so the "
                       "rate is not bounded by HBM alone")
    res["shape"] = [B, D]
    return res


def _compact(reps: int):
    """Headline shape, dopri5, func k_r * (y @ A.T) with k_r over logspace(-1, 1.5): ms per solve, plain / compact=0.5 /
    compact=1.0 alternated in one process after a warm-up round, then one more solve per setting with `repack` timed
    (synchronised on both sides, so that solve is not among the timed ones)."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd import rowwise
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)
    settings = (("plain", None), ("compact_0.5", 0.5), ("compact_1.0", 1.0))

    def solve(c):
        if c is None:
            return tda.odeint_rowwise(lambda t_, y: k * (y @ A.T), y0, t, rtol=1e-7, atol=1e-9, return_stats=True)
        return tda.odeint_rowwise(lambda t_, y, rows: k[rows] * (y @ A.T), y0, t, rtol=1e-7, atol=1e-9,
                                  return_stats=True, compact=c)
    res = {name: {"ms_per_solve": []} for name, _ in settings}
    sols = {}
    with torch.no_grad():
        for rep in range(reps + 1):
            for name, c in settings:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sol, st = solve(c)
                torch.cuda.synchronize()
                if rep:                       # the first round warms up
                    res[name]["ms_per_solve"].append((time.perf_counter() - t0) * 1e3)
                sols[name] = sol
                trials = st["n_accepted"] + st["n_rejected"]
                res[name].update(nfe=st["nfe"], nfe_times_B=st["nfe"] * B, row_evals=st.get("row_evals", st["nfe"] * B),
                                 n_repacks=st.get("n_repacks", 0), trials_min=int(trials.min()),
                                 trials_median=float(trials.median()), trials_max=int(trials.max()))
        inside = [0.0]
        plain_repack = rowwise.HipRowKernels.repack

        def timed_repack(self, y, f0, n_keep):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = plain_repack(self, y, f0, n_keep)
            torch.cuda.synchronize()
            inside[0] += (time.perf_counter() - t0) * 1e3
            return out
        rowwise.HipRowKernels.repack = timed_repack
        try:
            for name, c in settings[1:]:
                inside[0] = 0.0
                solve(c)
                res[name]["ms_inside_repack"] = inside[0]
        finally:
            rowwise.HipRowKernels.repack = plain_repack
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    for name, _ in settings:
        r = res[name]
        r["ms_per_solve_median"] = med(r["ms_per_solve"])
        r["bit_identical_to_plain"] = bool(torch.equal(sols[name], sols["plain"]))
        r["speedup_bound"] = r["nfe_times_B"] / r["row_evals"]
        r["speedup"] = med(res["plain"]["ms_per_solve"]) / r["ms_per_solve_median"]
    return {"B": B, "L": D, "dtype": "float32", "method": "dopri5", "rtol": 1e-7, "atol": 1e-9,
            "rate_spread": "k_r in logspace(-1, 1.5), shuffled; func k_r * (y @ A.T)", **res}


def _event(reps: int, plain_only: bool):
    """One process's figures: ms per trial step of the plain headline solve and (unless `plain_only`) of the event solve."""
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)
    level = y0[:, 0] - 0.25
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

    def f(t_, y):
        return y @ A.T

    def ev(t_, y):
        return y[:, 0] - level

    def timed(solve):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solve()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    res = {}
    with torch.no_grad():
        ms = []
        for rep in range(reps + 1):
            took, (_, st) = timed(lambda: tda.odeint_rowwise(f, y0, t, rtol=1e-7, atol=1e-9, return_stats=True))
            trials = (st["nfe"] - 2) / 6
            if rep:                           # the first solve warms up
                ms.append(took / trials)
        res["plain"] = {"ms_per_trial": ms, "median_ms_per_trial": med(ms), "trials_per_solve": trials}
        if plain_only:
            return res
        from torchdiffeq_amd import rowwise_event
        solve = lambda fn=ev: tda.odeint_rowwise_event(f, y0, 0.0, event_fn=fn, t_end=0.5, rtol=1e-7, atol=1e-9,      # noqa: E731
                                                        return_stats=True)
        ms = []
        for rep in range(reps + 1):
            took, (_, _, st) = timed(solve)
            if rep:
                ms.append(took)
        trials = (st["nfe"] - 2) / 6
        # one more solve, instrumented: event_fn during the trial steps and the whole final bisection between synchronisations
        inside = {"event_fn": 0.0, "bisection": 0.0, "in_bisection": False}

        def timed_ev(t_, y):
            if inside["in_bisection"]:
                return ev(t_, y)
            took, out = timed(lambda: ev(t_, y))
            inside["event_fn"] += took
            return out
        plain_locate = rowwise_event._locate

        def timed_locate(*a):
            inside["in_bisection"] = True
            took, out = timed(lambda: plain_locate(*a))
            inside["bisection"] += took
            return out
        rowwise_event._locate = timed_locate
        try:
            solve(timed_ev)
        finally:
            rowwise_event._locate = plain_locate
        n_steps_calls = 1 + int(trials)                       # event_fn at t0 and once per trial step
        res["event"] = {"ms_per_solve": ms, "median_ms_per_solve": med(ms), "trials_per_solve": trials,
                        "rows_fired": int(st["fired"].sum()), "n_event_evals": st["n_event_evals"],
                        "bisection_rounds": st["n_event_evals"] - n_steps_calls,
                        "ms_inside_bisection": inside["bisection"], "ms_inside_event_fn_while_stepping": inside["event_fn"],
                        "median_ms_per_trial_without_bisection": (med(ms) - inside["bisection"]) / trials,
                        "event_fn_ms_per_trial": inside["event_fn"] / n_steps_calls}
    return res


def _event_compact(reps: int, setting: str):
    """One process's figures for one setting ("plain", "0.5", "1.0") of the rate-spread event solve."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd import rowwise_event
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    level = y0[:, 0] - 0.25
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    kw = dict(t_end=0.5, rtol=1e-7, atol=1e-9, return_stats=True)

    def solve(c, field=lambda y: y @ A.T):
        if c is None:
            return tda.odeint_rowwise_event(lambda t_, y: k * field(y), y0, 0.0, event_fn=lambda t_, y: y[:, 0] - level, **kw)
        return tda.odeint_rowwise_event(lambda t_, y, rows: k[rows] * field(y), y0, 0.0,
                                        event_fn=lambda t_, y, rows: y[:, 0] - level[rows], compact=c, **kw)

    def same_outputs(a, b):
        return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(
            torch.equal(a[2][n], b[2][n]) for n in ("n_accepted", "n_rejected", "fired")) and all(
            a[2][n] == b[2][n] for n in ("nfe", "n_event_evals")))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    c = None if setting == "plain" else float(setting)
    with torch.no_grad():
        plain = solve(None)                                   # warms up, and is what the setting's outputs are compared to
        ms = []
        for rep in range(reps + 1):
            took, (event_t, sol, st) = timed(lambda: solve(c))
            if rep:                                           # the first solve warms up
                ms.append(took)
        same = same_outputs((event_t, sol, st), plain)
        # the GEMM picks its algorithm by batch size, so this func is not batch-invariant; the same comparison with an
        # elementwise field (k_r * -y: rows independent to the bit) is the feature's contract at this shape
        decay = lambda y: -y      # noqa: E731
        same_elementwise = same_outputs(solve(c, decay), solve(None, decay))
        inside = [0.0]
        plain_locate = rowwise_event._locate

        def timed_locate(*a):
            took, out = timed(lambda: plain_locate(*a))
            inside[0] += took
            return out
        rowwise_event._locate = timed_locate
        try:
            solve(c)
        finally:
            rowwise_event._locate = plain_locate
    trials = st["n_accepted"] + st["n_rejected"]
    row_evals = st.get("row_evals", st["nfe"] * B)
    return {"setting": setting, "ms_per_solve": ms, "median_ms_per_solve": med(ms), "ms_inside_bisection": inside[0],
            "median_ms_per_solve_without_bisection": med(ms) - inside[0], "nfe": st["nfe"], "nfe_times_B": st["nfe"] * B,
            "row_evals": row_evals, "n_event_evals": st["n_event_evals"],
            "event_row_evals": st.get("event_row_evals", st["n_event_evals"] * B), "n_repacks": st.get("n_repacks", 0),
            "speedup_bound": st["nfe"] * B / row_evals, "bit_identical_to_plain": bool(same),
            "bit_identical_to_plain_elementwise_func": same_elementwise,
            "rows_fired": int(st["fired"].sum()), "trials_min": int(trials.min()), "trials_median": float(trials.median()),
            "trials_max": int(trials.max())}


def _dense(reps: int, Q: int = 16):
    """Solve with and without the store, and the evaluation of the dense object, in one process."""
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    func = lambda t_, y: k * (y @ A.T)           # noqa: E731
    kw = dict(rtol=1e-7, atol=1e-9, return_stats=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    plain_ms, dense_ms = [], []
    with torch.no_grad():
        for rep in range(reps + 1):                           # the first pair warms up; the two alternate
            a, (_, st_p) = timed(lambda: tda.odeint_rowwise(func, y0, t, **kw))
            b, (dense, st) = timed(lambda: tda.odeint_rowwise_dense(func, y0, 0.0, 0.5, **kw))
            if rep:
                plain_ms.append(a)
                dense_ms.append(b)
        tq = torch.rand(Q, B, generator=g, dtype=torch.float64).to(dev) * 0.5
        eval_ms, search_ms = [], []
        for rep in range(reps + 1):
            a, out = timed(lambda: dense(tq, check=False))
            b, (_, _, status) = timed(lambda: dense.search(tq))          # (increasing time: solver time is true time)
            if rep:
                eval_ms.append(a)
                search_ms.append(b)
        finite = bool(torch.isfinite(out).all()) and int(status) == 0x7FFFFFFF
    trials = st["n_accepted"] + st["n_rejected"]
    moved = 6 * Q * B * D * 4
    held = dense.coeffs.numel() * 4 + 2 * 8 * dense.n_segments + 8 * (B + 1)
    return {"plain_ms_per_solve": plain_ms, "dense_ms_per_solve": dense_ms, "plain_median_ms": med(plain_ms),
            "dense_median_ms": med(dense_ms), "extra_ms": med(dense_ms) - med(plain_ms),
            "same_counters_as_plain": bool(torch.equal(st["n_accepted"], st_p["n_accepted"])) and st["nfe"] == st_p["nfe"],
            "trial_steps": (st["nfe"] - 2) // 6, "n_segments": st["n_segments"], "n_chunks": st["n_chunks"],
            "bytes_held": held, "accepted_min": int(st["n_accepted"].min()), "accepted_median": float(st["n_accepted"].median()),
            "accepted_max": int(st["n_accepted"].max()), "trials_max": int(trials.max()),
            "eval": {"Q": Q, "ms_per_call": eval_ms, "median_ms": med(eval_ms), "bytes_moved": moved,
                     "achieved_TBs": moved / (med(eval_ms) * 1e-3) / 1e12, "hbm_peak_TBs": PEAK_TBS,
                     "search_alone_ms": search_ms, "search_alone_median_ms": med(search_ms), "all_finite": finite}}


def _impulse_summary(paths, out):
    """Fold the `--impulse` file with the JSON lines of alternated fresh processes of the parent tree and of this tree —
    `--event` (plain rowwise solve and plain event solve), `--dense` and `bench.py --gpus 1 --steps 200 --warmup 20`; the
    first line of every file is the warm-up round — and say whether this tree's medians lie inside the parent's spread."""
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

    def fold(vals):
        return {"per_process": [round(v, 4) for v in vals], "median": round(med(vals), 4), "min": round(min(vals), 4),
                "max": round(max(vals), 4)}

    def pair(parent, new):
        p, n = fold(parent), fold(new)
        return {"parent": p, "new": n, "new_median_inside_parent_min_max": p["min"] <= n["median"] <= p["max"],
                "new_median_not_above_parent_max": n["median"] <= p["max"]}      # (every figure: lower is better)
    lines = lambda path: [json.loads(x) for x in open(path) if x.strip().startswith("{")][1:]      # noqa: E731
    res = json.load(open(paths[0]))
    pe, ne, pd, nd, pb, nb = (lines(path) for path in paths[1:7])
    res["paths_without_the_option_against_parent"] = {
        "what": "parent commit and this tree alternated in fresh processes in one session, the first round of processes "
                "dropped: tools/rowwise_bench.py --event --reps 3 (func y @ A.T), tools/rowwise_bench.py --dense --reps 3 and "
                "bench.py --gpus 1 --steps 200 --warmup 20",
        "plain_rowwise_ms_per_trial": pair([r["plain"]["median_ms_per_trial"] for r in pe],
                                           [r["plain"]["median_ms_per_trial"] for r in ne]),
        "rowwise_event_ms_per_solve": pair([r["event"]["median_ms_per_solve"] for r in pe],
                                           [r["event"]["median_ms_per_solve"] for r in ne]),
        "rowwise_dense_ms_per_solve": pair([r["dense"]["dense_median_ms"] for r in pd],
                                           [r["dense"]["dense_median_ms"] for r in nd]),
        "bench_ms_per_step": pair([r["ms_per_step"] for r in pb], [r["ms_per_step"] for r in nb])}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["paths_without_the_option_against_parent"]))


def _dense_calculus(reps: int, Q: int = 16):
    """The calculus on the record of the `--dense` solve, in one process: the prefix build (dropped and rebuilt `reps` times
    after a warm-up) against the bytes it must move — five T words read and one fp64 word written per segment element — and
    `derivative`, `antiderivative`, `integral` next to `dense(t)` for the same Q times per row, the four alternated."""
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    func = lambda t_, y: k * (y @ A.T)           # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    with torch.no_grad():
        dense, st = tda.odeint_rowwise_dense(func, y0, 0.0, 0.5, rtol=1e-7, atol=1e-9, return_stats=True)
        tq = torch.rand(Q, B, generator=g, dtype=torch.float64).to(dev) * 0.5
        tq2 = torch.rand(Q, B, generator=g, dtype=torch.float64).to(dev) * 0.5
        prefix_ms = []
        for rep in range(reps + 1):                           # the first build warms up
            dense.drop_integral_cache()
            ms, P = timed(dense._integral_prefix)
            if rep:
                prefix_ms.append(ms)
        calls = {"dense(t)": lambda: dense(tq, check=False), "derivative": lambda: dense.derivative(tq, check=False),
                 "antiderivative": lambda: dense.antiderivative(tq, check=False),
                 "integral": lambda: dense.integral(tq, tq2, check=False)}
        ms_of, finite = {name: [] for name in calls}, True
        for rep in range(reps + 1):
            for name, fn in calls.items():
                ms, out = timed(fn)
                finite = finite and bool(torch.isfinite(out).all())
                if rep:
                    ms_of[name].append(ms)
    n_el = dense.n_segments * D
    prefix_bytes = n_el * (5 * 4 + 8)
    word = Q * B * D
    moved = {"dense(t)": 6 * 4 * word, "derivative": 5 * 4 * word, "antiderivative": (6 * 4 + 8) * word,
             "integral": (11 * 4 + 2 * 8) * word}
    res = {"n_segments": dense.n_segments, "accepted_median": float(st["n_accepted"].median()),
           "accepted_max": int(st["n_accepted"].max()), "all_finite": finite, "hbm_peak_TBs": PEAK_TBS,
           "prefix": {"bytes_held": P.numel() * 8, "bytes_moved": prefix_bytes, "ms_per_build": prefix_ms,
                      "median_ms": med(prefix_ms), "achieved_TBs": prefix_bytes / (med(prefix_ms) * 1e-3) / 1e12},
           "eval": {"Q": Q}}
    for name in calls:
        res["eval"][name] = {"ms_per_call": ms_of[name], "median_ms": med(ms_of[name]), "bytes_moved": moved[name],
                             "achieved_TBs": moved[name] / (med(ms_of[name]) * 1e-3) / 1e12,
                             "ratio_to_dense(t)": med(ms_of[name]) / med(ms_of["dense(t)"])}
    return res


def _dense_calculus_summary(paths, out):
    """Fold the `--dense-calculus` file with the JSON lines of alternated fresh processes of the parent tree and of this tree
    — `--dense --reps 3` (the plain dense solve and `dense(t)`) and `bench.py --gpus 1 --steps 200 --warmup 20`; the first
    line of every file is the warm-up round — and say whether this tree's medians lie inside the parent's spread."""
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

    def fold(vals):
        return {"per_process": [round(v, 4) for v in vals], "median": round(med(vals), 4), "min": round(min(vals), 4),
                "max": round(max(vals), 4)}

    def pair(parent, new):
        p, n = fold(parent), fold(new)
        return {"parent": p, "new": n, "new_median_inside_parent_min_max": p["min"] <= n["median"] <= p["max"],
                "new_median_not_above_parent_max": n["median"] <= p["max"]}      # (every figure: lower is better)
    lines = lambda path: [json.loads(x) for x in open(path) if x.strip().startswith("{")][1:]      # noqa: E731
    res = json.load(open(paths[0]))
    pd, nd, pb, nb = (lines(path) for path in paths[1:5])
    res["unchanged_paths_against_parent"] = {
        "what": "parent commit and this tree alternated in fresh processes in one session, the first round of processes "
                "dropped: tools/rowwise_bench.py --dense --reps 3 and bench.py --gpus 1 --steps 200 --warmup 20",
        "rowwise_dense_ms_per_solve": pair([r["dense"]["dense_median_ms"] for r in pd],
                                           [r["dense"]["dense_median_ms"] for r in nd]),
        "dense_eval_ms_per_call": pair([r["dense"]["eval"]["median_ms"] for r in pd],
                                       [r["dense"]["eval"]["median_ms"] for r in nd]),
        "bench_ms_per_step": pair([r["ms_per_step"] for r in pb], [r["ms_per_step"] for r in nb])}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["unchanged_paths_against_parent"]))


def _dense_summary(paths, out):
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

    def fold(vals):
        return {"per_process": [round(v, 4) for v in vals], "median": round(med(vals), 4), "min": round(min(vals), 4),
                "max": round(max(vals), 4)}

    def pair(parent, new):
        p, n = fold(parent), fold(new)
        return {"parent": p, "new": n, "new_median_inside_parent_min_max": p["min"] <= n["median"] <= p["max"]}
    lines = lambda path: [json.loads(x) for x in open(path) if x.strip().startswith("{")]      # noqa: E731
    res = json.load(open(paths[0]))
    pe, ne = lines(paths[1])[1:], lines(paths[2])[1:]                         # the first round warms up
    pb, nb = lines(paths[3]), lines(paths[4])
    res["plain_paths_against_parent"] = {
        "what": "parent tree and this tree alternated in fresh processes in one session; tools/rowwise_bench.py --event "
                "--reps 3 (func y @ A.T; the median of 3 solves per process after a warm-up solve, the first round of "
                "processes dropped) and bench.py --gpus 1 --steps 200 --warmup 20 (every process kept)",
        "plain_rowwise_ms_per_trial": pair([r["plain"]["median_ms_per_trial"] for r in pe],
                                           [r["plain"]["median_ms_per_trial"] for r in ne]),
        "plain_event_ms_per_solve": pair([r["event"]["median_ms_per_solve"] for r in pe],
                                         [r["event"]["median_ms_per_solve"] for r in ne]),
        "bench_rk_stages_per_s": pair([r["value"] for r in pb], [r["value"] for r in nb])}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["plain_paths_against_parent"]))


def _event_compact_summary(paths, out):
    """Fold the JSON lines of the alternated fresh processes (one file, every setting; the first line of each setting is
    the warm-up round).  With two more files — `--event` lines of the parent tree and of this tree, alternated — also the
    plain event solve of the two trees."""
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

    def fold(vals):
        return {"per_process": [round(v, 4) for v in vals], "median": round(med(vals), 4), "min": round(min(vals), 4),
                "max": round(max(vals), 4)}
    lines = [json.loads(x) for x in open(paths[0]) if x.strip().startswith("{")]
    res = {"what": "tools/rowwise_bench.py --event --compact: 65536 x 128 fp32 dopri5, func k_r * (y @ A.T) with k_r in "
                   "logspace(-1, 1.5) shuffled, event: y[:, 0] falls 0.25 below its start, t_end 0.5, rtol 1e-7, atol 1e-9; "
                   "every figure the median of 5 solves of one fresh process, the settings alternated, the first round "
                   "a warm-up"}
    for setting in ("plain", "0.5", "1.0"):
        mine = [r["event_compact"] for r in lines if r["event_compact"]["setting"] == setting][1:]
        last = mine[-1]
        res["plain" if setting == "plain" else "compact_" + setting] = {
            "ms_per_solve": fold([r["median_ms_per_solve"] for r in mine]),
            "bisection_ms_per_solve": fold([r["ms_inside_bisection"] for r in mine]),
            "ms_per_solve_without_bisection": fold([r["median_ms_per_solve_without_bisection"] for r in mine]),
            "bit_identical_to_plain": all(r["bit_identical_to_plain"] for r in mine),
            "bit_identical_to_plain_elementwise_func": all(r["bit_identical_to_plain_elementwise_func"] for r in mine),
            **{key: last[key] for key in ("nfe", "nfe_times_B", "row_evals", "n_event_evals", "event_row_evals", "n_repacks",
                                          "speedup_bound", "rows_fired", "trials_min", "trials_median", "trials_max")}}
    for name in ("compact_0.5", "compact_1.0"):
        res[name]["speedup"] = round(res["plain"]["ms_per_solve"]["median"] / res[name]["ms_per_solve"]["median"], 4)
    if len(paths) == 3:
        parent, new = ([json.loads(x) for x in open(p) if x.strip().startswith("{")][1:] for p in paths[1:])
        pe = fold([r["event"]["median_ms_per_solve"] for r in parent])
        ne = fold([r["event"]["median_ms_per_solve"] for r in new])
        res["plain_event_solve_func_y_At"] = {"parent_ms_per_solve": pe, "new_ms_per_solve": ne,
                                              "new_median_inside_parent_min_max": pe["min"] <= ne["median"] <= pe["max"]}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


def _event_summary(paths, out):
    """Fold the JSON lines of the alternated fresh processes (parent plain, this tree plain, this tree event; the first
    line of each file is the warm-up round) into medians and spreads."""
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    lines = [[json.loads(x) for x in open(p) if x.strip().startswith("{")][1:] for p in paths]
    parent, new_plain, new_event = lines

    def fold(vals):
        return {"per_process": [round(v, 4) for v in vals], "median": round(med(vals), 4), "min": round(min(vals), 4),
                "max": round(max(vals), 4)}
    res = {"what": "tools/rowwise_bench.py --event: 65536 x 128 fp32 dopri5, func y @ A.T, rtol 1e-7, atol 1e-9; every figure "
                   "the median of 5 solves of one fresh process; parent tree (plain), this tree (plain) and this tree (event "
                   "solve: y[:, 0] falls 0.25 below its start, t_end 0.5) alternated, %d rounds after a warm-up round" % len(parent),
           "parent_plain_ms_per_trial": fold([r["plain"]["median_ms_per_trial"] for r in parent]),
           "new_plain_ms_per_trial": fold([r["plain"]["median_ms_per_trial"] for r in new_plain]),
           "event_ms_per_trial_without_bisection": fold([r["event"]["median_ms_per_trial_without_bisection"] for r in new_event]),
           "event_fn_ms_per_trial": fold([r["event"]["event_fn_ms_per_trial"] for r in new_event]),
           "bisection_ms_per_solve": fold([r["event"]["ms_inside_bisection"] for r in new_event]),
           "event_ms_per_solve": fold([r["event"]["median_ms_per_solve"] for r in new_event]),
           "event_solve": {k: new_event[-1]["event"][k] for k in ("trials_per_solve", "rows_fired", "n_event_evals",
                                                                   "bisection_rounds")},
           "plain_trials_per_solve": new_plain[-1]["plain"]["trials_per_solve"]}
    pp, npl = res["parent_plain_ms_per_trial"], res["new_plain_ms_per_trial"]
    res["new_plain_median_inside_parent_min_max"] = pp["min"] <= npl["median"] <= pp["max"]
    extra = res["event_ms_per_trial_without_bisection"]["median"] - pp["median"]
    res["event_extra_ms_per_trial_over_parent_plain"] = round(extra, 4)
    res["event_fn_share_of_extra"] = round(res["event_fn_ms_per_trial"]["median"] / extra, 3) if extra > 0 else None
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


def _grad_headline(reps: int):
    """ms per trial step of forward + backward: odeint_rowwise(differentiable=True) and odeint (eager launches)."""
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B, D = 65536, 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    t = torch.tensor([0.0, 0.5], device=dev)
    calls = [0]

    def f(t_, y):
        calls[0] += 1
        return y @ A.T
    res = {"rowwise_grad_ms_per_trial": [], "odeint_grad_ms_per_trial": []}
    for _ in range(reps + 1):
        for which in ("rowwise", "odeint"):
            calls[0] = 0
            y = y0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if which == "rowwise":
                sol = tda.odeint_rowwise(f, y, t, rtol=1e-7, atol=1e-9, differentiable=True)
            else:
                sol = tda.odeint(f, y, t, rtol=1e-7, atol=1e-9, options={"hip_graph": False})
            sol[-1].sum().backward()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            trials = (calls[0] - 2) / 6
            res[which + "_grad_ms_per_trial"].append(ms / trials)
            res[which + "_trials"] = trials
            del sol, y
    for k in ("rowwise_grad_ms_per_trial", "odeint_grad_ms_per_trial"):
        res[k] = res[k][1:]          # the first pair warms up
    res["ratio_rowwise_over_odeint"] = min(res["rowwise_grad_ms_per_trial"]) / min(res["odeint_grad_ms_per_trial"])
    return res


def _grad_parity():
    """Per-row deviation of the rowwise gradients from the reference's, every fixture case, host path and device."""
    import warnings
    import torchdiffeq_amd as tda
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from _rowwise_grad_cases import CASE_NAMES, row_bounds, solve_case
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        for name in CASE_NAMES:
            entry = {}
            for label, device in (("host", "cpu"), ("hip", torch.device("cuda", 0))):
                dev, spread, _, _ = solve_case(tda, name, device=device)
                entry[label] = {"per_row": [float(v) for v in dev], "worst": float(dev.max()),
                                "worst_row": int(dev.argmax())}
            entry["spread"], entry["bound"] = spread, 0.1 * spread
            entry["row_bounds"] = [float(v) for v in row_bounds(name)]       # (what the tests hold each row to)
            out[name] = entry
    return out


def _grad_stats(paths, bench, n_words=65536 * 128, esize=4):
    """In-situ bandwidth of the backward's row_scale_many launches, (1 + n_out) words per element, from one
    kernel_stats.csv per traced repeat: the per-run average share of the peak, so that their spread can be read."""
    import re
    out = {}
    for run, path in enumerate(paths):
        for r in csv.DictReader(open(path)):
            m = re.search(r"row_scale_many_kernel<float, (\d+), true>", r["Name"])
            if m:
                n_out = int(m.group(1))
                nbytes = (1 + n_out) * n_words * esize
                e = out.setdefault(f"row_scale_many<{n_out}>", {"words_per_element": 1 + n_out, "bytes": nbytes,
                                                                "calls_per_run": int(r["Calls"]), "avg_us": [],
                                                                "avg_share_of_peak": [], "min_share_of_peak": []})
                e["avg_us"].append(float(r["AverageNs"]) / 1e3)
                e["avg_share_of_peak"].append(nbytes / float(r["AverageNs"]) / 1e3 / PEAK_TBS)
                e["min_share_of_peak"].append(nbytes / float(r["MinNs"]) / 1e3 / PEAK_TBS)
            elif "row_dot_" in r["Name"]:
                e = out.setdefault(r["Name"].split("(")[0].replace("void tdeq::", ""),
                                   {"calls_per_run": int(r["Calls"]), "avg_us": []})
                e["avg_us"].append(float(r["AverageNs"]) / 1e3)
    bench["in_situ"] = out
    return bench


def _launch_bytes(B=65536, L=128, esize=4):
    """Algorithmic bytes of each streaming launch of one dopri5 trial step (carried partial sums, tableaus.carry_plan)."""
    from torchdiffeq_amd.tableaus import carry_plan
    plan = carry_plan("dopri5")
    n = B * L * esize
    out = {}
    out["row_combine[0]"] = 3 * n                          # y0, f0 -> y1
    for i, op in enumerate(plan.ops):
        if op is None:
            continue
        out[f"row_combine[{i}]"] = (len(op.idx) + 1 + (1 if op.continues else 0) + len(op.targets)) * n
    out["row_reduce(err)"] = (1 + len(plan.err_idx) + 2) * n      # partial, remaining stages, y0, y1
    out["row_dense_commit(no outputs)"] = 4 * n                     # y1, f1 -> y0, f0 (accepted rows)
    return out


def _mixed():
    import numpy as np
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    B = 1024
    k = torch.logspace(-1, 3, B, dtype=torch.float64, device=dev)[:, None]
    y0 = torch.linspace(0.5, 2.0, B, dtype=torch.float64, device=dev)[:, None]
    t = torch.linspace(0, 5, 9, dtype=torch.float64, device=dev)

    def f(t_, y):
        return -k * (y - torch.sin(3.0 * (t_[:, None] if t_.dim() else t_)))
    acc = [0]
    rej = [0]

    def f_ode(t_, y):
        return f(t_, y)
    f_ode.callback_accept_step = lambda *a: acc.__setitem__(0, acc[0] + 1)
    f_ode.callback_reject_step = lambda *a: rej.__setitem__(0, rej[0] + 1)
    with torch.no_grad():
        _, st = tda.odeint_rowwise(f, y0, t, rtol=1e-6, atol=1e-8, return_stats=True)
        tda.odeint(f_ode, y0, t, rtol=1e-6, atol=1e-8)
    n = st["n_accepted"].numpy()
    return {"B": B, "k_range": [0.1, 1000.0], "rowwise_accepted_min": int(n.min()), "rowwise_accepted_median":
            float(np.median(n)), "rowwise_accepted_max": int(n.max()), "rowwise_rejected_total":
            int(st["n_rejected"].sum()), "rowwise_func_calls": st["nfe"], "odeint_whole_batch_accepted": acc[0],
            "odeint_whole_batch_rejected": rej[0]}


# headline launches (fp32, 65536 x 128): kernel-name prefix -> (streams of N words, what it is).  The single-stage combine
# serves two launches of the carried plan (row 0: f0, y0 -> y1, 3 streams; row 4: carried prefix + k4 + y0 -> y5, 4
# streams), taken at their mean.  The dense-output launch is taken at its fastest call (a step without an output time:
# y1, f1 in, y0, f0 out).
_HEADLINE_LAUNCHES = {
    "row_combine_kernel<float, 1, true>": (3.5, "rows 0 and 4 (mean of 3 and 4 streams)", "avg"),
    "row_combine_kernel<float, 2, true>": (4, "row 1", "avg"),
    "row_combine_kernel<float, 3, true>": (5, "row 2", "avg"),
    "row_combine_kernel<float, 4, true>": (7, "row 3 + carried prefix of row 4", "avg"),
    "row_combine_kernel<float, 5, true>": (8, "row 5 (= y1) + partial error", "avg"),
    "row_reduce_wave_kernel<float, 1, 0, true, true, false>": (4, "error (partial + k6) + row sums", "avg"),
    "row_dense_commit_kernel<float, 6, true>": (4, "commit y1 -> y0, f1 -> f0 (no output time)", "min"),
}


def _stats(path, bench, n_words=65536 * 128, esize=4):
    """In-situ bandwidth of the headline's streaming launches from a rocprofv3 kernel_stats.csv."""
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r["Name"]
        for key, (streams, what, which) in _HEADLINE_LAUNCHES.items():
            if key in name:
                ns = float(r["AverageNs"] if which == "avg" else r["MinNs"])
                nbytes = streams * n_words * esize
                out[key] = {"launch": what, "calls": int(r["Calls"]), "us": ns / 1e3, "timing": which,
                            "bytes": nbytes, "TB_s": nbytes / ns / 1e3, "share_of_peak": nbytes / ns / 1e3 / PEAK_TBS}
        if "row_ctrl_kernel<float" in name:
            out["row_ctrl_kernel<float>"] = {"launch": "per-row controller (65536 rows, not streaming)",
                                             "calls": int(r["Calls"]), "us": float(r["AverageNs"]) / 1e3}
    bench["in_situ"] = out
    return bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--parity", default=None)
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--rowtol", action="store_true")
    ap.add_argument("--event", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--event-summary", default=None)
    ap.add_argument("--setting", default="plain", choices=("plain", "0.5", "1.0"))
    ap.add_argument("--event-compact-summary", default=None)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--dense-calculus", action="store_true")
    ap.add_argument("--dense-calculus-summary", default=None)
    ap.add_argument("--dense-summary", default=None)
    ap.add_argument("--impulse", action="store_true")
    ap.add_argument("--impulse-summary", default=None)
    a = ap.parse_args()
    if a.impulse_summary:
        _impulse_summary(a.impulse_summary.split(","), a.out)
        return
    if a.impulse:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "what": "tools/rowwise_bench.py --impulse: 65536 x 128 fp32 dopri5, func y @ A.T, one bolus per row at tj_r in "
                       "(0.1, 0.4), t = [0, 0.5], rtol 1e-7, atol 1e-9; one process, the two solves alternated, the first "
                       "pair a warm-up",
               "impulse": _impulse(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.dense_summary:
        _dense_summary(a.dense_summary.split(","), a.out)
        return
    if a.dense_calculus_summary:
        _dense_calculus_summary(a.dense_calculus_summary.split(","), a.out)
        return
    if a.dense_calculus:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "what": "tools/rowwise_bench.py --dense-calculus: the record of the --dense solve (65536 x 128 fp32 dopri5, func "
                       "k_r * (y @ A.T), t0 = 0, t1 = 0.5, rtol 1e-7, atol 1e-9); one process: the prefix build, then dense(t), "
                       "derivative, antiderivative and integral alternated for 16 random times per row, check=False, the first "
                       "round a warm-up; host clock around a device synchronise",
               "dense_calculus": _dense_calculus(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.dense:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "what": "tools/rowwise_bench.py --dense: 65536 x 128 fp32 dopri5, func k_r * (y @ A.T) with k_r in "
                       "logspace(-1, 1.5) shuffled, t0 = 0, t1 = 0.5, rtol 1e-7, atol 1e-9; one process, the plain and the "
                       "dense solve alternated, the first pair a warm-up",
               "dense": _dense(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.steps:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "what": "tools/rowwise_bench.py --steps: 65536 x 128 fp32 dopri5, func y @ A.T + 0.5 sign(t - tj_r), one jump "
                       "point per row at tj_r in (0.1, 0.4), t = [0, 0.5], rtol 1e-7, atol 1e-9; one process, the two solves "
                       "alternated, the first pair a warm-up",
               "steps": _steps(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.event_summary:
        _event_summary(a.event_summary.split(","), a.out)
        return
    if a.event_compact_summary:
        _event_compact_summary(a.event_compact_summary.split(","), a.out)
        return
    if a.event and a.compact:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "event_compact": _event_compact(a.reps, a.setting)}
        print(json.dumps(res))
        return
    if a.event:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               **_event(a.reps, a.plain_only)}
        print(json.dumps(res))
        return
    if a.compact:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "compact": _compact(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.grad and a.stats:
        bench = _grad_stats(a.stats.split(","), json.load(open(a.bench)))
        json.dump(bench, open(a.bench, "w"), indent=1)
        print(json.dumps(bench["in_situ"], indent=1))
        return
    if a.grad:
        res = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
               "headline_grad": _grad_headline(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        if a.parity:
            par = _grad_parity()
            os.makedirs(os.path.dirname(a.parity) or ".", exist_ok=True)
            json.dump(par, open(a.parity, "w"), indent=1)
            print(json.dumps({k: {"host": v["host"]["worst"], "hip": v["hip"]["worst"], "bound": v["bound"]}
                              for k, v in par.items()}))
        return
    if a.stats:
        bench = json.load(open(a.bench))
        bench = _stats(a.stats, bench)
        json.dump(bench, open(a.bench, "w"), indent=1)
        print(json.dumps(bench["in_situ"], indent=1))
        return
    res = {"device": torch.cuda.get_device_name(0), "headline": _headline(a.reps, a.rowtol)}
    lb = _launch_bytes()
    res["launch_bytes"] = lb
    res["launch_us_at_peak"] = {k: v / (PEAK_TBS * 1e12) * 1e6 for k, v in lb.items()}
    res["mixed_stiffness"] = _mixed()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
