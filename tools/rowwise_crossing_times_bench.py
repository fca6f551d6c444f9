"""`RowDenseOutput.crossing_times` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows of
D = 128 fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]) — the solve, the levels and the windows
of tools/rowwise_level_bench.py.

    python tools/rowwise_crossing_times_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_crossing_times_bench.json]

One process, one solve; then, alternated `reps` times after a warm-up round, over two kinds of window per row:
  whole     [t0, t1]: the lane walks every accepted step of its row
  segment   the middle 80 % of one step of the row (chosen at random): one segment per lane
with the level of every element halfway between its `minimum` and `maximum` on the window (computed outside the timed calls),
so that every lane crosses at least once:
    crossing_times   dense.crossing_times(level, ta, tb, max_count=4, check=False)
    crossings        dense.crossings(level, ta, tb, check=False): the same walk, which keeps the first and the last crossing only
Reported per call: the times, their median, the ratio to `crossings`, the counts per direction, the share of lists that
overflow `max_count`, and whether the counts add up to `crossings.count`.  Times include the two searches and the allocation
of the outputs (16 * max_count bytes per element and window for the lists); nothing is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_COUNT = 4


def run(reps: int, B: int = 65536):
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    D = 128
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
        count = dense.offsets[1:] - dense.offsets[:-1]
        pick = dense.offsets[:-1] + (torch.rand(B, generator=g, dtype=torch.float64).to(dev) * count).long().clamp(max=count - 1)
        lo, hi = dense.seg_start[pick], torch.minimum(dense.seg_end[pick], dense.t1)
        windows = {"whole": (dense.t0[None].clone(), dense.t1[None].clone()),
                   "segment": ((lo + 0.1 * (hi - lo))[None], (lo + 0.9 * (hi - lo))[None])}
        res = {"shape": [B, D], "dtype": "float32", "max_count": MAX_COUNT, "n_segments": dense.n_segments,
               "accepted_median": float(st["n_accepted"].median()), "accepted_max": int(st["n_accepted"].max())}
        for name, (ta, tb) in windows.items():
            level = 0.5 * (dense.maximum(ta, tb, check=False).values[0] + dense.minimum(ta, tb, check=False).values[0])
            calls = {"crossing_times": lambda: dense.crossing_times(level, ta, tb, max_count=MAX_COUNT, check=False),
                     "crossings": lambda: dense.crossings(level, ta, tb, check=False)}
            ms_of, outs = {n: [] for n in calls}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the two alternate
                for n, fn in calls.items():
                    outs.pop(n, None)                                        # (the lists of the round before are freed first)
                    ms, outs[n] = timed(fn)
                    if rep:
                        ms_of[n].append(ms)
            got, walked = outs["crossing_times"], outs["crossings"]
            res[name] = {"counts_add_up": bool(torch.equal(got.n_rising + got.n_falling, walked.count)),
                         "all_counted": bool((got.n_rising >= 0).all()) and bool((got.n_falling >= 0).all()),
                         "list_bytes": 2 * got.rising.numel() * got.rising.element_size()}
            for which, n in (("rising", got.n_rising), ("falling", got.n_falling)):
                res[name][f"n_{which}"] = {"min": int(n.min()), "max": int(n.max()), "mean": float(n.double().mean()),
                                          "share_overflowing": float((n > MAX_COUNT).float().mean())}
            res[name]["share_of_elements_with_an_overflowing_list"] = float(
                ((got.n_rising > MAX_COUNT) | (got.n_falling > MAX_COUNT)).float().mean())
            for n in calls:
                res[name][n] = {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n])}
            res[name]["crossing_times"]["ratio_to_crossings"] = med(ms_of["crossing_times"]) / med(ms_of["crossings"])
            del outs, got, walked
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = json.dumps(run(args.reps, args.rows), indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
