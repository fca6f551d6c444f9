"""`RowDenseOutput.quantiles` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows of
D = 128 fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]) — the solve of
tools/rowwise_crossing_times_bench.py.

    python tools/rowwise_quantiles_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_quantiles_bench.json]

One process, one solve; then, for Q = 1 and Q = 64 shared times spread over (t0, t1) and the ranks of the probabilities 0.05,
0.5 and 0.95, alternated `reps` times after a warm-up round:
    quantiles    dense.quantiles(t, PROBS, check=False): one search, then the radix select (1 + 2 * 4 launches per slice)
    dense_sort   what a user does without it: per time dense(t_q, check=False), torch.sort(dim=0), index three rows
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64: windows of tens of milliseconds), divided by the calls.  Reported per call: the times, their median, the ratio,
`torch.cuda.max_memory_allocated` above what was allocated before the batch (the record and the solve's leftovers), and
whether the two answers have the same bits.  Times include the searches and every allocation of the call; nothing is claimed
beyond the file.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.05, 0.5, 0.95)
CALLS_PER_SAMPLE = {1: 100, 64: 5}        # a Q = 1 call is half a millisecond: a sample is a batch of calls, not one


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
    ranks = [int(math.floor(p * (B - 1))) for p in PROBS]

    def timed(fn, calls):
        """`calls` back-to-back calls between two synchronisations -> (ms per call, peak bytes above the start, the last result)."""
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls, torch.cuda.max_memory_allocated() - base, out

    with torch.no_grad():
        dense, st = tda.odeint_rowwise_dense(func, y0, 0.0, 0.5, rtol=1e-7, atol=1e-9, return_stats=True)
        res = {"shape": [B, D], "dtype": "float32", "probs": list(PROBS), "ranks": ranks, "n_segments": dense.n_segments,
               "record_bytes": dense.coeffs.numel() * dense.coeffs.element_size(),
               "accepted_median": float(st["n_accepted"].median())}
        for Q, calls_per_sample in ((1, CALLS_PER_SAMPLE[1]), (64, CALLS_PER_SAMPLE[64])):
            t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]

            def dense_sort():
                out = torch.empty(len(ranks), Q, D, device=dev)
                for j in range(Q):
                    out[:, j] = torch.sort(dense(t[j], check=False), dim=0).values[ranks]
                return out
            calls = {"quantiles": lambda: dense.quantiles(t, PROBS, check=False), "dense_sort": dense_sort}
            ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the two alternate
                for n, fn in calls.items():
                    outs.pop(n, None)
                    ms, peak_of[n], outs[n] = timed(fn, calls_per_sample)
                    if rep:
                        ms_of[n].append(ms)
            res[f"Q={Q}"] = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]}
                             for n in calls}
            res[f"Q={Q}"]["calls_per_sample"] = calls_per_sample
            res[f"Q={Q}"]["ratio_quantiles_to_dense_sort"] = med(ms_of["quantiles"]) / med(ms_of["dense_sort"])
            res[f"Q={Q}"]["same_bits"] = bool(torch.equal(outs["quantiles"].view(torch.int32), outs["dense_sort"].view(torch.int32)))
            del outs
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
