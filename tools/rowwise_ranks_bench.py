"""`RowDenseOutput.ranks` on the MI355X at the rowwise bench shape (B = 65536 rows of D = 128 fp32 elements, the solve of
tools/rowwise_quantiles_bench.py).

    python tools/rowwise_ranks_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_ranks_bench.json]

One process, one solve; then, for Q = 1 and Q = 64 shared times spread over (t0, t1), V = 3 and V = 16 thresholds per time
and element (the population's own quantiles, so `equal` is nonzero), unweighted and under w = 0.5 + rand [B], alternated
`reps` times after a warm-up round:
    ranks        dense.ranks(t, values, [weights=w,] check=False): one search, a clear launch and ONE counting pass (weighted:
                 the scale, units and finish launches as well, per slice of the times)
    torch_route  what a user does without it: per time dense(t_q, check=False), then per threshold `(y < v).sum(0)` and `(y ==
                 v).sum(0)`; weighted: the fp64 sums `(w[:, None] * (y < v)).sum(0)` and the same for `==`
    quantiles    dense.quantiles(t, (0.05, 0.5, 0.95), [weights=w,] check=False): the yardstick of one counting pass against
                 the sizeof(dtype) passes of the radix select
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64), divided by the calls.  Reported per call: the times, their median, `torch.cuda.max_memory_allocated` above what was
allocated before the batch, the ratios ranks / torch_route and ranks / quantiles, whether the counts of `ranks` and
`torch_route` agree (unweighted: every count; weighted: the largest difference of the two CDFs, floating-point sums against
fixed-point units), and the cost of V = 16 against V = 3 (four threshold groups against one).  Times include the searches and
every allocation of the call; nothing is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.05, 0.5, 0.95)
CALLS_PER_SAMPLE = {1: 100, 64: 5}


def run(reps: int, B: int = 65536):
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    D = 128
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    func = lambda t_, y: k * (y @ A.T)           # noqa: E731

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
        res = {"shape": [B, D], "dtype": "float32", "n_segments": dense.n_segments,
               "record_bytes": dense.coeffs.numel() * dense.coeffs.element_size(),
               "accepted_median": float(st["n_accepted"].median())}
        print("solved:", res, file=sys.stderr, flush=True)
        for Q in (1, 64):
            t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]
            for V in (3, 16):
                probs = PROBS if V == 3 else torch.linspace(0.02, 0.98, V).tolist()
                values = dense.quantiles(t, probs, check=False)                           # [V, Q, D]
                for weights in (None, w):
                    kw = {} if weights is None else {"weights": weights}

                    def torch_route():
                        below, equal = (torch.empty(V, Q, D, dtype=torch.int64 if weights is None else torch.float64, device=dev)
                                        for _ in range(2))
                        for j in range(Q):
                            y = dense(t[j], check=False)
                            for v in range(V):
                                lt, eq = y < values[v, j], y == values[v, j]
                                below[v, j] = lt.sum(0) if weights is None else (weights[:, None] * lt).sum(0)
                                equal[v, j] = eq.sum(0) if weights is None else (weights[:, None] * eq).sum(0)
                        return below, equal
                    calls = {"ranks": lambda: dense.ranks(t, values, check=False, **kw), "torch_route": torch_route,
                             "quantiles": lambda: dense.quantiles(t, PROBS, check=False, **kw)}
                    ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
                    for rep in range(reps + 1):                              # the first round warms up; the three alternate
                        for n, fn in calls.items():
                            outs.pop(n, None)
                            ms, peak_of[n], outs[n] = timed(fn, CALLS_PER_SAMPLE[Q])
                            if rep:
                                ms_of[n].append(ms)
                    r = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]}
                         for n in calls}
                    r["calls_per_sample"] = CALLS_PER_SAMPLE[Q]
                    r["ratio_ranks_to_torch_route"] = r["ranks"]["median_ms"] / r["torch_route"]["median_ms"]
                    r["ratio_ranks_to_quantiles"] = r["ranks"]["median_ms"] / r["quantiles"]["median_ms"]
                    got, (t_below, t_equal) = outs["ranks"], outs["torch_route"]
                    if weights is None:
                        r["counts_agree"] = bool(torch.equal(got.below, t_below) and torch.equal(got.equal, t_equal))
                    else:
                        cdf = (got.below + got.equal).double() / got.total.double()[:, None]
                        r["max_cdf_difference"] = float((cdf - (t_below + t_equal) / weights.sum()).abs().max())
                    name = f"Q={Q} V={V} {'unweighted' if weights is None else 'weighted'}"
                    res[name] = r
                    print(name, {n: round(r[n]["median_ms"], 4) for n in calls}, file=sys.stderr, flush=True)     # progress
                    del outs
            for name in ("unweighted", "weighted"):
                res[f"Q={Q} {name} ratio_V16_to_V3"] = (res[f"Q={Q} V=16 {name}"]["ranks"]["median_ms"]
                                                        / res[f"Q={Q} V=3 {name}"]["ranks"]["median_ms"])
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
