"""`RowDenseOutput.moments` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows of
D = 128 fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]) — the solve of
tools/rowwise_quantiles_bench.py.

    python tools/rowwise_moments_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_moments_bench.json]

One process, one solve; then, for Q = 1 and Q = 64 shared times spread over (t0, t1), alternated `reps` times after a warm-up
round:
    moments       dense.moments(t, check=False): one search, the sum and finish kernels twice (5 launches per slice)
    torch_var     what a user does without it: per time dense(t_q, check=False).double(), torch.mean and torch.var over the rows
    moments_cov   dense.moments(t, covariance=True, check=False): the Gram kernel instead of the centred sums
    torch_cov     per time dense(t_q, check=False).double(), torch.mean and torch.cov of the transpose
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64), divided by the calls.  Reported per call: the times, their median, the ratios, `torch.cuda.max_memory_allocated` above
what was allocated before the batch (the record and the solve's leftovers) next to what the workspace formula and the search's
lists predict for `moments`, and the largest difference between the two answers relative to the largest entry.  Times include
the searches and every allocation of the call; nothing is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS_PER_SAMPLE = {1: 100, 64: 5}        # a Q = 1 call is well under a millisecond: a sample is a batch of calls, not one


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

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    with torch.no_grad():
        dense, st = tda.odeint_rowwise_dense(func, y0, 0.0, 0.5, rtol=1e-7, atol=1e-9, return_stats=True)
        res = {"shape": [B, D], "dtype": "float32", "n_segments": dense.n_segments,
               "record_bytes": dense.coeffs.numel() * dense.coeffs.element_size(),
               "accepted_median": float(st["n_accepted"].median())}
        for Q, calls_per_sample in ((1, CALLS_PER_SAMPLE[1]), (64, CALLS_PER_SAMPLE[64])):
            t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]

            def torch_var():
                mean, var = (torch.empty(Q, D, dtype=torch.float64, device=dev) for _ in range(2))
                for j in range(Q):
                    y = dense(t[j], check=False).double()
                    mean[j], var[j] = torch.mean(y, dim=0), torch.var(y, dim=0)
                return mean, var

            def torch_cov():
                mean, cov = torch.empty(Q, D, dtype=torch.float64, device=dev), torch.empty(Q, D, D, dtype=torch.float64, device=dev)
                for j in range(Q):
                    y = dense(t[j], check=False).double()
                    mean[j], cov[j] = torch.mean(y, dim=0), torch.cov(y.T)
                return mean, cov
            calls = {"moments": lambda: dense.moments(t, check=False), "torch_var": torch_var,
                     "moments_cov": lambda: dense.moments(t, covariance=True, check=False), "torch_cov": torch_cov}
            ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the four alternate
                for n, fn in calls.items():
                    outs.pop(n, None)
                    ms, peak_of[n], outs[n] = timed(fn, calls_per_sample)
                    if rep:
                        ms_of[n].append(ms)
            row = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]} for n in calls}
            lists = Q * B * (4 + 4 + 8)                                      # seg, x and the fp64 [Q, B] times of the search
            for n, cov in (("moments", False), ("moments_cov", True)):
                per_time = dense._k.row_dense_moments_workspace_bytes(cov, 1, B, D, torch.float32)
                step = min(Q, max(1, (256 << 20) // per_time))
                row[n]["predicted_bytes"] = {"workspace": dense._k.row_dense_moments_workspace_bytes(cov, step, B, D, torch.float32),
                                             "search_lists": lists, "outputs": Q * (8 + 16 * D + (8 * D * D if cov else 0))}
            row["calls_per_sample"] = calls_per_sample
            row["ratio_moments_to_torch_var"] = med(ms_of["moments"]) / med(ms_of["torch_var"])
            row["ratio_moments_cov_to_torch_cov"] = med(ms_of["moments_cov"]) / med(ms_of["torch_cov"])
            row["rel_diff"] = {"mean": rel(outs["moments"].mean, outs["torch_var"][0]),
                               "variance": rel(outs["moments"].variance, outs["torch_var"][1]),
                               "covariance": rel(outs["moments_cov"].covariance, outs["torch_cov"][1])}
            res[f"Q={Q}"] = row
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
