"""`RowDenseOutput.cross_covariance` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows
of D = 128 fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]) — the solve of
tools/rowwise_moments_bench.py.

    python tools/rowwise_cross_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_cross_bench.json]

One process, one solve; then, for M = 8 and M = 128 covariates (fp64 [B, M], standard normal plus 50) and Q = 1 and Q = 64
shared times spread over (t0, t1), alternated `reps` times after a warm-up round:
    cross        dense.cross_covariance(t, other, check=False): one search and 6 launches per slice of the times; M = 8 runs
                 the 64 x 16 block (NB = 1), M = 128 the 64 x 64 block (NB = 4)
    torch        what a user does without it: per time dense(t_q, check=False).double(), centre both, y.T @ z / (n - 1)
    cross_nb4    M = 8 only: the same covariates padded with 9 zero columns to M = 17, which takes the 64 x 64 block — what the
                 16-column block saves (the padded columns cost the z sums and the finish a little as well)
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64), divided by the calls.  Reported per call: the times, their median, the ratio, `torch.cuda.max_memory_allocated` above
what was allocated before the batch (the record, the covariates and the solve's leftovers), and the largest difference between
the two answers relative to the largest entry.  Times include the searches and every allocation of the call; nothing is
claimed beyond the file.
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

    with torch.no_grad():
        dense, st = tda.odeint_rowwise_dense(func, y0, 0.0, 0.5, rtol=1e-7, atol=1e-9, return_stats=True)
        res = {"shape": [B, D], "dtype": "float32", "n_segments": dense.n_segments,
               "record_bytes": dense.coeffs.numel() * dense.coeffs.element_size(),
               "accepted_median": float(st["n_accepted"].median())}
        for M in (8, 128):
            z = (50 + torch.randn(B, M, generator=g, dtype=torch.float64)).to(dev)
            padded = torch.cat([z, torch.zeros(B, 9, dtype=torch.float64, device=dev)], dim=1)
            for Q, calls_per_sample in CALLS_PER_SAMPLE.items():
                t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]

                def torch_cross():
                    out = torch.empty(Q, D, M, dtype=torch.float64, device=dev)
                    for j in range(Q):
                        y = dense(t[j], check=False).double()
                        out[j] = (y - y.mean(dim=0)).T @ (z - z.mean(dim=0)) / (B - 1)
                    return out
                calls = {"cross": lambda: dense.cross_covariance(t, z, check=False), "torch": torch_cross}
                if M == 8:
                    calls["cross_nb4"] = lambda: dense.cross_covariance(t, padded, check=False)
                ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
                for rep in range(reps + 1):                                  # the first round warms up; the calls alternate
                    for n, fn in calls.items():
                        outs.pop(n, None)
                        ms, peak_of[n], outs[n] = timed(fn, calls_per_sample)
                        if rep:
                            ms_of[n].append(ms)
                row = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]} for n in calls}
                row["calls_per_sample"] = calls_per_sample
                row["workspace_bytes_per_time"] = dense._k.row_dense_cross_workspace_bytes(1, B, D, M, torch.float32)
                row["ratio_cross_to_torch"] = med(ms_of["cross"]) / med(ms_of["torch"])
                row["rel_diff"] = float((outs["cross"] - outs["torch"]).abs().max() / outs["torch"].abs().max())
                if M == 8:
                    row["ratio_cross_to_cross_nb4"] = med(ms_of["cross"]) / med(ms_of["cross_nb4"])
                    row["nb4_same_bits_as_nb1"] = bool(torch.equal(outs["cross"], outs["cross_nb4"][:, :, :M]))
                res[f"M={M},Q={Q}"] = row
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
