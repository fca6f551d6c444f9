"""`weights=` of `RowDenseOutput.moments` / `.cross_covariance` on the MI355X at the rowwise bench shape (B = 65536 rows of D =
128 fp32 elements, the solve of tools/rowwise_moments_bench.py).

    python tools/rowwise_weighted_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_weighted_bench.json]

One process, one solve; then for Q = 1 and Q = 64 shared times spread over (t0, t1) and `[Q, B]` weights 0.5 + rand, five
cases — moments, moments with covariance, and the cross-covariance with M = 8 and M = 128 covariates — each with three calls
alternated `reps` times after a warm-up round:
    weighted     the method with weights=w: the row_dense_w* kernels
    unweighted   the same method without weights: the kernels and launches of the parent commit, untouched by this change
    torch        what a user does without it: per time dense(t_q, check=False).double(), then the weighted mean and variance,
                 torch.cov(aweights=w_q), or the centred y.T @ (w z) / D
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64), divided by the calls.  Reported per call: the times, their median, the ratios, `torch.cuda.max_memory_allocated` above
what was allocated before the batch, and the largest difference between the weighted answer and torch's relative to the
largest entry.  Times include the searches and every allocation of the call; nothing is claimed beyond the file.
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
        zs = {M: (50 + torch.randn(B, M, generator=g, dtype=torch.float64)).to(dev) for M in (8, 128)}
        for Q, calls_per_sample in CALLS_PER_SAMPLE.items():
            t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]
            w = (0.5 + torch.rand(Q, B, generator=g, dtype=torch.float64)).to(dev)

            def torch_route(case, M):
                outs = []
                for j in range(Q):
                    y, wj = dense(t[j], check=False).double(), w[j]
                    if case == "covariance":
                        outs.append(torch.cov(y.T, aweights=wj))
                        continue
                    W1 = wj.sum()
                    div = W1 - (wj * wj).sum() / W1
                    dy = y - (wj[:, None] * y).sum(dim=0) / W1
                    if case == "moments":
                        outs.append((wj[:, None] * dy * dy).sum(dim=0) / div)
                    else:
                        z = zs[M]
                        outs.append(dy.T @ (wj[:, None] * (z - (wj[:, None] * z).sum(dim=0) / W1)) / div)
                return torch.stack(outs)

            cases = {"moments": (lambda **kw: dense.moments(t, check=False, **kw).variance, None),
                     "covariance": (lambda **kw: dense.moments(t, covariance=True, check=False, **kw).covariance, None),
                     "cross_M8": (lambda **kw: dense.cross_covariance(t, zs[8], check=False, **kw), 8),
                     "cross_M128": (lambda **kw: dense.cross_covariance(t, zs[128], check=False, **kw), 128)}
            for case, (method, M) in cases.items():
                calls = {"weighted": lambda: method(weights=w), "unweighted": lambda: method(),
                         "torch": lambda: torch_route(case.split("_")[0], M)}
                ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
                for rep in range(reps + 1):                                  # the first round warms up; the calls alternate
                    for n, fn in calls.items():
                        outs.pop(n, None)
                        ms, peak_of[n], outs[n] = timed(fn, calls_per_sample)
                        if rep:
                            ms_of[n].append(ms)
                row = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]} for n in calls}
                row["calls_per_sample"] = calls_per_sample
                row["ratio_weighted_to_unweighted"] = med(ms_of["weighted"]) / med(ms_of["unweighted"])
                row["ratio_weighted_to_torch"] = med(ms_of["weighted"]) / med(ms_of["torch"])
                row["rel_diff"] = float((outs["weighted"].reshape(outs["torch"].shape) - outs["torch"]).abs().max()
                                        / outs["torch"].abs().max())
                res[f"{case},Q={Q}"] = row
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
