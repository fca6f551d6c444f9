"""`RowDenseOutput.quantiles(weights=)` on the MI355X at the rowwise bench shape (B = 65536 rows of D = 128 fp32 elements, the
solve of tools/rowwise_quantiles_bench.py).

    python tools/rowwise_wquantiles_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_wquantiles_bench.json]

One process, one solve; then, for Q = 1 and Q = 64 shared times spread over (t0, t1) and the probabilities 0.05, 0.5 and 0.95,
alternated `reps` times after a warm-up round:
    weighted     dense.quantiles(t, PROBS, weights=w, check=False), w = 0.5 + rand [B]: one search, then the scale and units
                 kernels and the 64-bit radix select (3 + 2 * 4 launches per slice)
    subgroup     the same call with 0/1 weights that keep one row in eight
    unweighted   dense.quantiles(t, PROBS, check=False): the reference for the overhead of the weights
    torch_route  what a user does without it, the reference for speed: per time dense(t_q, check=False), torch.sort(dim=0),
                 the gathered weights, an fp64 cumsum and a searchsorted of p times the total
A sample is the host time of a batch of back-to-back calls between two device synchronisations (100 calls for Q = 1, 5 for Q =
64), divided by the calls.  Reported per call: the times, their median, `torch.cuda.max_memory_allocated` above what was
allocated before the batch, the ratios weighted / torch_route, weighted / unweighted and subgroup / weighted, the share of the
elements where `weighted` and `torch_route` (floating-point sums: not the same definition to the last unit) pick the same
value, and the workspace of a slice against its formula.  Times include the searches and every allocation of the call; nothing
is claimed beyond the file.
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
    from torchdiffeq_amd import rowwise_dense
    dev = torch.device("cuda", 0)
    D, P = 128, len(PROBS)
    g = torch.Generator().manual_seed(0)
    G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
    A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
    y0 = torch.randn(B, D, generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)).to(dev)
    one_in_eight = (torch.arange(B) % 8 == 3).double().to(dev)
    probs = torch.tensor(PROBS, dtype=torch.float64, device=dev)
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
        res = {"shape": [B, D], "dtype": "float32", "probs": list(PROBS), "n_segments": dense.n_segments,
               "record_bytes": dense.coeffs.numel() * dense.coeffs.element_size(),
               "accepted_median": float(st["n_accepted"].median())}
        for Q, calls_per_sample in ((1, CALLS_PER_SAMPLE[1]), (64, CALLS_PER_SAMPLE[64])):
            t = torch.linspace(0.0, 0.5, Q + 2, dtype=torch.float64, device=dev)[1:-1]

            def torch_route():
                out = torch.empty(P, Q, D, device=dev)
                for j in range(Q):
                    vals, idx = torch.sort(dense(t[j], check=False), dim=0)
                    cum = w[idx].cumsum(dim=0).T.contiguous()                               # [D, B] fp64
                    at = torch.searchsorted(cum, cum[:, -1:] * probs[None, :]).clamp_max(B - 1)
                    out[:, j] = vals.gather(0, at.T)
                return out
            calls = {"weighted": lambda: dense.quantiles(t, PROBS, weights=w, check=False),
                     "subgroup": lambda: dense.quantiles(t, PROBS, weights=one_in_eight, check=False),
                     "unweighted": lambda: dense.quantiles(t, PROBS, check=False), "torch_route": torch_route}
            ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the four alternate
                for n, fn in calls.items():
                    outs.pop(n, None)
                    ms, peak_of[n], outs[n] = timed(fn, calls_per_sample)
                    if rep:
                        ms_of[n].append(ms)
            r = {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]} for n in calls}
            m = {n: r[n]["median_ms"] for n in calls}
            r["calls_per_sample"] = calls_per_sample
            r["ratio_weighted_to_torch_route"] = m["weighted"] / m["torch_route"]
            r["ratio_weighted_to_unweighted"] = m["weighted"] / m["unweighted"]
            r["ratio_subgroup_to_weighted"] = m["subgroup"] / m["weighted"]
            r["share_equal_to_torch_route"] = float((outs["weighted"] == outs["torch_route"]).double().mean())
            per_time = dense._k.row_dense_quantiles_weighted_workspace_bytes(P, 1, B, D, torch.float32)
            step = min(Q, max(1, rowwise_dense.QUANTILES_WORKSPACE_BYTES // per_time))
            r["slice_times"] = step
            r["workspace_bytes"] = step * per_time
            r["workspace_formula_bytes"] = step * ((P + 1) * ((D + 31) // 32) * 65536 + 32 + 16 * P * D + 8 * B)
            res[f"Q={Q}"] = r
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
