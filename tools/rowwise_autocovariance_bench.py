"""`RowDenseOutput.autocovariance` on the MI355X at three shapes (65536 x 3, 32768 x 16, 2048 x 64, fp32; the solve of
tools/rowwise_time_moments_bench.py), ONE window per row, the whole interval [t0, t1] of length T.

    python tools/rowwise_autocovariance_bench.py [--reps 5] [--scale 1] [--out profiles/rowwise_autocovariance_bench.json]

One process; per shape one solve; per case (K = 1 with lag 0, K = 16 with lags k T / 32; covariance False and True) the calls
alternate `reps` times after a warm-up round.
    autocovariance   dense.autocovariance(t0, t1, lags, covariance=.., check=False): three searches, the walk kernel of
                     time_moments, then the two-cursor walk kernel or the lagged Gram kernel
    torch_route      the only route without it: dense(t) and dense(t + lag) at the Gauss-Legendre nodes of the steps under t
                     clipped to the overlap — [5 * (most steps of a row), B] times per lag, rows with fewer steps padded with
                     zero weights; nodes and weights are prepared OUTSIDE the timing — the weighted whole-window mean, then
                     per lag an `einsum` of the two deviations in fp64 on the device.  Across a step boundary of t + lag this
                     route is NOT exact (the second factor is no single quartic on a step of t); the difference is reported
    time_moments     dense.time_moments(t0, t1, covariance=.., check=False) on the same windows: at K = 1, lag 0 the ratio is
                     the cost of the second cursor
A sample is the host time of a batch of back-to-back calls between two device synchronisations, divided by the calls.
Reported per call: the times, their median, `torch.cuda.max_memory_allocated` above what was allocated before the batch, the
ratios, and the largest difference of the two routes relative to the largest entry.  Times include the searches and every
allocation of the call; nothing is claimed beyond the file.  `--scale s` divides the row counts by s.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS_PER_SAMPLE = 3
SHAPES = ((65536, 3), (32768, 16), (2048, 64))


def gauss_nodes(dense, tau: float):
    """The nodes of the steps under t for the overlap [t0, t1 - tau] of every row -> (t [N, B] true time, W [N, B] fp64, zero
    for padding and for steps beyond the overlap).  (An ascending solve: true time is solver time.)"""
    from torchdiffeq_amd.rowwise import HostRowKernels
    off, dev = dense.offsets, dense.coeffs.device
    counts = off[1:] - off[:-1]
    N = int(counts.max())
    step = torch.arange(N, device=dev)[:, None]
    live = step < counts[None]
    s = torch.where(live, off[:-1][None] + step, off[:-1][None])
    end = (dense._t1 - tau)[None]
    ta, tb = torch.minimum(dense._ta[s], end), torch.minimum(dense._tb[s], end)
    t = torch.cat([ta + (tb - ta) * n for n, _ in HostRowKernels._TIME_RULE])
    W = torch.cat([torch.where(live, (tb - ta) * w, 0.0) for _, w in HostRowKernels._TIME_RULE])
    return t.contiguous(), W.contiguous()


def run(reps: int, scale: int = 1):
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731
    T = 0.5

    def timed(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(CALLS_PER_SAMPLE):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / CALLS_PER_SAMPLE, torch.cuda.max_memory_allocated() - base, out

    def solve(B, D):
        g = torch.Generator().manual_seed(0)
        G = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5
        A = (0.5 * (G - G.T) - 0.1 * torch.eye(D, dtype=torch.float64)).float().to(dev)
        k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None].float().to(dev)
        y0 = torch.randn(B, D, generator=g).to(dev)
        dense, st = tda.odeint_rowwise_dense(lambda t_, y: k * (y @ A.T), y0, 0.0, T, rtol=1e-7, atol=1e-9, return_stats=True)
        return dense, {"shape": [B, D], "n_segments": dense.n_segments, "accepted_median": float(st["n_accepted"].median()),
                       "accepted_max": int(st["n_accepted"].max())}

    def compare(calls):
        ms_of, peak_of, outs = {n: [] for n in calls}, {}, {}
        for rep in range(reps + 1):                                  # the first round warms up; the calls alternate
            for n, fn in calls.items():
                outs.pop(n, None)
                ms, peak_of[n], outs[n] = timed(fn)
                if rep:
                    ms_of[n].append(ms)
        return {n: {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n]), "peak_bytes_above_start": peak_of[n]}
                for n in calls}, outs

    res = {"dtype": "float32", "calls_per_sample": CALLS_PER_SAMPLE, "window": [0.0, T]}
    with torch.no_grad():
        for B, D in SHAPES:
            dense, info = solve(max(B // scale, 64), D)
            res[f"{B // scale} x {D}"] = shape_res = dict(info)
            whole = gauss_nodes(dense, 0.0)
            for K in (1, 16):
                lags = [k * T / 32 for k in range(K)]
                nodes = [whole if tau == 0.0 else gauss_nodes(dense, tau) for tau in lags]
                lag_dev = torch.tensor(lags, dtype=torch.float64, device=dev)
                for cov in (False, True):
                    def torch_route():
                        y = dense(whole[0], check=False).double()                             # [N, B, D]
                        mean = (whole[1][:, :, None] * y).sum(0) / whole[1].sum(0)[:, None]
                        outs = []
                        for tau, (t, W) in zip(lags, nodes):
                            v = (y if tau == 0.0 else dense(t, check=False).double()) - mean
                            v2 = v if tau == 0.0 else dense(torch.minimum(t + tau, dense._t1[None]), check=False).double() - mean
                            total = W.sum(0)
                            outs.append(torch.einsum("kb,kbi,kbj->bij", W, v, v2) / total[:, None, None] if cov else
                                        torch.einsum("kb,kbi,kbi->bi", W, v, v2) / total[:, None])
                        return torch.stack(outs)
                    r, outs = compare({
                        "autocovariance": lambda: dense.autocovariance(0.0, T, lag_dev, covariance=cov, check=False),
                        "torch_route": torch_route,
                        "time_moments": lambda: dense.time_moments(0.0, T, covariance=cov, check=False)})
                    auto = outs["autocovariance"]
                    got, ref = (auto.covariance if cov else auto.autocovariance).reshape(outs["torch_route"].shape), \
                        outs["torch_route"]
                    r["ratio_autocovariance_to_torch_route"] = r["autocovariance"]["median_ms"] / r["torch_route"]["median_ms"]
                    r["ratio_autocovariance_to_time_moments"] = r["autocovariance"]["median_ms"] / r["time_moments"]["median_ms"]
                    r["peak_ratio_autocovariance_to_torch_route"] = \
                        r["autocovariance"]["peak_bytes_above_start"] / max(r["torch_route"]["peak_bytes_above_start"], 1)
                    r["peak_ratio_autocovariance_to_time_moments"] = \
                        r["autocovariance"]["peak_bytes_above_start"] / max(r["time_moments"]["peak_bytes_above_start"], 1)
                    r["max_difference_over_max_entry"] = float((got - ref).abs().max() / ref.abs().max())
                    shape_res[f"K={K} covariance={cov}"] = {"node_times_per_lag": whole[0].shape[0], **r}
                    print(f"{B // scale} x {D} K={K} covariance={cov}",
                          {n: round(v["median_ms"], 4) for n, v in r.items() if isinstance(v, dict)}, file=sys.stderr, flush=True)
                    del outs, auto, got, ref
            del dense, whole, nodes
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = json.dumps(run(args.reps, args.scale), indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
