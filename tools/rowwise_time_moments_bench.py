"""`RowDenseOutput.time_moments` on the MI355X at the rowwise bench shape (B = 65536 rows of D = 128 fp32 elements, the solve of
tools/rowwise_ranks_bench.py) and at a small system (D = 3).

    python tools/rowwise_time_moments_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_time_moments_bench.json]

One process; per shape one solve and ONE window per row, the whole interval [t0, t1]; the calls of a case alternate `reps`
times after a warm-up round.
  walk, D = 128 and D = 3 at `rows` rows:
    time_moments   dense.time_moments(t0, t1, check=False): two searches and the walk kernel (two walks of the steps)
    exposure       dense.exposure(0.0, t0, t1, check=False): the same searches, the same reads, ONE walk with the level machine
                   — the ratio is reported as the cost of the second walk
  covariance, D = 3, 16, 64 with `rows` reduced so that the [B, D, D] output stays near 64 MiB:
    time_gram      dense.time_moments(t0, t1, covariance=True, check=False): the walk kernel and the Gram kernel
    torch_route    the only route without it: dense(t) at the same Gauss-Legendre nodes — [5 * (most steps of a row), B] times,
                   rows with fewer steps padded with zero weights; the nodes and weights are prepared OUTSIDE the timing — then
                   the weighted mean and `einsum` of the deviations in fp64 on the device
A sample is the host time of a batch of back-to-back calls between two device synchronisations, divided by the calls.
Reported per call: the times, their median, `torch.cuda.max_memory_allocated` above what was allocated before the batch, the
ratios, and the largest difference of the two covariances relative to the largest entry.  Times include the searches and
every allocation of the call; nothing is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS_PER_SAMPLE = 5


def gauss_nodes(dense):
    """The nodes of `time_moments` for the whole interval of every row -> (t [K, B] true time, W [K, B] fp64, zero for padding)."""
    from torchdiffeq_amd.rowwise import HostRowKernels
    off, dev = dense.offsets, dense.coeffs.device
    counts = off[1:] - off[:-1]
    K, B = int(counts.max()), counts.numel()
    step = torch.arange(K, device=dev)[:, None]
    live = step < counts[None]
    s = torch.where(live, off[:-1][None] + step, off[:-1][None])
    ta, tb = dense._ta[s], torch.minimum(dense._tb[s], dense._t1[None])          # (the last step may end beyond t1)
    t = torch.cat([ta + (tb - ta) * n for n, _ in HostRowKernels._TIME_RULE])
    W = torch.cat([torch.where(live, (tb - ta) * w, 0.0) for _, w in HostRowKernels._TIME_RULE])
    return (t * dense._sign).contiguous(), W.contiguous()


def run(reps: int, rows: int = 65536):
    import torchdiffeq_amd as tda
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]       # noqa: E731

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
        dense, st = tda.odeint_rowwise_dense(lambda t_, y: k * (y @ A.T), y0, 0.0, 0.5, rtol=1e-7, atol=1e-9, return_stats=True)
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

    res = {"dtype": "float32", "calls_per_sample": CALLS_PER_SAMPLE}
    with torch.no_grad():
        for D in (128, 3):
            dense, info = solve(rows, D)
            r, _ = compare({"time_moments": lambda: dense.time_moments(0.0, 0.5, check=False),
                            "exposure": lambda: dense.exposure(0.0, 0.0, 0.5, check=False)})
            r["ratio_time_moments_to_exposure"] = r["time_moments"]["median_ms"] / r["exposure"]["median_ms"]
            res[f"walk D={D}"] = {**info, **r}
            print(f"walk D={D}", {n: round(v["median_ms"], 4) for n, v in r.items() if isinstance(v, dict)}, file=sys.stderr,
                  flush=True)
            del dense
        for D in (3, 16, 64):
            B = min(rows, max(256, (64 << 20) // (8 * D * D)))
            dense, info = solve(B, D)
            t, W = gauss_nodes(dense)

            def torch_route():
                y = dense(t, check=False).double()                                        # [K, B, D]
                total = W.sum(0)
                mean = (W[:, :, None] * y).sum(0) / total[:, None]
                v = y - mean
                return mean, torch.einsum("kb,kbi,kbj->bij", W, v, v) / total[:, None, None]
            r, outs = compare({"time_gram": lambda: dense.time_moments(0.0, 0.5, covariance=True, check=False),
                               "torch_route": torch_route})
            r["ratio_time_gram_to_torch_route"] = r["time_gram"]["median_ms"] / r["torch_route"]["median_ms"]
            cov, ref = outs["time_gram"].covariance, outs["torch_route"][1]
            r["max_difference_over_max_entry"] = float((cov - ref).abs().max() / ref.abs().max())
            res[f"covariance D={D}"] = {**info, "node_times": t.shape[0], **r}
            print(f"covariance D={D}", {n: round(v["median_ms"], 4) for n, v in r.items() if isinstance(v, dict)},
                  file=sys.stderr, flush=True)
            del dense, outs
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
