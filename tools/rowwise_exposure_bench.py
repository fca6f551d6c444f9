"""`RowDenseOutput.exposure` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows of D = 128
fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]) — the solve and the windows of
tools/rowwise_level_bench.py.

    python tools/rowwise_exposure_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_exposure_bench.json]

One process, one solve; then, alternated `reps` times after a warm-up round, over two kinds of window per row:
  whole     [t0, t1]: the lane walks every accepted step of its row
  segment   the middle 80 % of one step of the row (chosen at random): one segment per lane
with the level of every element halfway between its `minimum` and `maximum` on the window (computed outside the timed calls),
so that every lane has area on both sides:
    exposure       dense.exposure(level, ta, tb, check=False)
    crossings      dense.crossings(level, ta, tb, check=False): the same walk without the area function
    sampled_area   the workaround the method replaces: the trapezoid rule on relu(dense(t) - level) over `samples` equidistant
                   times per window (256 for `whole`, 32 for `segment`)
Reported per call: the times, their median, the ratio to `crossings`, and how far `sampled_area` is from `area_above`, absolute
and relative to the largest `area_above` of the run.  Times include the two searches and the allocation of the outputs; nothing
is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        res = {"shape": [B, D], "dtype": "float32", "n_segments": dense.n_segments,
               "accepted_median": float(st["n_accepted"].median()), "accepted_max": int(st["n_accepted"].max())}
        for name, (ta, tb) in windows.items():
            level = 0.5 * (dense.maximum(ta, tb, check=False).values[0] + dense.minimum(ta, tb, check=False).values[0])
            samples = 32 if name == "segment" else 256
            u = torch.linspace(0, 1, samples, dtype=torch.float64, device=dev)[:, None]
            grid = ta + u * (tb - ta)
            weight = torch.full((samples, 1, 1), 1.0 / (samples - 1), device=dev)
            weight[0] = weight[-1] = 0.5 / (samples - 1)
            span = (tb - ta)[:, :, None].float()

            def sampled():
                over = torch.relu_(dense(grid, check=False).sub_(level))
                return (over.mul_(weight)).sum(dim=0, keepdim=True) * span
            calls = {"exposure": lambda: dense.exposure(level, ta, tb, check=False),
                     "crossings": lambda: dense.crossings(level, ta, tb, check=False),
                     "sampled_area": sampled}
            ms_of, outs = {n: [] for n in calls}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the three alternate
                for n, fn in calls.items():
                    ms, outs[n] = timed(fn)
                    if rep:
                        ms_of[n].append(ms)
            got, walked = outs["exposure"], outs["crossings"]
            off = (outs["sampled_area"].double() - got.area_above.double()).abs()
            top = float(got.area_above.max())
            res[name] = {"samples": samples,
                         "all_finite": all(bool(torch.isfinite(v).all()) for v in got),
                         "time_above_equals_crossings": bool(torch.equal(got.time_above, walked.time_above)),
                         "area_above": {"max": top, "mean": float(got.area_above.double().mean())},
                         "area_below": {"max": float(got.area_below.max()), "mean": float(got.area_below.double().mean())},
                         "sampled_area_off_area_above": {"max": float(off.max()), "mean": float(off.mean()),
                                                         "max_over_largest_area": float(off.max()) / top,
                                                         "mean_over_mean_area": float(off.mean() / got.area_above.double().mean())}}
            for n in calls:
                res[name][n] = {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n])}
            for n in ("exposure", "sampled_area"):
                res[name][n]["ratio_to_crossings"] = med(ms_of[n]) / med(ms_of["crossings"])
            del outs, grid, got, walked
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
