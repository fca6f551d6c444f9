"""`RowDenseOutput.maximum` on the MI355X at the rowwise bench shape (tools/rowwise_bench.py --dense: B = 65536 rows of D = 128
fp32 elements, k_r * (y @ A.T) with k_r over logspace(-1, 1.5), t in [0, 0.5]).

    python tools/rowwise_extremum_bench.py [--reps 5] [--rows 65536] [--out profiles/rowwise_dense_extremum_bench.json]

One process, one solve; then, alternated `reps` times after a warm-up round, over two kinds of window per row:
  whole     [t0, t1]: the lane walks every accepted step of its row
  segment   the middle 80 % of one step of the row (chosen at random): one segment per lane
    maximum      dense.maximum(ta, tb, check=False)
    integral     dense.integral(ta, tb, check=False): reads the same five planes at the window's ends only — a floor for
                 "one launch over [n, D] after two searches", not for the walk
    sampled_max  the workaround the method replaces: dense(t) on `samples` times per window, then max over them (32 per step:
                 32 for `segment`, 32 * the median accepted steps but at most 256 for `whole`, whose output is samples * B * D words)
Reported per call: the times, their median, and for `maximum` the share of (segment, element) pairs and of lanes that start a
bisection (from the record: a sign change of y' over the step or of y'' over one of its pieces), and how far `sampled_max`
falls below `maximum`.  Times include the two searches and the allocation of the outputs; nothing is claimed beyond the file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _bisecting(dense):
    """bool [n_seg, D]: the whole-step walk of this element starts a bisection on this segment (evaluated in fp64)."""
    _, d, c, b, a = dense.coeffs.double().unbind(0)
    neg = lambda v: v < 0                        # noqa: E731
    c2, b6, a12 = c + c, 6 * b, 12 * a
    g1 = lambda x: c2 + x * (b6 + x * a12)       # noqa: E731
    x1 = -b / (4 * a)
    inside = (a != 0) & (x1 > 0) & (x1 < 1)
    mid = torch.where(inside, g1(torch.where(inside, x1, torch.zeros_like(x1))), c2)
    curvature = (neg(c2) != neg(mid)) | (neg(mid) != neg(c2 + b6 + a12))
    slope = neg(d) != neg(d + c2 + 3 * b + 4 * a)
    return curvature | slope


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
        dense._integral_prefix()                                             # (built once, outside the timed calls)
        count = dense.offsets[1:] - dense.offsets[:-1]
        pick = dense.offsets[:-1] + (torch.rand(B, generator=g, dtype=torch.float64).to(dev) * count).long().clamp(max=count - 1)
        lo, hi = dense.seg_start[pick], torch.minimum(dense.seg_end[pick], dense.t1)
        windows = {"whole": (dense.t0[None].clone(), dense.t1[None].clone()),
                   "segment": ((lo + 0.1 * (hi - lo))[None], (lo + 0.9 * (hi - lo))[None])}
        steps = int(st["n_accepted"].median())
        bis = _bisecting(dense)
        row_of = torch.repeat_interleave(torch.arange(B, device=dev), count)
        lanes = torch.zeros(B, D, device=dev).index_add_(0, row_of, bis.float()) > 0
        res = {"shape": [B, D], "dtype": "float32", "n_segments": dense.n_segments, "accepted_median": float(steps),
               "accepted_max": int(st["n_accepted"].max()),
               "bisecting_share": {"segment_elements": float(bis.float().mean()),
                                   "lanes_whole": float(lanes.float().mean()),
                                   "lanes_segment": float(bis[pick].float().mean())}}
        for name, (ta, tb) in windows.items():
            samples = 32 if name == "segment" else min(32 * steps, 256)
            u = torch.linspace(0, 1, samples, dtype=torch.float64, device=dev)[:, None]
            grid = ta + u * (tb - ta)
            calls = {"maximum": lambda: dense.maximum(ta, tb, check=False).values,
                     "integral": lambda: dense.integral(ta, tb, check=False),
                     "sampled_max": lambda: dense(grid, check=False).amax(dim=0, keepdim=True)}
            ms_of, outs = {n: [] for n in calls}, {}
            for rep in range(reps + 1):                                      # the first round warms up; the three alternate
                for n, fn in calls.items():
                    ms, outs[n] = timed(fn)
                    if rep:
                        ms_of[n].append(ms)
            short = (outs["maximum"] - outs["sampled_max"]).double()
            res[name] = {"samples": samples,
                         "all_finite": all(bool(torch.isfinite(o).all()) for o in outs.values()),
                         "sampled_max_below_maximum": {"max": float(short.max()), "min": float(short.min()),
                                                       "share_strictly_below": float((short > 0).float().mean())}}
            for n in calls:
                res[name][n] = {"ms_per_call": ms_of[n], "median_ms": med(ms_of[n])}
            for n in ("integral", "sampled_max"):
                res[name][n]["ratio_to_maximum"] = med(ms_of[n]) / med(ms_of["maximum"])
            del outs, grid
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
