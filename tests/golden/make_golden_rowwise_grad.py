"""Generate tests/golden/rowwise_grad.npz: per-row GRADIENTS of the REFERENCE's `odeint`, every row solved ALONE.

Run in the build container only (the reference is mounted read-only at /root/reference and does not exist on the GPU
box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rowwise_grad.py

The problems, 16 rows, parameters and grids are those of rowwise.npz (make_golden_rowwise.py).  Each row's parameter and
initial state are leaves; the row is solved with the reference in grad mode, loss_r = sum(sol_r * W_r) with the fixed
weights W stored in the file, and d loss_r / d y0_r, d loss_r / d param_r are stored.  Every case is solved a second
time with tolerances 100x smaller; spread[case] = max over rows of max|g - g_tight| / max|g_tight| (g = the row's y0
gradient and parameter gradient concatenated) is the reference's own discretisation spread, the yardstick of the
tests' tolerance; the per-row values are stored as spread_rows[case].

Where spread[case] > 1 the loose and the tight gradient of some row do not share a digit: backprop through a step
sequence at the stability limit is chaotic there, and a tenth of such a spread bounds nothing.  For these cases the
maker also measures how far the reference's OWN gradient of each row moves when func's output is scaled by 1 +- 2^-52
(what a last-bit difference of `sin` or of a product between two machines does at every evaluation):
noise_rows[case] = the larger of the two responses, in the same measure.  Only numbers are stored.
"""
import os
import sys
import time

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import torchdiffeq  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(1)

OMEGA = 3.0
# (name, problem, method, grid kind, rtol, atol, fixed first step)
CASES = [
    ("decay_dopri5_t1d", "decay", "dopri5", "t1d", 1e-6, 1e-8, False),
    ("decay_tsit5_t1d", "decay", "tsit5", "t1d", 1e-6, 1e-8, False),
    ("vdp_dopri5_t1d", "vdp", "dopri5", "t1d", 1e-6, 1e-8, False),
    ("vdp_tsit5_t1d", "vdp", "tsit5", "t1d", 1e-6, 1e-8, False),
    ("vdp_dopri5_t2d", "vdp", "dopri5", "t2d", 1e-6, 1e-8, False),
    ("decay_dopri5_t1d_fs", "decay", "dopri5", "t1d", 1e-6, 1e-8, True),
    ("decay_bosh3_t1d", "decay", "bosh3", "t1d", 1e-4, 1e-6, False),
    ("decay_fehlberg2_t1d", "decay", "fehlberg2", "t1d", 1e-4, 1e-6, False),
]


class Row(torch.nn.Module):
    """One row's right-hand side as the reference sees it (state [1, L], t 0-dim), its parameter a leaf."""

    def __init__(self, problem, p, scale=1.0):
        super().__init__()
        self.problem, self.scale = problem, scale
        self.p = torch.nn.Parameter(torch.tensor(float(p), dtype=torch.float64))

    def forward(self, t, y):
        if self.problem == "decay":
            out = -self.p * (y - torch.sin(OMEGA * t))
        else:
            x, v = y[..., 0:1], y[..., 1:2]
            out = torch.cat([v, self.p * (1 - x * x) * v - x], dim=-1)
        return out if self.scale == 1.0 else out * self.scale


def row_grads(problem, p, y0_row, t, w_row, method, rtol, atol, first_step, scale=1.0):
    f = Row(problem, p, scale)
    y0 = torch.tensor(y0_row[None], dtype=torch.float64, requires_grad=True)
    opts = None if first_step is None else {"first_step": float(first_step)}
    sol = torchdiffeq.odeint(f, y0, torch.tensor(t, dtype=torch.float64), rtol=rtol, atol=atol, method=method,
                             options=opts)
    loss = (sol[:, 0] * torch.tensor(w_row)).sum()
    gy, gp = torch.autograd.grad(loss, [y0, f.p])
    return gy[0].numpy(), float(gp)


def main():
    base = np.load(os.path.join(HERE, "rowwise.npz"))
    out = {}
    for name, problem, method, kind, rtol, atol, fixed in CASES:
        start = time.time()
        params, y0, tg = base[f"{problem}_params"], base[f"{problem}_y0"], base[f"{problem}_{kind}"]
        B, L, T = y0.shape[0], y0.shape[1], tg.shape[0]
        W = np.cos(np.arange(T * B * L, dtype=np.float64)).reshape(T, B, L)
        fs = 1e-3 * (1.0 + np.arange(B) / B) if fixed else None
        gy, gp, gy_t, gp_t = [], [], [], []
        for r in range(B):
            t = tg if kind == "t1d" else tg[:, r]
            step = None if fs is None else fs[r]
            a, b = row_grads(problem, params[r], y0[r], t, W[:, r], method, rtol, atol, step)
            c, d = row_grads(problem, params[r], y0[r], t, W[:, r], method, rtol * 1e-2, atol * 1e-2, step)
            gy.append(a), gp.append(b), gy_t.append(c), gp_t.append(d)
        gy, gp, gy_t, gp_t = np.stack(gy), np.array(gp), np.stack(gy_t), np.array(gp_t)
        g = np.concatenate([gy, gp[:, None]], axis=1)
        g_t = np.concatenate([gy_t, gp_t[:, None]], axis=1)
        per_row = np.abs(g - g_t).max(axis=1) / np.abs(g_t).max(axis=1)
        out[name + "_W"] = W
        out[name + "_gy"], out[name + "_gp"] = gy, gp
        out[name + "_gy_tight"], out[name + "_gp_tight"] = gy_t, gp_t
        out[name + "_spread"] = np.array(per_row.max())
        out[name + "_spread_rows"] = per_row
        if per_row.max() > 1:
            noise = np.zeros(B)
            for r in range(B):
                t = tg if kind == "t1d" else tg[:, r]
                step = None if fs is None else fs[r]
                for scale in (1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52):
                    a, b = row_grads(problem, params[r], y0[r], t, W[:, r], method, rtol, atol, step, scale)
                    moved = np.abs(np.append(a, b) - g[r]).max() / np.abs(g[r]).max()
                    noise[r] = max(noise[r], moved)
            out[name + "_noise_rows"] = noise
            print(name, "noise per row", " ".join(f"{v:.1e}" for v in noise), flush=True)
        out[name + "_tol"] = np.array([rtol, atol])
        if fs is not None:
            out[name + "_first_step"] = fs
        print(name, "spread", float(per_row.max()), "per row", float(per_row.min()), "..", float(per_row.max()),
              f"{time.time() - start:.0f} s", flush=True)
    np.savez_compressed(os.path.join(HERE, "rowwise_grad.npz"), **out)


if __name__ == "__main__":
    main()
