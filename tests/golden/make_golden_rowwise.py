"""Generate tests/golden/rowwise.npz by running the REFERENCE's `odeint` on every row ALONE.

Run in the build container only (the reference is mounted read-only at /root/reference and does not exist on the GPU
box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rowwise.py

Two fp64 problems, 16 rows each, with parameters spread so that the rows' step counts differ by more than 10x:
  * "decay":  y' = -k_r (y - sin(w t)), one element per row, k_r from 0.1 to 1000 (non-autonomous: func uses t)
  * "vdp":    the Van der Pol oscillator x' = v, v' = mu_r (1 - x^2) v - x, mu_r from 0.1 to 60
each solved with dopri5 and tsit5 on a shared 1-D output grid and on a per-row 2-D grid.  The accepted / rejected
counts come from the reference's step callbacks.  Only numbers are stored.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import torchdiffeq  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(1)

B = 16
RTOL, ATOL = 1e-6, 1e-8
OMEGA = 3.0
PARAMS = {"decay": np.logspace(-1, 3, B), "vdp": np.geomspace(0.1, 60.0, B)}
T_END = {"decay": 5.0, "vdp": 10.0}


def y0_of(problem):
    if problem == "decay":
        return np.linspace(0.5, 2.0, B)[:, None]
    return np.stack([np.linspace(1.0, 2.0, B), np.linspace(0.0, -0.5, B)], axis=1)


def grids(problem):
    """(shared [T], per-row [T, B]): the per-row grid has its own end time and uneven spacing per row."""
    n = 9
    shared = np.linspace(0.0, T_END[problem], n)
    frac = np.linspace(0.0, 1.0, n)[:, None] ** 1.5
    ends = T_END[problem] * (0.4 + 0.6 * np.arange(B) / (B - 1))
    starts = 0.05 * np.arange(B)
    per_row = starts[None, :] + frac * (ends - starts)[None, :]
    return shared, per_row


class Row(torch.nn.Module):
    """One row's right-hand side, as the reference sees it: state [1, L], t 0-dim."""

    def __init__(self, problem, p):
        super().__init__()
        self.problem, self.p = problem, float(p)
        self.n_acc = self.n_rej = 0

    def forward(self, t, y):
        if self.problem == "decay":
            return -self.p * (y - torch.sin(OMEGA * t))
        x, v = y[..., 0:1], y[..., 1:2]
        return torch.cat([v, self.p * (1 - x * x) * v - x], dim=-1)

    def callback_accept_step(self, t0, y0, dt):
        self.n_acc += 1

    def callback_reject_step(self, t0, y0, dt):
        self.n_rej += 1


def main():
    out = {}
    for problem in ("decay", "vdp"):
        y0 = y0_of(problem)
        shared, per_row = grids(problem)
        out[f"{problem}_params"] = PARAMS[problem]
        out[f"{problem}_y0"] = y0
        out[f"{problem}_t1d"] = shared
        out[f"{problem}_t2d"] = per_row
        for method in ("dopri5", "tsit5"):
            for kind in ("t1d", "t2d"):
                sols, acc, rej = [], [], []
                for r in range(B):
                    f = Row(problem, PARAMS[problem][r])
                    t = torch.tensor(shared if kind == "t1d" else per_row[:, r], dtype=torch.float64)
                    with torch.no_grad():
                        s = torchdiffeq.odeint(f, torch.tensor(y0[r:r + 1]), t, rtol=RTOL, atol=ATOL, method=method)
                    sols.append(s[:, 0].numpy())
                    acc.append(f.n_acc)
                    rej.append(f.n_rej)
                key = f"{problem}_{method}_{kind}"
                out[key + "_sol"] = np.stack(sols, axis=1)          # [T, B, L]
                out[key + "_n_acc"] = np.array(acc, dtype=np.int64)
                out[key + "_n_rej"] = np.array(rej, dtype=np.int64)
                print(key, "accepted", min(acc), "..", max(acc), "rejected", sum(rej))
    np.savez_compressed(os.path.join(HERE, "rowwise.npz"), **out)


if __name__ == "__main__":
    main()
