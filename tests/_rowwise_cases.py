"""Right-hand sides of tests/golden/rowwise.npz (make_golden_rowwise.py) in the batched form `odeint_rowwise` calls:
func(t_rows [B], y [B, L]) with one parameter per row."""
import numpy as np
import torch

OMEGA = 3.0
RTOL, ATOL = 1e-6, 1e-8
GOLDEN = "rowwise.npz"


class Batched(torch.nn.Module):
    def __init__(self, problem, params, device="cpu"):
        super().__init__()
        self.problem = problem
        self.register_buffer("p", torch.as_tensor(np.asarray(params), dtype=torch.float64, device=device)[:, None])

    def forward(self, t, y):
        p = self.p.to(y.dtype)
        if self.problem == "decay":
            return -p * (y - torch.sin(OMEGA * t[:, None]))
        x, v = y[:, 0:1], y[:, 1:2]
        return torch.cat([v, p * (1 - x * x) * v - x], dim=-1)


def cases(golden):
    """(problem, method, kind, func params, y0 [B, L], t, expected solution, n_acc, n_rej) for every stored solve."""
    for problem in ("decay", "vdp"):
        for method in ("dopri5", "tsit5"):
            for kind in ("t1d", "t2d"):
                key = f"{problem}_{method}_{kind}"
                yield (problem, method, kind, golden[f"{problem}_params"], golden[f"{problem}_y0"],
                       golden[f"{problem}_{kind}"], golden[key + "_sol"], golden[key + "_n_acc"], golden[key + "_n_rej"])
