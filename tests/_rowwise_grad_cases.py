"""Shared by tests/test_rowwise_grad.py (host path) and tests/test_rowwise_grad_gpu.py (HIP kernels): the right-hand
sides of tests/golden/rowwise_grad.npz (make_golden_rowwise_grad.py) in the batched form `odeint_rowwise` calls, with
the [B] row parameters as ONE leaf nn.Parameter, and the measure the gradient checks use."""
import os

import numpy as np
import torch

OMEGA = 3.0
HERE = os.path.dirname(os.path.abspath(__file__))
# (name, problem, method, grid kind, fixed first step) — the cases of make_golden_rowwise_grad.py
CASES = [
    ("decay_dopri5_t1d", "decay", "dopri5", "t1d", False),
    ("decay_tsit5_t1d", "decay", "tsit5", "t1d", False),
    ("vdp_dopri5_t1d", "vdp", "dopri5", "t1d", False),
    ("vdp_tsit5_t1d", "vdp", "tsit5", "t1d", False),
    ("vdp_dopri5_t2d", "vdp", "dopri5", "t2d", False),
    ("decay_dopri5_t1d_fs", "decay", "dopri5", "t1d", True),
    ("decay_bosh3_t1d", "decay", "bosh3", "t1d", False),
    ("decay_fehlberg2_t1d", "decay", "fehlberg2", "t1d", False),
]
CASE_NAMES = [c[0] for c in CASES]
METHODS = ["dopri5", "tsit5", "bosh3", "fehlberg2", "adaptive_heun", "dopri8"]


class BatchedLeaf(torch.nn.Module):
    """func(t_rows [B], y [B, L]) of the `decay` / `vdp` problems; the row parameters are one leaf Parameter [B]."""

    def __init__(self, problem, params, device="cpu", dtype=torch.float64):
        super().__init__()
        self.problem = problem
        self.p = torch.nn.Parameter(torch.as_tensor(np.asarray(params), dtype=dtype).to(device))

    def forward(self, t, y):
        p = self.p[:, None].to(y.dtype)
        if self.problem == "decay":
            return -p * (y - torch.sin(OMEGA * t[:, None]))
        x, v = y[:, 0:1], y[:, 1:2]
        return torch.cat([v, p * (1 - x * x) * v - x], dim=-1)


def load():
    return (np.load(os.path.join(HERE, "golden", "rowwise.npz")),
            np.load(os.path.join(HERE, "golden", "rowwise_grad.npz")))


def row_deviation(gy, gp, ref_gy, ref_gp):
    """Per row: max|g - g_ref| / max|g_ref| with g = the row's y0 gradient and parameter gradient concatenated — the
    measure of `spread` in make_golden_rowwise_grad.py."""
    to = lambda v: torch.as_tensor(v).detach().to("cpu", torch.float64)      # noqa: E731
    g = torch.cat([to(gy).reshape(len(to(gp)), -1), to(gp)[:, None]], dim=1)
    g_ref = torch.cat([to(ref_gy).reshape(len(to(ref_gp)), -1), to(ref_gp)[:, None]], dim=1)
    return (g - g_ref).abs().amax(dim=1) / g_ref.abs().amax(dim=1)


def row_bounds(name):
    """The bound of every row of a fixture case, from the reference alone.

    The issue's bound: a tenth of spread[case], the largest per-row difference between the reference's gradients at
    the case's tolerances and at tolerances 100x smaller.  Where spread[case] > 1 that bounds nothing (the reference's
    loose and tight gradients of some row share no digit: backprop through a step sequence at the stability limit is
    chaotic), so there each row is ALSO held to its own yardsticks: a tenth of ITS spread, plus ten times the
    distance the reference's own gradient of the row moves under a one-ulp scaling of func's output (noise_rows, two
    samples: an order-of-magnitude estimate of what rounding differences between implementations and machines do to
    the row, hence one order of margin).  Rows whose reference gradient is itself rounding noise keep a vacuous bound
    and say so through it; every other row of these cases is held to 5e-8 .. 2e-3.  No row is skipped."""
    grad = load()[1]
    spread = float(grad[name + "_spread"])
    n = len(grad[name + "_gp"])
    bounds = torch.full((n,), 0.1 * spread, dtype=torch.float64)
    if spread > 1:
        own = 0.1 * torch.as_tensor(grad[name + "_spread_rows"]) + 10 * torch.as_tensor(grad[name + "_noise_rows"])
        bounds = torch.minimum(bounds, own)
    return bounds


def solve_case(tda, name, device="cpu"):
    """The rowwise solve of one fixture case with gradients: (per-row deviation from the fixture, spread, stats,
    (n_acc, n_rej) of rowwise.npz or None when that file has no such solve)."""
    base, grad = load()
    _, problem, method, kind, fixed = next(c for c in CASES if c[0] == name)
    rtol, atol = (float(v) for v in grad[name + "_tol"])
    func = BatchedLeaf(problem, base[f"{problem}_params"], device=device)
    y0 = torch.tensor(base[f"{problem}_y0"], device=device, requires_grad=True)
    t = torch.tensor(base[f"{problem}_{kind}"], device=device)
    opts = {"first_step": torch.tensor(grad[name + "_first_step"])} if fixed else None
    sol, stats = tda.odeint_rowwise(func, y0, t, rtol=rtol, atol=atol, method=method, options=opts, return_stats=True,
                                    differentiable=True)
    loss = (sol * torch.tensor(grad[name + "_W"], device=device)).sum()
    gy, gp = torch.autograd.grad(loss, [y0, func.p])
    dev = row_deviation(gy, gp, grad[name + "_gy"], grad[name + "_gp"])
    counts = None
    if name + "_n_acc" in base.files:
        counts = (base[name + "_n_acc"].tolist(), base[name + "_n_rej"].tolist())
    return dev, float(grad[name + "_spread"]), stats, counts


def random_problem(B, L, dtype, seed):
    """A field that is elementwise in the row index, with per-row rate and frequency; `make(device, idx)` builds it for
    the rows `idx` (all rows when None)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None]
    w = (torch.rand(B, 1, generator=g, dtype=torch.float64) * 4)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64)

    def make(device, idx=None):
        kk, ww = (k, w) if idx is None else (k[idx], w[idx])
        kk, ww = kk.to(device, dtype), ww.to(device, dtype)

        def f(t, y):
            return -kk * y + torch.sin(ww * t[:, None]) * torch.roll(y, 1, dims=1)
        return f
    return y0.to(dtype), make


def loss_weights(shape, dtype, device="cpu"):
    """Fixed weights of the scalar loss sum(sol * W) used by the gradient tests (per element, so rows stay separable)."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64)).reshape(shape).to(device, dtype)
