"""Per-row tolerances of `odeint_rowwise` on the HIP kernels (tdeq_row_reduce_tol inside a solve): the statements of
tests/test_rowwise_tol.py on the device.  Row r of a solve with [B] tolerances has the bits and counts of the one-row
device solve with the row's two scalars; constant vectors have the bits of the scalar solve; a compacted solve those of
the plain one; a recorded solve the forward bits of the plain one."""
import warnings

import pytest
import torch

from _rowwise_compact_oracle import assert_same_solve, random_problem
from _rowwise_kernels import LONG_NV, row_lengths
from _rowwise_tol_oracle import MIXED_B, mixed_problem

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _same(a, b):
    (sa, ta), (sb, tb) = a, b
    assert torch.equal(sa, sb)
    assert torch.equal(ta["n_accepted"], tb["n_accepted"]) and torch.equal(ta["n_rejected"], tb["n_rejected"])
    assert ta["nfe"] == tb["nfe"]


def _assert_rows_are_one_row_solves(sol, stats, y0, t, rtol, atol, subset, method):
    for r in range(y0.shape[0]):
        with torch.no_grad():
            one, st = tda.odeint_rowwise(subset(slice(r, r + 1)), y0[r:r + 1], t, rtol=float(rtol[r]), atol=float(atol[r]),
                                         method=method, return_stats=True)
        assert torch.equal(one[:, 0], sol[:, r]), r
        assert int(st["n_accepted"][0]) == int(stats["n_accepted"][r]), r
        assert int(st["n_rejected"][0]) == int(stats["n_rejected"][r]), r


@pytest.mark.parametrize("method", ["dopri5", "dopri8"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_hip_mixed_tolerances(dtype, method):
    y0, t, rtol, atol, plain, by_rows, subset = mixed_problem(dtype, DEV)
    t = t.to(DEV)
    with torch.no_grad():
        mixed = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, method=method, return_stats=True)
        _, loose = tda.odeint_rowwise(plain, y0, t, rtol=float(rtol.max()), atol=float(atol.max()), method=method,
                                      return_stats=True)
    sol, stats = mixed
    assert sol.device.type == "cuda"
    trials = stats["n_accepted"] + stats["n_rejected"]
    trials_loose = loose["n_accepted"] + loose["n_rejected"]
    print(f"{dtype} {method}: trials per row {trials.tolist()}, at the loosest pair {trials_loose.tolist()}")
    # the tolerances are looked at: with every row at the loosest pair the rows take another number of trial steps.  At
    # least half of them for dopri5 (tests/test_rowwise_tol.py's condition); an order-8 pair's step count moves with
    # tol^(-1/8), 2.4 x over fp32's three decades on rows of 3 to 16 steps, so there one row is asked for
    assert int((trials != trials_loose).sum()) >= (MIXED_B // 2 if method == "dopri5" else 1)
    _assert_rows_are_one_row_solves(sol, stats, y0, t, rtol, atol, subset, method)
    # a compacted solve: the tolerance vectors follow the rows through every repack
    with torch.no_grad():
        compact = tda.odeint_rowwise(by_rows, y0, t, rtol=rtol, atol=atol, method=method, return_stats=True, compact=1.0)
    _, repacks = assert_same_solve(mixed, compact, 1.0, method)
    assert repacks >= 1
    # constant vectors: the scalar solve
    x_r, x_a = (1e-6, 1e-8) if dtype == F64 else (1e-4, 1e-6)
    with torch.no_grad():
        scalar = tda.odeint_rowwise(plain, y0, t, rtol=x_r, atol=x_a, method=method, return_stats=True)
        vector = tda.odeint_rowwise(plain, y0, t, rtol=torch.full((MIXED_B,), x_r, dtype=F64),
                                    atol=torch.full((MIXED_B,), x_a, dtype=F64, device=DEV), method=method, return_stats=True)
    _same(vector, scalar)


def test_hip_recorded_solve():
    """Forward bits of the plain solve; the y0 gradient of every row against the host path's within the bound
    tests/test_rowwise_grad_gpu.py::test_hip_gradient_matches_host_path_fp64 holds dopri5 to, device against host path:
    max|g - g_host| / max|g_host| < 1e-12 per row."""
    y0, t, rtol, atol, plain, _, _ = mixed_problem(F64, DEV)
    with torch.no_grad():
        ref = tda.odeint_rowwise(plain, y0, t.to(DEV), rtol=rtol, atol=atol, return_stats=True)
    y = y0.clone().requires_grad_(True)
    sol, stats = tda.odeint_rowwise(plain, y, t.to(DEV), rtol=rtol, atol=atol, return_stats=True, differentiable=True)
    assert sol.requires_grad
    _same((sol.detach(), stats), ref)
    gpu, = torch.autograd.grad(sol.pow(2).sum(), y)
    y0c, _, _, _, plain_c, _, _ = mixed_problem(F64, "cpu")
    yc = y0c.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        sol_c, stats_c = tda.odeint_rowwise(plain_c, yc, t, rtol=rtol, atol=atol, return_stats=True, differentiable=True)
    cpu, = torch.autograd.grad(sol_c.pow(2).sum(), yc)
    a, b = gpu.cpu(), cpu
    rel = (a - b).abs().amax(dim=1) / b.abs().amax(dim=1).clamp_min(1e-300)
    print("per row deviation from the host path: " + " ".join(f"{float(x):.1e}" for x in rel))
    print(f"trials per row: device {(stats['n_accepted'] + stats['n_rejected']).tolist()}, "
          f"host {(stats_c['n_accepted'] + stats_c['n_rejected']).tolist()}")
    for r in range(MIXED_B):
        assert float(rel[r]) < 1e-12, (r, float(rel[r]))


def test_hip_long_rows_take_the_chunk_kernel():
    """B = 3 rows of the first several-partials length (fp32): the chunk kernel's per-row tolerances inside a solve."""
    L = row_lengths(F32, LONG_NV)[0]
    B = 3
    y0, plain, _, subset = random_problem(B, L, F32, 5, DEV)
    t = torch.linspace(0, 1.0, 3, dtype=F64, device=DEV)
    rtol = torch.tensor([1e-2, 1e-5, 1e-3], dtype=F64)
    atol = rtol * 1e-2
    with torch.no_grad():
        sol, stats = tda.odeint_rowwise(plain, y0, t, rtol=rtol, atol=atol, return_stats=True)
        _, loose = tda.odeint_rowwise(plain, y0, t, rtol=1e-2, atol=1e-4, return_stats=True)
    trials = stats["n_accepted"] + stats["n_rejected"]
    trials_loose = loose["n_accepted"] + loose["n_rejected"]
    print(f"L = {L}: trials per row {trials.tolist()}, at the loosest pair {trials_loose.tolist()}")
    assert int((trials != trials_loose).sum()) >= 1
    _assert_rows_are_one_row_solves(sol, stats, y0, t, rtol, atol, subset, "dopri5")
