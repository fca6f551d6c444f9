"""odeint_rowwise on the HIP kernels (csrc/tdeq_kernels_rowwise.hpp): fixtures, the host path as the comparison,
batch invariance on the device, row shapes from L = 1 to the long-row reduction, decreasing time, per-row first
steps and the per-row max_num_steps error."""
import os
import warnings

import numpy as np
import pytest
import torch

from _rowwise_cases import ATOL, GOLDEN, RTOL, Batched, cases

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _rel(a, b):
    a = torch.as_tensor(a).to("cpu", torch.float64)
    b = torch.as_tensor(b).to("cpu", torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", list(range(8)))
def test_hip_matches_reference_rows(case):
    golden = np.load(os.path.join(HERE, "golden", GOLDEN))
    problem, method, kind, params, y0, t, expected, n_acc, n_rej = list(cases(golden))[case]
    func = Batched(problem, params, device=DEV)
    sol, stats = tda.odeint_rowwise(func, torch.tensor(y0, device=DEV), torch.tensor(t, device=DEV), rtol=RTOL,
                                    atol=ATOL, method=method, return_stats=True)
    assert stats["n_accepted"].tolist() == n_acc.tolist()
    assert stats["n_rejected"].tolist() == n_rej.tolist()
    for r in range(y0.shape[0]):
        # (the bound of tests/test_rowwise.py: left-to-right stage sums against the reference's torch.sum)
        bound = 1e-12 if n_acc[r] < 100 else 0.1 * RTOL
        assert _rel(sol[:, r], expected[:, r]) < bound, (problem, method, kind, r)


def _random_problem(B, L, dtype, seed):
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


@pytest.mark.parametrize("method", ["dopri5", "tsit5", "bosh3", "fehlberg2", "adaptive_heun", "dopri8"])
def test_hip_matches_host_path_fp64(method):
    y0, make = _random_problem(96, 5, torch.float64, 1)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    cpu, sc = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
    gpu, sg = tda.odeint_rowwise(make(DEV), y0.to(DEV), t.to(DEV), rtol=1e-6, atol=1e-8, method=method,
                                 return_stats=True)
    assert sg["n_accepted"].tolist() == sc["n_accepted"].tolist()
    assert sg["n_rejected"].tolist() == sc["n_rejected"].tolist()
    assert sg["nfe"] == sc["nfe"]
    bound = 1e-7 if method == "dopri8" else 1e-12
    for r in range(96):
        assert _rel(gpu[:, r], cpu[:, r]) < bound, r


def test_hip_matches_host_path_fp32():
    y0, make = _random_problem(200, 8, torch.float32, 2)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float32)
    cpu, sc = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-4, atol=1e-6, return_stats=True)
    gpu, sg = tda.odeint_rowwise(make(DEV), y0.to(DEV), t.to(DEV), rtol=1e-4, atol=1e-6, return_stats=True)
    differ = (sg["n_accepted"] != sc["n_accepted"]) | (sg["n_rejected"] != sc["n_rejected"])
    assert int(differ.sum()) <= 2          # at most 1 % of the rows
    for r in range(200):
        if not differ[r]:
            assert _rel(gpu[:, r], cpu[:, r]) < 1e-5, r


@pytest.mark.parametrize("B", [1, 37, 4096])
def test_hip_batch_invariance(B):
    y0, make = _random_problem(4096, 6, torch.float64, 3)
    t = torch.linspace(0, 1, 3, dtype=torch.float64, device=DEV)
    full = tda.odeint_rowwise(make(DEV), y0.to(DEV), t, rtol=1e-6, atol=1e-8)
    idx = torch.randperm(4096, generator=torch.Generator().manual_seed(B))[:B]
    part = tda.odeint_rowwise(make(DEV, idx), y0[idx].to(DEV), t, rtol=1e-6, atol=1e-8)
    assert torch.equal(part, full[:, idx.to(DEV)])


@pytest.mark.parametrize("B,L", [(65536, 1), (64, 3), (64, 128), (64, 129), (2, 1 << 20), (1, 1 << 22),
                                 (64, 1500), (64, 4100), (16, 8192), (64, 4096), (16, 8196)])
def test_hip_shapes(B, L):
    """Every row reduction shape: several rows per wave (L = 1, 3), a group of lanes per row (128, 129: 16-byte and
    scalar elements), chunked long rows (2^20, 2^22), long rows of ONE chunk (1500 scalar, 4100 and 8192 16-byte
    elements) with the last short length (4096) and the first two-chunk one (8196) on either side — checked against
    the same rows solved alone (batch invariance) and against the host path on a few rows."""
    g = torch.Generator().manual_seed(L)
    k = torch.logspace(-1, 1, B, dtype=torch.float64)[:, None]
    y0 = torch.randn(B, L, generator=g, dtype=torch.float32)

    def make(kk):
        kk = kk.to(torch.float32)
        return lambda t, y: -kk * y + (1 - t * t)[:, None]      # (no transcendental: the same func bits on both sides)
    t = torch.tensor([0.0, 0.5, 1.0])
    sol, st = tda.odeint_rowwise(make(k.to(DEV)), y0.to(DEV), t.to(DEV), rtol=1e-5, atol=1e-7, return_stats=True)
    assert torch.isfinite(sol).all()
    for r in sorted({0, B - 1}):
        one = tda.odeint_rowwise(make(k[r:r + 1].to(DEV)), y0[r:r + 1].to(DEV), t.to(DEV), rtol=1e-5, atol=1e-7)
        assert torch.equal(one[:, 0], sol[:, r])
        if L <= 1 << 20:
            cpu, sc = tda.odeint_rowwise(make(k[r:r + 1]), y0[r:r + 1], t, rtol=1e-5, atol=1e-7, return_stats=True)
            # (fp32: the fp64 row sums of the two paths differ in their order, so a ratio near 1 may decide differently
            #  — then the solutions differ by the local error, a fraction of rtol)
            same = int(sc["n_accepted"][0]) == int(st["n_accepted"][r]) and \
                int(sc["n_rejected"][0]) == int(st["n_rejected"][r])
            assert _rel(sol[:, r], cpu[:, 0]) < (1e-5 if same else 1e-4), same
            assert abs(int(sc["n_accepted"][0]) - int(st["n_accepted"][r])) <= 1


def test_hip_decreasing_time_first_step_and_max_steps():
    y0, make = _random_problem(5, 4, torch.float64, 4)
    t = torch.linspace(1, 0, 4, dtype=torch.float64)
    fs = torch.tensor([1e-3, 2e-3, 3e-3, 4e-3, 5e-3], dtype=torch.float64)
    for opts in (None, {"first_step": fs}):
        cpu = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-7, atol=1e-9, options=opts)
        gpu = tda.odeint_rowwise(make(DEV), y0.to(DEV), t.to(DEV), rtol=1e-7, atol=1e-9,
                                 options=None if opts is None else {"first_step": fs.to(DEV)})
        assert _rel(gpu, cpu) < 1e-12
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=torch.float64, device=DEV)
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(\d+>=50\) in row 2"):
        tda.odeint_rowwise(lambda t_, y: -k * (y - torch.sin(t_)[:, None]), torch.ones(4, 1, dtype=torch.float64,
                           device=DEV), torch.tensor([0.0, 5.0], device=DEV), rtol=1e-5, atol=1e-7,
                           options={"max_num_steps": 50})


def test_hip_finished_rows_ignore_nan():
    B = 8
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64, device=DEV)[:, None]
    y0 = torch.randn(B, 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(DEV)
    tg = (torch.linspace(0, 1, 5, dtype=torch.float64)[:, None] * torch.linspace(0.3, 1.0, B, dtype=torch.float64)).to(DEV)
    last = [None]

    def f(t, y, poison):
        out = -k * y + torch.cos(t)[:, None]
        if poison and last[0] is not None:
            out[t == last[0]] = float("nan")
        last[0] = t.clone()
        return out
    clean = tda.odeint_rowwise(lambda t, y: f(t, y, False), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    last[0] = None
    poisoned = tda.odeint_rowwise(lambda t, y: f(t, y, True), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    assert torch.equal(clean, poisoned)
