"""odeint_rowwise on the torch-op host path (CPU): per-row step control against the reference's per-row solves, batch
invariance, B = 1 against odeint, finished rows, per-row grids and input validation."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from _rowwise_cases import ATOL, GOLDEN, RTOL, Batched, cases

import torchdiffeq_amd as tda

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ["dopri5", "bosh3", "tsit5", "fehlberg2", "adaptive_heun", "dopri8"]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _golden():
    return np.load(os.path.join(HERE, "golden", GOLDEN))


@pytest.mark.parametrize("case", list(range(8)))
def test_matches_reference_rows(case):
    problem, method, kind, params, y0, t, expected, n_acc, n_rej = list(cases(_golden()))[case]
    func = Batched(problem, params)
    with torch.no_grad():
        sol, stats = tda.odeint_rowwise(func, torch.tensor(y0), torch.tensor(t), rtol=RTOL, atol=ATOL, method=method,
                                        return_stats=True)
    assert stats["n_accepted"].tolist() == n_acc.tolist()
    assert stats["n_rejected"].tolist() == n_rej.tolist()
    # Every stage sum here is formed left to right (the HIP kernels' order), the reference's by `torch.sum` over the
    # stacked stages: the rounding differs.  Short solves stay within 1e-12; rows that run hundreds to thousands of
    # steps at their stability limit (k_r ~ 1000, mu_r ~ 60) amplify it, but never beyond a tenth of rtol.
    for r in range(y0.shape[0]):
        bound = 1e-12 if n_acc[r] < 100 else 0.1 * RTOL
        assert _rel(sol[:, r], expected[:, r]) < bound, (problem, method, kind, r)
    assert max(n_acc) >= 10 * min(n_acc)


def _elementwise_problem(B, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-1, 2, B, dtype=torch.float64)[torch.randperm(B, generator=g)]
    y0 = torch.randn(B, 3, generator=g, dtype=torch.float64)
    w = torch.rand(B, 1, generator=g, dtype=torch.float64) * 4

    def make(idx):
        kk, ww = k[idx][:, None].to(dtype), w[idx].to(dtype)

        def f(t, y):
            return -kk * y + torch.sin(ww * t[:, None]) * torch.roll(y, 1, dims=1)
        return f
    return y0.to(dtype), make


def test_batch_invariance():
    y0, make = _elementwise_problem(64)
    t = torch.linspace(0, 2, 6, dtype=torch.float64)
    full = tda.odeint_rowwise(make(torch.arange(64)), y0, t, rtol=1e-6, atol=1e-8)
    for r in (0, 17, 63):
        alone = tda.odeint_rowwise(make(torch.tensor([r])), y0[r:r + 1], t, rtol=1e-6, atol=1e-8)
        assert torch.equal(alone[:, 0], full[:, r])
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5))[:37]
    part = tda.odeint_rowwise(make(perm), y0[perm], t, rtol=1e-6, atol=1e-8)
    assert torch.equal(part, full[:, perm])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("method", METHODS)
def test_single_row_matches_odeint(method, dtype):
    g = torch.Generator().manual_seed(1)
    A = (torch.randn(4, 4, generator=g, dtype=torch.float64) * 0.5).to(dtype)
    y0 = torch.randn(1, 4, generator=g, dtype=torch.float64).to(dtype)
    t = torch.linspace(0, 2, 5, dtype=dtype)
    rtol, atol = (1e-6, 1e-8) if dtype == torch.float64 else (1e-4, 1e-6)
    calls = [0]

    def f_rows(t_, y):
        calls[0] += 1
        return torch.sin(t_)[:, None] * (y @ A.T) - 0.3 * y

    def f_ode(t_, y):
        calls[0] += 1
        return torch.sin(t_) * (y @ A.T) - 0.3 * y

    sol, stats = tda.odeint_rowwise(f_rows, y0, t, rtol=rtol, atol=atol, method=method, return_stats=True)
    nfe_rows, calls[0] = calls[0], 0
    n_acc, n_rej = [0], [0]
    f_ode.callback_accept_step = lambda *a: n_acc.__setitem__(0, n_acc[0] + 1)
    f_ode.callback_reject_step = lambda *a: n_rej.__setitem__(0, n_rej[0] + 1)
    ref = tda.odeint(f_ode, y0, t, rtol=rtol, atol=atol, method=method)
    assert stats["nfe"] == nfe_rows == calls[0]
    assert stats["n_accepted"].tolist() == n_acc and stats["n_rejected"].tolist() == n_rej
    # (the stage sums are formed left to right here and by ATen's `torch.sum` on odeint's host path: the same steps, a
    #  rounding apart — except dopri8, whose first error estimate is below the rounding level of the state and thus a
    #  rounding-noise ratio: the step sizes then differ in their last digits from the second step on)
    if method == "dopri8":
        bound = 0.1 * rtol if dtype == torch.float64 else 10 * rtol
    else:
        bound = 1e-13 if dtype == torch.float64 else 1e-5
    assert _rel(sol, ref) < bound
    assert torch.equal(sol[0], y0)


def test_finished_rows_are_frozen_and_ignored():
    B = 8
    g = torch.Generator().manual_seed(2)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[:, None]
    y0 = torch.randn(B, 2, generator=g, dtype=torch.float64)
    tg = torch.linspace(0, 1, 5, dtype=torch.float64)[:, None] * torch.linspace(0.3, 1.0, B, dtype=torch.float64)
    last = [None]
    frozen_seen = [0]

    def f(t, y, poison):
        out = -k * y + torch.cos(t)[:, None]
        if last[0] is not None:
            same = t == last[0]
            frozen_seen[0] += int(same.sum())
            if poison:
                out[same] = float("nan")
        last[0] = t.clone()
        return out

    clean = tda.odeint_rowwise(lambda t, y: f(t, y, False), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    assert frozen_seen[0] > 0, "rows with shorter grids finish first and keep being evaluated"
    last[0] = None
    poisoned = tda.odeint_rowwise(lambda t, y: f(t, y, True), y0, tg, method="bosh3", rtol=1e-6, atol=1e-8)
    assert torch.equal(clean, poisoned)


def test_two_d_grid_equals_one_d_solves():
    y0, make = _elementwise_problem(6, seed=3)
    base = torch.linspace(0, 1, 7, dtype=torch.float64)
    tg = base[:, None] * torch.linspace(0.5, 3.0, 6, dtype=torch.float64) + 0.1 * torch.arange(6)
    sol = tda.odeint_rowwise(make(torch.arange(6)), y0, tg, rtol=1e-7, atol=1e-9, method="tsit5")
    for r in range(6):
        one = tda.odeint_rowwise(make(torch.tensor([r])), y0[r:r + 1], tg[:, r], rtol=1e-7, atol=1e-9, method="tsit5")
        assert torch.equal(one[:, 0], sol[:, r])


def test_decreasing_time_and_first_step():
    y0, make = _elementwise_problem(5, seed=4)
    t = torch.linspace(1, 0, 4, dtype=torch.float64)
    sol = tda.odeint_rowwise(make(torch.arange(5)), y0, t, rtol=1e-7, atol=1e-9)
    for r in range(5):
        f1 = make(torch.tensor([r]))
        ref = tda.odeint(lambda t_, y: f1(t_.reshape(1), y), y0[r:r + 1], t, rtol=1e-7, atol=1e-9)
        assert _rel(sol[:, r], ref[:, 0]) < 1e-12
    fs = torch.tensor([1e-3, 2e-3, 3e-3, 4e-3, 5e-3], dtype=torch.float64)
    solf = tda.odeint_rowwise(make(torch.arange(5)), y0, t, rtol=1e-7, atol=1e-9, options={"first_step": fs})
    one = tda.odeint_rowwise(make(torch.tensor([3])), y0[3:4], t, rtol=1e-7, atol=1e-9,
                             options={"first_step": float(fs[3])})
    assert torch.equal(one[:, 0], solf[:, 3])


def test_max_num_steps_names_the_row():
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=torch.float64)
    y0 = torch.ones(4, 1, dtype=torch.float64)
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(\d+>=50\) in row 2"):
        tda.odeint_rowwise(lambda t, y: -k * (y - torch.sin(t)[:, None]), y0, torch.tensor([0.0, 5.0]),
                           rtol=1e-5, atol=1e-7, options={"max_num_steps": 50})


def test_validation():
    f = lambda t, y: -y  # noqa: E731
    y0 = torch.ones(3, 2, dtype=torch.float64)
    t = torch.tensor([0.0, 1.0])
    with pytest.raises(ValueError, match="norm"):
        tda.odeint_rowwise(f, y0, t, options={"norm": lambda x: x})
    for opt in ("step_t", "jump_t", "grid_points", "hip_graph", "dtype"):
        with pytest.raises(ValueError, match=opt):
            tda.odeint_rowwise(f, y0, t, options={opt: None})
    with pytest.raises(ValueError, match="tuple"):
        tda.odeint_rowwise(f, (y0, y0), t)
    with pytest.raises(ValueError, match="vector"):
        tda.odeint_rowwise(f, y0, t, rtol=torch.ones(2))
    with pytest.raises(ValueError, match="bfloat16"):
        tda.odeint_rowwise(f, y0.bfloat16(), t)
    with pytest.raises(ValueError, match="complex"):
        tda.odeint_rowwise(f, y0.to(torch.complex128), t)
    with pytest.raises(ValueError, match="method"):
        tda.odeint_rowwise(f, y0, t, method="rk4")
    with pytest.raises(ValueError, match="event_fn"):
        tda.odeint_rowwise(f, y0, t, event_fn=lambda t, y: y.sum())
    with pytest.raises(ValueError, match="monotone"):
        tda.odeint_rowwise(f, y0, torch.tensor([0.0, 1.0, 0.5]))
    with pytest.raises(ValueError, match=r"\[T, B\]"):
        tda.odeint_rowwise(f, y0, torch.zeros(3, 2))
    with pytest.raises(NotImplementedError, match="odeint_adjoint"):
        tda.odeint_rowwise(f, y0.clone().requires_grad_(True), t)
    lin = torch.nn.Linear(2, 2).double()
    with pytest.raises(NotImplementedError, match="odeint_adjoint"):
        tda.odeint_rowwise(lambda t_, y: lin(y), y0, t)
    with torch.no_grad():
        out = tda.odeint_rowwise(lambda t_, y: lin(y), y0, t)
    assert out.shape == (2, 3, 2)


def test_host_path_warns_once_and_is_batch_invariant_sum():
    from torchdiffeq_amd.rowwise import _row_sum
    x = torch.rand(37, 1000, dtype=torch.float64)
    s = _row_sum(x)
    for r in (0, 5, 36):
        assert torch.equal(_row_sum(x[r:r + 1])[0], s[r])
    assert math.isclose(float(s[3]), float(x[3].sum()), rel_tol=1e-12)
