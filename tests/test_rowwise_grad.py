"""Gradients through `odeint_rowwise(..., differentiable=True)` on the torch-op host path (CPU): the reference's per-row
gradients, forward bits, batch invariance, B = 1 against `odeint`, shared parameters, accept / finish masks, refusals
and a finite-difference check.  The host path is the oracle of tests/test_rowwise_grad_gpu.py."""
import warnings

import numpy as np
import pytest
import torch

from _rowwise_grad_cases import (CASE_NAMES, METHODS, load, loss_weights, random_problem, row_bounds, row_deviation,
                                 solve_case)

import torchdiffeq_amd as tda


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _grads(func, y0, t, params=(), **kw):
    """(d loss / d y0, *d loss / d params, stats) of loss = sum(sol * W) for a recorded rowwise solve."""
    y0 = y0.detach().clone().requires_grad_(True)
    sol, stats = tda.odeint_rowwise(func, y0, t, return_stats=True, differentiable=True, **kw)
    loss = (sol * loss_weights(sol.shape, sol.dtype, sol.device)).sum()
    return (*torch.autograd.grad(loss, [y0, *params]), stats)


# -- 1. the reference's per-row gradients -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_rows(name):
    """Every row's gradient (y0 and parameter) against the reference solving that row alone: less than a tenth of the
    reference's own discretisation spread of the case, in the measure of the fixture maker; where that spread is
    vacuous (bosh3, fehlberg2: stiff rows at the stability limit) also less than the row's own bound
    (`_rowwise_grad_cases.row_bounds`)."""
    dev, spread, stats, counts = solve_case(tda, name)
    bounds = row_bounds(name)
    print(f"{name}: worst row deviation {float(dev.max()):.3e} (row {int(dev.argmax())}), case bound {0.1 * spread:.3e}")
    print("   per row deviation / bound: " + " ".join(f"{float(d):.1e}/{float(b):.1e}" for d, b in zip(dev, bounds)))
    if counts is not None:
        assert stats["n_accepted"].tolist() == counts[0]
        assert stats["n_rejected"].tolist() == counts[1]
    for r in range(len(dev)):
        assert float(dev[r]) < 0.1 * spread, (name, r, float(dev[r]), spread)
        assert float(dev[r]) < float(bounds[r]), (name, r, float(dev[r]), float(bounds[r]))


# -- 2. forward bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["t1d", "t2d"])
@pytest.mark.parametrize("method", METHODS)
def test_forward_bits(method, kind):
    y0, make = random_problem(7, 3, torch.float64, 11)
    t = torch.linspace(0, 1.5, 5, dtype=torch.float64)
    if kind == "t2d":
        t = t[:, None] * torch.linspace(0.4, 1.0, 7, dtype=torch.float64) + 0.05 * torch.arange(7)
    with torch.no_grad():
        plain, sp = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
    rec, sr = tda.odeint_rowwise(make("cpu"), y0.clone().requires_grad_(True), t, rtol=1e-6, atol=1e-8, method=method,
                                 return_stats=True, differentiable=True)
    assert rec.requires_grad
    assert torch.equal(rec, plain)
    assert sr["nfe"] == sp["nfe"]
    assert torch.equal(sr["n_accepted"], sp["n_accepted"]) and torch.equal(sr["n_rejected"], sp["n_rejected"])
    with torch.no_grad():       # under no_grad the argument has no effect
        off = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-6, atol=1e-8, method=method, differentiable=True)
    assert not off.requires_grad and torch.equal(off, plain)


# -- 3. batch invariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_gradient_batch_invariance(method):
    B = 24
    y0, make = random_problem(B, 3, torch.float64, 5)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    W = loss_weights((4, B, 3), torch.float64)

    def grad_of(idx):
        y = y0[idx].clone().requires_grad_(True)
        sol = tda.odeint_rowwise(make("cpu", idx), y, t, rtol=1e-6, atol=1e-8, method=method, differentiable=True)
        return torch.autograd.grad((sol * W[:, idx]).sum(), y)[0]
    full = grad_of(torch.arange(B))
    for r in (0, 9, B - 1):
        assert torch.equal(grad_of(torch.tensor([r]))[0], full[r])
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))[:11]
    assert torch.equal(grad_of(perm), full[perm])


# -- 4. B = 1 against odeint ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,case", [("dopri5", "decay_dopri5_t1d"), ("tsit5", "decay_tsit5_t1d")])
def test_single_row_matches_odeint(method, case):
    """One row of the `decay` problem, automatic first step (the initial-step graph and the time anchor of the later
    steps are exercised): `odeint` on the host path is the reference bit for bit, so the bound is that of
    test_reference_rows with the stored spread of the problem.  Measured: below 1e-12."""
    base, grad = load()
    spread = float(grad[case + "_spread"])
    worst = 0.0
    for r in (2, 7, 12):
        k0, y0 = float(base["decay_params"][r]), torch.tensor(base["decay_y0"][r:r + 1])
        t = torch.tensor(base["decay_t1d"])
        W = loss_weights((len(t), 1, 1), torch.float64)
        kr = torch.tensor([k0], dtype=torch.float64, requires_grad=True)
        yr = y0.clone().requires_grad_(True)
        sol = tda.odeint_rowwise(lambda t_, y: -kr[:, None] * (y - torch.sin(3.0 * t_[:, None])), yr, t, rtol=1e-6,
                                 atol=1e-8, method=method, differentiable=True)
        gy, gk = torch.autograd.grad((sol * W).sum(), [yr, kr])
        ko = torch.tensor([k0], dtype=torch.float64, requires_grad=True)
        yo = y0.clone().requires_grad_(True)
        ref = tda.odeint(lambda t_, y: -ko[:, None] * (y - torch.sin(3.0 * t_)), yo, t, rtol=1e-6, atol=1e-8,
                         method=method)
        ry, rk = torch.autograd.grad((ref * W).sum(), [yo, ko])
        worst = max(worst, float(row_deviation(gy, gk, ry, rk)[0]))
    print(f"B = 1 against odeint ({method}): worst deviation {worst:.3e}, bound {0.1 * spread:.3e}")
    assert worst < 0.1 * spread


# -- 5. shared parameters -------------------------------------------------------------------------------------------------
def test_shared_parameters_sum_over_rows():
    """An nn.Linear field: the weight's gradient from the whole batch is the sum of the single-row gradients.  64 fp64
    terms: the sum itself is good to 64 * 2^-53 ~ 7e-15 relative; the bound 1e-10 leaves room for the field's matmul
    rounding differently for 64 rows and for one."""
    B, D = 64, 4
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(D, D).double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(D, D, generator=g, dtype=torch.float64) * 0.5 - 0.3 * torch.eye(D))
    y0 = torch.randn(B, D, generator=g, dtype=torch.float64)
    t = torch.tensor([0.0, 0.4, 1.0], dtype=torch.float64)
    W = loss_weights((3, B, D), torch.float64)
    field = lambda t_, y: torch.tanh(lin(y)) * torch.cos(t_)[:, None]      # noqa: E731
    sol = tda.odeint_rowwise(field, y0, t, rtol=1e-6, atol=1e-8, differentiable=True)
    gw, gb = torch.autograd.grad((sol * W).sum(), [lin.weight, lin.bias])
    sw, sb = torch.zeros_like(gw), torch.zeros_like(gb)
    for r in range(B):
        one = tda.odeint_rowwise(field, y0[r:r + 1], t, rtol=1e-6, atol=1e-8, differentiable=True)
        a, b = torch.autograd.grad((one * W[:, r:r + 1]).sum(), [lin.weight, lin.bias])
        sw, sb = sw + a, sb + b
    rel = max(float((gw - sw).abs().max() / sw.abs().max()), float((gb - sb).abs().max() / sb.abs().max()))
    print(f"shared parameters: relative difference to the sum of single-row gradients {rel:.3e}")
    assert rel < 1e-10


# -- 6. masks -------------------------------------------------------------------------------------------------------------
def test_finished_and_rejected_rows():
    """Rows with shorter grids finish early, some trial steps are rejected for some rows only: every gradient is finite
    and equals the row's single-row solve bit for bit (a finished or rejected row sends zeros into func's backward)."""
    B = 10
    y0, make = random_problem(B, 2, torch.float64, 21)
    tg = torch.linspace(0, 1, 5, dtype=torch.float64)[:, None] ** 1.5 * torch.linspace(0.3, 3.0, B, dtype=torch.float64)
    W = loss_weights((5, B, 2), torch.float64)
    y = y0.clone().requires_grad_(True)
    sol, stats = tda.odeint_rowwise(make("cpu"), y, tg, rtol=1e-5, atol=1e-7, method="bosh3", return_stats=True,
                                    differentiable=True)
    n_rej = stats["n_rejected"]
    assert int((n_rej > 0).sum()) > 0 and int((n_rej == 0).sum()) > 0, n_rej.tolist()
    assert int(stats["n_accepted"].max()) > 2 * int(stats["n_accepted"].min())
    full = torch.autograd.grad((sol * W).sum(), y)[0]
    assert torch.isfinite(full).all()
    for r in range(B):
        idx = torch.tensor([r])
        yr = y0[idx].clone().requires_grad_(True)
        one = tda.odeint_rowwise(make("cpu", idx), yr, tg[:, r], rtol=1e-5, atol=1e-7, method="bosh3",
                                 differentiable=True)
        assert torch.equal(torch.autograd.grad((one * W[:, idx]).sum(), yr)[0][0], full[r]), r


# -- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    f = lambda t, y: -y  # noqa: E731
    y0 = torch.ones(3, 2, dtype=torch.float64)
    t = torch.tensor([0.0, 1.0])
    # the default is unchanged: no gradients without the argument
    with pytest.raises(NotImplementedError, match="odeint_adjoint"):
        tda.odeint_rowwise(f, y0.clone().requires_grad_(True), t)
    lin = torch.nn.Linear(2, 2).double()
    with pytest.raises(NotImplementedError, match="odeint_adjoint"):
        tda.odeint_rowwise(lambda t_, y: lin(y), y0, t)
    # time gradients
    with pytest.raises(NotImplementedError, match="time gradients"):
        tda.odeint_rowwise(f, y0.clone().requires_grad_(True), t.clone().requires_grad_(True), differentiable=True)
    # second order: the recorded backward raises instead of returning something wrong
    y = y0.clone().requires_grad_(True)
    sol = tda.odeint_rowwise(lambda t_, yy: -yy * yy, y, t, differentiable=True)
    with pytest.raises(NotImplementedError, match="second-order"):
        torch.autograd.grad(sol.pow(2).sum(), y, create_graph=True)
    # everything odeint_rowwise refuses today, with the argument set
    yg = y0.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="norm"):
        tda.odeint_rowwise(f, yg, t, options={"norm": lambda x: x}, differentiable=True)
    for opt in ("step_t", "jump_t", "grid_points", "hip_graph", "dtype"):
        with pytest.raises(ValueError, match=opt):
            tda.odeint_rowwise(f, yg, t, options={opt: None}, differentiable=True)
    with pytest.raises(ValueError, match="tuple"):
        tda.odeint_rowwise(f, (yg, yg), t, differentiable=True)
    with pytest.raises(ValueError, match="vector"):
        tda.odeint_rowwise(f, yg, t, rtol=torch.ones(2), differentiable=True)
    with pytest.raises(ValueError, match="bfloat16"):
        tda.odeint_rowwise(f, y0.bfloat16().requires_grad_(True), t, differentiable=True)
    with pytest.raises(ValueError, match="complex"):
        tda.odeint_rowwise(f, y0.to(torch.complex128).requires_grad_(True), t, differentiable=True)
    with pytest.raises(ValueError, match="method"):
        tda.odeint_rowwise(f, yg, t, method="rk4", differentiable=True)
    with pytest.raises(ValueError, match="event_fn"):
        tda.odeint_rowwise(f, yg, t, event_fn=lambda t_, y_: y_.sum(), differentiable=True)
    with pytest.raises(ValueError, match="monotone"):
        tda.odeint_rowwise(f, yg, torch.tensor([0.0, 1.0, 0.5]), differentiable=True)

    class WithCallback(torch.nn.Module):
        def forward(self, t_, y_):
            return -y_

        def callback_step(self, *a):
            pass
    with pytest.raises(ValueError, match="callback_step"):
        tda.odeint_rowwise(WithCallback(), yg, t, differentiable=True)


# -- 8. finite differences ------------------------------------------------------------------------------------------------
def test_finite_differences():
    """Central differences on a tiny fp64 problem whose step sequence cannot move: `first_step` = 1e-3 is given, and the
    tolerances (rtol = atol = 0.1) are so loose that every error ratio stays below (safety / ifactor)^5 = 5.9e-6, where
    the controller's factor saturates at `ifactor`: each row steps 1e-3, 1e-2, 1e-1, 1 whatever the state, so the solve
    is a smooth function of (y0, k).  Perturbation eps = 1e-5: the third-derivative term eps^2 f''' / 6 ~ 1e-10 relative,
    rounding 2^-53 / eps ~ 1e-11; bound 1e-7."""
    B, L = 3, 2
    g = torch.Generator().manual_seed(2)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64)
    k0 = torch.tensor([0.3, 0.8, 1.3], dtype=torch.float64)
    t = torch.tensor([0.0, 0.3, 0.6], dtype=torch.float64)
    W = loss_weights((3, B, L), torch.float64)
    kw = dict(rtol=0.1, atol=0.1, options={"first_step": 1e-3}, return_stats=True)

    def loss_of(y, k, **extra):
        sol, st = tda.odeint_rowwise(lambda t_, yy: -k[:, None] * yy + torch.sin(t_)[:, None] * torch.roll(yy, 1, 1) ** 2,
                                     y, t, **kw, **extra)
        assert st["n_accepted"].tolist() == [4] * B and st["n_rejected"].tolist() == [0] * B
        return (sol * W).sum()
    y, k = y0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    gy, gk = torch.autograd.grad(loss_of(y, k, differentiable=True), [y, k])
    eps = 1e-5
    with torch.no_grad():
        for r in range(B):
            for c in range(L):
                d = torch.zeros_like(y0)
                d[r, c] = eps
                fd = float(loss_of(y0 + d, k0) - loss_of(y0 - d, k0)) / (2 * eps)
                assert abs(fd - float(gy[r, c])) < 1e-7 * max(1.0, float(gy.abs().max())), (r, c, fd, float(gy[r, c]))
            d = torch.zeros_like(k0)
            d[r] = eps
            fd = float(loss_of(y0, k0 + d) - loss_of(y0, k0 - d)) / (2 * eps)
            assert abs(fd - float(gk[r])) < 1e-7 * max(1.0, float(gk.abs().max())), (r, fd, float(gk[r]))


def test_float32_and_decreasing_time():
    """fp32 states, decreasing time and a per-row first step are recorded as well (values equal the plain solve)."""
    y0, make = random_problem(5, 4, torch.float32, 9)
    t = torch.linspace(1, 0, 4, dtype=torch.float32)
    fs = torch.tensor([1e-3, 2e-3, 3e-3, 4e-3, 5e-3], dtype=torch.float64)
    for opts in (None, {"first_step": fs}):
        with torch.no_grad():
            plain = tda.odeint_rowwise(make("cpu"), y0, t, rtol=1e-4, atol=1e-6, options=opts)
        gy, stats = _grads(make("cpu"), y0, t, rtol=1e-4, atol=1e-6, options=opts)
        assert gy.dtype == torch.float32 and torch.isfinite(gy).all() and float(gy.abs().max()) > 0
        rec = tda.odeint_rowwise(make("cpu"), y0.clone().requires_grad_(True), t, rtol=1e-4, atol=1e-6, options=opts,
                                 differentiable=True)
        assert torch.equal(rec, plain)
    # a single output time: the solution is y0 itself, with its graph
    y = y0.clone().requires_grad_(True)
    one = tda.odeint_rowwise(make("cpu"), y, t[:1], differentiable=True)
    assert torch.equal(torch.autograd.grad(one.sum(), y)[0], torch.ones_like(y0))
    assert np.isfinite(float(one.sum()))
