"""`odeint_rowwise_event` on the HIP kernels against the host path, compared the way tests/test_rowwise_gpu.py compares
plain rowwise solves: equal counts and a rounding-level bound in fp64; in fp32 at most 1 % of the rows may take other
steps, the others agree to 1e-5.  func and event_fn are elementwise without transcendentals (the same bits on both
sides), every row reaches its event with |dg/dt| >= 0.2 (`decay_event_problem`).

The bound on the event time: each side's bisection ends within atol / 2 of the root of its own interpolant, and two
interpolants S apart cross the threshold S / |dg/dt| apart — |event_t - host| <= atol + S / |dg/dt| with S the bound on
the states (rel * max|y|); the state at the event may differ by S plus the trajectory's speed times that."""
import warnings

import pytest
import torch

from _rowwise_event_oracle import METHODS, decay_event_problem

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _tols(method, dtype):
    rtol, atol = (1e-6, 1e-8) if dtype == F64 else (1e-4, 1e-6)
    # (the order-2 pairs take hundreds of launch-bound steps per row at the tight pair; at rtol = 1e-2 their steps are
    #  bound by stability on the stiff rows, where fehlberg2's estimate lets an unstable step pass)
    loosen = 100 if dtype == F64 else 10
    return (rtol * loosen, atol * loosen) if method in ("adaptive_heun", "fehlberg2") else (rtol, atol)


def _both(B, L, dtype, seed, **kw):
    """((event_t, solution, stats) on the host path, the same on the device, the speed |f| [B, L] at the host's events)."""
    out = []
    for device in ("cpu", DEV):
        y0, func, event_fn, k = decay_event_problem(B, L, dtype, seed, device)
        with torch.no_grad():
            out.append(tda.odeint_rowwise_event(func, y0, 0.0, event_fn=event_fn, return_stats=True, **kw))
        if device == "cpu":
            speed = func(out[0][0].to(dtype), out[0][1][1]).abs().double()
    return out[0], out[1], speed


def _compare(host, dev, speed, atol, rel, same_rows=None):
    (th, sh, xh), (td, sd, xd) = host, dev
    assert td.device.type == "cuda" and sd.device.type == "cuda" and td.dtype == F64
    td, sd = td.cpu(), sd.cpu()
    rows = torch.ones(th.shape[0], dtype=torch.bool) if same_rows is None else same_rows
    assert torch.equal(xd["fired"][rows], xh["fired"][rows])
    fired = xh["fired"]
    S = rel * float(sh.abs().max())
    atol = torch.as_tensor(atol, dtype=F64).expand(th.shape[0])
    slope = speed[:, 0]
    assert float(slope[fired].min()) >= 0.2 * 0.99
    bound = torch.where(fired, atol + S / slope, torch.zeros_like(slope))      # an unfired row: t_end exactly
    diff = (td - th).abs()
    print(f"max |event_t - host| {float(diff[rows].max()):.3e} (bound {float(bound[rows].max()):.3e}); "
          f"max |y - host| {float((sd - sh).abs().max()):.3e}")
    assert bool((diff <= bound)[rows].all())
    dy = (sd[1].double() - sh[1].double()).abs().max(dim=1).values
    assert bool((dy <= S + speed.max(dim=1).values * bound)[rows].all())
    assert torch.equal(sd[0], sh[0])


@pytest.mark.parametrize("B,L", [(12, 5), (96, 24)])
@pytest.mark.parametrize("method", METHODS)
def test_hip_matches_host_path_fp64(method, B, L):
    rtol, atol = _tols(method, F64)
    host, dev, speed = _both(B, L, F64, 1, rtol=rtol, atol=atol, method=method)
    xh, xd = host[2], dev[2]
    assert bool(xh["fired"].all()) and len(set((xh["n_accepted"] + xh["n_rejected"]).tolist())) >= 3
    for name in ("n_accepted", "n_rejected"):
        assert xd[name].tolist() == xh[name].tolist(), name
    assert xd["nfe"] == xh["nfe"] and xd["n_event_evals"] == xh["n_event_evals"]
    _compare(host, dev, speed, atol, 1e-7 if method == "dopri8" else 1e-12)


@pytest.mark.parametrize("B,L", [(12, 5), (96, 24)])
@pytest.mark.parametrize("method", METHODS)
def test_hip_matches_host_path_fp32(method, B, L):
    rtol, atol = _tols(method, F32)
    host, dev, speed = _both(B, L, F32, 2, rtol=rtol, atol=atol, method=method)
    xh, xd = host[2], dev[2]
    assert bool(xh["fired"].all())
    differ = (xd["n_accepted"] != xh["n_accepted"]) | (xd["n_rejected"] != xh["n_rejected"])
    print(f"{method} {B} x {L}: rows whose counts differ {int(differ.sum())}")
    assert int(differ.sum()) <= B // 100                     # at most 1 % of the rows
    _compare(host, dev, speed, atol, 1e-5, same_rows=~differ)


def test_hip_row_tolerances():
    """[B] tolerance vectors: the device against the host path, and row r on the device against its one-row device solve
    with the two scalars (bit for bit)."""
    B, L = 12, 5
    g = torch.Generator().manual_seed(11)
    rtol = torch.logspace(-4, -8, B, dtype=F64)[torch.randperm(B, generator=g)]
    atol = rtol * 1e-2
    host, dev, speed = _both(B, L, F64, 3, rtol=rtol, atol=atol)
    for name in ("n_accepted", "n_rejected"):
        assert dev[2][name].tolist() == host[2][name].tolist(), name
    _compare(host, dev, speed, atol, 1e-12)
    y0, func, event_fn, k = decay_event_problem(B, L, F64, 3, DEV)
    level = y0[:, 0] - event_fn(None, y0)                    # the thresholds
    for r in (0, 5, 11):
        kr = k[r:r + 1]
        with torch.no_grad():
            t1, s1, x1 = tda.odeint_rowwise_event(lambda t, y: -kr * y * (1 + t)[:, None], y0[r:r + 1], 0.0,
                                                  event_fn=lambda t, y: y[:, 0] - level[r:r + 1], rtol=float(rtol[r]),
                                                  atol=float(atol[r]), return_stats=True)
        assert torch.equal(t1[0], dev[0][r]) and torch.equal(s1[:, 0], dev[1][:, r])
        assert int(x1["n_accepted"][0]) == int(dev[2]["n_accepted"][r])


def test_hip_decreasing_time_and_rows_fired_at_t0():
    """Decreasing time on the kernels, with two rows whose event value is zero at t0: they start inactive
    (`deactivate_rows` before the initial-step launches), take no step and keep y0; the others run the mirror image of
    `decay_event_problem` (y' = k (1 - t) y from 0 towards t_end = -3) to the same thresholds."""
    B, L = 12, 5
    at_t0 = torch.zeros(B, dtype=torch.bool)
    at_t0[[2, 9]] = True
    out = []
    for device in ("cpu", DEV):
        y0, _, _, k = decay_event_problem(B, L, F64, 5, device)
        q = torch.linspace(0.9, 0.2, B, dtype=F64)[torch.randperm(B, generator=torch.Generator().manual_seed(6))]
        q[at_t0] = 1.0
        level = (y0[:, 0] * q.to(device)).clone()
        func = lambda t, y, k=k: k * y * (1 - t)[:, None]                      # noqa: E731
        with torch.no_grad():
            out.append(tda.odeint_rowwise_event(func, y0, 0.0, event_fn=lambda t, y, c=level: y[:, 0] - c, t_end=-3.0,
                                                rtol=1e-6, atol=1e-8, return_stats=True))
        if device == "cpu":
            speed = func(out[0][0], out[0][1][1]).abs()
    host, dev = out
    for name in ("n_accepted", "n_rejected", "fired"):
        assert dev[2][name].tolist() == host[2][name].tolist(), name
    assert dev[2]["nfe"] == host[2]["nfe"] and dev[2]["n_event_evals"] == host[2]["n_event_evals"]
    assert bool(host[2]["fired"].all())
    event_t, sol = dev[0].cpu(), dev[1].cpu()
    assert bool((event_t[at_t0] == 0.0).all()) and torch.equal(sol[1][at_t0], sol[0][at_t0])
    assert (dev[2]["n_accepted"] + dev[2]["n_rejected"])[at_t0].tolist() == [0, 0]
    assert bool((event_t[~at_t0] < 0.0).all()) and bool((event_t > -3.0).all())
    assert int((dev[2]["n_accepted"])[~at_t0].min()) >= 2
    _compare(host, dev, speed, 1e-8, 1e-12)


def test_hip_t_end():
    """A t_end that stops more than half of the rows before their event."""
    B, L = 96, 24
    host, dev, speed = _both(B, L, F64, 4, rtol=1e-6, atol=1e-8, t_end=0.12)
    fired = host[2]["fired"]
    assert B // 4 <= int(fired.sum()) <= 3 * B // 4
    for name in ("n_accepted", "n_rejected", "fired"):
        assert dev[2][name].tolist() == host[2][name].tolist(), name
    assert bool((dev[0].cpu()[~fired] == 0.12).all())
    # an unfired row holds y(t_end): the plain rowwise solve's bound
    S = 1e-12 * float(host[1].abs().max())
    assert float((dev[1][1].cpu() - host[1][1])[~fired].abs().max()) <= S
    speed = torch.where(fired[:, None], speed, torch.ones_like(speed))      # (the slope is only used for rows that fired)
    _compare(host, dev, speed, 1e-8, 1e-12)
