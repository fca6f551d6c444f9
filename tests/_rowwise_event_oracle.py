"""Shared pieces of the `odeint_rowwise_event` tests: the CPU row oracle extended by the three event operations, stated
in torch (the quartic's expressions are those of `HostRowKernels._dense_commit`), the device driver on it, and the
problems."""
import contextlib

import pytest
import torch

from _rowwise_tol_oracle import TolOracle, quiet, random_problem  # noqa: F401

from torchdiffeq_amd import _native, rowwise

METHODS = ["dopri5", "tsit5", "bosh3", "fehlberg2", "adaptive_heun", "dopri8"]


def event_sign(g):
    return (g > 0).to(torch.int32) - (g < 0).to(torch.int32)


class EventOracle(TolOracle):
    """The tolerance oracle plus `row_event_detect`, `row_event_fit` and `row_event_eval`."""

    def row_event_detect(self, g1, sign0, ctrl, st, dts, times, fired, fired_now, lo, hi) -> None:
        v = {name: torch.from_numpy(a) for name, a in self._inner._state_views(st).items()}      # views, written in place
        n = int(st.n_rows)
        assert g1.shape == sign0.shape == fired.shape == fired_now.shape == lo.shape == hi.shape == dts.shape == (n,)
        now = (v["accepted"] != 0) & (fired == 0) & (event_sign(g1) != sign0)
        fired_now.copy_(now.to(torch.int32))
        fired[now] = 1
        lo[now] = v["tprev"][now]
        hi[now] = v["t0"][now]
        leave = now & (v["active"] != 0)
        v["active"][leave] = 0
        v["status"][0] -= int(leave.sum())
        dts[leave] = 0                                       # frozen as a finished row is: no step, every stage time t0
        frozen = torch.tensor(ctrl.time_sign, dtype=dts.dtype) * v["t0"].to(dts.dtype)
        tt = times.view(-1, n)
        for i in range(int(ctrl.n_times)):
            tt[i][leave] = frozen[leave]

    @staticmethod
    def row_event_fit(q, fired_now, y0, y1, f0, f1, ks, coefs, dts) -> None:
        idx = torch.nonzero(fired_now).view(-1)
        if idx.numel() == 0:
            return
        d = dts[idx][:, None]
        y0r, y1r, f0r, f1r = y0[idx], y1[idx], f0[idx], f1[idx]
        acc = None
        for k, c in zip(ks, coefs):
            term = k[idx] * (torch.tensor(c, dtype=y0.dtype) * d)
            acc = term if acc is None else acc + term
        ymid = y0r + acc
        two_dt = torch.tensor(2.0, dtype=y0.dtype) * d
        qa = ((f1r - f0r) * two_dt - (y1r + y0r) * 8.0) + ymid * 16.0
        qb = (((f0r * 5.0 - f1r * 3.0) * d + y0r * 18.0) + y1r * 14.0) - ymid * 32.0
        qc = (((f1r - f0r * 4.0) * d - y0r * 11.0) - y1r * 5.0) + ymid * 16.0
        qd = f0r * d
        q[:, idx] = torch.stack([y0r, qd, qc, qb, qa])

    @staticmethod
    def row_event_eval(out, q, x, mask) -> None:
        idx = torch.nonzero(mask).view(-1)
        if idx.numel() == 0:
            return
        e, d, c, b, a = q[:, idx].unbind(0)
        x1 = x[idx][:, None]
        x2 = x1 * x1
        x3 = x2 * x1
        x4 = x3 * x1
        total = e + d * x1
        total = total + c * x2
        total = total + b * x3
        total = total + a * x4
        out[idx] = total


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_tol_oracle.py's fixture with the extended oracle: inside `with device_driver():` a CPU state is
    solved by `HipRowKernels` on the oracle's row operations."""
    wrapped = EventOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def threshold_event(c):
    """event_fn of the crossing y[:, 0] = c_r (c: [B] tensor in the state's dtype on its device)."""
    return lambda t, y: y[:, 0] - c


def decay_event_problem(B, L, dtype, seed, device="cpu"):
    """Rows y' = -k_r (1 + t) y with k_r from 1 to 30 and y0 in (1, 2): elementwise, no transcendental (the same func bits
    on every backend), and the event y[:, 0] = q_r y0[:, 0] with q_r from 0.9 to 0.2 in an order unrelated to k, so that
    the rows fire at different times after different numbers of steps.  Every row reaches it (at k (t + t^2 / 2) =
    -ln q) with |dg/dt| = k (1 + t) q y0 >= 0.2.  -> (y0, func, event_fn, k)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(0, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None]
    q = torch.linspace(0.9, 0.2, B, dtype=torch.float64)[torch.randperm(B, generator=g)]
    y0 = 1 + torch.rand(B, L, generator=g, dtype=torch.float64)
    k, y0 = k.to(device, dtype), y0.to(device, dtype)
    level = (y0[:, 0] * q.to(device, dtype)).clone()
    return y0, (lambda t, y: -k * y * (1 + t)[:, None]), threshold_event(level), k
