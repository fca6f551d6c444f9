"""Shared pieces of the `odeint_rowwise(compact=...)` tests: the CPU row oracle extended by the two entry points of the
compaction, the device driver on it, the problems, and a simulator of the repack schedule written from the policy's text
(never imported from the package):

    after every poll — the one after the initial step included — with `cur` rows carried and `n_active` of them still
    active: 0 < n_active < cur and n_active <= c * cur repacks the batch to the active rows.
"""
import contextlib
import warnings

import pytest
import torch

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native, rowwise

METHODS = ["dopri5", "tsit5", "bosh3", "fehlberg2", "dopri8", "adaptive_heun"]
STAGES = {"dopri5": 6, "tsit5": 6, "bosh3": 3, "fehlberg2": 2, "dopri8": 13, "adaptive_heun": 1}    # func calls per trial step


class CompactOracle:
    """The `oracle_kernels` fixture's object plus `row_gather` and `row_dense_commit_mapped`, both stated through what the
    oracle already has."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    @staticmethod
    def row_gather(outs, srcs, idx) -> None:
        for out, src in zip(outs, srcs):
            torch.index_select(src, 0, idx.to(torch.int64), out=out)

    def row_dense_commit_mapped(self, sol, row_map, y0, y1, f0, f1, ks, coefs, dts, st) -> None:
        rows = row_map.to(torch.int64)
        tmp = sol[:, rows].contiguous()
        self._inner.row_dense_commit(tmp, y0, y1, f0, f1, ks, coefs, dts, st)
        sol[:, rows] = tmp


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/test_rowwise_oracle.py's fixture with the extended oracle: inside `with device_driver():` a CPU state is
    solved by `HipRowKernels` on the oracle's row operations."""
    wrapped = CompactOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


@pytest.fixture(autouse=True)
def quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


# -- the schedule ------------------------------------------------------------------------------------------------------------
def simulate(trials, c):
    """trials[r] = n_accepted[r] + n_rejected[r] of the plain solve -> ([cur_i]: the rows carried in trial step i, the
    number of repacks).  After i trial steps (i = 0: after the initial step) the active rows are those with
    trials[r] > i; that poll decides how many rows trial step i + 1 carries."""
    trials = [int(x) for x in trials]
    cur, carried, repacks = len(trials), [], 0
    for i in range(max(trials)):
        n_active = sum(1 for x in trials if x > i)          # the poll before trial step i
        if 0 < n_active < cur and n_active <= c * cur:
            cur = n_active
            repacks += 1
        carried.append(cur)
    return carried, repacks


def expected_row_evals(trials, c, method, first_step_given=False):
    """B * (1 + probe) + S * sum_i cur_i, and the number of repacks."""
    carried, repacks = simulate(trials, c)
    probe = 0 if first_step_given else 1
    return len(trials) * (1 + probe) + STAGES[method] * sum(carried), repacks


def assert_same_solve(plain, compact, c, method, first_step_given=False):
    """`plain`, `compact`: (solution, stats) of the same problem without and with `compact=c` on the same backend."""
    (sol_p, st_p), (sol_c, st_c) = plain, compact
    assert torch.equal(sol_c, sol_p)
    assert torch.equal(st_c["n_accepted"], st_p["n_accepted"])
    assert torch.equal(st_c["n_rejected"], st_p["n_rejected"])
    assert st_c["nfe"] == st_p["nfe"]
    assert "row_evals" not in st_p and "n_repacks" not in st_p
    trials = (st_p["n_accepted"] + st_p["n_rejected"]).tolist()
    evals, repacks = expected_row_evals(trials, c, method, first_step_given)
    assert st_c["row_evals"] == evals, (st_c["row_evals"], evals)
    assert st_c["n_repacks"] == repacks, (st_c["n_repacks"], repacks)
    if c == 1.0 and not first_step_given:
        assert evals == 2 * len(trials) + STAGES[method] * sum(trials)
    return trials, repacks


# -- the problems ------------------------------------------------------------------------------------------------------------
def random_problem(B, L, dtype, seed, device="cpu"):
    """`_random_problem` of tests/test_rowwise_gpu.py (rows of different stiffness, coupled inside a row only) ->
    (y0, plain func, func taking `rows`, maker of the plain func of a subset of the rows)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(-1, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None]
    w = (torch.rand(B, 1, generator=g, dtype=torch.float64) * 4)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64)
    k, w = k.to(device, dtype), w.to(device, dtype)

    def subset(idx):
        kk, ww = k[idx], w[idx]
        return lambda t, y: -kk * y + torch.sin(ww * t[:, None]) * torch.roll(y, 1, dims=1)

    def by_rows(t, y, rows):
        return -k[rows] * y + torch.sin(w[rows] * t[:, None]) * torch.roll(y, 1, dims=1)
    return y0.to(device, dtype), subset(slice(None)), by_rows, subset


def decay_problem(B, L, seed, device="cpu", lo=-1.0, hi=1.5):
    """fp32 rows of differing stiffness with a func without transcendentals (the same func bits on every backend)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(lo, hi, B, dtype=torch.float64)[:, None].to(device, torch.float32)
    y0 = torch.randn(B, L, generator=g, dtype=torch.float64).to(device, torch.float32)

    def plain(t, y):
        return -k * y + (1 - t * t)[:, None]

    def by_rows(t, y, rows):
        return -k[rows] * y + (1 - t * t)[:, None]
    return y0, plain, by_rows


def solve_both(plain, by_rows, y0, t, c, **kw):
    """((solution, stats) of the plain solve, (solution, stats) with compact=c)."""
    with torch.no_grad():
        a = tda.odeint_rowwise(plain, y0, t, return_stats=True, **kw)
        b = tda.odeint_rowwise(by_rows, y0, t, return_stats=True, compact=c, **kw)
    return a, b
