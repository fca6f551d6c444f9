"""`odeint_rowwise(compact=...)` on the HIP kernels: a compacted solve gives the bits, counters and `nfe` of the plain
one on the same device, `func` sees the rows the schedule prescribes (the simulator of
tests/_rowwise_compact_oracle.py), and an error after a repack names the original row."""
import pytest
import torch

from _rowwise_compact_oracle import METHODS, assert_same_solve, decay_problem, quiet, random_problem, solve_both  # noqa: F401

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_PLAIN = {}


def _plain_random(method):
    """The plain device solve of the random problem, computed once per method and left unchanged."""
    if method not in _PLAIN:
        y0, plain, by_rows, _ = random_problem(96, 5, torch.float64, 1, DEV)
        t = torch.linspace(0, 1.5, 4, dtype=torch.float64, device=DEV)
        with torch.no_grad():
            res = tda.odeint_rowwise(plain, y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
        _PLAIN[method] = (y0, t, by_rows, res)
    return _PLAIN[method]


# -- 1. device solves, compact against plain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method,c", [(m, 0.5) for m in METHODS] + [(m, 1.0) for m in METHODS if m != "adaptive_heun"])
def test_hip_compact_equals_plain_fp64(method, c):
    y0, t, by_rows, plain = _plain_random(method)
    with torch.no_grad():
        compact = tda.odeint_rowwise(by_rows, y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True, compact=c)
    _, repacks = assert_same_solve(plain, compact, c, method)
    assert repacks >= 3


# -- 2. row shapes: every reduction geometry, 16-byte and scalar elements -------------------------------------------------------
@pytest.mark.parametrize("B,L", [(4096, 1), (64, 3), (64, 128), (64, 129), (16, 1500), (16, 4100), (16, 8196)])
def test_hip_compact_shapes(B, L):
    y0, plain, by_rows = decay_problem(B, L, L, DEV, hi=1.0)
    t = torch.tensor([0.0, 0.5, 1.0], device=DEV)
    for c in (0.5, 1.0):
        res = solve_both(plain, by_rows, y0, t, c, rtol=1e-5, atol=1e-7)
        _, repacks = assert_same_solve(*res, c, "dopri5")
        assert repacks >= 2


# -- 3. grids and options -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["t2d", "decreasing", "first_step"])
def test_hip_compact_grids_and_options(kind):
    B = 12
    y0, plain, by_rows, _ = random_problem(B, 3, torch.float64, 7, DEV)
    t = torch.linspace(0, 1.2, 4, dtype=torch.float64)
    opts = None
    if kind == "t2d":            # rows that end at different times
        t = t[:, None] * torch.linspace(0.2, 1.0, B, dtype=torch.float64) + 0.05 * torch.arange(B).to(torch.float64)
    elif kind == "decreasing":
        t = torch.linspace(1, 0, 4, dtype=torch.float64)
    else:
        opts = {"first_step": torch.linspace(1e-3, 5e-3, B, dtype=torch.float64)}
    for c in (0.5, 1.0):
        res = solve_both(plain, by_rows, y0, t.to(DEV), c, rtol=1e-6, atol=1e-8, options=opts)
        _, repacks = assert_same_solve(*res, c, "dopri5", first_step_given=kind == "first_step")
        assert repacks >= 1


# -- 4. an error after a repack names the original row ---------------------------------------------------------------------------------
def test_hip_compact_max_num_steps_names_the_original_row():
    k = torch.tensor([[0.1], [0.1], [5000.0], [0.1]], dtype=torch.float64, device=DEV)
    y0 = torch.ones(4, 1, dtype=torch.float64, device=DEV)
    lengths = []

    def func(t, y, rows):
        assert rows.device == y.device and rows.dtype == torch.int64
        lengths.append(len(rows))
        return -k[rows] * (y - torch.sin(t)[:, None])
    with pytest.raises(AssertionError, match=r"max_num_steps exceeded \(\d+>=50\) in row 2"):
        tda.odeint_rowwise(func, y0, torch.tensor([0.0, 5.0], device=DEV), rtol=1e-5, atol=1e-7,
                           options={"max_num_steps": 50}, compact=1.0)
    assert lengths[-1] == 1                                           # the stiff row was alone by then: compact row 0
