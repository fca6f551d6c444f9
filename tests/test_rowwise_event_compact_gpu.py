"""`odeint_rowwise_event(compact=...)` on the HIP kernels against the SAME device solve without `compact`: every output
bit for bit (a row's bits do not depend on the rows it shares a launch with), and rows did leave.  func and event_fn are
those of `decay_event_problem`, indexed by `rows` (tests/_rowwise_event_compact_oracle.py)."""
import functools
import warnings

import pytest
import torch

from _rowwise_event_compact_oracle import METHODS, decay_event_problem_rows

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
COMPACT = [pytest.param(True, id="half"), pytest.param(1.0, id="every")]
SEEDS = {F64: 3, F32: 1}                                     # (those of tests/test_rowwise_event_compact.py)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _tols(method, dtype):
    """Those of tests/test_rowwise_event_compact.py: tight enough that the rows of every method stop in different trial
    steps; the order-2 pairs a hundred times looser."""
    rtol, atol = (1e-7, 1e-9) if dtype == F64 else (1e-6, 1e-8)
    return (rtol * 100, atol * 100) if method in ("adaptive_heun", "fehlberg2") else (rtol, atol)


def _solve(func, y0, t0, event_fn, **kw):
    with torch.no_grad():
        out = tda.odeint_rowwise_event(func, y0, t0, event_fn=event_fn, return_stats=True, **kw)
    torch.cuda.synchronize()
    return out


def _assert_same(plain, compact):
    (tp, sp, xp), (tc, sc, xc) = plain, compact
    assert tc.device.type == "cuda" and sc.device.type == "cuda"
    assert torch.equal(tc, tp) and torch.equal(sc, sp)
    for name in ("n_accepted", "n_rejected", "fired"):
        assert torch.equal(xc[name], xp[name]), name
    assert xc["nfe"] == xp["nfe"] and xc["n_event_evals"] == xp["n_event_evals"]
    n = tp.shape[0]
    print(f"n_repacks {xc['n_repacks']}, row_evals {xc['row_evals']} of {n * xc['nfe']}, event_row_evals "
          f"{xc['event_row_evals']} of {n * xc['n_event_evals']}")
    assert xc["n_repacks"] >= 1
    assert xc["row_evals"] < n * xc["nfe"] and xc["event_row_evals"] < n * xc["n_event_evals"]


@functools.lru_cache(maxsize=None)
def _plain(B, L, method, dtype, t_end_key):
    """The plain device solve of one configuration: computed once, shared by the `compact` values."""
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEEDS[dtype], DEV)
    rtol, atol = _tols(method, dtype)
    return _solve(lambda t, y: func(t, y), y0, 0.0, lambda t, y: event_fn(t, y), t_end=_t_end(t_end_key, B), rtol=rtol,
                  atol=atol, method=method)


def _t_end(key, B):
    return {"none": None, "number": 0.15, "vector": torch.linspace(0.05, 0.4, B, dtype=F64)}[key]


def _compact_against_plain(B, L, method, dtype, t_end_key, compact):
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEEDS[dtype], DEV)
    rtol, atol = _tols(method, dtype)
    plain = _plain(B, L, method, dtype, t_end_key)
    got = _solve(func, y0, 0.0, event_fn, t_end=_t_end(t_end_key, B), rtol=rtol, atol=atol, method=method, compact=compact)
    _assert_same(plain, got)
    return plain, got


@pytest.mark.parametrize("compact", COMPACT)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_compact_equals_plain_12x5(method, dtype, compact):
    plain, _ = _compact_against_plain(12, 5, method, dtype, "none", compact)
    assert bool(plain[2]["fired"].all())


@pytest.mark.parametrize("compact", COMPACT)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_compact_equals_plain_96x24(method, dtype, compact):
    """L = 24: 16-byte elements in both dtypes (12 x 5 takes the scalar kernels)."""
    plain, got = _compact_against_plain(96, 24, method, dtype, "none", compact)
    assert bool(plain[2]["fired"].all())


@pytest.mark.parametrize("compact", COMPACT)
@pytest.mark.parametrize("t_end", ["number", "vector"])
@pytest.mark.parametrize("B,L", [(12, 5), (96, 24)])
def test_t_end(B, L, t_end, compact):
    """Rows that reach t_end leave like rows that fired; their solution row comes from the mapped dense output."""
    plain, _ = _compact_against_plain(B, L, "dopri5", F64, t_end, compact)
    assert 0 < int(plain[2]["fired"].sum()) < B


@pytest.mark.parametrize("compact", COMPACT)
def test_decreasing_time_with_rows_fired_at_t0(compact):
    """The mirror image of the problem (y' = k (1 - t) y from 0 towards t_end = -3), rows 2 and 9 with g(t0) == 0: never
    active (`deactivate_rows`), they leave at the first repack and keep y0."""
    B, L = 12, 5
    y0, _, _, k, _ = decay_event_problem_rows(B, L, F64, 5, DEV)
    q = torch.linspace(0.9, 0.2, B, dtype=F64)[torch.randperm(B, generator=torch.Generator().manual_seed(6))]
    q[[2, 9]] = 1.0
    level = (y0[:, 0] * q.to(DEV)).clone()
    kw = dict(t_end=-3.0, rtol=1e-6, atol=1e-8)
    plain = _solve(lambda t, y: k * y * (1 - t)[:, None], y0, 0.0, lambda t, y: y[:, 0] - level, **kw)
    got = _solve(lambda t, y, rows: k[rows] * y * (1 - t)[:, None], y0, 0.0, lambda t, y, rows: y[:, 0] - level[rows],
                 compact=compact, **kw)
    _assert_same(plain, got)
    event_t, sol, x = got
    assert bool(x["fired"].all()) and bool((event_t[[2, 9]] == 0.0).all()) and torch.equal(sol[1][[2, 9]], y0[[2, 9]])
    assert (x["n_accepted"] + x["n_rejected"])[[2, 9]].tolist() == [0, 0]


@pytest.mark.parametrize("compact", COMPACT)
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_tolerances(dtype, compact):
    """[B] tolerances: re-selected at a repack for the kernels, read for all rows by the bisection."""
    B, L = 12, 5
    y0, func, event_fn, _, _ = decay_event_problem_rows(B, L, dtype, SEEDS[dtype], DEV)
    lo, hi = (-4, -8) if dtype == F64 else (-2, -5)
    g = torch.Generator().manual_seed(11)
    rtol = torch.logspace(lo, hi, B, dtype=F64)[torch.randperm(B, generator=g)]
    atol = rtol * 1e-2
    plain = _solve(lambda t, y: func(t, y), y0, 0.0, lambda t, y: event_fn(t, y), t_end=0.3, rtol=rtol, atol=atol)
    got = _solve(func, y0, 0.0, event_fn, t_end=0.3, rtol=rtol, atol=atol, compact=compact)
    _assert_same(plain, got)
    assert 0 < int(plain[2]["fired"].sum()) < B
