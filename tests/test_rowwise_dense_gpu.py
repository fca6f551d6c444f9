"""`odeint_rowwise_dense` on the MI355X: the device solve and the device evaluation against the device `odeint_rowwise` on
the per-row grid [t0, the queries sorted, t1], bit for bit — the contract of tests/test_rowwise_dense.py on the HIP kernels —
with `compact`, forced small chunks and the NaN rows of `check=False`."""
import functools

import pytest
import torch

from _rowwise_dense_oracle import METHODS, decay_problem, grid_reference, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SEED, Q = 3, 7
SHAPES = {"12x5": (12, 5), "96x24": (96, 24)}


def _dense(func, y0, t0, t1, **kw):
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, t1, return_stats=True, **kw)


@functools.lru_cache(maxsize=None)
def _solved(shape, method, dtype):
    B, L = SHAPES[shape]
    y0, func, _ = decay_problem(B, L, dtype, SEED, DEV)
    return _dense(func, y0, 0.0, per_row_t1(B, DEV), method=method, **tolerances(method, dtype))


def _assert_equals_grid(dense, q, func, y0, t0, t1, **kw):
    def solve(grid):
        with torch.no_grad():
            return tda.odeint_rowwise(func, y0, grid, **kw)
    got = dense(q)
    ref = grid_reference(solve, q.cpu(), t0.cpu(), t1.cpu())
    assert got.device == ref.device == y0.device and got.shape == (q.shape[0], *y0.shape)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,method", [("12x5", m) for m in METHODS] + [("96x24", "dopri5"), ("96x24", "bosh3")])
def test_dense_equals_the_grid_solve(shape, method, dtype):
    """[B] `t1`, unsorted per-row queries plus both ends of every row."""
    B, L = SHAPES[shape]
    y0, func, _ = decay_problem(B, L, dtype, SEED, DEV)
    t0, t1 = torch.zeros(B, dtype=F64, device=DEV), per_row_t1(B, DEV)
    dense, stats = _solved(shape, method, dtype)
    q = torch.cat([random_queries(Q, t0, t1, seed=11), t1[None], t0[None]])
    _assert_equals_grid(dense, q, func, y0, t0, t1, method=method, **tolerances(method, dtype))
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(stats["n_accepted"], 0)
    assert torch.equal(dense.offsets.cpu(), off) and dense.coeffs.shape == (5, int(off[-1]), L) and dense.coeffs.device == y0.device
    a, b = dense.seg_start.cpu(), dense.seg_end.cpu()
    inner = torch.ones(int(off[-1]), dtype=torch.bool)
    inner[off[1:] - 1] = False                                               # every segment but a row's last
    assert torch.equal(a[1:][inner[:-1]], b[:-1][inner[:-1]]) and bool((a[off[:-1]] == 0).all())
    assert bool((b[off[1:] - 1] >= t1.cpu()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_number_t1_and_decreasing_time(dtype):
    B, L = SHAPES["12x5"]
    y0, func, _ = decay_problem(B, L, dtype, SEED, DEV)
    kw = dict(method="dopri5", **tolerances("dopri5", dtype))
    t0 = torch.zeros(B, dtype=F64, device=DEV)
    t1 = torch.full((B,), 0.45, dtype=F64, device=DEV)
    dense, _ = _dense(func, y0, 0.0, 0.45, **kw)
    _assert_equals_grid(dense, random_queries(Q, t0, t1, seed=6), func, y0, t0, t1, **kw)
    t0 = torch.full((B,), 0.3, dtype=F64, device=DEV)
    t1 = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64, device=DEV)
    dense, _ = _dense(func, y0, 0.3, t1, **kw)
    q = torch.cat([random_queries(Q, t0, t1, seed=2), t0[None], t1[None]])
    _assert_equals_grid(dense, q, func, y0, t0, t1, **kw)
    assert bool((dense.seg_end < dense.seg_start).all())


@pytest.mark.parametrize("compact", [True, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,method", [("12x5", "dopri5"), ("12x5", "dopri8"), ("96x24", "bosh3")])
def test_compact_equals_plain(shape, method, dtype, compact):
    B, L = SHAPES[shape]
    y0, func, _ = decay_problem(B, L, dtype, SEED, DEV)
    t0, t1 = torch.zeros(B, dtype=F64, device=DEV), per_row_t1(B, DEV)
    plain, st_p = _solved(shape, method, dtype)
    dense, st_c = _dense(func, y0, 0.0, t1, method=method, compact=compact, **tolerances(method, dtype))
    for name in ("t0", "t1", "offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(dense, name), getattr(plain, name)), name
    q = random_queries(Q, t0, t1, seed=4)
    assert torch.equal(dense(q), plain(q))
    assert torch.equal(st_c["n_accepted"], st_p["n_accepted"]) and torch.equal(st_c["n_rejected"], st_p["n_rejected"])
    assert st_c["n_repacks"] >= 1 and st_c["row_evals"] < B * st_c["nfe"]


@pytest.mark.parametrize("compact", [None, 1.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_chunks_pack_to_the_same_arrays(dtype, compact):
    B, L = SHAPES["12x5"]
    y0, func, _ = decay_problem(B, L, dtype, SEED, DEV)
    kw = dict(method="dopri5", compact=compact, **tolerances("dopri5", dtype))
    one, st_one = _dense(func, y0, 0.0, per_row_t1(B, DEV), options={"dense_chunk_rows": 4096}, **kw)
    many, st_many = _dense(func, y0, 0.0, per_row_t1(B, DEV), options={"dense_chunk_rows": 1}, **kw)
    assert st_one["n_chunks"] == 1 and st_many["n_chunks"] >= 3
    for name in ("offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(many, name), getattr(one, name)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range(dtype):
    B, L = SHAPES["12x5"]
    t0, t1 = torch.zeros(B, dtype=F64, device=DEV), per_row_t1(B, DEV)
    dense, _ = _solved("12x5", "dopri5", dtype)
    good = random_queries(3, t0, t1, seed=9)
    want = dense(good)
    q = good.clone()
    q[2, 1], q[1, 9], q[1, 3] = float("nan"), 5.0, -2.0
    with pytest.raises(ValueError, match=r"query 1 of row 3 "):
        dense(q)
    got = dense(q, check=False)
    bad = torch.isnan(got).all(dim=2)
    assert bad.nonzero().tolist() == [[1, 3], [1, 9], [2, 1]]
    assert torch.equal(got[~bad], want[~bad])
    assert not bool(torch.isnan(dense(t1[None])).any())                      # t1 itself is valid
