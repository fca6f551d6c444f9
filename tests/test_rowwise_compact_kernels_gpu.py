"""Kernel parity of the two entry points of the rowwise compaction, `tdeq_row_gather` and `tdeq_row_dense_commit_mapped`.

A gather copies bits, so it is compared with `torch.equal` against `index_select`; the mapped dense commit is the
arithmetic of `tdeq_row_dense_commit` at other addresses, so it agrees BIT FOR BIT with the oracle's plain commit run on
the mapped solution rows (tests/_rowwise_compact_oracle.py).  Every output sits in a sentinel-bordered buffer."""
import numpy as np
import pytest
import torch

from _rowwise_compact_oracle import CompactOracle
from _rowwise_kernels import SENTINEL, RowVectors, lane_elems, row_lengths, seeded
from test_rowwise_kernels_gpu import WIDE_MID

from torchdiffeq_amd.rowwise import _METHODS
from torchdiffeq_amd.tableaus import SparseRow

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
METHODS = sorted(_METHODS)


class _Placed:
    """CPU tensors copied into views of sentinel-filled device buffers, `offset` elements in (0: 16-byte aligned; 1: the
    scalar elements) and with a guard on both sides: `intact()` tells that nothing outside the views was written."""

    def __init__(self, offset=0, guard=16):
        self.offset, self.guard, self.bufs = offset, guard, []

    def __call__(self, t):
        n, lo = t.numel(), self.guard + self.offset
        buf = torch.full((lo + n + self.guard,), SENTINEL, dtype=t.dtype, device="cuda")
        view = buf[lo:lo + n].view(t.shape)
        view.copy_(t)
        self.bufs.append((buf, lo, n))
        return view

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()) for b, lo, n in self.bufs)


# ------------------------------------------------------------------------------------------------------------------------
# tdeq_row_gather
# ------------------------------------------------------------------------------------------------------------------------
N_ROWS = 37
INDEX_SETS = {"one": [5], "ends": [0, N_ROWS - 1], "every_third": list(range(1, N_ROWS, 3)), "all": list(range(N_ROWS))}
LENGTHS = [1, 3, 4, 129, 1500, 2050]      # fp32: scalar 1, 3, 129, 2050 and 16-byte 4, 1500; fp64: scalar 1, 3, 129 and 16-byte 4, 1500, 2050


def _gather(kern, srcs, idx, offset=0, src_offset=0):
    """One launch -> (outputs on the CPU, nothing outside them was written)."""
    out_put, src_put = _Placed(offset), _Placed(src_offset)
    L = srcs[0].shape[1]
    outs = [out_put(torch.full((len(idx), L), SENTINEL, dtype=srcs[0].dtype)) for _ in srcs]
    kern.row_gather(outs, [src_put(s) for s in srcs], torch.tensor(idx, dtype=torch.int32, device="cuda"))
    ok = out_put.intact() and src_put.intact()
    return [o.cpu() for o in outs], ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_gather(hip_kernels, dtype):
    lv = lane_elems(dtype)
    assert {L % lv == 0 for L in LENGTHS} == {True, False}
    for L in LENGTHS:
        srcs = [seeded((N_ROWS, L), dtype, 100 * L + m) for m in range(4)]
        srcs[1][3, 0] = float("nan")                     # a copy of bits: non-finite values travel like any other
        srcs[1][N_ROWS - 1, L - 1] = float("inf")
        for name, idx in INDEX_SETS.items():
            want = [s.index_select(0, torch.tensor(idx)) for s in srcs]
            for n_src in (1, 2, 3, 4):
                got, intact = _gather(hip_kernels, srcs[:n_src], idx)
                assert intact, (L, name, n_src)
                for m in range(n_src):
                    assert torch.equal(got[m].view(torch.uint8), want[m].view(torch.uint8)), (L, name, n_src, m)
        # buffers one element off 16-byte alignment take scalar elements: the same bits, the same bounds
        idx = INDEX_SETS["every_third"]
        want = [s.index_select(0, torch.tensor(idx)) for s in srcs]
        for offset, src_offset in ((0, 1), (1, 0), (1, 1)):
            got, intact = _gather(hip_kernels, srcs[:3], idx, offset, src_offset)
            assert intact, (L, offset, src_offset)
            for m in range(3):
                assert torch.equal(got[m].view(torch.uint8), want[m].view(torch.uint8)), (L, offset, src_offset, m)


def test_row_gather_no_rows(hip_kernels):
    src = seeded((4, 8), torch.float32, 1).cuda()
    out = torch.full((0, 8), SENTINEL, dtype=torch.float32, device="cuda")
    hip_kernels.row_gather([out], [src], torch.empty(0, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# tdeq_row_dense_commit_mapped
# ------------------------------------------------------------------------------------------------------------------------
N_OUT, SOL_ROWS, ROW_MAP = 5, 7, (1, 4, 6)


def _mapped_rows(kinds, seed):
    """Per compact row: not accepted, or accepted with 0, 1 (x = 1: the output time is the step's end) or 2 output times."""
    B = len(kinds)
    g = np.random.default_rng(seed)
    tprev, t1 = 0.25 + 0.125 * g.random(B), 0.75 + 0.125 * g.random(B)
    lo = g.integers(1, 3, B)
    hi = lo + np.array([0, 0, 1, 2])[kinds]
    tgrid = np.zeros((N_OUT, B))
    for r in range(B):
        tgrid[:, r] = t1[r] + 1 + np.arange(N_OUT)
        tgrid[:lo[r], r] = tprev[r] - 1
        for j in range(lo[r], hi[r]):
            tgrid[j, r] = t1[r] if j == hi[r] - 1 and kinds[r] == 2 else tprev[r] + (t1[r] - tprev[r]) * (j - lo[r] + 1) / 4
    return tgrid, dict(tprev=tprev, t0=t1, accepted=(np.asarray(kinds) > 0).astype(np.int32), out_lo=lo, out_hi=hi)


def _run_mapped(kern, oracle, L, dtype, mid, kinds, seed, offset=0):
    B = len(kinds)
    tgrid, state = _mapped_rows(kinds, seed)
    y0, y1, f0, f1 = (seeded((B, L), dtype, seed + j) for j in range(4))
    ks = [seeded((B, L), dtype, seed + 10 + j) for j in range(max(mid.idx) + 1)]
    dts = seeded((B,), dtype, seed + 30, 0.1)
    sol = torch.full((N_OUT, SOL_ROWS, L), SENTINEL, dtype=dtype)
    row_map = torch.tensor(ROW_MAP, dtype=torch.int32)
    res = []
    for dev, k in (("cuda", kern), ("cpu", oracle)):
        rows = RowVectors(dev, B, L, tgrid, **state)
        put = _Placed(offset) if dev == "cuda" else (lambda t: t.clone())
        s, a, b = put(sol), put(y0), put(f0)
        k.row_dense_commit_mapped(s, row_map.to(dev), a, put(y1), b, put(f1), [put(ks[j]) for j in mid.idx], mid.coef,
                                  dts.to(dev), rows.st)
        if dev == "cuda":
            assert put.intact()
        res.append((s.cpu(), a.cpu(), b.cpu()))
    return res, (y0, y1, f0, f1), state


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_dense_commit_mapped(hip_kernels, oracle_kernels, dtype):
    """The case matrix of tests/test_rowwise_kernels_gpu.py::test_row_dense_commit with 3 compact rows mapped into 7
    solution rows: the oracle's quartic bit for bit at the MAPPED rows, y0 <- y1 and f0 <- f1 at the COMPACT index for the
    accepted rows, every other word — unmapped solution rows, other slots, the guards — untouched."""
    oracle = CompactOracle(oracle_kernels)
    lv = lane_elems(dtype)
    cases = [(m, L) for m in METHODS + [WIDE_MID] for L in (5, 8 * lv)]               # (WIDE_MID: 14 terms)
    cases += [("dopri5", L) for L in row_lengths(dtype, (1, 3, 17, 257, 1024, 1500, 2049))]
    seen = set()
    for n, (method, L) in enumerate(cases):
        kinds = [(n + r) % 4 for r in range(3)]
        seen |= set(kinds)
        mid = SparseRow.from_dense(method if method is WIDE_MID else _METHODS[method].tableau.c_mid)
        (dev, ref), (y0, y1, f0, f1), state = _run_mapped(hip_kernels, oracle, L, dtype, mid, kinds, L + n)
        for name, g, e in zip(("sol", "y0", "f0"), dev, ref):
            assert torch.equal(g, e), (method, L, kinds, name)
        acc = torch.as_tensor(state["accepted"] != 0)
        sol, ny0, nf0 = dev
        assert torch.equal(ny0[acc], y1[acc]) and torch.equal(nf0[acc], f1[acc])
        assert torch.equal(ny0[~acc], y0[~acc]) and torch.equal(nf0[~acc], f0[~acc])
        unmapped = [q for q in range(SOL_ROWS) if q not in ROW_MAP]
        assert bool((sol[:, unmapped] == SENTINEL).all()), (method, L, kinds)
        for r, q in enumerate(ROW_MAP):
            lo, hi = (int(state["out_lo"][r]), int(state["out_hi"][r])) if acc[r] else (0, 0)
            outside = [j for j in range(N_OUT) if not lo <= j < hi]
            assert bool((sol[outside, q] == SENTINEL).all()), (method, L, kinds, r)
            assert bool((sol[lo:hi, q] != SENTINEL).all())
            assert hi - lo == (0, 0, 1, 2)[kinds[r]]
        (off, _), _, _ = _run_mapped(hip_kernels, oracle, L, dtype, mid, kinds, L + n, offset=1)
        for g, e in zip(off, dev):
            assert torch.equal(g, e), (method, L, kinds, "one element off")
    assert seen == {0, 1, 2, 3}


def test_row_dense_commit_mapped_offsets_past_2_31(hip_kernels, oracle_kernels):
    """Offsets into `sol` beyond 2^31 elements: fp32, two outputs, L = 1024, 2^20 + 8 solution rows (about 8.6 GB, never
    initialised as a whole); two compact rows go to the first and the last solution row."""
    L, sol_rows, n_out = 1024, (1 << 20) + 8, 2
    assert (n_out * sol_rows - 1) * L > 1 << 31
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 1024 ** 3:
        pytest.skip("needs 16 GB of free device memory")
    dtype = torch.float32
    mid = SparseRow.from_dense(_METHODS["dopri5"].tableau.c_mid)
    tprev, t1 = np.array([0.25, 0.3]), np.array([0.75, 0.8])
    tgrid = np.stack([tprev + 0.25 * (t1 - tprev), t1])                       # both outputs inside both rows' steps
    state = dict(tprev=tprev, t0=t1, accepted=np.ones(2, dtype=np.int32), out_lo=np.zeros(2), out_hi=np.full(2, 2))
    y0, y1, f0, f1 = (seeded((2, L), dtype, 7 + j) for j in range(4))
    ks = [seeded((2, L), dtype, 20 + j) for j in range(max(mid.idx) + 1)]
    dts = seeded((2,), dtype, 30, 0.1)
    # the oracle on a two-row solution
    ref = torch.full((n_out, 2, L), SENTINEL, dtype=dtype)
    rows = RowVectors("cpu", 2, L, tgrid, **state)
    a, b = y0.clone(), f0.clone()
    oracle_kernels.row_dense_commit(ref, a, y1, b, f1, [ks[j] for j in mid.idx], mid.coef, dts, rows.st)
    sol = torch.empty(n_out, sol_rows, L, dtype=dtype, device="cuda")
    watched = [0, 1, sol_rows - 2, sol_rows - 1]
    sol[:, watched] = SENTINEL
    rows = RowVectors("cuda", 2, L, tgrid, **state)
    ya, fa = y0.cuda(), f0.cuda()
    row_map = torch.tensor([0, sol_rows - 1], dtype=torch.int32, device="cuda")
    hip_kernels.row_dense_commit_mapped(sol, row_map, ya, y1.cuda(), fa, f1.cuda(), [ks[j].cuda() for j in mid.idx], mid.coef,
                                        dts.cuda(), rows.st)
    torch.cuda.synchronize()
    got = sol[:, watched].cpu()
    assert torch.equal(got[:, [0, 3]], ref)
    assert bool((got[:, [1, 2]] == SENTINEL).all())
    assert torch.equal(ya.cpu(), a) and torch.equal(fa.cpu(), b)
