"""The three dense-output kernels of csrc/tdeq_kernels_rowwise_dense.hpp on the MI355X against the CPU oracle
(tests/_rowwise_dense_oracle.py): the slots on hand-made controller states (sets, not orders: the slot order inside a chunk
is arrival order), the pack and the search bit for bit, every output inside sentinel borders, and the chain search ->
row_event_eval_mapped against row_dense_commit."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import NONE, DenseOracle
from _rowwise_kernels import SENTINEL, RowVectors, seeded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
BORDER = 8                                                   # elements: the payload stays 16-byte aligned
ISENT = -77


@pytest.fixture(scope="module")
def oracle(oracle_kernels):
    return DenseOracle(oracle_kernels)


def _bordered(shape, dtype, device, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER,), fill, dtype=dtype, device=device)
    return buf, buf[BORDER:BORDER + n].view(*shape)


def _borders_intact(buf, fill=SENTINEL):
    return bool((buf[:BORDER] == fill).all()) and bool((buf[-BORDER:] == fill).all())


# -- slots -------------------------------------------------------------------------------------------------------------------------
def _run_slots(kern, device, n, accepted, row_map, cap, base):
    r = np.arange(n)
    rv = RowVectors(device, n, 3, np.stack([np.zeros(n), np.full(n, 100.0)]), accepted=accepted, t0=1.0 + 0.125 * r,
                    tprev=0.5 + 0.125 * r, n_acc=1 + (r * 7) % 11)
    counter = torch.tensor([base, 0], dtype=torch.int32, device=device)
    bufs = {}
    for name, dtype, size, fill in (("slot_row", torch.int32, cap, ISENT), ("slot_ord", torch.int32, cap, ISENT),
                                    ("slot_ta", F64, cap, SENTINEL), ("slot_tb", F64, cap, SENTINEL),
                                    ("slot", torch.int32, n, ISENT), ("mask", torch.int32, n, ISENT)):
        bufs[name] = _bordered((size,), dtype, device, fill)
    kern.row_dense_slots(rv.st, None if row_map is None else row_map.to(device), cap, counter,
                         *[bufs[name][1] for name in ("slot_row", "slot_ord", "slot_ta", "slot_tb", "slot", "mask")])
    if device != "cpu":
        torch.cuda.synchronize()
    out = {name: buf.cpu() for name, (buf, _) in bufs.items()}
    out["counter"] = counter.cpu()
    out["state"] = rv.cpu()
    return out


def _payload(out, name):
    return out[name][BORDER:-BORDER]


@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "row_map"])
@pytest.mark.parametrize("pattern", ["none", "all", "mixed"])
@pytest.mark.parametrize("n", [5, 70, 300])
def test_slots(n, pattern, mapped, hip_kernels, oracle):
    """n = 70: two waves; 300: two workgroups.  `counter[0]` starts at 3."""
    r = np.arange(n)
    accepted = {"none": np.zeros(n), "all": np.ones(n), "mixed": ((r * 5) % 7 < 3)}[pattern].astype(np.int32)
    row_map = ((torch.arange(n) * 37 + 11) % n + 1000).to(torch.int32) if mapped else None      # non-monotone (37, n coprime)
    count, base = int(accepted.sum()), 3
    cap = base + count + 4
    ref = _run_slots(oracle, "cpu", n, accepted, row_map, cap, base)
    got = _run_slots(hip_kernels, DEV, n, accepted, row_map, cap, base)
    acc = torch.from_numpy(accepted)
    for out in (ref, got):
        assert out["counter"].tolist() == [base + count, 0]
        assert torch.equal(_payload(out, "mask"), acc)
        slot = _payload(out, "slot")
        assert bool((slot[acc == 0] == -1).all())
        taken = slot[acc == 1].to(torch.int64)
        assert sorted(taken.tolist()) == list(range(base, base + count))                         # unique, in [base, base + count)
        used = torch.zeros(cap, dtype=torch.bool)
        used[taken] = True
        for name, fill in (("slot_row", ISENT), ("slot_ord", ISENT), ("slot_ta", SENTINEL), ("slot_tb", SENTINEL)):
            assert _borders_intact(out[name], fill) and bool((_payload(out, name)[~used] == fill).all()), name
        assert _borders_intact(out["slot"], ISENT) and _borders_intact(out["mask"], ISENT)
        # the slot a row took holds that row's metadata
        rows = torch.nonzero(acc).view(-1)
        want_row = rows.to(torch.int32) if row_map is None else row_map[rows]
        assert torch.equal(_payload(out, "slot_row")[taken], want_row)
        assert torch.equal(_payload(out, "slot_ord")[taken], (out["state"]["n_acc"][rows] - 1).to(torch.int32))
        assert torch.equal(_payload(out, "slot_ta")[taken], out["state"]["tprev"][rows])
        assert torch.equal(_payload(out, "slot_tb")[taken], out["state"]["t0"][rows])
    # the sets of (row, ord, ta, tb) over the used slots are the oracle's
    def records(out):
        s = slice(base, base + count)
        return sorted(zip(*[_payload(out, name)[s].tolist() for name in ("slot_row", "slot_ord", "slot_ta", "slot_tb")]))
    assert records(got) == records(ref)
    for name in got["state"]:                                                                    # the state is only read
        assert torch.equal(got["state"][name], ref["state"][name]), name


@pytest.mark.parametrize("n", [70, 300])
def test_slots_overflow_writes_nothing_beyond_cap(n, hip_kernels, oracle):
    """`cap` two short of the demand: no write at or beyond cap (the borders), counter[1] == 1, two rows without a slot."""
    accepted = np.ones(n, dtype=np.int32)
    base = 3
    cap = base + n - 2
    for kern, device in ((oracle, "cpu"), (hip_kernels, DEV)):
        out = _run_slots(kern, device, n, accepted, None, cap, base)
        assert out["counter"].tolist() == [base + n, 1]
        mask, slot = _payload(out, "mask"), _payload(out, "slot")
        assert int(mask.sum()) == n - 2 and bool((slot[mask == 0] == -1).all())
        assert sorted(slot[mask == 1].tolist()) == list(range(base, cap))
        for name, fill in (("slot_row", ISENT), ("slot_ord", ISENT), ("slot_ta", SENTINEL), ("slot_tb", SENTINEL)):
            assert _borders_intact(out[name], fill), name
            assert bool((_payload(out, name)[:base] == fill).all()) and not bool((_payload(out, name)[base:] == fill).any())


# -- pack --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [3, 8, 1028])
def test_pack(L, dtype, hip_kernels, oracle):
    """L = 3: scalar elements; 8, 1028: 16-byte elements (1028: more than one workgroup)."""
    src = seeded((5, 6, L), dtype, 31)
    dest = torch.tensor([7, 0, 3, 8], dtype=torch.int64)
    outs = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        buf, dst = _bordered((5, 9, L), dtype, device)
        kern.row_dense_pack(dst, src.to(device), dest.to(device), 4)
        kern.row_dense_pack(dst, src.to(device), dest[:0].to(device), 0)                          # nothing
        if device != "cpu":
            torch.cuda.synchronize()
        outs.append(buf.cpu())
    ref, got = outs
    assert torch.equal(got, ref) and _borders_intact(got)
    dst = got[BORDER:-BORDER].view(5, 9, L)
    assert torch.equal(dst[:, dest], src[:, :4])
    assert bool((dst[:, [1, 2, 4, 5, 6]] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shifted", ["dst", "src", "both"])
def test_pack_misaligned_base_and_empty_call(shifted, dtype, hip_kernels, oracle):
    """L = 8 allows 16-byte elements, but a base one element off a 16-byte boundary must take the scalar path: bit for bit
    the oracle's, borders intact.  And `n_used == 0` at the entry point itself (the binding returns before it): no write."""
    L, one = 8, 1
    src = seeded((5, 6, L), dtype, 33)
    dest = torch.tensor([7, 0, 3, 8], dtype=torch.int64)
    outs = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        n_dst, n_src = 5 * 9 * L, 5 * 6 * L
        d_off = BORDER + (one if shifted in ("dst", "both") else 0)
        s_off = one if shifted in ("src", "both") else 0
        buf = torch.full((n_dst + 2 * BORDER + one,), SENTINEL, dtype=dtype, device=device)
        dst = buf[d_off:d_off + n_dst].view(5, 9, L)
        src_buf = torch.empty(n_src + one, dtype=dtype, device=device)
        src_dev = src_buf[s_off:s_off + n_src].view(5, 6, L)
        src_dev.copy_(src)
        if device != "cpu":
            assert (dst.data_ptr() % 16 != 0) == (shifted != "src") and (src_dev.data_ptr() % 16 != 0) == (shifted != "dst")
            from torchdiffeq_amd import _native
            code = kern.lib.tdeq_row_dense_pack(dst.data_ptr(), 9, src_dev.data_ptr(), 6, dest.to(device).data_ptr(), 0, L,
                                                _native.dtype_code(dtype), None)
            torch.cuda.synchronize()
            assert code == 0 and bool((buf == SENTINEL).all())
        kern.row_dense_pack(dst, src_dev, dest.to(device), 4)
        if device != "cpu":
            torch.cuda.synchronize()
        outs.append((buf.cpu(), d_off))
    (ref, d_off), (got, _) = outs
    assert torch.equal(got, ref)
    assert bool((got[:d_off] == SENTINEL).all()) and bool((got[d_off + 5 * 9 * L:] == SENTINEL).all())
    dst = got[d_off:d_off + 5 * 9 * L].view(5, 9, L)
    assert torch.equal(dst[:, dest], src[:, :4]) and bool((dst[:, [1, 2, 4, 5, 6]] == SENTINEL).all())


# -- search ------------------------------------------------------------------------------------------------------------------------
def _segments(counts, seed):
    """Rows with the given numbers of segments: t0_r = 0.1 r, random positive widths, t1_r inside the last segment."""
    g = torch.Generator().manual_seed(seed)
    ta, tb, t0, t1, off = [], [], [], [], [0]
    for r, n in enumerate(counts):
        edges = 0.1 * r + torch.cat([torch.zeros(1, dtype=F64), torch.cumsum(0.05 + torch.rand(n, generator=g, dtype=F64), 0)])
        ta += edges[:-1].tolist()
        tb += edges[1:].tolist()
        t0.append(float(edges[0]))
        t1.append(float(edges[-2] + 0.75 * (edges[-1] - edges[-2])))
        off.append(off[-1] + n)
    f = lambda v: torch.tensor(v, dtype=F64)      # noqa: E731
    return torch.tensor(off, dtype=torch.int64), f(ta), f(tb), f(t0), f(t1)


def _queries(off, ta, tb, t0, t1):
    """Per row: t0, t1, an exact interior breakpoint (t1 again for a one-segment row), two interior points and one
    out-of-range point — below t0, beyond t1 (inside the last segment) and NaN in turn over the rows."""
    B = t0.numel()
    q = torch.empty(6, B, dtype=F64)
    for r in range(B):
        lo, hi = int(off[r]), int(off[r + 1])
        outside = (float(t0[r]) - 1e-3, float(t1[r] + (tb[hi - 1] - t1[r]) / 2), float("nan"))[r % 3]
        q[:, r] = torch.tensor([float(t0[r]), float(t1[r]), float(tb[lo + (hi - lo) // 2 - 1]) if hi - lo > 1 else float(t1[r]),
                                float(t0[r] + 0.3 * (t1[r] - t0[r])), outside, float(t0[r] + 0.9 * (t1[r] - t0[r]))], dtype=F64)
    return q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("counts", [(1, 2, 3, 7, 1), tuple(1 + (r * 5) % 9 for r in range(70))], ids=["B5", "B70"])
def test_search(counts, dtype, hip_kernels, oracle):
    """B = 70: 420 queries over seven waves and two workgroups — the status minimum (query 4 of row 0) crosses waves."""
    off, ta, tb, t0, t1 = _segments(counts, 17)
    B = len(counts)
    q = _queries(off, ta, tb, t0, t1)
    outs = []
    for device, kern in (("cpu", oracle), (DEV, hip_kernels)):
        to = lambda t: t.to(device)      # noqa: E731
        seg_buf, seg = _bordered((6 * B,), torch.int32, device, ISENT)
        x_buf, x = _bordered((6 * B,), dtype, device)
        status = torch.tensor([NONE], dtype=torch.int32, device=device)
        kern.row_dense_search(to(q), to(off), to(ta), to(tb), to(t0), to(t1), seg, x, status)
        clean = torch.tensor([NONE], dtype=torch.int32, device=device)                            # the valid queries alone
        kern.row_dense_search(to(q[:4].contiguous()), to(off), to(ta), to(tb), to(t0), to(t1), seg.clone()[:4 * B],
                              x.clone()[:4 * B], clean)
        if device != "cpu":
            torch.cuda.synchronize()
        outs.append((seg_buf.cpu(), x_buf.cpu(), int(status), int(clean)))
    (seg_ref, x_ref, st_ref, clean_ref), (seg_got, x_got, st_got, clean_got) = outs
    assert torch.equal(seg_got, seg_ref) and _borders_intact(seg_got, ISENT) and _borders_intact(x_got)
    assert torch.equal(x_got.view(torch.uint8), x_ref.view(torch.uint8)) or \
        (torch.equal(torch.isnan(x_got), torch.isnan(x_ref)) and torch.equal(x_got.nan_to_num(7.0), x_ref.nan_to_num(7.0)))
    assert st_got == st_ref == 4 * B and clean_got == clean_ref == NONE
    # what the oracle must have found, stated once more from the rule
    seg, x = seg_ref[BORDER:-BORDER].view(6, B), x_ref[BORDER:-BORDER].view(6, B)
    assert torch.equal(seg[0], off[:-1].to(torch.int32)) and bool((x[0] == 0).all())             # t0: first segment, x = 0
    assert torch.equal(seg[1], (off[1:] - 1).to(torch.int32)) and bool((x[1] < 1).all())         # t1: inside the last one
    multi = torch.tensor([n > 1 for n in counts])
    assert bool((x[2][multi] == 1).all())                                                        # a breakpoint: the earlier step
    assert bool(torch.isnan(x[4]).all()) and torch.equal(seg[4], off[:-1].to(torch.int32))
    assert not bool(torch.isnan(x[[0, 1, 2, 3, 5]]).any())


# -- chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_then_eval_reproduces_row_dense_commit(dtype, hip_kernels):
    """One accepted step per row with two output times inside it: `row_dense_commit` writes the solution rows; the same
    step's quartic through `row_event_fit`, searched and evaluated at the same times, gives the same bits (L = 8)."""
    B, L, nt = 5, 8, 6
    y0, y1, f0, f1 = (seeded((B, L), dtype, 40 + i).to(DEV) for i in range(4))
    ks = [seeded((B, L), dtype, 50 + j).to(DEV) for j in range(nt)]
    coefs = [0.37 / (j + 1) * (-1) ** j for j in range(nt)]
    r = torch.arange(B, dtype=F64)
    ta, tb = 0.5 + 0.125 * r, 0.5 + 0.125 * r + 0.05 * (1 + r)
    dts = (tb - ta).to(dtype).to(DEV)
    tgrid = torch.stack([ta - 1.0, ta + 0.3 * (tb - ta), ta + 0.8 * (tb - ta), tb + 1.0])
    rv = RowVectors(DEV, B, L, tgrid, accepted=np.ones(B), tprev=ta, t0=tb, out_lo=np.ones(B), out_hi=np.full(B, 3))
    sol = torch.full((4, B, L), SENTINEL, dtype=dtype, device=DEV)
    q = torch.empty(5, B, L, dtype=dtype, device=DEV)
    hip_kernels.row_event_fit(q, torch.ones(B, dtype=torch.int32, device=DEV), y0, y1, f0, f1, ks, coefs, dts)
    hip_kernels.row_dense_commit(sol, y0.clone(), y1, f0.clone(), f1, ks, coefs, dts, rv.st)
    tq = tgrid[1:3].contiguous().to(DEV)
    seg = torch.empty(2 * B, dtype=torch.int32, device=DEV)
    x = torch.empty(2 * B, dtype=dtype, device=DEV)
    status = torch.tensor([NONE], dtype=torch.int32, device=DEV)
    off = torch.arange(B + 1, dtype=torch.int64, device=DEV)
    hip_kernels.row_dense_search(tq, off, ta.to(DEV), tb.to(DEV), ta.to(DEV), tb.to(DEV), seg, x, status)
    out = torch.empty(2 * B, L, dtype=dtype, device=DEV)
    hip_kernels.row_event_eval_mapped(out, None, q, seg, x)
    torch.cuda.synchronize()
    assert int(status) == NONE and seg.view(2, B).cpu().tolist() == [list(range(B))] * 2
    assert torch.equal(out.view(2, B, L), sol[1:3])
    assert bool((sol[[0, 3]] == SENTINEL).all())
