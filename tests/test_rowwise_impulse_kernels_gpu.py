"""The device code of `jump_dy` on the MI355X against the CPU oracle (tests/_rowwise_impulse_oracle.py), bit for bit:
`tdeq_row_impulse` on sentinel-bordered buffers whose unselected entries are NaN, and the IMPULSE variant of the per-row
controller on hand-made states — rows prepared to land exactly on their jump point, rows cut short of it, rows on their
last point, inactive rows.  As in tests/test_rowwise_steps_kernels_gpu.py every compared value is an integer, an fp64 value
or a T value formed by the same operations on both sides."""
import ctypes
import math

import numpy as np
import pytest
import torch

from _rowwise_impulse_oracle import ImpulseOracle
from _rowwise_kernels import LONG_NV, SENTINEL, ctrl_for, np_type, row_lengths
from _rowwise_steps_oracle import PointVectors, RowVectors3, StepsOracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
I32 = torch.int32
NAN, INF = math.nan, math.inf
EINVAL = -1


@pytest.fixture(scope="module")
def oracle(oracle_kernels):
    return ImpulseOracle(oracle_kernels)


# -- tdeq_row_impulse ---------------------------------------------------------------------------------------------------------------
class _Placed:
    """CPU tensors copied into views of sentinel-filled device buffers, `offset` elements in (0: 16-byte aligned) and with a
    guard on both sides: `intact()` tells that nothing outside the views was written."""

    def __init__(self, guard=16):
        self.guard, self.bufs = guard, []

    def __call__(self, t, offset):
        n, lo = t.numel(), self.guard + offset
        buf = torch.full((lo + n + self.guard,), SENTINEL, dtype=t.dtype, device="cuda")
        view = buf[lo:lo + n].view(t.shape)
        view.copy_(t)
        self.bufs.append((buf, lo, n))
        return view

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()) for b, lo, n in self.bufs)


N, K, KS = 5, 3, 2                                           # carried rows, the caller's entries, sorted positions
ROW_MAP9 = [7, 2, 8, 0, 4]                                   # a compacted batch: 5 of 9 original rows


@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 1, 0, 7, 1]], ids=["none", "all", "mixed"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [1, 3, 8, 1028])
def test_row_impulse(L, dtype, mask, hip_kernels, oracle):
    """L = 1, 3: scalar elements; 8, 1028: 16-byte elements when both bases allow (1028: more than one workgroup)."""
    g = torch.Generator().manual_seed(L)
    jumped = torch.tensor(mask, dtype=I32)
    for mapped in (False, True):
        n_orig = 9 if mapped else N
        row_map = torch.tensor(ROW_MAP9, dtype=I32) if mapped else None
        orig = ROW_MAP9 if mapped else list(range(N))
        hit = torch.tensor([1, 0, 1, 1, 0], dtype=I32)
        index = torch.randint(0, K, (KS, n_orig), generator=g).to(I32)
        index[int(hit[4]), orig[4]] = -1                     # row 4 ended on a point without an entry: nothing is added
        for dy_rows in (1, n_orig):
            # every entry of dy is NaN but those a row of the mask takes
            dy = torch.full((K, dy_rows, L), NAN, dtype=dtype)
            for r in range(N):
                k = int(index[int(hit[r]), orig[r]])
                if mask[r] and k >= 0:
                    dy[k, orig[r] if dy_rows > 1 else 0] = torch.randn(L, generator=g, dtype=F64).to(dtype)
            y0 = torch.randn(N, L, generator=g, dtype=F64).to(dtype)
            ref = y0.clone()
            oracle.row_impulse(ref, dy, index, hit, jumped, row_map)
            for off_y in (0, 1):
                for off_dy in (0, 1):
                    put = _Placed()
                    y, dy_d = put(y0, off_y), put(dy, off_dy)
                    hip_kernels.row_impulse(y, dy_d, index.to(DEV), hit.to(DEV), jumped.to(DEV),
                                            None if row_map is None else row_map.to(DEV))
                    assert put.intact()
                    got = y.cpu()
                    where = (L, mapped, dy_rows, off_y, off_dy)
                    assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), where
                    assert bool(torch.isfinite(got).all()), where
                    keep = (jumped == 0) | torch.tensor([False, False, False, False, True])
                    assert torch.equal(got[keep].view(torch.uint8), y0[keep].view(torch.uint8)), where
                    assert torch.equal(dy_d.cpu().view(torch.uint8), dy.view(torch.uint8))
            if any(mask):
                assert not torch.equal(ref, y0)


def test_row_impulse_arguments(hip_kernels):
    from torchdiffeq_amd._native import dtype_code
    L, dtype = 8, F32
    y = torch.ones(N, L, dtype=dtype, device=DEV)
    dy = torch.ones(K, N, L, dtype=dtype, device=DEV)
    index = torch.zeros(KS, N, dtype=I32, device=DEV)
    hit, jumped = torch.zeros(N, dtype=I32, device=DEV), torch.ones(N, dtype=I32, device=DEV)
    good = dict(y=y.data_ptr(), dy=dy.data_ptr(), dy_rows=N, dy_index=index.data_ptr(), n_orig=N, jump_hit=hit.data_ptr(),
                jumped=jumped.data_ptr(), row_map=None, n_rows=N, row_len=L, dtype=dtype_code(dtype), stream=None)
    order = ("y", "dy", "dy_rows", "dy_index", "n_orig", "jump_hit", "jumped", "row_map", "n_rows", "row_len", "dtype", "stream")

    def call(**kw):
        a = dict(good, **kw)
        return hip_kernels.lib.tdeq_row_impulse(*[a[name] for name in order])
    assert call() == 0
    for name in ("y", "dy", "dy_index", "jump_hit", "jumped"):
        assert call(**{name: None}) == EINVAL, name
    assert call(dy_rows=2) == EINVAL and call(dy_rows=0) == EINVAL
    assert call(row_len=0) == EINVAL and call(n_rows=-1) == EINVAL
    assert call(n_orig=0, dy_rows=1) == EINVAL and call(n_orig=-1, dy_rows=1) == EINVAL
    for other in (torch.bfloat16, torch.float16):
        assert call(dtype=dtype_code(other)) == EINVAL, other
    assert call(dtype=99) == EINVAL
    assert call(n_rows=0) == 0
    torch.cuda.synchronize()
    assert bool((y == 2).all())                              # the one good call, and nothing else, added the ones


# -- the IMPULSE controller -----------------------------------------------------------------------------------------------------------
ALPHA = (0.2, 0.3, 0.8, 1.0)
DOWN = float(np.nextafter(1.25, 0.0))
SMALL, LARGE = 2.0 ** -20, 4096.0                            # error ratios: growth capped at ifactor / cut to dfactor
# One trial step from t0 = 1 of size 0.25 per row; after an accepted step the next one is prepared from 1.25 with bounds
# [0, 0.25]: it would end at 1.5 exactly.
BASE = dict(active=1, on=0, clip=-3.25, ratio=SMALL, step=(), jump=(), nj=0, end=100.0)
SCENARIOS = [
    dict(jump=(1.5,)),                                       # 0 the prepared step lands on the point: closed rule, on = 2
    dict(jump=(1.4,)),                                       # 1 cut short of it
    dict(on=2, clip=DOWN, jump=(DOWN, 1.4)),                 # 2 an accepted step onto point 0; the next one is cut at point 1
    dict(on=2, clip=DOWN, jump=(DOWN,)),                     # 3 ... onto the row's last point: the index stays
    dict(on=2, clip=DOWN, jump=(1.1, DOWN), nj=1),           # 4 ... onto point 1
    dict(active=0, jump=(1.4,)),                             # 5 an inactive row
    dict(step=(1.5,)),                                       # 6 a STEP point the step lands on: open rule, not cut
    dict(step=(1.5,), jump=(1.75,)),                         # 7 nothing of the jump table in reach
    dict(on=2, clip=DOWN, jump=(DOWN, 1.3), end=1.2),        # 8 jumps and finishes in the same step
    dict(ratio=LARGE, jump=(1.02,)),                         # 9 rejected; the retry is cut
    dict(),                                                  # 10 no point in either table
    dict(step=(1.5,), jump=(1.5 + 2.0 ** -40,)),             # 11 the jump point just behind the landing: not reached
]
EXPECT = {0: (2, None), 1: (2, None), 2: (2, 0), 3: (0, 0), 4: (0, 1), 5: (0, None), 6: (0, None), 7: (0, None), 8: (0, 0),
          9: (2, None), 10: (0, None), 11: (0, None)}     # scenario -> (on_point after the launch, jump_hit written)
HIT_FILL = -5


def _launch(kern, device, B, L, nch, dtype, sign, impulse):
    T = np_type(dtype)
    rows = [dict(BASE, **SCENARIOS[r % len(SCENARIOS)]) for r in range(B)]
    tgrid = np.stack([np.zeros(B), np.array([sc["end"] for sc in rows])])
    state = dict(t0=[1.0] * B, tprev=[0.5] * B, dt=[0.25] * B, active=[sc["active"] for sc in rows], next_out=[1] * B,
                 since=[3] * B, bad_y=[0] * B, n_acc=[7] * B, n_rej=[2] * B)
    rv = RowVectors3(device, B, L, tgrid, order=1, **state)
    ctrl = ctrl_for(ALPHA, 1, sign, T)
    ctrl.min_step, ctrl.max_step = 0.0, 0.25
    part = torch.zeros(3, B, nch, dtype=F64)
    part[0, :, 0] = torch.tensor([L * sc["ratio"] ** 2 for sc in rows], dtype=F64)
    dts = torch.full((B,), SENTINEL, dtype=dtype, device=device)
    times = torch.full((len(ALPHA), B), SENTINEL, dtype=dtype, device=device)
    step, jump = np.full((2, B), INF), np.full((2, B), INF)
    for r, sc in enumerate(rows):
        step[:len(sc["step"]), r] = sc["step"]
        jump[:len(sc["jump"]), r] = sc["jump"]
    pv = PointVectors(device, B, dtype, step, jump, step_count=[len(sc["step"]) for sc in rows],
                      jump_count=[len(sc["jump"]) for sc in rows], next_step=[0 if sc["step"] else -1 for sc in rows],
                      next_jump=[sc["nj"] if sc["jump"] else -1 for sc in rows], on_point=[sc["on"] for sc in rows],
                      clip_t=[sc["clip"] for sc in rows])
    if impulse:
        pv.v["jump_hit"] = torch.full((B,), HIT_FILL, dtype=I32).to(device)
        pv.pts.jump_hit, pv.pts.jump_closed = pv.v["jump_hit"].data_ptr(), 1
    kern.row_control_points(0, part.reshape(-1).to(device), ctrl, rv.st, pv.pts, dts, times, dtype)
    if device != "cpu":
        torch.cuda.synchronize()
    out = rv.cpu()
    out.update(dts=dts.cpu(), times=times.cpu())
    out.update({"pt_" + k: v for k, v in pv.cpu().items() if v is not None})
    return out


def _assert_same(got, ref):
    assert sorted(got) == sorted(ref)
    for name in sorted(ref):
        assert torch.equal(got[name].view(torch.uint8), ref[name].view(torch.uint8)), name     # bit for bit, fillers too


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_impulse_controller(B, form, dtype, sign, hip_kernels, oracle, oracle_kernels):
    if form == "lane":
        L, nch = 3, 1
    else:
        L = row_lengths(dtype, LONG_NV[:1])[0]
        nch = hip_kernels.row_partials(L, dtype)
        assert nch > 1
    ref = _launch(oracle, "cpu", B, L, nch, dtype, sign, True)
    got = _launch(hip_kernels, DEV, B, L, nch, dtype, sign, True)
    _assert_same(got, ref)                                   # every vector, jump_hit and the three status words
    n_jumped = 0
    for r in range(B):
        k = r % len(SCENARIOS)
        on, hit = EXPECT[k]
        assert int(ref["pt_on_point"][r]) == on, (r, k)
        assert int(ref["pt_jump_hit"][r]) == (HIT_FILL if hit is None else hit), (r, k)
        assert int(ref["pt_jumped"][r]) == int(hit is not None), (r, k)
        n_jumped += hit is not None
    assert int(ref["status"][2]) == n_jumped
    if B > 4:
        assert ref["pt_next_jump"][[2, 3, 4]].tolist() == [1, 0, 1]
        assert float(ref["pt_clip_t"][0]) == 1.5 and float(ref["dt"][0]) == 0.25
    # without jump_hit: the outputs of the controller as it was (the open rule; the oracle of the step options states it)
    was = _launch(StepsOracle(oracle_kernels), "cpu", B, L, nch, dtype, sign, False)
    now = _launch(hip_kernels, DEV, B, L, nch, dtype, sign, False)
    _assert_same(now, was)
    assert int(was["pt_on_point"][0]) == 0                   # (the landing row is not cut there)


def test_impulse_controller_arguments(hip_kernels):
    """`jump_hit` without a jump table or without `jump_closed`, and `jump_closed` without `jump_hit`: TDEQ_EINVAL before any
    launch."""
    B, L, dtype = 4, 3, F64
    rv = RowVectors3(DEV, B, L, np.stack([np.zeros(B), np.ones(B)]), order=1, t0=[0.0] * B, dt=[0.1] * B, active=[1] * B,
                     next_out=[1] * B, since=[0] * B)
    ctrl = ctrl_for(ALPHA, 1, 1.0, np_type(dtype))
    part = torch.zeros(3 * B, dtype=F64, device=DEV)
    dts, times = torch.zeros(B, dtype=dtype, device=DEV), torch.zeros(len(ALPHA), B, dtype=dtype, device=DEV)
    hit = torch.zeros(B, dtype=I32, device=DEV)
    from torchdiffeq_amd._native import dtype_code

    def call(pv):
        return hip_kernels.lib.tdeq_row_control_points(0, part.data_ptr(), ctypes.byref(ctrl), ctypes.byref(rv.st),
                                                       ctypes.byref(pv.pts), dts.data_ptr(), times.data_ptr(),
                                                       dtype_code(dtype), None)
    pv = PointVectors(DEV, B, dtype)                         # no jump table
    pv.pts.jump_hit, pv.pts.jump_closed = hit.data_ptr(), 1
    assert call(pv) == EINVAL
    pv = PointVectors(DEV, B, dtype, None, np.full((1, B), 0.5), jump_count=[1] * B, next_jump=[0] * B)
    pv.pts.jump_hit, pv.pts.jump_closed = hit.data_ptr(), 0
    assert call(pv) == EINVAL
    pv.pts.jump_hit, pv.pts.jump_closed = None, 1
    assert call(pv) == EINVAL
    pv.pts.jump_hit, pv.pts.jump_closed = hit.data_ptr(), 1
    assert call(pv) == 0
    torch.cuda.synchronize()
