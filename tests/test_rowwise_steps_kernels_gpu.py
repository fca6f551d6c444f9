"""The per-row step options of csrc/tdeq_kernels_rowwise.hpp on the MI355X against the CPU oracle
(tests/_rowwise_steps_oracle.py): the controller variant on hand-made states that hit every rule of the per-row bounds
and points, bit for bit, and the row select on sentinel-bordered buffers.

Every compared value is an integer, an fp64 value or a T value formed by the same operations on both sides: the error
ratios are powers of two so small or so large that the growth factor is one of its two caps (no result of `pow`, which is
a few ulp apart between the GPU and libm, reaches an output), and a row's sum sits in its first partial."""
import math

import numpy as np
import pytest
import torch

from _rowwise_kernels import (F64_VECTORS, I32_VECTORS, I64_VECTORS, LONG_NV, SENTINEL, RowVectors, ctrl_for, np_type,
                              row_lengths)
from _rowwise_steps_oracle import PointVectors, RowVectors3, StepsOracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
ALPHA = (0.2, 0.3, 0.8, 1.0)
INF, NAN = math.inf, math.nan
UP = float(np.nextafter(1.25, 2.0))
DOWN = float(np.nextafter(1.25, 0.0))
SMALL, LARGE = 2.0 ** -20, 4096.0                            # error ratios: growth capped at ifactor / cut to dfactor

# One trial step from t0 = 1 of size 0.25 per row; `ratio` decides it.  After an accepted step the next one is prepared
# from 1.25 (bounds [0, 0.25]: it would end at 1.5), after a rejected one from 1 with dt = 0.05.
BASE = dict(active=1, dt=0.25, on=0, clip=-3.25, ratio=SMALL, lo=0.0, hi=0.25, step=(), jump=(), ns=0, nj=0, end=100.0, bad=0)
SCENARIOS = [
    dict(step=(5.0,)),                                       # nothing in reach
    dict(step=(1.3,)),                                       # cut at a step point
    dict(jump=(1.4,)),                                       # cut at a jump point
    dict(step=(1.45,), jump=(1.35,)),                        # both inside the step: the jump point wins
    dict(step=(1.3,), jump=(1.4,)),                          # both inside the step, the jump point behind the cut
    dict(step=(1.25, 1.6)),                                  # a point equal to t0
    dict(step=(1.5,)),                                       # a point equal to t0 + dt: not cut
    dict(on=1, clip=UP, step=(UP, 1.4)),                     # an accepted cut step: t0 = the point's bits, the index moves
    dict(on=1, clip=UP, step=(UP,)),                         # ... at the last index: it stays
    dict(on=2, clip=DOWN, jump=(DOWN, 1.45)),                # an accepted step onto a jump point
    dict(),                                                  # a padded row: no point in either table
    dict(active=0, on=0, step=(1.3,), jump=(1.4,)),          # an inactive row
    dict(ratio=LARGE, lo=0.25, step=(1.3,)),                 # forced accept at min_step_r
    dict(hi=0.2, step=(1.1,)),                               # forced reject above max_step_r
    dict(ratio=LARGE, step=(1.03,), jump=(1.04,)),           # rejected by the error; the retry is cut
    dict(end=1.2, step=(1.3,)),                              # the row finishes: no prepared step
    dict(bad=1, jump=(1.3,)),                                # non-finite y: code 3
    dict(on=2, clip=DOWN, jump=(DOWN,), end=1.2),            # jumps and finishes in the same step
]
K = 2


def _rows(B):
    off = 2 if B == 1 else 0                                 # (one row: the cut at a jump point)
    return [dict(BASE, **SCENARIOS[(r + off) % len(SCENARIOS)]) for r in range(B)]


def _tables(rows, vectors):
    B = len(rows)
    step, jump = np.full((K, B), INF), np.full((K, B), INF)
    for r, sc in enumerate(rows):
        step[:len(sc["step"]), r] = sc["step"]
        jump[:len(sc["jump"]), r] = sc["jump"]
    init = dict(step_count=[len(sc["step"]) for sc in rows], jump_count=[len(sc["jump"]) for sc in rows],
                next_step=[sc["ns"] if sc["step"] else -1 for sc in rows],
                next_jump=[sc["nj"] if sc["jump"] else -1 for sc in rows],
                on_point=[sc["on"] for sc in rows], clip_t=[sc["clip"] for sc in rows])
    if vectors:
        init.update(min_step=[sc["lo"] for sc in rows], max_step=[sc["hi"] for sc in rows])
    return step, jump, init


def _launch(kern, device, mode, B, L, nch, dtype, sign, rows, state, sums, vectors, tables=True, plain=False, order=1):
    """One controller launch -> every vector it can write, on the CPU."""
    T = np_type(dtype)
    tgrid = np.stack([np.zeros(B), np.array([sc["end"] for sc in rows])])
    cls = RowVectors if plain else RowVectors3
    rv = cls(device, B, L, tgrid, order=order, **state)
    # (scalar bounds: those of the rows that have the default ones)
    ctrl = ctrl_for(ALPHA, 1, sign, T)
    if not vectors:
        ctrl.min_step, ctrl.max_step = 0.0, 0.25
    part = torch.zeros(3, B, nch, dtype=F64)
    part[:, :, 0] = torch.as_tensor(sums, dtype=F64)
    dts = torch.full((B,), SENTINEL, dtype=dtype, device=device)
    times = torch.full((len(ALPHA), B), SENTINEL, dtype=dtype, device=device)
    if plain:
        kern.row_control(mode, part.reshape(-1).to(device), ctrl, rv.st, dts, times, dtype)
        pv = None
    else:
        step, jump, init = _tables(rows, vectors)
        pv = PointVectors(device, B, dtype, step if tables else None, jump if tables else None,
                          **{k: v for k, v in init.items() if tables or not k.startswith(("step_", "jump_", "next_"))})
        kern.row_control_points(mode, part.reshape(-1).to(device), ctrl, rv.st, pv.pts, dts, times, dtype)
    if device != "cpu":
        torch.cuda.synchronize()
    out = rv.cpu()
    out.update(dts=dts.cpu(), times=times.cpu())
    if pv is not None:
        out.update({"pt_" + k: v for k, v in pv.cpu().items() if v is not None})
    return out


def _assert_same(got, ref):
    assert sorted(got) == sorted(ref)
    for name in sorted(ref):
        assert torch.equal(got[name].view(torch.uint8), ref[name].view(torch.uint8)), name     # bit for bit, fillers too


def _geometry(form, dtype, hip_kernels):
    if form == "lane":
        return [(3, 1)]
    out = [(L, hip_kernels.row_partials(L, dtype)) for L in row_lengths(dtype, LONG_NV[:1])]
    assert all(nch > 1 for _, nch in out)
    return out


@pytest.fixture(scope="module")
def oracle(oracle_kernels):
    return StepsOracle(oracle_kernels)


@pytest.mark.parametrize("vectors", [True, False], ids=["bound_vectors", "scalar_bounds"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_control_points_trial_step(B, form, dtype, sign, vectors, hip_kernels, oracle):
    rows = _rows(B)
    if not vectors:
        rows = [dict(sc, lo=0.0, hi=0.25) for sc in rows]
    for L, nch in _geometry(form, dtype, hip_kernels):
        state = dict(t0=[1.0] * B, tprev=[0.5] * B, dt=[sc["dt"] for sc in rows], active=[sc["active"] for sc in rows],
                     next_out=[1] * B, since=[3] * B, bad_y=[0] * B, n_acc=[7] * B, n_rej=[2] * B)
        sums = torch.tensor([[L * sc["ratio"] ** 2 for sc in rows], [0.0] * B, [float(sc["bad"]) for sc in rows]], dtype=F64)
        ref = _launch(oracle, "cpu", 0, B, L, nch, dtype, sign, rows, state, sums, vectors)
        got = _launch(hip_kernels, DEV, 0, B, L, nch, dtype, sign, rows, state, sums, vectors)
        _assert_same(got, ref)
        # what the oracle must have done, stated once more from the rule, scenario by scenario
        T = np_type(dtype)
        n_jumped = 0
        for r, sc in enumerate(rows):
            accepted = sc["active"] and (sc["ratio"] == SMALL and not sc["dt"] > sc["hi"] or sc["dt"] <= sc["lo"])
            assert int(ref["accepted"][r]) == int(bool(accepted)), r
            if not sc["active"]:
                # untouched: everything but accepted, dts, times, jumped and the jump time
                for name in ("t0", "dt", "n_acc", "n_rej", "since", "pt_on_point", "pt_clip_t"):
                    assert float(ref[name][r]) == {"t0": 1.0, "dt": 0.25, "n_acc": 7, "n_rej": 2, "since": 3,
                                                   "pt_on_point": 0, "pt_clip_t": -3.25}[name], (r, name)
                assert float(ref["dts"][r]) == 0.0
                continue
            if accepted:
                end = sc["clip"] if sc["on"] else 1.25
                assert float(ref["t0"][r]) == end and float(ref["tprev"][r]) == 1.0, r
                jumped = sc["on"] == 2
                n_jumped += jumped
                assert int(ref["pt_jumped"][r]) == int(jumped)
                tj = np.nextafter(T(end), T(end) + T(1)) if jumped else T(end)
                assert float(ref["pt_jump_times"][r]) == float(T(sign) * tj), r
            else:
                assert float(ref["t0"][r]) == 1.0 and int(ref["pt_jumped"][r]) == 0, r
        assert int(ref["status"][2]) == n_jumped
        assert int(ref["status"][0]) == sum(1 for sc in rows if sc["active"] and sc["end"] > 1.25)
        expect_on = {1: 1, 2: 2, 3: 2, 4: 1, 5: 0, 6: 0, 7: 1, 8: 0, 9: 2, 10: 0, 12: 1, 13: 1, 14: 1, 15: 0, 16: 2, 17: 0}
        off = 2 if B == 1 else 0
        for r in range(B):
            k = (r + off) % len(SCENARIOS)
            if k in expect_on and (vectors or k not in (12, 13)):      # (12, 13: the rows the per-row bounds force)
                assert int(ref["pt_on_point"][r]) == expect_on[k], (r, k)
        if B >= 63:
            assert int(ref["pt_next_step"][7]) == 1 and int(ref["pt_next_step"][8]) == 0 and int(ref["pt_next_jump"][9]) == 1
            assert int(ref["status"][1]) == 16 and int(ref["code"][16]) == 3


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_control_points_first_step(B, mode, form, dtype, sign, hip_kernels, oracle):
    """Modes 2 and 3 prepare the first trial step from t0 = 1: dt = 0.4 from the heuristic (order 1: the sqrt path) or 0.47
    given, inside bounds [0, 0.5] — so the points at 1.25 .. 1.45 of the scenarios cut it —, a non-finite dt becomes
    min_step_r, and an inactive row (it never starts) is frozen."""
    rows = [dict(sc, lo=0.125 if r % 5 == 4 else 0.0, hi=0.5, on=5, clip=-3.25) for r, sc in enumerate(_rows(B))]
    for L, nch in _geometry(form, dtype, hip_kernels):
        state = dict(t0=[1.0] * B, active=[sc["active"] for sc in rows], since=[0] * B, bad_y=[0] * B)
        if mode == 3:
            state["dt"] = [INF if r % 5 == 4 else 0.47 for r in range(B)]
            sums = torch.tensor([[0.0] * B, [0.0] * B, [float(sc["bad"]) for sc in rows]], dtype=F64)
        else:
            state.update(h0=[0.004] * B, dt=[2.0 ** -6] * B, bad_y=[sc["bad"] for sc in rows])
            sums = torch.tensor([[L * 2.0 ** -28] * B, [0.0] * B, [0.0] * B], dtype=F64)
        ref = _launch(oracle, "cpu", mode, B, L, nch, dtype, sign, rows, state, sums, True)
        got = _launch(hip_kernels, DEV, mode, B, L, nch, dtype, sign, rows, state, sums, True)
        _assert_same(got, ref)
        assert int(ref["status"][2]) == 0
        for r, sc in enumerate(rows):
            if not sc["active"]:
                assert int(ref["pt_on_point"][r]) == 0 and float(ref["dts"][r]) == 0.0
            elif mode == 3 and r % 5 == 4 and not sc["step"] and not sc["jump"]:
                assert float(ref["dt"][r]) == 0.125, r       # non-finite -> min_step_r
        # untouched by these modes
        assert bool((ref["pt_jumped"] == 9).all()) and bool((ref["pt_jump_times"] == -77.0).all())
        for name in ("tprev", "ratio", "n_acc", "n_rej", "out_lo", "out_hi", "accepted"):
            filler = {"tprev": -3.25, "ratio": -3.25, "n_acc": 5, "n_rej": 5}.get(name, 0)
            assert bool((got[name] == filler).all()), name
        if B >= 63:
            assert [int(ref["pt_on_point"][r]) for r in (1, 2, 3, 5, 6)] == [1, 2, 2, 1, 0]
            assert int(ref["pt_on_point"][4]) == (1 if mode == 2 else 0)      # (mode 3: dt = min_step_r ends before the point)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_control_points_without_points_is_row_control(mode, form, dtype, hip_kernels):
    """Null tables and null bound vectors: every output of `tdeq_row_control` on the same inputs has the same bits.
    Mode 1 (d1 parked in `dt`; with s1 = 0 the heuristic takes h0 = 1e-6, so no result of `pow` reaches an output)
    prepares no step: `on_point`, `jumped` and `jump_times` keep their fillers."""
    B = 65
    rows = [dict(sc, lo=0.0, hi=0.25, on=0) for sc in _rows(B)]
    for L, nch in _geometry(form, dtype, hip_kernels):
        state = dict(t0=[1.0] * B, tprev=[0.5] * B, dt=[0.25] * B, active=[sc["active"] for sc in rows], h0=[0.004] * B,
                     next_out=[1] * B, since=[3] * B, bad_y=[0] * B, n_acc=[7] * B, n_rej=[2] * B)
        sums = torch.tensor([[L * sc["ratio"] ** 2 for sc in rows], [0.0] * B, [float(sc["bad"]) for sc in rows]], dtype=F64)
        plain = _launch(hip_kernels, DEV, mode, B, L, nch, dtype, 1.0, rows, state, sums, False, plain=True)
        got = _launch(hip_kernels, DEV, mode, B, L, nch, dtype, 1.0, rows, state, sums, False, tables=False)
        assert got["status"][:2].tolist() == plain["status"].tolist()
        assert int(got["status"][2]) == 0 and bool((got["pt_on_point"] == 0)[torch.tensor([sc["active"] for sc in rows]) != 0].all())
        for name in F64_VECTORS + I32_VECTORS + I64_VECTORS + ("dts", "times"):
            assert torch.equal(got[name].view(torch.uint8), plain[name].view(torch.uint8)), name
        if mode == 1:
            kept = _launch(hip_kernels, DEV, mode, B, L, nch, dtype, 1.0, [dict(sc, on=5) for sc in rows], state, sums, False,
                           tables=False)
            assert bool((kept["pt_on_point"] == 5).all()) and bool((kept["pt_jumped"] == 9).all())
            assert bool((kept["pt_jump_times"] == -77.0).all())
            assert bool((got["pt_jumped"] == 9).all()) and bool((got["pt_jump_times"] == -77.0).all())


# -- tdeq_row_select ------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("mask", [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 1, 0, 7, 1]], ids=["none", "all", "mixed"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 8, 1028])
def test_row_select(L, dtype, mask, offset, hip_kernels, oracle):
    """L = 3: scalar elements; 8, 1028: 16-byte elements (1028: more than one workgroup for the five rows)."""
    B = 5
    g = torch.Generator().manual_seed(L)
    dst0 = torch.randn(B, L, generator=g, dtype=F64).to(dtype)
    src = torch.randn(B, L, generator=g, dtype=F64).to(dtype)
    m = torch.tensor(mask, dtype=torch.int32)
    src[m == 0] = NAN                                        # a row outside the mask is not read
    put = _Placed(offset)
    dst, src_d = put(dst0), put(src)
    hip_kernels.row_select(dst, src_d, m.to(DEV))
    assert put.intact()
    ref = dst0.clone()
    oracle.row_select(ref, src, m)
    got = dst.cpu()
    assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))
    assert torch.equal(got[m == 0], dst0[m == 0]) and torch.equal(got[m != 0], src[m != 0])
    assert torch.equal(src_d.cpu().view(torch.uint8), src.view(torch.uint8))
