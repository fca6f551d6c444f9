"""The bfloat16 / float16 kernel family on the MI355X, kernel by kernel (csrc/tdeq_kernels_lp.hpp, csrc/tdeq_abi_lp.hpp and
the 16-bit branches of norm_finalize_ctrl_kernel in csrc/tdeq_kernels.hpp) against oracle/lp_kernels.py — the reference's
torch expressions on CPU tensors of the state's type, pinned to the reference by tests/test_lowp_oracle.py:

  a. the error norm on every path: each error-row length of the tableaus, element counts around the 8-element group and
     the reduction chunk, both chunk sizes, the 16-byte and the scalar instantiation, with and without the materialised
     quotient, segmented layouts, the non-finite census, the float16 range case;
  b. the step controller in the state's type (tdeq_error_norm_partial_ctrl with err_partial = NULL) against
     `step_controller` on the oracle's quotient: inline and presummed finalize, inline and device segment table, both time
     signs, both step bounds, `n_norm_seg < n_seg`, `leading_abs`, the step kept on the device;
  c. the look-ahead first stage (lp::sel_kernel) and the captured combine (16-bit tdeq_stage_combine_dev);
  d. out-of-bounds writes of every 16-bit entry point (sentinel-bordered windows, as tests/test_kernel_bounds_gpu.py does
     for fp32 / fp64).

Every elementwise comparison runs on randn inputs and on an edge tensor (`_lowp_kernels.draw_edge`: the float16 subnormal
range, products that overflow the type, +-0, +-inf, NaN): finite and infinite results bit for bit, NaN for NaN.

Out of scope: bfloat16 subnormals (they are float32 subnormals).  The grid-stride branches of lp::map_kernel and
lp::sel_kernel past the grid cap, which need more than 10^8 elements, are in tests/test_grid_stride_gpu.py.  No state here
has more than 3 * 2048 + 17 elements (a layout of S segments occupies S reduction chunks at least, whatever its segments
hold)."""
import math

import numpy as np
import pytest
import torch

from _lowp_kernels import COEFS, DT, Window, bits, dev, draw, draw_edge, kernels, same, to_type
from oracle import lp_kernels as olp
from torchdiffeq_amd import _native
from torchdiffeq_amd.tableaus import ADAPTIVE_TABLEAUS, BOSH3, DOPRI5, DOPRI8, TSIT5, SparseRow

pytestmark = pytest.mark.gpu
CUDA = torch.device("cuda:0")
LOWS = ["bf16", "f16"]
NORM_SIZES = [1, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17]
STREAM_SIZES = [1, 7, 8, 9, 2047, 2049]

# the non-zero error rows of the adaptive tableaus, by length: {2: adaptive_heun / fehlberg2, 4: bosh3, 6: dopri5, 7: tsit5, 9: dopri8}
ERR_ROWS = {}
for _tab in ADAPTIVE_TABLEAUS.values():
    _row = SparseRow.from_dense(_tab.c_error)
    ERR_ROWS.setdefault(len(_row.idx), _row.coef)


def test_error_row_lengths_are_those_the_solvers_launch():
    assert sorted(ERR_ROWS) == [2, 4, 6, 7, 9]


def close(got, ref, rel=1e-12):
    """fp64 sums: equal to `rel`; NaN for NaN, inf for inf."""
    if math.isnan(ref) or math.isinf(ref):
        return math.isnan(got) if math.isnan(ref) else got == ref
    return got == pytest.approx(ref, rel=rel, abs=0.0)


def same_number(got, ref):
    return (math.isnan(got) and math.isnan(ref)) or got == ref


def non_finite(y0, y1):
    return float(((~torch.isfinite(y0.float())) | (~torch.isfinite(y1.float()))).sum())


def plant(y0, y1, chunk_small=1024):
    """inf / NaN into the state rows at the first element, the middle, the start of the last chunk and the last element
    (the `n % 8` tail where there is one) — alternating between y0 and y1."""
    n = y0.numel()
    y0, y1 = y0.clone(), y1.clone()
    where = sorted({0, n // 2, ((n - 1) // chunk_small) * chunk_small, n - 1})
    for j, p in enumerate(where):
        (y0 if j % 2 == 0 else y1)[p] = [math.inf, math.nan, -math.inf][j % 3]
    assert non_finite(y0, y1) == len(where)
    return y0, y1


# ---------------------------------------------------------------------------------------------------------------------
# a. error norm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", sorted(ERR_ROWS))
@pytest.mark.parametrize("low", LOWS)
def test_error_norm_every_path(low, nt):
    dtype, k, coefs, dt = DT[low], kernels(DT[low]), ERR_ROWS[nt], 0.0371
    for n in NORM_SIZES:
        for kind in ("randn", "planted", "edge"):
            y0, y1, *ks = (draw_edge if kind == "edge" else draw)(n, 100 + n, dtype, 2 + nt)
            if kind == "planted":
                y0, y1 = plant(y0, y1)
            q = olp.error_quotient(y0, y1, ks, coefs, dt, 1e-2, 1e-3)
            sumsq, rms, n_bad = olp.norm_terms(q)[0], olp.segment_norm(q), non_finite(y0, y1)
            assert (n_bad > 0) == (kind == "planted") or kind == "edge"
            for offset in (0, 3):       # 3: ONE input off a 16-byte boundary -> the scalar instantiation
                y0d, y1d, *ksd = dev([y0, y1] + ks[:-1]) + dev(ks[-1:], offset)
                for chunk in (1024, 2048):
                    plan = k.make_plan([(0, n, 1e-2, 1e-3)], n, chunk, CUDA)
                    for with_scaled in (True, False):
                        where = (n, kind, offset, chunk, with_scaled)
                        scaled = torch.empty_like(y0d) if with_scaled else None
                        k.error_norm(plan, y0d, y1d, ksd, coefs, dt, scaled_out=scaled)
                        s0, _, bad = k.read_norms(plan)
                        if with_scaled:
                            same(scaled, q, where)
                        assert close(s0[0], sumsq), (where, s0[0], sumsq)
                        assert same_number(plan.rms0[0], rms), (where, plan.rms0[0], rms)
                        assert bad == [n_bad], (where, bad, n_bad)
                        if n == 1:
                            assert same_number(plan.abs0[0], float(q.abs()))


@pytest.mark.parametrize("sizes", [[1, 1500, 37], [8, 1024, 1, 2049]], ids=["1-1500-37", "8-1024-1-2049"])
@pytest.mark.parametrize("low", LOWS)
def test_error_norm_segmented_layouts(low, sizes):
    """Segments with their own tolerances, a one-element segment first and not first, padding between them: the padding
    of the inputs is never read (it holds NaN) and the padding of the quotient is zero-filled."""
    dtype, k = DT[low], kernels(DT[low])
    tols = [(1e-2, 1e-3), (2e-2, 1e-3), (1e-1, 1e-2), (5e-2, 2e-3)][:len(sizes)]
    for chunk in (1024, 2048):
        offs, total = [], 0
        for s in sizes:
            offs.append(total)
            total += -(-s // chunk) * chunk
        live = torch.zeros(total, dtype=torch.bool)
        for o, s in zip(offs, sizes):
            live[o:o + s] = True
        plan = k.make_plan([(o, s, rt, at) for o, s, (rt, at) in zip(offs, sizes, tols)], total, chunk, CUDA)
        for nt in (2, 7):
            coefs = ERR_ROWS[nt]
            for kind in ("planted", "edge"):
                y0, y1, *ks = (draw_edge if kind == "edge" else draw)(total, 7 + nt, dtype, 2 + nt)
                if kind == "planted":
                    for o, s in zip(offs, sizes):
                        y0[o:o + s], y1[o:o + s] = plant(y0[o:o + s], y1[o:o + s])
                padded = [torch.where(live, t, torch.full_like(t, math.nan)) for t in [y0, y1] + ks]
                for offset in (0, 3):
                    y0d, y1d, *ksd = dev(padded[:1], offset) + dev(padded[1:])
                    scaled = torch.full((total,), math.nan, dtype=dtype, device="cuda")
                    k.error_norm(plan, y0d, y1d, ksd, coefs, 0.05, scaled_out=scaled)
                    s0, _, bad = k.read_norms(plan)
                    got = scaled.cpu()
                    for i, (o, s, (rt, at)) in enumerate(zip(offs, sizes, tols)):
                        where, sl = (chunk, nt, kind, offset, i), slice(o, o + s)
                        q = olp.error_quotient(y0[sl], y1[sl], [kk[sl] for kk in ks], coefs, 0.05, rt, at)
                        same(got[sl], q, where)
                        assert close(s0[i], olp.norm_terms(q)[0]), (where, s0[i])
                        assert same_number(plan.rms0[i], olp.segment_norm(q)), (where, plan.rms0[i])
                        assert bad[i] == non_finite(y0[sl], y1[sl]), (where, bad[i])
                        if s == 1:
                            assert same_number(plan.abs0[i], float(q.abs())), where
                    assert bool((bits(got)[~live] == 0).all()), (chunk, nt, kind, offset, "padding of the quotient not zero")
                    k.error_norm(plan, y0d, y1d, ksd, coefs, 0.05)          # the sums alone: the same words
                    s0_plain, _, bad_plain = k.read_norms(plan)
                    assert np.array_equal(s0_plain, s0, equal_nan=True) and bad_plain == bad


def test_error_norm_float16_sum_of_squares_beyond_the_type():
    """Every quotient about 200 at n = 5000: the sum of squares (2e8) is beyond float16's range, the mean (4e4) is not —
    the norm is 200 in the type, from `read_norms` and from the device controller alike."""
    dtype, k, n = torch.float16, kernels(torch.float16), 5000
    atol = to_type(1e-3, dtype)
    err = (200 * atol) * torch.where(draw(n, 5, dtype, 1)[0] < 0, -1.0, 1.0).to(dtype)
    zero = torch.zeros(n, dtype=dtype)
    q = olp.error_quotient(zero, zero, [err], (1.0,), 1.0, 0.0, 1e-3)
    assert 199 < float(q.abs().min()) and float(q.abs().max()) < 201 and olp.norm_terms(q)[0] > 65504 * 1000
    assert olp.segment_norm(q) == float(q.abs().pow(2).mean().sqrt()) == 200.0
    zd, ed = dev([zero, err])
    plan = k.make_plan([(0, n, 0.0, 1e-3)], n, 1024, CUDA)
    k.error_norm(plan, zd, zd, [ed], (1.0,), 1.0)
    s0, _, bad = k.read_norms(plan)
    assert close(s0[0], olp.norm_terms(q)[0]) and bad == [0.0] and plan.rms0[0] == 200.0
    c = make_ctrl(DOPRI5, dtype, 0.3, 0.0371)
    times = torch.empty(c.n_times, dtype=dtype, device="cuda")
    k.error_norm_ctrl(plan, zd, zd, [ed], (1.0,), 1.0, c, times)
    accept, _, ratio, _ = k.read_ctrl(plan)
    assert ratio == 200.0 and not accept


# ---------------------------------------------------------------------------------------------------------------------
# b. the step controller in the state's type
# ---------------------------------------------------------------------------------------------------------------------
def make_ctrl(tab, dtype, t0, dt, sign=1.0, lo=0.0, hi=math.inf, n_norm_seg=1, leading_abs=0):
    """`tdeq_step_ctrl` as solvers/adaptive.py fills it for a state of `dtype`: abscissae rounded to the type."""
    c = _native.step_ctrl([float(to_type(a, dtype)) for a in tab.alpha], [a == 1.0 for a in tab.alpha], tab.order,
                          0.9, 10.0, 0.2, lo, hi, sign, n_norm_seg)
    c.t0, c.dt, c.leading_abs = t0, dt, leading_abs
    return c


NINE = [1, 300, 8, 1025, 37, 1, 700, 9, 64]
TWENTY = [5, 1, 130, 8, 17, 33, 2, 1024, 9, 1] * 2
CTRL_CONFIGS = {
    # n_seg 1, 3, 4: the inline finalize + controller; 9: presummed, inline segment table; 20: presummed, device table
    "1seg": dict(sizes=[1031], tab=DOPRI5, t0=0.37, dt=0.0123),
    "1seg_decreasing": dict(sizes=[2049], tab=DOPRI8, t0=-2.5, dt=0.31, sign=-1.0),
    "decreasing_from_zero": dict(sizes=[37], tab=DOPRI5, t0=0.0, dt=0.0123, sign=-1.0),        # stage times of -0
    "above_max_step": dict(sizes=[37], tab=TSIT5, t0=1e3, dt=0.5, lo=0.1, hi=0.4),            # forced reject
    "at_min_step": dict(sizes=[37], tab=BOSH3, t0=0.0, dt=0.05, lo=0.05, hi=1.0),             # forced accept
    "3seg_leading_rms": dict(sizes=[1, 1500, 37], tab=DOPRI8, t0=-2.5, dt=0.31, sign=-1.0, which=0),
    "3seg_leading_abs": dict(sizes=[1, 1500, 37], tab=DOPRI8, t0=-2.5, dt=0.31, sign=-1.0, which=0, leading_abs=1),
    "3seg_two_in_norm": dict(sizes=[1, 1500, 37], tab=TSIT5, t0=0.37, dt=0.0123, which=1, n_norm_seg=2),
    "4seg_single_not_first": dict(sizes=[8, 1024, 1, 2049], tab=BOSH3, t0=0.37, dt=0.0123, which=2),
    "9seg": dict(sizes=NINE, tab=TSIT5, t0=-2.5, dt=0.31, sign=-1.0, which=5),
    "9seg_five_in_norm": dict(sizes=NINE, tab=DOPRI5, t0=0.37, dt=0.0123, which=3, n_norm_seg=5),
    "9seg_leading_abs": dict(sizes=NINE, tab=BOSH3, t0=0.37, dt=0.0123, which=0, leading_abs=1),
    "20seg": dict(sizes=TWENTY, tab=DOPRI5, t0=0.37, dt=0.0123, which=17),
    "1seg_step_on_device": dict(sizes=[1031], tab=DOPRI5, t0=0.37, dt=0.25, in_dev=True),
    "9seg_step_on_device": dict(sizes=NINE, tab=DOPRI8, t0=-2.5, dt=0.25, sign=-1.0, which=6, in_dev=True),
}


def ratio_values(dtype, atol_T, single):
    """Error values k with k / T(atol) = the ratio named: exact ones, not drawn ones."""
    one_up = torch.nextafter(atol_T, atol_T + 1)
    vals = {"zero": torch.zeros((), dtype=dtype), "tiny": atol_T * 2.0 ** -10, "one": atol_T, "one_up": one_up,
            "thirty": to_type(30 * float(atol_T), dtype), "inf": torch.tensor(torch.finfo(dtype).max, dtype=dtype),
            "nan": torch.tensor(math.nan, dtype=dtype)}
    if single:
        # a one-element segment: |x| and sqrt(fl(|x|^2)) agree wherever the square is a normal number of the type (its
        # rounding error is halved by the root); they part where the square overflows — |x| = 300 in float16, 2^70 in bfloat16
        v = to_type((300.0 if dtype == torch.float16 else 2.0 ** 70) * float(atol_T), dtype)
        q = (v / atol_T).reshape(1)
        assert math.isinf(olp.segment_norm(q, False)) and olp.segment_norm(q, True) == float(q)
        vals["abs_is_not_rms"] = v
    return vals


@pytest.mark.parametrize("config", list(CTRL_CONFIGS))
@pytest.mark.parametrize("low", LOWS)
def test_device_controller_in_the_states_type(low, config):
    cfg = dict(sign=1.0, lo=0.0, hi=math.inf, which=0, n_norm_seg=None, leading_abs=0, in_dev=False)
    cfg.update(CTRL_CONFIGS[config])
    dtype, k, sizes, which, chunk = DT[low], kernels(DT[low]), cfg["sizes"], cfg["which"], 1024
    n_seg = len(sizes)
    n_norm_seg = cfg["n_norm_seg"] or n_seg
    t0, dt, sign, in_dev = cfg["t0"], cfg["dt"], cfg["sign"], cfg["in_dev"]
    atols = [1e-3 * (1 + s % 3) for s in range(n_seg)]
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += -(-s // chunk) * chunk
    plan = k.make_plan([(o, s, 0.0, a) for o, s, a in zip(offs, sizes, atols)], total, chunk, CUDA)
    assert (plan.hip.segs_dev is not None) == (n_seg > 16)
    zero = torch.zeros(total, dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(len(config))
    signs = [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0).to(dtype) for s in sizes]
    # the norm launch's own step size: 1 (q = k / T(atol)) — or, with the step on the device, sign * T(dt) from ctrl_dev[1],
    # a power of two here, undone exactly by the factor 1 / dt on k
    dt_T = float(to_type(dt, dtype))
    norm_dt, unscale = (sign * dt_T, 1.0 / dt_T) if in_dev else (1.0, 1.0)
    assert not in_dev or math.frexp(dt_T)[0] == 0.5
    for case, value in ratio_values(dtype, to_type(atols[which], dtype), sizes[which] == 1).items():
        rows = []
        for s in range(n_seg):
            a_T = to_type(atols[s], dtype)
            if s == which:
                v = value
            elif s >= n_norm_seg:
                v = torch.tensor(math.nan, dtype=dtype) if s % 2 else to_type(1000 * float(a_T), dtype)   # must be ignored
            else:
                big = case in ("inf", "nan", "abs_is_not_rms")
                v = (a_T if big else value * (a_T / to_type(atols[which], dtype))) * 0.125     # an eighth of the ratio
            rows.append(signs[s] * (v * unscale))
        kbuf = torch.full((total,), math.nan, dtype=dtype)          # padding: never read
        for o, s, r in zip(offs, sizes, rows):
            kbuf[o:o + s] = r
        c = make_ctrl(cfg["tab"], dtype, t0, dt, sign, cfg["lo"], cfg["hi"], n_norm_seg, cfg["leading_abs"])
        if in_dev:      # the trial step lives in ctrl_dev {-, sign * T(dt), t0, dt}; the host's copies are decoys
            plan.ctrl_dev.copy_(torch.tensor([0.0, sign * dt_T, t0, dt], dtype=torch.float64))
            c.t0, c.dt = 99.0, 77.0
        times = torch.full((c.n_times,), math.nan, dtype=dtype, device="cuda")
        k.error_norm_ctrl(plan, zero, zero, [kbuf.cuda()], (1.0,), 5.0 if in_dev else 1.0, c, times, state_in_dev=in_dev)
        words = k._hip._read_out(plan.hip)         # [sums | - | non-finite | accept, dt_next, ratio, t0']
        sums, bad = words[:n_seg], words[2 * n_seg:3 * n_seg]
        accept, dt_next, ratio, t0_next = words[3 * n_seg:3 * n_seg + 4]
        ctrl_dev = plan.ctrl_dev.cpu().tolist()
        # the oracle: quotient, per-segment norms, controller
        norms = []
        for s in range(n_seg):
            z = torch.zeros(sizes[s], dtype=dtype)
            q = olp.error_quotient(z, z, [rows[s]], (1.0,), norm_dt, 0.0, atols[s])
            norms.append(olp.segment_norm(q, leading_abs=bool(cfg["leading_abs"]) and s == 0))
            ref_sum = float(q.abs()) if sizes[s] == 1 else olp.norm_terms(q)[0]
            assert close(sums[s], ref_sum), (case, s, sums[s], ref_sum)
        assert bad == [0.0] * n_seg
        c.t0, c.dt = t0, dt
        o_accept, o_dt_next, o_ratio, o_t0_next, _, _ = olp.step_controller(norms, t0, dt, c, dtype)
        where = (case, words[3 * n_seg:], (o_accept, o_dt_next, o_ratio, o_t0_next))
        assert same_number(ratio, o_ratio), where
        assert (accept != 0.0) == o_accept and accept in (0.0, 1.0), where
        assert t0_next == o_t0_next, where
        if math.isnan(o_dt_next):
            assert math.isnan(dt_next), where
        else:       # the GPU's pow against libm's: the 4 ulp of fp64 tests/test_lookahead.py grants
            assert abs(dt_next - o_dt_next) <= 4 * np.spacing(abs(o_dt_next)), where
        # what the construction is for: ratio exactly 1 accepts, one unit in the last place above it rejects
        exact = {"zero": 0.0, "one": 1.0, "one_up": 1.0 + float(torch.finfo(dtype).eps), "inf": math.inf}
        assert case not in exact or ratio == exact[case], where
        assert case != "nan" or math.isnan(ratio), where
        if config == "above_max_step":
            assert accept == 0.0, where
        elif config == "at_min_step":
            assert accept == 1.0, where
        elif case != "abs_is_not_rms":
            assert (accept != 0.0) == (case in ("zero", "tiny", "one")), where
        # the device's words: {accept, sign * T(dt'), t0', dt'} with dt' the step the next trial takes
        o_dt_new = min(max(o_dt_next if math.isfinite(o_dt_next) else cfg["lo"], cfg["lo"]), cfg["hi"])
        assert ctrl_dev[0] == accept and ctrl_dev[2] == t0_next, where
        assert abs(ctrl_dev[3] - o_dt_new) <= 4 * np.spacing(abs(o_dt_new)), (where, ctrl_dev)
        assert ctrl_dev[1] == sign * float(to_type(ctrl_dev[3], dtype)), (where, ctrl_dev)
        # stage times: the oracle's on the device's own (t0', dt') — pow does not enter
        same(times, olp.stage_times(ctrl_dev[2], ctrl_dev[3], c, dtype), where)


# ---------------------------------------------------------------------------------------------------------------------
# c. look-ahead first stage, captured combine
# ---------------------------------------------------------------------------------------------------------------------
def step_sizes(dtype):
    return [float(to_type(0.0371, dtype)), -float(to_type(0.25, dtype))]


@pytest.mark.parametrize("low", LOWS)
def test_stage_combine_sel_bit_exact(low):
    dtype, k = DT[low], kernels(DT[low])
    for n in STREAM_SIZES:
        plan = k.make_plan([(0, n, 1e-2, 1e-3)], n, 1024, CUDA)
        for kind in ("randn", "edge"):
            ts = (draw_edge if kind == "edge" else draw)(n, 7 + n, dtype, 4)
            for offset in (0, 3):
                td = dev(ts, offset)
                for accept in (0.0, 1.0):
                    for dt_T in step_sizes(dtype):
                        where = (n, kind, offset, accept, dt_T)
                        plan.ctrl_dev[:2].copy_(torch.tensor([accept, dt_T], dtype=torch.float64))
                        out = dev([torch.zeros(n, dtype=dtype)], offset)[0]
                        k.stage_combine_sel(out, td[0], td[1], td[2], td[3], 0.2, plan)
                        same(out, olp.stage_combine_sel(ts[0], ts[1], ts[2], ts[3], 0.2, accept, dt_T), where)
                        # ... and the host-driven combine on the selected pair with the host's step size
                        ref = torch.empty_like(out)
                        ysel, fsel = (td[0], td[1]) if accept else (td[2], td[3])
                        k.stage_combine(ref, ysel, [fsel], (0.2,), dt_T)
                        same(out, ref.cpu(), where)


@pytest.mark.parametrize("nt", [1, 6, 13])
@pytest.mark.parametrize("low", LOWS)
def test_stage_combine_dev_bit_exact(low, nt):
    dtype, k, coefs = DT[low], kernels(DT[low]), COEFS[:nt]
    for n in STREAM_SIZES:
        plan = k.make_plan([(0, n, 1e-2, 1e-3)], n, 1024, CUDA)
        for kind in ("randn", "edge"):
            y0, *ks = (draw_edge if kind == "edge" else draw)(n, 11 + n, dtype, 1 + nt)
            for offset in (0, 3):
                y0d, *ksd = dev([y0] + ks, offset)
                for dt_T in step_sizes(dtype):
                    where = (n, kind, offset, dt_T)
                    plan.ctrl_dev[:2].copy_(torch.tensor([1.0, dt_T], dtype=torch.float64))
                    out = dev([torch.zeros(n, dtype=dtype)], offset)[0]
                    k.stage_combine_dev(out, None, y0d, ksd, coefs, None, plan)
                    same(out, olp.stage_combine(y0, ks, coefs, dt_T), where)
                    ref = torch.empty_like(out)
                    k.stage_combine(ref, y0d, ksd, coefs, dt_T)
                    same(out, ref.cpu(), where)


# ---------------------------------------------------------------------------------------------------------------------
# d. write bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 3], ids=["aligned", "off1", "off3"])
@pytest.mark.parametrize("low", LOWS)
def test_entry_points_write_only_their_window(low, offset):
    """Every output of every 16-bit entry point sits in a sentinel-bordered window: the borders stay, the payload is
    written in full.  (A single-segment quotient ends at n: the words after it stay, whatever the chunk.)"""
    dtype, k = DT[low], kernels(DT[low])
    failures = []
    for n in [1, 7, 8, 9, 2047, 2048, 2049, 4099]:
        y0, y1, *ks = dev(draw(n, 40 + n, dtype, 16))
        plan = k.make_plan([(0, n, 1e-2, 1e-3)], n, 1024, CUDA)
        plan.ctrl_dev.copy_(torch.tensor([1.0, float(to_type(0.0371, dtype)), 0.3, 0.0371], dtype=torch.float64))
        W = lambda rows=1: Window(n, dtype, offset, rows)

        def run(name, wins, launch):
            launch()
            torch.cuda.synchronize()
            for i, w in enumerate(wins):
                if not (w.intact() and w.written()):
                    failures.append((n, f"{name}[{i}]", "borders" if not w.intact() else "payload"))

        for nt in (1, 2, 7, 14):
            w = W()
            run(f"stage_combine<{nt}>", [w], lambda: k.stage_combine(w.t, y0, ks[:nt], COEFS[:nt], 0.1))
            w = W()
            run(f"stage_combine_dev<{nt}>", [w], lambda: k.stage_combine_dev(w.t, None, y0, ks[:nt], COEFS[:nt], None, plan))
        w, wt = W(), Window(6, dtype, offset)
        run("stage_combine_fill", [w, wt], lambda: k.stage_combine_fill(w.t, y0, ks[:1], COEFS[:1], 0.1, wt.t,
                                                                        [0.3, 0.31, 0.32, 0.33, 0.34, 0.35]))
        w0, w1 = W(), W()
        run("stage_combine_err", [w0, w1], lambda: k.stage_combine_err(w0.t, w1.t, y0, ks[:6], COEFS[:6], COEFS[6:12], 0.1))
        for accept in (0.0, 1.0):
            plan.ctrl_dev[:1].fill_(accept)
            w = W()
            run(f"stage_combine_sel<{accept}>", [w], lambda: k.stage_combine_sel(w.t, y0, ks[0], y1, ks[1], 0.2, plan))
        for nt in (2, 9):
            w = W()
            run(f"error_norm<{nt}>", [w], lambda: k.error_norm(plan, y0, y1, ks[:nt], COEFS[:nt], 0.1, scaled_out=w.t))
            k.read_norms(plan)
        w0, w1 = W(), W()
        run("init_scaled<0>", [w0, w1], lambda: k.init_scaled(plan, 0, ks[0], ks[1], y0, w0.t, w1.t))
        w = W()
        run("init_scaled<1>", [w], lambda: k.init_scaled(plan, 1, ks[0], ks[1], y0, w.t))
        dense = (y0, y1, ks[0], ks[6], ks[1:6], COEFS[:5], 0.1)
        w = W()
        run("dense_eval", [w], lambda: k.dense_eval(w.t, *dense, 0.37))
        xs = [0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0]
        for m in (2, 3, 5, 6, 7):
            w = W(m)
            run(f"dense_eval_multi<{m}>", [w], lambda: k.dense_eval_multi(w.t, *dense, xs[:m]))
            # a dropped output (fewer rows than the launch's four) aliases the first row of its group: every row must
            # still be the single-row launch's
            for r in range(m):
                single = torch.empty(n, dtype=dtype, device="cuda")
                k.dense_eval(single, *dense, xs[r])
                if not torch.equal(bits(w.t[r]), bits(single)):
                    failures.append((n, f"dense_eval_multi<{m}>", f"row {r} differs from the single-row launch"))
        w = W(5)
        run("interp_fit", [w], lambda: k.interp_fit(w.t, *dense))
        for stage in (1, 2, 3, 4):
            w = W()
            run(f"rk4_stage{stage}", [w], lambda: k.rk4_stage(stage, w.t, y0, ks[0], ks[1] if stage > 1 else None,
                                                              ks[2] if stage > 2 else None, ks[3] if stage > 3 else None, 0.1))
        w = W()
        run("lerp", [w], lambda: k.lerp(w.t, y0, y1, 0.3))
        for mode, nt in ((1, 1), (0, 1), (0, 4)):
            w = W()
            run(f"fixed_stage<{mode},{nt}>", [w], lambda: k.fixed_stage(mode, w.t, y0, ks[:nt], [0.25, 0.1, 0.75, 0.5][:nt], 0.1))
        for nt in (1, 8):
            w = W()
            run(f"weighted_sum<{nt}>", [w], lambda: k.weighted_sum(w.t, ks[:nt], [0.1 * (j + 1) for j in range(nt)]))
    assert not failures, failures
