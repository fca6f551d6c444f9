"""The CPU twins of the per-element-tolerance kernels (oracle_error_norm_vec, oracle_error_norm_vec_ctrl,
oracle_init_norms_vec) — no GPU.

  * the twins against the reference's expressions evaluated literally by ATen on the CPU (misc.py:80-82, :50-56, 68), on
    every segmented layout the GPU kernel tests use, with NaN in every padding element;
  * the controller's ratio type: fp64 for either state type (an fp32-rounded ratio would accept a step the reference
    rejects), seminorm, the device-resident trial step (`state_in_dev`);
  * the product's host logic on the fused route: with the twins in place the solver takes error_norm_vec[_ctrl] and
    init_norms_vec under the CPU backend too, never the raw-error route.
tests/test_vec_tol_kernels_gpu.py compares the HIP kernels with these twins."""
import math

import numpy as np
import pytest
import torch

import torchdiffeq_amd as tda
from torchdiffeq_amd.tableaus import DOPRI5

from _cases import TUPLE_TOL_LIST_FORMS, T, load, rel_err
from _vec_tol_cases import (COEFS, DT, LAYOUTS, Inputs, Layout, aten_error_sums, aten_init_sums, band_inputs, close,
                            ctrl_rows, step_ctrl)

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
FORMS = ["both", "rtol_only", "atol_only"]


def _np(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


# ---------------------------------------------------------------------------------------------------------------------
# the twins against ATen
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_terms", [1, 6, 7, 14])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_error_norm_vec_twin_equals_the_references_expression(oracle_kernels, name, dtype, form, n_terms):
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=n_terms)
    rtol, atol = x.tolerances(form)
    plan = lay.plan(oracle_kernels)
    oracle_kernels.error_norm_vec(plan, x.y0, x.y1, x.ks[:n_terms], COEFS[:n_terms], DT, rtol, atol)
    sums, _, bad = oracle_kernels.read_norms(plan)
    want = aten_error_sums(lay, x.y0, x.y1, x.ks[:n_terms], COEFS[:n_terms], DT, rtol, atol)
    assert all(math.isfinite(v) and v > 0 for v in want)
    assert close(sums, want), (sums, want)
    assert bad == [0.0] * lay.n_seg


@pytest.mark.parametrize("n_rest", [0, 1, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["one_1031", "three", "five", "seventeen"])
def test_error_norm_vec_twin_continues_a_partial_row(oracle_kernels, name, dtype, form, n_rest):
    """`partial` + the remaining 0 / 1 / 2 stages: against ATen continuing the same partial row, and bit-equal to the whole
    row when the partial is the row's own leading run (stage_combine_err's left-to-right sum)."""
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=10 + n_rest)
    rtol, atol = x.tolerances(form)
    plan = lay.plan(oracle_kernels)
    n_lead = 6 - n_rest
    err_coefs = COEFS[1:7]
    y1, part = torch.empty_like(x.y0), torch.empty_like(x.y0)
    oracle_kernels.stage_combine_err(y1, part, x.y0, x.ks[:n_lead], COEFS[:n_lead], err_coefs[:n_lead], DT)
    ks, cf = x.ks[n_lead:6], err_coefs[n_lead:]
    oracle_kernels.error_norm_vec(plan, x.y0, y1, ks, cf, DT, rtol, atol, partial=part)
    split = oracle_kernels.read_norms(plan)
    assert close(split[0], aten_error_sums(lay, x.y0, y1, ks, cf, DT, rtol, atol, partial=part))
    oracle_kernels.error_norm_vec(plan, x.y0, y1, x.ks[:6], err_coefs, DT, rtol, atol)
    whole = oracle_kernels.read_norms(plan)
    assert split[0] == whole[0] and split[2] == whole[2] == [0.0] * lay.n_seg


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_init_norms_vec_twin_equals_the_references_expression(oracle_kernels, name, dtype, form, mode):
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=20 + mode)
    rtol, atol = x.tolerances(form)
    plan = lay.plan(oracle_kernels)
    plan.out.fill_(-1.0)
    oracle_kernels.init_norms_vec(plan, mode, x.a, x.b, x.yscale, rtol, atol)
    s0, s1, bad = oracle_kernels.read_norms(plan)
    w0, w1 = aten_init_sums(lay, mode, x.a, x.b, x.yscale, rtol, atol)
    assert close(s0, w0), (s0, w0)
    if mode == 0:
        assert close(s1, w1), (s1, w1)
    else:
        assert s1 == [-1.0] * lay.n_seg         # one sum: the second block is not written
    assert bad == [0.0] * lay.n_seg


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_poisoned_padding_is_a_real_guard(oracle_kernels, dtype):
    """The padding of every stream is NaN and the sums are finite (above).  The same NaN in ONE VALID element of any stream
    does reach the sum of its segment — and only that one: so a read of padding could not go unnoticed."""
    lay = Layout("five")
    x = Inputs(lay, dtype, seed=3)
    plan = lay.plan(oracle_kernels)
    assert all(bool(torch.isnan(s[~lay.valid]).all()) and bool(torch.isfinite(s[lay.valid]).all())
               for s in (*x.streams(), x.rtol_v, x.atol_v))
    streams = {"y0": x.y0, "y1": x.y1, "k3": x.ks[3], "rtol_v": x.rtol_v, "atol_v": x.atol_v}
    for seg, (which, s) in zip(range(lay.n_seg), streams.items()):
        i = lay.index(seg, lay.numels[seg] - 1)          # the LAST valid element: next to the padding
        keep = s[i].clone()
        s[i] = float("nan")
        oracle_kernels.error_norm_vec(plan, x.y0, x.y1, x.ks[:7], COEFS[:7], DT, x.rtol_v, x.atol_v)
        sums, _, bad = oracle_kernels.read_norms(plan)
        # (fmax drops a NaN of one of y0 / y1 as the kernel's does: there the census is what reports it)
        hit = [math.isnan(v) for v in sums] if which not in ("y0", "y1") else [b != 0 for b in bad]
        assert hit == [q == seg for q in range(lay.n_seg)], (which, sums, bad)
        s[i] = keep
    for seg, (which, s) in enumerate({"a": x.a, "b": x.b, "yscale": x.yscale}.items()):
        i = lay.index(seg + 1, 0)                        # the FIRST valid element: next to the previous segment's padding
        keep = s[i].clone()
        s[i] = float("nan")
        oracle_kernels.init_norms_vec(plan, 0, x.a, x.b, x.yscale, x.rtol_v, x.atol_v)
        s0, s1, bad = oracle_kernels.read_norms(plan)
        nan0, nan1 = [math.isnan(v) for v in s0], [math.isnan(v) for v in s1]
        only = [q == seg + 1 for q in range(lay.n_seg)]
        assert (nan0, nan1) == {"a": (only, [False] * 5), "b": ([False] * 5, only), "yscale": (only, only)}[which]
        assert [b != 0 for b in bad] == (only if which == "yscale" else [False] * 5)
        s[i] = keep


def test_twins_refuse_what_the_abi_refuses(oracle_kernels):
    lay = Layout("one_1031")
    x = Inputs(lay, torch.float64)
    plan = lay.plan(oracle_kernels)
    tn = torch.empty(7, dtype=torch.float64)
    c = step_ctrl(0.0, 0.1, 5, DOPRI5)
    with pytest.raises(RuntimeError):           # two 0-dim tolerances: the scalar-tolerance kernels' business
        oracle_kernels.error_norm_vec(plan, x.y0, x.y1, x.ks[:2], COEFS[:2], DT, 1e-3, 1e-6)
    with pytest.raises(RuntimeError):
        oracle_kernels.error_norm_vec_ctrl(plan, x.y0, x.y1, x.ks[:2], COEFS[:2], DT, 1e-3, 1e-6, c, tn)
    with pytest.raises(RuntimeError):
        oracle_kernels.init_norms_vec(plan, 0, x.a, x.b, x.yscale, 1e-3, 1e-6)
    with pytest.raises(RuntimeError):           # no stages and no partial row
        oracle_kernels.error_norm_vec(plan, x.y0, x.y1, [], [], DT, x.rtol_v, 1e-6)
    with pytest.raises(RuntimeError):
        oracle_kernels.error_norm_vec_ctrl(plan, x.y0, x.y1, [], [], DT, x.rtol_v, 1e-6, c, tn)
    oracle_kernels.error_norm_vec(plan, x.y0, x.y1, [], [], DT, x.rtol_v, 1e-6, partial=x.ks[0])     # ... with one: fine


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_tolerances_as_the_reference_has_them(oracle_kernels, dtype):
    """0 / 0, x / 0, an infinite state, a subnormal tolerance: the twin's sums are ATen's, NaN and inf included."""
    lay = Layout("three")
    x = Inputs(lay, dtype, seed=5)
    plan = lay.plan(oracle_kernels)
    ks, cf = x.ks[:7], COEFS[:7]

    def run():
        oracle_kernels.error_norm_vec(plan, x.y0, x.y1, ks, cf, DT, 0.0, x.atol_v)
        sums, _, bad = oracle_kernels.read_norms(plan)
        assert close(sums, aten_error_sums(lay, x.y0, x.y1, ks, cf, DT, 0.0, x.atol_v)), sums
        return sums, bad
    i = lay.index(1, 17)
    # atol = 0, y0 = y1 = 0, e = 0 (all k zero there): 0 / 0
    x.atol_v[i] = 0.0
    x.y0[i] = x.y1[i] = 0.0
    saved = [k[i].clone() for k in ks]
    for k in ks:
        k[i] = 0.0
    sums, bad = run()
    assert math.isnan(sums[1]) and math.isfinite(sums[0]) and math.isfinite(sums[2]) and bad == [0.0] * 3
    # atol = 0 with e != 0: inf
    for k, v in zip(ks, saved):
        k[i] = v
    sums, bad = run()
    assert sums[1] == math.inf and math.isfinite(sums[0]) and math.isfinite(sums[2]) and bad == [0.0] * 3
    # a subnormal atol with y = 0: e / 5e-324 overflows to inf in fp64, its square too
    x.atol_v[i] = 5e-324
    sums, bad = run()
    assert sums[1] == math.inf and bad == [0.0] * 3
    # y1 = inf: counted in its segment only; tol = inf, the element adds 0
    x.atol_v[i] = 1e-6
    x.y1[lay.index(2, 1024)] = float("inf")
    oracle_kernels.error_norm_vec(plan, x.y0, x.y1, ks, cf, DT, x.rtol_v, x.atol_v)
    sums, _, bad = oracle_kernels.read_norms(plan)
    assert bad == [0.0, 0.0, 1.0] and all(math.isfinite(v) for v in sums)
    assert close(sums, aten_error_sums(lay, x.y0, x.y1, ks, cf, DT, x.rtol_v, x.atol_v))


# ---------------------------------------------------------------------------------------------------------------------
# the controller behind the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["reject", "accept"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["one_1", "one_5", "one_1031", "three", "five"])
def test_ratio_stays_fp64_inside_the_fp32_rounding_band(oracle_kernels, name, dtype, which):
    """ratio = 1 +/- 9.3e-10 (see _vec_tol_cases.BAND_ATOL): rounded to fp32 it is exactly 1 and the step is accepted either
    way.  The reference's ratio is an fp64 tensor for either state type (the tolerances promote it): 1 + 9.3e-10 rejects."""
    lay = Layout(name, [5] if name == "one_5" else None)
    y0, y1, part, atol_v = band_inputs(lay, dtype, which)
    # ATen's value of the reference's expression, per segment
    sums_ref = aten_error_sums(lay, y0, y1, [], [], DT, 0.0, atol_v, partial=part)
    ratio_ref = max(math.sqrt(s / n) for s, n in zip(sums_ref, lay.numels))
    assert (ratio_ref > 1.0) == (which == "reject") and ratio_ref != 1.0 and float(np.float32(ratio_ref)) == 1.0
    assert abs(ratio_ref - 1.0) == pytest.approx(2.0 ** -30, rel=1e-3)
    plan = lay.plan(oracle_kernels)
    t0, dt = 0.37, 0.0123
    c = step_ctrl(t0, dt, 5, DOPRI5, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
    tn = torch.empty(c.n_times, dtype=dtype)
    oracle_kernels.error_norm_vec_ctrl(plan, y0, y1, [], [], float(_np(dtype)(dt)), 0.0, atol_v, c, tn, partial=part)
    accept, dt_next, ratio, bad = oracle_kernels.read_ctrl(plan)
    t0_next = plan.out.tolist()[3 * lay.n_seg + 3]
    assert ratio == pytest.approx(ratio_ref, rel=1e-13) and bad == [0.0] * lay.n_seg
    if which == "reject":
        assert ratio > 1.0 and accept is False and t0_next == t0
        assert dt_next < dt
    else:
        assert ratio < 1.0 and accept is True and t0_next == t0 + dt
    # the controller alone on the same sums: the fp64 ratio kind is the twin's; the state's kind — the scalar-tolerance
    # callers' and the default — rounds the fp32 ratio to 1 and accepts
    sums = oracle_kernels.read_norms(plan)[0]
    out64, _ = oracle_kernels.step_controller(plan, sums, c, tn, dtype, ratio_dtype=torch.float64)
    assert (out64[0] != 0.0, out64[2], out64[3]) == (accept, ratio, t0_next)
    out_t, _ = oracle_kernels.step_controller(plan, sums, c, tn, dtype)
    if dtype == torch.float32:
        assert out_t[2] == 1.0 and out_t[0] == 1.0
    else:
        assert out_t == out64


SCALES = {"small": 1e-5, "unit": 1e-2, "large": 0.3, "zero": 0.0, "nan": 1e-2}


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_error_norm_vec_ctrl_twin(oracle_kernels, name, dtype, scale):
    """The ctrl entry = the plain entry's sums + the controller on them with the fp64 ratio kind; (t0, dt) from the
    device-resident words under `state_in_dev`, where the `dt` argument and c.t0 / c.dt are ignored."""
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=30, err_scale=SCALES[scale])
    mid = lay.n_seg // 2
    if scale == "nan":
        x.ks[2][lay.index(mid, 0)] = float("nan")
    plan, plan2 = lay.plan(oracle_kernels), lay.plan(oracle_kernels)
    ks, cf = x.ks[:7], COEFS[:7]
    for tab, order, sign, t0, dt, lo, hi in ctrl_rows():
        c = step_ctrl(t0, dt, order, tab, sign, lo, hi, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
        dts = float(_np(dtype)(dt)) * sign
        tn, tn2 = torch.empty(c.n_times, dtype=dtype), torch.empty(c.n_times, dtype=dtype)
        oracle_kernels.error_norm_vec(plan2, x.y0, x.y1, ks, cf, dts, x.rtol_v, x.atol_v)
        plain = oracle_kernels.read_norms(plan2)
        oracle_kernels.error_norm_vec_ctrl(plan, x.y0, x.y1, ks, cf, dts, x.rtol_v, x.atol_v, c, tn)
        words = plan.out.clone()
        n = lay.n_seg
        assert np.array_equal(words[:n].numpy(), np.array(plain[0]), equal_nan=True) and words[2 * n:3 * n].tolist() == plain[2]
        out, dev = oracle_kernels.step_controller(plan2, plain[0], c, tn2, dtype, ratio_dtype=torch.float64)
        assert np.array_equal(words[3 * n:].numpy(), np.array(out), equal_nan=True)
        assert plan.ctrl_dev.tolist() == dev == plan.ctrl_state.tolist()[:2]
        assert torch.equal(tn, tn2)
        accept, dt_next, ratio, t0_next = out
        state = plan.ctrl_state.tolist()
        assert state[2] == t0_next
        if scale == "zero":
            assert ratio == 0.0 and dt_next == min(max(dt * 10.0, lo), hi)
        if scale == "nan":
            assert math.isnan(ratio) and math.isnan(dt_next) and state[3] == lo
            assert accept == (1.0 if dt <= lo else 0.0)
        else:
            assert state[3] == dt_next
        # the same trial step read from the device-resident words
        plan2.ctrl_state.copy_(torch.tensor([0.0, dts, t0, dt], dtype=torch.float64))
        decoy = step_ctrl(t0 + 1.0, dt * 3.0, order, tab, sign, lo, hi, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
        oracle_kernels.error_norm_vec_ctrl(plan2, x.y0, x.y1, ks, cf, 5.0, x.rtol_v, x.atol_v, decoy, tn2, state_in_dev=True)
        assert np.array_equal(plan2.out.numpy(), words.numpy(), equal_nan=True)
        assert np.array_equal(plan2.ctrl_state.numpy(), plan.ctrl_state.numpy(), equal_nan=True)
        assert np.array_equal(tn2.numpy(), tn.numpy(), equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["three", "five", "seventeen"])
def test_seminorm_of_the_twin(oracle_kernels, name, dtype):
    """n_norm_seg < n_seg (an adjoint solve's seminorm): the trailing segments are summed and counted but stay out of the
    ratio — a NaN planted there does not reach it, one planted in the last counted segment does."""
    lay = Layout(name)
    for skip in sorted({1, lay.n_seg - 1}):
        n_norm = lay.n_seg - skip
        for planted in (n_norm, n_norm - 1):            # first skipped segment / last counted segment
            x = Inputs(lay, dtype, seed=40)
            x.ks[1][lay.index(planted, 0)] = float("nan")
            plan = lay.plan(oracle_kernels)
            c = step_ctrl(0.37, 0.0123, 5, DOPRI5, n_norm_seg=n_norm, np_dtype=_np(dtype))
            tn = torch.empty(c.n_times, dtype=dtype)
            oracle_kernels.error_norm_vec_ctrl(plan, x.y0, x.y1, x.ks[:7], COEFS[:7], DT, x.rtol_v, x.atol_v, c, tn)
            accept, dt_next, ratio, bad = oracle_kernels.read_ctrl(plan)
            sums = oracle_kernels.read_norms(plan)[0]
            assert [math.isnan(v) for v in sums] == [q == planted for q in range(lay.n_seg)]
            if planted >= n_norm:
                want = max(math.sqrt(s / m) for s, m in list(zip(sums, lay.numels))[:n_norm])
                assert ratio == want and math.isfinite(dt_next)
            else:
                assert math.isnan(ratio) and accept is False and math.isnan(dt_next)


# ---------------------------------------------------------------------------------------------------------------------
# the product's host logic on the fused route
# ---------------------------------------------------------------------------------------------------------------------
def _spied(monkeypatch, kern):
    calls = {"vec": 0, "vec_ctrl": 0, "init_vec": 0, "scaled": 0, "init_scaled": 0}

    def spy(name, key):
        real = getattr(kern, name)
        monkeypatch.setattr(kern, name, lambda *a, **k: (calls.__setitem__(key, calls[key] + 1), real(*a, **k))[1])
    for name, key in [("error_norm_vec", "vec"), ("error_norm_vec_ctrl", "vec_ctrl"), ("init_norms_vec", "init_vec"),
                      ("error_scaled", "scaled"), ("init_scaled", "init_scaled")]:
        spy(name, key)
    return calls


@pytest.mark.parametrize("form", ["rtol_list", "atol_list", "both", "numpy_and_tuple"])
@pytest.mark.parametrize("dname", ["f32", "f64"])
def test_tuple_tolerances_take_the_fused_route_on_the_cpu_backend(cpu_backend, monkeypatch, dname, form):
    """A no-grad dopri5 solve whose tuple tolerances hold list / tuple / numpy entries, host logic over the twins: every trial
    step's ratio comes from error_norm_vec[_ctrl], the initial step from init_norms_vec, the raw-error route is never taken;
    the result is the reference's (tests/golden/tuple_tol.npz `ttl_*`); with and without the look-ahead controller the same
    evaluations and the same accepted / rejected steps."""
    from torchdiffeq_amd import solvers
    z = load("tuple_tol.npz")
    dtype = torch.float32 if dname == "f32" else torch.float64
    x0, b0 = T(z[f"ttl_{dname}_x0"]), T(z[f"ttl_{dname}_b0"])
    w = torch.tensor([1.0, 3.0, 0.3], dtype=dtype)
    t = torch.tensor([0.0, 0.4, 1.1], dtype=dtype)
    rtol, atol = TUPLE_TOL_LIST_FORMS[form]
    calls = _spied(monkeypatch, cpu_backend)
    nfe = [0]

    class F(torch.nn.Module):
        def forward(self, t_, y_):
            nfe[0] += 1
            return -y_[0] * w * (1 + 0.2 * t_) + 0.1 * torch.sin(y_[0]), -0.4 * y_[1]
    made = []
    orig = solvers.RKAdaptiveStepsizeODESolver.__init__

    def spy_init(self, *a, **k):
        orig(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(solvers.RKAdaptiveStepsizeODESolver, "__init__", spy_init)
    key = f"ttl_{dname}_{form}"
    tol = 1e-11 if dname == "f64" else 2e-5
    out = {}
    for la in ("1", "0"):
        monkeypatch.setenv("TDEQ_LOOKAHEAD", la)
        for k_ in calls:
            calls[k_] = 0
        nfe[0] = 0
        with torch.no_grad():
            sa, sb = tda.odeint(F(), (x0, b0), t, rtol=rtol, atol=atol, method="dopri5")
        s = made[-1]
        assert s._vec_fused is not None and bool(s._lookahead) == (la == "1") and bool(s._vec_ctrl)
        assert calls["vec"] + calls["vec_ctrl"] == (nfe[0] - 2) // 6 == s.n_accepted + s.n_rejected
        assert (calls["vec_ctrl"] > 0) == (la == "1") and (calls["vec"] > 0) == (la == "0")
        assert calls["init_vec"] == 2 and calls["scaled"] == 0 and calls["init_scaled"] == 0
        assert rel_err(sa, z[f"{key}_ya"]) < tol and rel_err(sb, z[f"{key}_yb"]) < tol
        if dname == "f64":
            assert nfe[0] == int(z[f"{key}_nfe"])
        out[la] = (nfe[0], s.n_accepted, s.n_rejected, sa, sb)
    assert out["1"][:3] == out["0"][:3]
    # both loops run libm's pow on the same sums: the same steps to the last bit
    assert torch.equal(out["1"][3], out["0"][3]) and torch.equal(out["1"][4], out["0"][4])
