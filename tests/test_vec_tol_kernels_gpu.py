"""The per-element-tolerance kernels (error_norm_vec_kernel, init_norms_vec_kernel and the device controller behind
tdeq_error_norm_vec_ctrl) against their CPU twins, at kernel level, on every segment-table path:

    one segment | 2..4: inline table, fused controller | 5..16: inline table, parallel finalize + presummed controller |
    above 16: device table

Sums: rel 1e-12 against the twin's long-double sums (segments of <= 6000 elements); the non-finite census exact; wherever
the same kernel is launched twice (ctrl entry / plain entry, `state_in_dev` / host dt, misaligned / aligned bases, partial
row / whole row) the results are bit-equal.  Controller words: accept, ratio, t0' equal to the oracle controller's on the
device's own sums with the fp64 ratio kind; dt' to 4 ulp (the GPU's pow against libm's), stage times to 2 ulp of the time
scale.  Every padding element of every stream is NaN (tests/test_vec_tol_oracle.py shows that such a NaN in a valid
element does reach the sums)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from torchdiffeq_amd.tableaus import DOPRI5

from _vec_tol_cases import (COEFS, DT, LAYOUTS, Inputs, Layout, band_inputs, close, ctrl_rows, max_rel_diff, step_ctrl,
                            to_device)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
FORMS = ["both", "rtol_only", "atol_only"]
SEGMENTED = ["three", "five", "seventeen"]


def _np(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _cuda():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _shared(name, dtype, seed=0, err_scale=1e-4):
    """(layout, CPU inputs, their device copies) shared by the tests that do not write into them."""
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=seed, err_scale=err_scale)
    return lay, x, _on_device(x)


def _on_device(x, misalign=False):
    d = types.SimpleNamespace()
    mv = lambda t: to_device(t, misalign)
    d.y0, d.y1, d.ks, d.a, d.b, d.yscale = mv(x.y0), mv(x.y1), [mv(k) for k in x.ks], mv(x.a), mv(x.b), mv(x.yscale)
    d.rtol_v, d.atol_v = x.rtol_v.cuda(), x.atol_v.cuda()       # `double` loads: kept 8-byte (here 16-byte) aligned
    return d


def _tols(d, form):
    return (d.rtol_v if form != "atol_only" else 3e-4), (d.atol_v if form != "rtol_only" else 2e-6)


def _plan(hip, lay):
    plan = lay.plan(hip, _cuda())
    assert (plan.segs_dev is not None) == (lay.n_seg > 16)          # the device table exactly above the inline one
    return plan


def _report(what, dtype, got, want):
    print("max_rel_diff {} {} {:.3e}".format(what, "f32" if dtype == torch.float32 else "f64", max_rel_diff(got, want)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sums against the twin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_terms", [1, 6, 7, 14])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_error_norm_vec_equals_the_twin(hip_kernels, oracle_kernels, name, dtype, form, n_terms):
    lay, x, d = _shared(name, dtype)
    plan_d, plan_o = _plan(hip_kernels, lay), lay.plan(oracle_kernels)
    cf = COEFS[:n_terms]
    hip_kernels.error_norm_vec(plan_d, d.y0, d.y1, d.ks[:n_terms], cf, DT, *_tols(d, form))
    sums, _, bad = hip_kernels.read_norms(plan_d)
    oracle_kernels.error_norm_vec(plan_o, x.y0, x.y1, x.ks[:n_terms], cf, DT, *x.tolerances(form))
    want, _, bad_o = oracle_kernels.read_norms(plan_o)
    _report("error_norm_vec", dtype, sums, want)
    assert all(math.isfinite(v) and v > 0 for v in want)
    assert close(sums, want), (sums, want)
    assert bad == bad_o == [0.0] * lay.n_seg


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_init_norms_vec_equals_the_twin(hip_kernels, oracle_kernels, name, dtype, form, mode):
    """Mode 0 writes two sums per segment (finalize with n_sum = 2), mode 1 one — on every segment-table path."""
    lay, x, d = _shared(name, dtype)
    plan_d, plan_o = _plan(hip_kernels, lay), lay.plan(oracle_kernels)
    hip_kernels.init_norms_vec(plan_d, mode, d.a, d.b, d.yscale, *_tols(d, form))
    s0, s1, bad = hip_kernels.read_norms(plan_d)
    oracle_kernels.init_norms_vec(plan_o, mode, x.a, x.b, x.yscale, *x.tolerances(form))
    w0, w1, bad_o = oracle_kernels.read_norms(plan_o)
    _report("init_norms_vec", dtype, s0 + (s1 if mode == 0 else []), w0 + (w1 if mode == 0 else []))
    assert all(math.isfinite(v) and v > 0 for v in w0)
    assert close(s0, w0), (s0, w0)
    if mode == 0:
        assert close(s1, w1), (s1, w1)
    assert bad == bad_o == [0.0] * lay.n_seg


# ---------------------------------------------------------------------------------------------------------------------
# 2. partial rows, 3. misaligned bases: the same sums to the last bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lead", [6, 5, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", SEGMENTED)
def test_partial_row_continues_on_segmented_layouts(hip_kernels, oracle_kernels, name, dtype, n_lead):
    """stage_combine_err over the leading stages, error_norm_vec(partial=) over the rest: the whole-row launch's sums bit
    for bit, and the twin's (which continues the same partial row) to 1e-12."""
    lay, x, d = _shared(name, dtype)
    plan_d, plan_o = _plan(hip_kernels, lay), lay.plan(oracle_kernels)
    err_coefs = COEFS[1:7]
    y1, part = torch.empty_like(d.y0), torch.empty_like(d.y0)
    hip_kernels.stage_combine_err(y1, part, d.y0, d.ks[:n_lead], COEFS[:n_lead], err_coefs[:n_lead], DT)
    hip_kernels.error_norm_vec(plan_d, d.y0, y1, d.ks[:6], err_coefs, DT, d.rtol_v, d.atol_v)
    whole = hip_kernels.read_norms(plan_d)
    hip_kernels.error_norm_vec(plan_d, d.y0, y1, d.ks[n_lead:6], err_coefs[n_lead:], DT, d.rtol_v, d.atol_v, partial=part)
    split = hip_kernels.read_norms(plan_d)
    assert split[0] == whole[0] and split[2] == whole[2] == [0.0] * lay.n_seg
    oracle_kernels.error_norm_vec(plan_o, x.y0, y1.cpu(), x.ks[n_lead:6], err_coefs[n_lead:], DT, x.rtol_v, x.atol_v,
                                  partial=part.cpu())
    want = oracle_kernels.read_norms(plan_o)[0]
    _report("error_norm_vec(partial)", dtype, split[0], want)
    assert close(split[0], want), (split[0], want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["one_1031", "three"])
def test_misaligned_bases_give_the_same_sums(hip_kernels, name, dtype):
    """Every state-typed stream as a view one element into its allocation (the fp64 tolerance vectors stay aligned): scalar
    loads, no branch on alignment — the sums of the aligned launch bit for bit, for all three entry points."""
    lay, x, d = _shared(name, dtype)
    m = _on_device(x, misalign=True)
    assert all(t.data_ptr() % 16 == 0 for t in (d.y0, d.y1, d.a, d.b, d.yscale, *d.ks))
    plan = _plan(hip_kernels, lay)
    c = step_ctrl(0.37, 0.0123, 5, DOPRI5, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
    out = {}
    sums_and_census = lambda r: (r[0], r[2])        # (an error-norm launch writes one sum per segment: the second block is stale)
    for key, s in (("aligned", d), ("misaligned", m)):
        res = []
        for form in FORMS:
            hip_kernels.error_norm_vec(plan, s.y0, s.y1, s.ks[:7], COEFS[:7], DT, *_tols(d, form))
            res.append(sums_and_census(hip_kernels.read_norms(plan)))
            hip_kernels.error_norm_vec(plan, s.y0, s.y1, s.ks[1:3], COEFS[1:3], DT, *_tols(d, form), partial=s.ks[0])
            res.append(sums_and_census(hip_kernels.read_norms(plan)))
            launched = _launch_ctrl(hip_kernels, plan, s, s.ks[:7], COEFS[:7], DT, *_tols(d, form), c, dtype)
            res.append(launched[:4] + (launched[4].tolist(),))
            for mode in (0, 1):
                hip_kernels.init_norms_vec(plan, mode, s.a, s.b, s.yscale, *_tols(d, form))
                s0, s1, bad = hip_kernels.read_norms(plan)
                res.append((s0, s1 if mode == 0 else None, bad))
        out[key] = res
    assert out["aligned"] == out["misaligned"]
    assert all(math.isfinite(v) for v in out["aligned"][0][0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the controller behind the norm
# ---------------------------------------------------------------------------------------------------------------------
def _launch_ctrl(hip, plan, d, ks, cf, dts, rtol, atol, c, dtype, **kw):
    """tdeq_error_norm_vec_ctrl -> (sums, census, [accept, dt_next, ratio, t0'], ctrl_dev[4], stage times) as lists."""
    tn = torch.empty(c.n_times, dtype=dtype, device="cuda")
    hip.error_norm_vec_ctrl(plan, d.y0, d.y1, ks, cf, dts, rtol, atol, c, tn, **kw)
    full = hip._read_out(plan)
    n = plan.n_seg
    return full[:n], full[2 * n:3 * n], full[3 * n:3 * n + 4], plan.ctrl_dev.cpu().tolist(), tn.cpu()


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _check_against_oracle_controller(oracle, lay, sums, words, ctrl_dev, tn_d, c, dtype, t0, dt, sign):
    """The device controller's words against the oracle controller on the DEVICE's sums with the fp64 ratio kind: accept,
    ratio, t0' equal; dt' and sign * T(dt') to 4 ulp; stage times to 2 ulp of the time scale, equal when dt' is."""
    np_dtype = _np(dtype)
    plan_o = lay.plan(oracle)
    tn_o = torch.empty(c.n_times, dtype=dtype)
    out, dev_o = oracle.step_controller(plan_o, sums, c, tn_o, dtype, ratio_dtype=torch.float64)
    accept, dt_next, ratio, t0_next = words
    assert (accept != 0.0) == (out[0] != 0.0)
    assert _same([ratio, t0_next], [out[2], out[3]]), (ratio, out[2], t0_next, out[3])
    if math.isnan(out[1]):
        assert math.isnan(dt_next)
    else:
        assert abs(dt_next - out[1]) <= 4 * np.spacing(abs(out[1]))
    assert ctrl_dev[0] == dev_o[0] and ctrl_dev[2] == t0_next
    ulp = float(np.spacing(np_dtype(abs(dev_o[1]))))
    assert abs(ctrl_dev[1] - dev_o[1]) <= 4 * ulp
    assert ctrl_dev[1] == sign * float(np_dtype(ctrl_dev[3]))          # sign * T(dt') of the device's own dt'
    tol_t = 2 * float(np.spacing(np_dtype(max(abs(t0) + dt * 11, 1e-30))))
    assert float((tn_d.double() - tn_o.double()).abs().max()) <= tol_t
    if ctrl_dev[1] == dev_o[1]:
        assert torch.equal(tn_d, tn_o)
    return out


SCALES = {"small": 1e-5, "unit": 1e-2, "large": 0.3, "zero": 0.0, "nan": 1e-2}


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_error_norm_vec_ctrl_against_the_oracle_controller(hip_kernels, oracle_kernels, name, dtype, scale):
    lay = Layout(name)
    x = Inputs(lay, dtype, seed=30, err_scale=SCALES[scale])
    if scale == "nan":
        x.ks[2][lay.index(lay.n_seg // 2, 0)] = float("nan")          # a stage stream of one middle segment
    d = _on_device(x)
    plan, plan_o = _plan(hip_kernels, lay), lay.plan(oracle_kernels)
    ks, cf, n = d.ks[:7], COEFS[:7], lay.n_seg
    seen = set()
    for tab, order, sign, t0, dt, lo, hi in ctrl_rows():
        c = step_ctrl(t0, dt, order, tab, sign, lo, hi, n_norm_seg=n, np_dtype=_np(dtype))
        dts = float(_np(dtype)(dt)) * sign
        sums, bad, words, ctrl_dev, tn = _launch_ctrl(hip_kernels, plan, d, ks, cf, dts, d.rtol_v, d.atol_v, c, dtype)
        hip_kernels.error_norm_vec(plan, d.y0, d.y1, ks, cf, dts, d.rtol_v, d.atol_v)
        plain = hip_kernels.read_norms(plan)
        assert _same(sums, plain[0]) and bad == plain[2] == [0.0] * n      # (a NaN in a stage is not in the state census)
        oracle_kernels.error_norm_vec(plan_o, x.y0, x.y1, x.ks[:7], cf, dts, x.rtol_v, x.atol_v)
        want = oracle_kernels.read_norms(plan_o)[0]
        _report("error_norm_vec_ctrl", dtype, sums, want)
        assert close(sums, want), (sums, want)
        out = _check_against_oracle_controller(oracle_kernels, lay, plain[0], words, ctrl_dev, tn, c, dtype, t0, dt, sign)
        accept, dt_next, ratio = out[0], out[1], out[2]
        seen.add(accept)
        if scale == "zero":
            assert ratio == 0.0 and words[1] == min(max(dt * 10.0, lo), hi)
        elif scale == "nan":
            assert [math.isnan(v) for v in sums] == [q == n // 2 for q in range(n)]
            assert math.isnan(words[2]) and math.isnan(words[1]) and ctrl_dev[3] == lo
            assert (words[0] != 0.0) == (dt <= lo)          # rejected, unless the step is at min_step already
        else:
            assert math.isfinite(ratio) and ratio > 0.0 and ctrl_dev[3] == words[1]
    assert seen == {0.0, 1.0}       # (the forced rows see to both decisions)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", SEGMENTED)
def test_seminorm_on_every_controller_path(hip_kernels, oracle_kernels, name, dtype):
    """n_norm_seg < n_seg (an adjoint solve with per-element tolerances): the skipped trailing segments are summed and
    counted but stay out of the ratio — on the fused (three), presummed inline (five) and device-table (seventeen) paths."""
    lay = Layout(name)
    n = lay.n_seg
    for skip in sorted({1, n - 1}):
        n_norm = n - skip
        for planted in (n_norm, n_norm - 1):            # the first skipped segment / the last counted one
            x = Inputs(lay, dtype, seed=40)
            x.ks[1][lay.index(planted, 0)] = float("nan")
            d = _on_device(x)
            plan = _plan(hip_kernels, lay)
            t0, dt = 0.37, 0.0123
            c = step_ctrl(t0, dt, 5, DOPRI5, n_norm_seg=n_norm, np_dtype=_np(dtype))
            dts = float(_np(dtype)(dt))
            sums, bad, words, ctrl_dev, tn = _launch_ctrl(hip_kernels, plan, d, d.ks[:7], COEFS[:7], dts, d.rtol_v, d.atol_v,
                                                          c, dtype)
            assert [math.isnan(v) for v in sums] == [q == planted for q in range(n)] and bad == [0.0] * n
            _check_against_oracle_controller(oracle_kernels, lay, sums, words, ctrl_dev, tn, c, dtype, t0, dt, 1.0)
            if planted >= n_norm:
                want = max(math.sqrt(s / m) for s, m in list(zip(sums, lay.numels))[:n_norm])
                assert words[2] == want and math.isfinite(words[1])
            else:
                assert math.isnan(words[2]) and words[0] == 0.0 and math.isnan(words[1]) and words[3] == t0


@pytest.mark.parametrize("which", ["reject", "accept"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["one_1", "one_5", "one_1031", "three", "five"])
def test_ratio_is_not_rounded_to_fp32(hip_kernels, oracle_kernels, name, dtype, which):
    """err / tol = 1 / (1 -/+ 2^-30) in every element of every segment: ratio = 1 +/- 9.3e-10, which is 1.0 in fp32.  The
    ratio of a solve with per-element tolerances is fp64 for either state type: above 1 the step is rejected."""
    lay = Layout(name, [5] if name == "one_5" else None)
    y0, y1, part, atol_v = band_inputs(lay, dtype, which)
    d = types.SimpleNamespace(y0=y0.cuda(), y1=y1.cuda())
    plan = _plan(hip_kernels, lay)
    t0, dt = 0.37, 0.0123
    c = step_ctrl(t0, dt, 5, DOPRI5, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
    sums, bad, words, ctrl_dev, tn = _launch_ctrl(hip_kernels, plan, d, [], [], float(_np(dtype)(dt)), 0.0, atol_v.cuda(), c,
                                                  dtype, partial=part.cuda())
    plan_o = lay.plan(oracle_kernels)
    tn_o = torch.empty(c.n_times, dtype=dtype)
    oracle_kernels.error_norm_vec_ctrl(plan_o, y0, y1, [], [], float(_np(dtype)(dt)), 0.0, atol_v, c, tn_o, partial=part)
    accept_o, _, ratio_o, _ = oracle_kernels.read_ctrl(plan_o)
    print("band ratio - 1: device {:.6e} twin {:.6e}".format(words[2] - 1.0, ratio_o - 1.0))
    assert bad == [0.0] * lay.n_seg and float(np.float32(words[2])) == 1.0 and words[2] == pytest.approx(ratio_o, rel=1e-12)
    if which == "reject":
        assert words[2] > 1.0 and words[0] == 0.0 and words[3] == t0 and accept_o is False
    else:
        assert words[2] < 1.0 and words[0] == 1.0 and words[3] == t0 + dt and accept_o is True
    _check_against_oracle_controller(oracle_kernels, lay, sums, words, ctrl_dev, tn, c, dtype, t0, dt, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the trial step read from device memory (captured steps)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_partial", [False, True], ids=["whole", "partial"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["one_1031", "three", "seventeen"])
def test_state_in_dev_equals_the_host_step(hip_kernels, name, dtype, with_partial):
    """plan.ctrl_dev[1..3] = (sign * T(dt), t0, dt), a wrong `dt` argument and wrong c.t0 / c.dt: the kernel forms
    fl_T(fl_T(coef) * T(ctrl_dev[1])) itself and the controller starts from ctrl_dev[2..3] — sums, controller words, the
    rewritten ctrl_dev and the stage times are those of the host-dt launch with the right values, bit for bit."""
    lay, x, d = _shared(name, dtype, 50, 1e-2)
    plan_h, plan_g = _plan(hip_kernels, lay), _plan(hip_kernels, lay)
    ks, cf = (d.ks[1:3], COEFS[1:3]) if with_partial else (d.ks[:7], COEFS[:7])
    kw = {"partial": d.ks[0]} if with_partial else {}
    for tab, order, sign, t0, dt, lo, hi in ctrl_rows()[:2]:            # forward and backward in time
        c = step_ctrl(t0, dt, order, tab, sign, lo, hi, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
        dts = float(_np(dtype)(dt)) * sign
        host = _launch_ctrl(hip_kernels, plan_h, d, ks, cf, dts, d.rtol_v, d.atol_v, c, dtype, **kw)
        plan_g.ctrl_dev.copy_(torch.tensor([0.0, dts, t0, dt], dtype=torch.float64))
        decoy = step_ctrl(t0 + 1.0, dt * 3.0, order, tab, sign, lo, hi, n_norm_seg=lay.n_seg, np_dtype=_np(dtype))
        dev = _launch_ctrl(hip_kernels, plan_g, d, ks, cf, 5.0, d.rtol_v, d.atol_v, decoy, dtype, state_in_dev=True, **kw)
        assert all(math.isfinite(v) and v > 0 for v in host[0]) and host[3][2] == host[2][3]
        for h, g in zip(host[:4], dev[:4]):
            assert h == g
        assert torch.equal(host[4], dev[4])


# ---------------------------------------------------------------------------------------------------------------------
# 6. degenerate tolerances, 7. what the entry points refuse
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_tolerances_equal_the_twin(hip_kernels, oracle_kernels, dtype):
    """0 / 0 -> NaN, x / 0 -> inf (ratio inf: reject, dt' = dt * dfactor), a subnormal tolerance, an infinite state: what the
    twin gives — which tests/test_vec_tol_oracle.py holds against ATen for the same inputs."""
    lay = Layout("three")
    x = Inputs(lay, dtype, seed=5)
    plan, plan_o = _plan(hip_kernels, lay), lay.plan(oracle_kernels)
    cf = COEFS[:7]
    t0, dt = 0.37, 0.0123
    c = step_ctrl(t0, dt, 5, DOPRI5, n_norm_seg=3, np_dtype=_np(dtype))
    dts = float(_np(dtype)(dt))

    def run(rtol_is_vec):
        d = _on_device(x)
        rt_d, rt_o = (d.rtol_v, x.rtol_v) if rtol_is_vec else (0.0, 0.0)
        sums, bad, words, ctrl_dev, tn = _launch_ctrl(hip_kernels, plan, d, d.ks[:7], cf, dts, rt_d, d.atol_v, c, dtype)
        oracle_kernels.error_norm_vec(plan_o, x.y0, x.y1, x.ks[:7], cf, dts, rt_o, x.atol_v)
        want, _, bad_o = oracle_kernels.read_norms(plan_o)
        assert close(sums, want), (sums, want)
        assert bad == bad_o
        _check_against_oracle_controller(oracle_kernels, lay, sums, words, ctrl_dev, tn, c, dtype, t0, dt, 1.0)
        return sums, bad, words, ctrl_dev
    i = lay.index(1, 17)
    x.atol_v[i] = 0.0
    x.y0[i] = x.y1[i] = 0.0
    saved = [k[i].clone() for k in x.ks[:7]]
    for k in x.ks[:7]:
        k[i] = 0.0
    sums, bad, words, ctrl_dev = run(False)                 # 0 / 0
    assert [math.isnan(v) for v in sums] == [False, True, False] and bad == [0.0] * 3
    assert math.isnan(words[2]) and words[0] == 0.0 and ctrl_dev[3] == 0.0
    for k, v in zip(x.ks[:7], saved):
        k[i] = v
    sums, bad, words, ctrl_dev = run(False)                 # e / 0
    assert sums[1] == math.inf and math.isfinite(sums[0]) and math.isfinite(sums[2]) and bad == [0.0] * 3
    assert words[2] == math.inf and words[0] == 0.0 and words[3] == t0
    assert words[1] == pytest.approx(dt * 0.2, rel=1e-15)   # safety / pow(inf, .) = 0, then dfactor
    x.atol_v[i] = 5e-324
    sums, bad, words, ctrl_dev = run(False)                 # e / subnormal: inf in fp64, as the twin's
    assert sums[1] == math.inf and bad == [0.0] * 3
    x.atol_v[i] = 1e-6
    x.y1[lay.index(2, 1024)] = float("inf")
    sums, bad, words, ctrl_dev = run(True)
    assert bad == [0.0, 0.0, 1.0] and all(math.isfinite(v) for v in sums)


@pytest.mark.parametrize("bad_dtype", [torch.bfloat16, torch.float16, torch.complex64, torch.complex128],
                         ids=["bf16", "f16", "c64", "c128"])
def test_entry_points_refuse_other_state_types(hip_kernels, bad_dtype):
    """16-bit and complex states are not this family's: TDEQ_EINVAL (-1) from all three entry points, before any launch."""
    lay = Layout("one_1031")
    plan = _plan(hip_kernels, lay)
    z = lambda: torch.zeros(lay.total, dtype=bad_dtype, device="cuda")
    y0, y1, k0, a, b = z(), z(), z(), z(), z()
    tol = torch.ones(lay.total, dtype=torch.float64, device="cuda")
    c = step_ctrl(0.0, 0.1, 5, DOPRI5)
    tn = torch.empty(c.n_times, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec failed with code -1 "):
        hip_kernels.error_norm_vec(plan, y0, y1, [k0], [1.0], DT, tol, tol)
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec_ctrl failed with code -1 "):
        hip_kernels.error_norm_vec_ctrl(plan, y0, y1, [k0], [1.0], DT, tol, tol, c, tn)
    with pytest.raises(RuntimeError, match="tdeq_init_norms_vec failed with code -1 "):
        hip_kernels.init_norms_vec(plan, 0, a, b, y0, tol, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_entry_points_refuse_two_scalars_and_an_empty_row(hip_kernels, dtype):
    lay, x, d = _shared("one_1031", dtype)
    plan = _plan(hip_kernels, lay)
    c = step_ctrl(0.0, 0.1, 5, DOPRI5, np_dtype=_np(dtype))
    tn = torch.empty(c.n_times, dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec failed with code -1 "):
        hip_kernels.error_norm_vec(plan, d.y0, d.y1, d.ks[:2], COEFS[:2], DT, 1e-3, 1e-6)
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec_ctrl failed with code -1 "):
        hip_kernels.error_norm_vec_ctrl(plan, d.y0, d.y1, d.ks[:2], COEFS[:2], DT, 1e-3, 1e-6, c, tn)
    with pytest.raises(RuntimeError, match="tdeq_init_norms_vec failed with code -1 "):
        hip_kernels.init_norms_vec(plan, 0, d.a, d.b, d.yscale, 1e-3, 1e-6)
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec failed with code -1 "):
        hip_kernels.error_norm_vec(plan, d.y0, d.y1, [], [], DT, d.rtol_v, 1e-6)
    with pytest.raises(RuntimeError, match="tdeq_error_norm_vec_ctrl failed with code -1 "):
        hip_kernels.error_norm_vec_ctrl(plan, d.y0, d.y1, [], [], DT, d.rtol_v, 1e-6, c, tn)
    # ... and a refused call leaves the plan usable: the same row with its partial goes through
    hip_kernels.error_norm_vec(plan, d.y0, d.y1, [], [], DT, d.rtol_v, 1e-6, partial=d.ks[0])
    sums, _, bad = hip_kernels.read_norms(plan)
    assert math.isfinite(sums[0]) and sums[0] > 0 and bad == [0.0]
