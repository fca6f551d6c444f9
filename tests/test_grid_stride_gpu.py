"""The second grid pass of the flat-state entry points (csrc/tdeq_abi.hip `stream_grid`: beyond 65536 workgroups of 256
lanes = 2^24 items every streaming kernel walks a grid-stride loop), at the smallest sizes that reach it:
items = 2^24 + 773 — three full workgroups and five lanes of second pass — i.e.

    fp32, 16-byte form   n = 4 * items + 3 = 67,111,959        fp64, 16-byte form   n = 2 * items + 1 = 33,555,979
    bf16 / fp16          n = 8 * items + 7                     scalar form (a view one element off alignment)   n = items

(`tdeq_interp_fit` takes its 16-byte form only for whole 16-byte elements: n = lane * items there.)  Each case is checked as
tests/_launch_forms.py describes: windows against the CPU oracle, the whole tensor against slice-by-slice launches below
the cap, sentinel borders; all bit for bit on finite randn inputs.  At these sizes the 16-byte forms of the five
policy-taking entry points stream more than 512 MiB, so in this process they run with POLICY 3; the last test runs the
combine family once more in a child under TDEQ_COMBINE_POLICY=0 — the only route to the policy-0 forms that are not ONEPASS.
"""
import pytest
import torch

import _launch_forms as lf
from _launch_forms import Flat
from oracle import lp_kernels as olp
from torchdiffeq_amd.tableaus import DOPRI5

pytestmark = pytest.mark.gpu

ROW = max(DOPRI5.beta_rows(), key=lambda r: len(r.idx))          # dopri5's longest row: the one wide term count
NT, COEF = len(ROW.idx), tuple(float(c) for c in ROW.coef)
ERR = tuple(0.37 * (j + 1) * (-1) ** j for j in range(NT))
DT = -0.0371
XS = (0.0, 0.3, 1.0)


@pytest.fixture(autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()          # (the shared input pool stays; see the last test)


def _masked(coefs, mask):
    return tuple(c if (mask >> j) & 1 else 0.0 for j, c in enumerate(coefs))


FULL = (1 << NT) - 1
MULTI_ROWS = ((COEF, FULL, True),                                                   # the row's own stage input
              (_masked(ERR, 0b101101 & FULL), 0b101101 & FULL, False),              # structural zeros, no y0
              (_masked(COEF[::-1], 0b011011 & FULL), 0b011011 & FULL, True),
              (_masked(ERR[::-1], 0b000110 & FULL), 0b000110 & FULL, False))


# ---- the cases: x = input streams, o = outputs --------------------------------------------------------------------------
def _combine(k, x, o, env):
    k.stage_combine(o[0], x[0], x[1:], COEF, DT)


def _combine_err(k, x, o, env):
    k.stage_combine_err(o[0], o[1], x[0], x[1:], COEF, ERR, DT)


FILL = [0.1 * j + 1e-9 for j in range(6)]


def _combine_fill(k, x, o, env):
    pad = 0 if env.device is None else 2           # (the oracle's fill is a copy: exactly the values)
    fill = env.tensor([-7.0] * (len(FILL) + pad), env.dtype)
    k.stage_combine_fill(o[0], x[0], x[1:3], COEF[:2], DT, fill, FILL)
    assert torch.equal(fill.cpu(), torch.tensor(FILL + [-7.0] * pad, dtype=torch.float64).to(env.dtype))


def _multi(n_out, acc):
    rows = MULTI_ROWS[:n_out]

    def call(k, x, o, env):
        k.stage_combine_multi(o[:n_out], rows, x[0], x[NT + 1] if acc else None, x[1:NT + 1], DT)
        k.stage_combine_multi_dev(o[n_out:], rows, x[0], x[NT + 1] if acc else None, x[1:NT + 1], env.plan(1.0, DT))

    def ref(k, x, o, env):          # the step size on the device: the same T(dt) (tests/test_carry.py)
        for outs in (o[:n_out], o[n_out:]):
            k.stage_combine_multi(outs, rows, x[0], x[NT + 1] if acc else None, x[1:NT + 1], lf.as_type(DT, env.dtype))
    return Flat(f"multi{n_out}{'acc' if acc else ''}", NT + 2, [(1, None)] * (2 * n_out), call, ref)


def _combine_dev(k, x, o, env):
    plan = env.plan(1.0, DT)
    k.stage_combine_dev(o[0], None, x[0], x[1:], COEF, None, plan)
    k.stage_combine_dev(o[1], o[2], x[0], x[1:], COEF, ERR, plan)


def _combine_dev_ref(k, x, o, env):
    dt = lf.as_type(DT, env.dtype)
    k.stage_combine(o[0], x[0], x[1:], COEF, dt)
    k.stage_combine_err(o[1], o[2], x[0], x[1:], COEF, ERR, dt)


def _commit(k, x, o, env):           # o = (y_prev, f_prev, y_cur, f_cur) rejected, the same four accepted
    for flag, q in ((0.0, o[:4]), (1.0, o[4:])):
        k.step_commit(q[0], q[1], q[2], q[3], x[4], x[5], env.plan(flag, DT))


def _commit_ref(k, x, o, env):       # on accept (prev) <- (cur), (cur) <- (y1, f1); on reject nothing
    for dst, src in zip(o[4:], (x[2], x[3], x[4], x[5])):
        dst.copy_(src)


def _sel(k, x, o, env):
    for flag, out in ((1.0, o[0]), (0.0, o[1])):
        k.stage_combine_sel(out, x[0], x[1], x[2], x[3], 0.2, env.plan(flag, DT))


def _dense(k, x, o, env):
    k.dense_eval(o[0], x[0], x[1], x[2], x[3], x[4:], COEF, DT, 0.3)


def _dense_multi(k, x, o, env):
    k.dense_eval_multi(o[0], x[0], x[1], x[2], x[3], x[4:], COEF, DT, XS)


def _fit(k, x, o, env):
    k.interp_fit(o[0], x[0], x[1], x[2], x[3], x[4:], COEF, DT)


def _rk4(k, x, o, env):
    dt_dev = env.tensor([DT], torch.float64)
    for stage in (1, 2, 3, 4):
        ks = [x[1 + j] if j < stage else None for j in range(4)]
        k.rk4_stage(stage, o[stage - 1], x[0], *ks, DT)
        k.rk4_stage_dev(stage, o[3 + stage], x[0], *ks, dt_dev)


W4 = (0.1, 0.2, 0.3, 0.4)
W8 = tuple((-1) ** j * (0.3 + j / 7) for j in range(8))


def _fixed(k, x, o, env):
    dt_dev = env.tensor([DT], torch.float64)
    k.fixed_stage(0, o[0], x[0], x[1:5], W4, DT)
    k.fixed_stage(1, o[1], x[0], x[2:3], (1 / 3,), DT)
    k.fixed_stage_dev(0, o[2], x[0], x[1:5], W4, dt_dev)
    k.fixed_stage_dev(1, o[3], x[0], x[2:3], (1 / 3,), dt_dev)
    k.weighted_sum(o[4], x[1:9], W8)


def _lerp(k, x, o, env):
    k.lerp(o[0], x[0], x[1], 0.37)


def _scale(k, x, o, env):
    k.scale_many(o, x[0], COEF)


def _adams(k, x, o, env):
    k.adams_predict(o[0], x[0], x[1:], COEF, cm=ERR, dt=DT, dy_out=o[1], delta_out=o[2])
    k.adams_predict(o[3], x[0], x[1:], COEF)


def _grid_commit(k, x, o, env):      # o = (solution [3, n] with padded rows, y_cur): row counter + 1 = 1 and y_cur <- y_new
    k.grid_commit(o[0], o[1], x[1], env.tensor(0, torch.int64))


NEW = (1, None)
CASES = [
    Flat("stage_combine", NT + 1, [NEW], _combine),
    Flat("stage_combine_err", NT + 1, [NEW] * 2, _combine_err),
    Flat("stage_combine_fill", 3, [NEW], _combine_fill),
    _multi(1, True), _multi(1, False), _multi(2, True), _multi(2, False), _multi(4, True),
    Flat("stage_combine_dev", NT + 1, [NEW] * 3, _combine_dev, _combine_dev_ref),
    Flat("step_commit", 6, [(1, j) for j in (0, 1, 2, 3, 0, 1, 2, 3)], _commit, _commit_ref),
    Flat("stage_combine_sel", 4, [NEW] * 2, _sel),
    Flat("dense_eval", NT + 4, [NEW], _dense),
    Flat("dense_eval_multi", NT + 4, [(len(XS), None)], _dense_multi),
    Flat("interp_fit", NT + 4, [(5, None)], _fit, contiguous=True),
    Flat("rk4_stage", 5, [NEW] * 8, _rk4),
    Flat("fixed_stage_weighted_sum", 9, [NEW] * 5, _fixed),
    Flat("lerp", 2, [NEW], _lerp),
    Flat("scale_many", 1, [NEW] * NT, _scale),
    Flat("adams_predict", NT + 1, [NEW] * 4, _adams),
    Flat("grid_commit", 2, [(3, None), (1, 0)], _grid_commit, one_lane=True),
]
GEOMETRIES = [(d, f) for f in ("vec", "scalar") for d in lf.REAL]      # (cases of one geometry share one input pool)


def _id(case, dtype, form):
    return f"{case.name}-{lf.NAME[dtype]}-{form}"


@pytest.mark.parametrize("case,dtype,form", [pytest.param(c, d, f, id=_id(c, d, f)) for d, f in GEOMETRIES for c in CASES])
def test_flat(hip_kernels, oracle_kernels, case, dtype, form):
    lf.check_flat(case, dtype, form, hip_kernels, oracle_kernels)


# ---- the 16-bit routes of the combine family and of the look-ahead stage (lp::map_kernel, lp::sel_kernel) ----------------
def _ref(fn):
    def ref(k, x, o, env):
        res = fn(x, env)
        for out, r in zip(o, res if isinstance(res, (tuple, list)) else [res]):
            out.copy_(r)
    return ref


def _lp_dev(k, x, o, env):
    k.stage_combine_dev(o[0], None, x[0], x[1:], COEF, None, env.plan(1.0, DT))


LP_CASES = [
    Flat("stage_combine", NT + 1, [NEW], _combine, _ref(lambda x, env: olp.stage_combine(x[0], x[1:], COEF, DT))),
    Flat("stage_combine_err", NT + 1, [NEW] * 2, _combine_err,
         _ref(lambda x, env: olp.stage_combine_err(x[0], x[1:], COEF, ERR, DT))),
    Flat("stage_combine_dev", NT + 1, [NEW], _lp_dev,
         _ref(lambda x, env: olp.stage_combine(x[0], x[1:], COEF, lf.as_type(DT, env.dtype)))),
    Flat("stage_combine_sel", 4, [NEW] * 2, _sel,
         _ref(lambda x, env: [olp.stage_combine_sel(x[0], x[1], x[2], x[3], 0.2, flag, lf.as_type(DT, env.dtype))
                              for flag in (1.0, 0.0)])),
]


@pytest.mark.parametrize("case,dtype,form", [pytest.param(c, d, f, id=_id(c, d, f))
                                             for f in ("vec", "scalar") for d in lf.LOW for c in LP_CASES])
def test_flat_16_bit(oracle_kernels, case, dtype, form):
    from _lowp_kernels import kernels
    lf.check_flat(case, dtype, form, kernels(dtype), oracle_kernels)


# ---- policy 0 past the cap: a child process ---------------------------------------------------------------------------------
POLICY0_NODES = [f"tests/test_grid_stride_gpu.py::test_flat[{name}-{t}-vec]" for t in ("f32", "f64")
                 for name in ("stage_combine", "stage_combine_err", "multi1acc", "multi1", "multi2acc", "multi2", "multi4acc")]
# One plain child (no variable set) ran this list in 4.3 s on the MI355X (14 tests, 1.1 s inside pytest; the file is new, so
# there is no figure from the parent commit); the limit is 5 x that, rounded up, and at least 60 s.
POLICY0_TIMEOUT = 60


def test_combine_family_past_the_cap_under_policy_0():
    """More than 2^24 16-byte elements of at least 3 streams exceed the 512 MiB threshold, so the policy-0 forms that
    are not ONEPASS (stage_combine, stage_combine_err, the NOUTC / ACCC-specialised stage_combine_multi) are launched
    only when TDEQ_COMBINE_POLICY=0 says so."""
    lf.release()                      # the child needs the memory of this process's input pool
    lf.run_child(POLICY0_NODES, {"TDEQ_COMBINE_POLICY": "0"}, POLICY0_TIMEOUT)
