"""Every cache policy of the streaming launches (csrc/tdeq_abi.hip `stream_policy()`), at the small shapes of the kernel
tests.  Five entry points take a policy — stage_combine, stage_combine_err, stage_combine_multi, stage_combine_sel and
error_norm_partial: above 512 MiB of streams they launch the POLICY 1-3 instantiations (non-temporal loads / stores
through `ld_stream` / `st_stream`), and stage_combine_multi then always takes its generic kernel (run-time output count,
run-time `acc_in` test, the step size from either side, no ONEPASS).  The two variables that force a policy are read
once per process, so each setting gets ONE fresh pytest child that runs the kernel-against-oracle tests listed in `NODES`:

    TDEQ_COMBINE_POLICY = 0, 1, 2, 3          TDEQ_NT_THRESHOLD_MB = 0 (the size rule choosing policy 3 at every size)

A child must end with status 0, nothing failed, nothing skipped, and as many passed as the list holds when it is
collected with neither variable set.  A child that ends by signal or time limit fails its case and every later one
without another process being started.

`NODES` = the existing tests of the five entry points (fp32 and fp64; sizes 1, 255, 4099, 65536 + 7 or + 3, 2^20; the
unaligned scalar path, which ignores the policy; for stage_combine_multi the dopri5 / dopri8 / tsit5 plans: 1, 2 and more
outputs, with and without `acc_in`, masks with structural zeros, host and device dt) plus the comparisons below, which
give the launch sites no existing test ties to the oracle at those shapes: stage_combine_sel at 255, 4099 and 2^20 and
through unaligned views, stage_combine_multi at 255 and 4099, stage_combine_err and error_norm_partial through unaligned
views.  The tests below that START
children are never in a child's list (and refuse to run inside one).
"""
import pytest
import torch

import _launch_forms as lf
from torchdiffeq_amd.tableaus import DOPRI5, SparseRow

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]
HERE = "tests/test_launch_policy_gpu.py"

NODES = [
    "tests/test_kernels_gpu.py::test_stage_combine_all_rows",
    "tests/test_kernels_gpu.py::test_stage_combine_unaligned",
    "tests/test_kernels_gpu.py::test_fused_end_of_step_pair",
    "tests/test_kernels_gpu.py::test_stage_combine_dev_equals_host_dt_kernels",
    "tests/test_carry.py::test_planned_rows_equal_row_by_row_hip_and_oracle",
    "tests/test_carry.py::test_multi_with_the_step_size_on_the_device_equals_host_dt",
    "tests/test_carry.py::test_multi_unaligned_views_take_the_scalar_path",
    "tests/test_lookahead.py::test_stage_combine_sel_bit_exact",
    "tests/test_lookahead.py::test_controller_kernel_vs_oracle",
    "tests/test_lookahead.py::test_controller_kernel_many_segments",
    "tests/test_lookahead.py::test_norm_launch_also_writes_the_last_stage_for_captured_steps",
    "tests/test_graph_mode_gpu.py::test_adaptive_graph_mode_equals_eager",
    f"{HERE}::test_sel_against_the_oracle",
    f"{HERE}::test_multi_against_the_oracle",
    f"{HERE}::test_fused_pair_through_unaligned_views_against_the_oracle",
]
STARTS_CHILDREN = ("test_every_policy_in_a_child", "test_no_child_list_names_a_test_that_starts_children")
# One plain child (neither variable set) ran the twelve existing tests of this list in 14.2 s on the MI355X at the parent
# commit (257 tests, 10.7 s inside pytest), and the whole list in 14.6 s with this file in place (287 tests, 11.0 s); the
# limit is 5 x that = 73 s, rounded up.
CHILD_SECONDS_MEASURED = 14.6
CHILD_TIMEOUT = 75

SETTINGS = [{"TDEQ_COMBINE_POLICY": "0"}, {"TDEQ_COMBINE_POLICY": "1"}, {"TDEQ_COMBINE_POLICY": "2"},
            {"TDEQ_COMBINE_POLICY": "3"}, {"TDEQ_NT_THRESHOLD_MB": "0"}]


def test_no_child_list_names_a_test_that_starts_children():
    for node in NODES:
        assert "::" in node and not any(node.endswith(name) for name in STARTS_CHILDREN), node
    assert CHILD_TIMEOUT >= max(60, 5 * CHILD_SECONDS_MEASURED)


@pytest.mark.parametrize("setting", SETTINGS, ids=["policy0", "policy1", "policy2", "policy3", "threshold0"])
def test_every_policy_in_a_child(setting):
    torch.cuda.empty_cache()
    lf.run_child(NODES, setting, CHILD_TIMEOUT)


# ---- comparisons the existing tests do not make (listed in NODES) ---------------------------------------------------------
def _rand(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float64).to(dtype)


def _dev(t, offset):
    """On the GPU; offset 1: a view one element past a 16-byte boundary (the scalar path, which takes no policy)."""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    buf[offset:].copy_(t)
    assert (buf[offset:].data_ptr() % 16 == 0) == (offset == 0)
    return buf[offset:]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", [1, 255, 4099, 65536 + 7, 1 << 20])
def test_sel_against_the_oracle(hip_kernels, oracle_kernels, dtype, offset, n):
    ts = [_rand(n, dtype, 70 + j) for j in range(4)]
    td = [_dev(t, offset) for t in ts]
    plan_d = hip_kernels.make_plan([(0, n, 1e-6, 1e-8)], n, 1024, torch.device("cuda:0"))
    plan_o = oracle_kernels.make_plan([(0, n, 1e-6, 1e-8)], n, 1024, None)
    for accept in (0.0, 1.0):
        for dt in (0.0371, -0.25):
            words = torch.tensor([accept, lf.as_type(dt, dtype)], dtype=torch.float64)
            plan_d.ctrl_dev[:2].copy_(words)
            plan_o.ctrl_dev.copy_(words)
            out = lf.Window((n,), dtype, offset)
            ref = torch.empty_like(ts[0])
            hip_kernels.stage_combine_sel(out.t, td[0], td[1], td[2], td[3], 0.2, plan_d)
            oracle_kernels.stage_combine_sel(ref, ts[0], ts[1], ts[2], ts[3], 0.2, plan_o)
            lf.same_bits(out.t.cpu(), ref, (n, offset, accept, dt))
            assert out.intact()


MULTI_COEF = (0.0371, -0.211, 0.5, 1.25, -0.0625, 0.33)
MULTI_ROWS = ((MULTI_COEF, 0b111111, True), ((0.0, 0.7, 0.0, -0.3, 0.9, 0.0), 0b011010, False),         # structural zeros
              ((0.4, 0.0, 0.0, 0.2, 0.0, -1.5), 0b101001, True), ((0.0, 0.0, 0.6, 0.0, 0.0, 0.0), 0b000100, False))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [255, 4099])
def test_multi_against_the_oracle(hip_kernels, oracle_kernels, dtype, n):
    """stage_combine_multi with 1, 2 and 4 outputs, with and without `acc_in`, the step size from the host and from the
    device, at the two sizes tests/test_carry.py does not have on the GPU."""
    y0, acc, *ks = [_rand(n, dtype, 30 + j) for j in range(8)]
    y0d, accd, *ksd = [_dev(t, 0) for t in (y0, acc, *ks)]
    plan = hip_kernels.make_plan([(0, n, 1e-6, 1e-8)], n, 1024, torch.device("cuda:0"))
    for dt in (0.37, -0.011):
        dtT = lf.as_type(dt, dtype)
        plan.ctrl_dev[:2].copy_(torch.tensor([1.0, dtT], dtype=torch.float64))
        for n_out in (1, 2, 4):
            rows = MULTI_ROWS[:n_out]
            for with_acc in (True, False):
                ref = [torch.empty_like(y0) for _ in rows]
                oracle_kernels.stage_combine_multi(ref, rows, y0, acc if with_acc else None, ks, dtT)
                for on_device in (False, True):
                    outs = [lf.Window((n,), dtype) for _ in rows]
                    if on_device:
                        hip_kernels.stage_combine_multi_dev([w.t for w in outs], rows, y0d, accd if with_acc else None, ksd, plan)
                    else:
                        hip_kernels.stage_combine_multi([w.t for w in outs], rows, y0d, accd if with_acc else None, ksd, dtT)
                    for o, (w, r) in enumerate(zip(outs, ref)):
                        lf.same_bits(w.t.cpu(), r, (n, dt, n_out, with_acc, on_device, o))
                        assert w.intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [255, 4099, 65536 + 7])
def test_fused_pair_through_unaligned_views_against_the_oracle(hip_kernels, oracle_kernels, dtype, n):
    """stage_combine_err and error_norm_partial on views one element off alignment (dopri5's last row and error row):
    elementwise outputs bit for bit; the fp64 sums to 1e-12 as in tests/test_kernels_gpu.py (the two sides add the same
    per-element values in another order)."""
    last, err = DOPRI5.beta_rows()[-1], SparseRow.from_dense(DOPRI5.c_error)
    n_lead, dt = len(last.idx), -0.0371
    y0, y1 = _rand(n, dtype, 1), _rand(n, dtype, 2)
    ks = [_rand(n, dtype, 10 + j) for j in range(DOPRI5.n_stages + 1)]
    y0d, y1d, ksd = _dev(y0, 1), _dev(y1, 1), [_dev(k, 1) for k in ks]
    out_ref, ep_ref = torch.empty_like(y0), torch.empty_like(y0)
    oracle_kernels.stage_combine_err(out_ref, ep_ref, y0, [ks[j] for j in last.idx], last.coef, err.coef[:n_lead], dt)
    out, ep = lf.Window((n,), dtype, 1), lf.Window((n,), dtype, 1)
    hip_kernels.stage_combine_err(out.t, ep.t, y0d, [ksd[j] for j in last.idx], last.coef, err.coef[:n_lead], dt)
    lf.same_bits(out.t.cpu(), out_ref)
    lf.same_bits(ep.t.cpu(), ep_ref)
    assert out.intact() and ep.intact()
    for chunk in (1024, 2048):
        pg = hip_kernels.make_plan([(0, n, 1e-3, 1e-4)], n, chunk, torch.device("cuda:0"))
        pc = oracle_kernels.make_plan([(0, n, 1e-3, 1e-4)], n, chunk, None)
        rest_idx, rest_coef = err.idx[n_lead:], err.coef[n_lead:]
        hip_kernels.error_norm_partial(pg, ep.t, y0d, y1d, [ksd[j] for j in rest_idx], rest_coef, dt)
        got, _, bad = hip_kernels.read_norms(pg)
        oracle_kernels.error_norm_partial(pc, ep_ref, y0, y1, [ks[j] for j in rest_idx], rest_coef, dt)
        want, _, _ = oracle_kernels.read_norms(pc)
        assert bad == [0.0] and got[0] == pytest.approx(want[0], rel=1e-12)
