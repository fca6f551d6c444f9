"""The multi-GPU path's collectives through RCCL on the GPU box (the 1-GPU lease can only run world
size 1, so the process group is handed over explicitly and nothing is short-circuited) and the device guard."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_rccl_world1_allreduce_tail_and_lockstep():
    """tests/_rccl_world1.py in its own process (own process group; a hung collective cannot stall the suite)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29631")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_rccl_world1.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_WORLD1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _run_bench(argv, env, tmp_path, timeout):
    """bench.py as a subprocess: (return code, the contract line = the ONLY stdout line starting with '{', the extras
    file's content or None, raw stdout/stderr tails)."""
    import json
    env = dict(env, TDEQ_BENCH_EXTRAS_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "bench.py")] + argv, env=env,
                       capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    extras = None
    for f in os.listdir(tmp_path):
        if f.startswith("bench_extras_n") and f.endswith(".json"):
            extras = json.load(open(os.path.join(tmp_path, f)))
    return r, lines, extras


def test_bench_self_launches_two_ranks_gloo(tmp_path):
    """`python bench.py --gpus 2` as a plain command (no torchrun wrapper): it re-launches itself as 2 ranks; with
    fewer GPUs than ranks the ranks share the device over gloo and the line says so.  ONE stdout JSON line < 4 KB
    (the contract: scalars only) with n_gpus 2 and one scalar pair per regime; the per-rank breakdowns, the adjoint
    objects with their all-reduce and the census are in the extras file the line names."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    if torch.cuda.device_count() < 2:
        env["TDEQ_DIST_BACKEND"] = "gloo"
    r, lines, out = _run_bench(["--gpus", "2", "--steps", "10", "--warmup", "3", "--full"], env, tmp_path, 900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-2000:]
    assert len(lines[0]) < 4096, len(lines[0])
    line = json.loads(lines[0])
    two_gpus = torch.cuda.device_count() >= 2
    # the contract line: N > 1 defaults to STRONG scaling (BASELINE.json's metric is quoted at batch 65536 in total)
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0 and line["steps"] == 10
    assert line["config"]["global_batch"] == 65536 and line["config"]["rows_per_gpu"] == 32768
    assert line["strong"]["value"] > 0 and line["weak"]["value"] > 0 and line["lockstep"]["value"] > 0
    assert line["backend"] == ("nccl" if two_gpus else "gloo") and line["rccl_ranks"] == (2 if two_gpus else None)
    assert line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"]
    for mode in ("strong", "weak"):
        assert line["adjoint"][mode]["allreduce_calls"] == 1 and line["adjoint"][mode]["ms_per_pass"] > 0
    assert not any(isinstance(v, list) for v in line.values())          # no per-rank arrays in the contract line
    assert line["extras_file"].endswith("bench_extras_n2.json") and out is not None
    # the extras file: everything else
    assert out["value"] == pytest.approx(line["value"], rel=1e-5)
    assert out["weak"]["config"]["global_batch"] == 2 * 65536
    bd = out["breakdown"]
    assert [r_["rank"] for r_ in bd["per_rank"]] == [0, 1] and bd["floor_ms"] > 0
    for r_ in bd["per_rank"]:
        assert r_["solver_dispatches_per_call"] >= 7 and r_["func_dispatches_per_call"] >= 6
        assert r_["solver_kernel_us"] > 0 and r_["func_kernel_us"] > 0
    assert abs(bd["floor_ms"] - (max(r_["floor_us"] for r_ in bd["per_rank"]) * 1e-3)) < 1e-9
    assert out["adjoint"]["strong"]["breakdown"]["floor_ms"] > 0
    for mode in ("strong", "weak"):
        ar = out["adjoint"][mode]["allreduce"]
        assert ar["calls"] == 1 and ar["bytes"] >= 4 * 98880 and ar["ms"] > 0
    assert out["comm"]["comm_ranks"] == 2 and [d["rank"] for d in out["comm"]["devices"]] == [0, 1]
    assert "extras_timed_out" not in out and set(out["extras_s"]) >= {"weak", "lockstep", "adjoint"}


@pytest.mark.skipif(torch.cuda.device_count() >= 8, reason="on an 8-GPU node the driver's own run covers N = 8 over RCCL")
def test_bench_self_launches_eight_ranks_gloo(tmp_path):
    """r06: the N = 8 control flow — the command the driver runs on an 8-GPU node, `python bench.py
    --gpus 8` — executed once on the 1-GPU lease with the ranks sharing the device over gloo: 8 self-launched ranks, the
    strong split at 8192 rows per rank, weak / lock-step / adjoint regimes, the watchdog, ONE stdout line < 4 KB.  Nothing
    here measures scaling (one GPU serves all ranks); it shows that the N = 8 path cannot fail on the day an 8-GPU node
    exists for a reason findable today."""
    import json
    import time
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TDEQ_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    t0 = time.time()
    r, lines, out = _run_bench(["--gpus", "8", "--steps", "5", "--warmup", "2", "--full"], env, tmp_path, 900)
    elapsed = time.time() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-2000:]
    assert len(lines[0]) < 4096, len(lines[0])
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["scaling"] == "strong" and line["value"] > 0 and line["steps"] == 5
    assert line["config"]["global_batch"] == 65536 and line["config"]["rows_per_gpu"] == 8192
    assert line["backend"] == "gloo" and line["rccl_ranks"] is None
    assert not any(isinstance(v, list) for v in line.values())
    hung = (out or {}).get("extras_hung_in") or line.get("extras_hung_in")
    for regime in ("strong", "weak", "lockstep"):
        assert (regime in line and line[regime]["value"] > 0) or (hung and regime in str(hung)), (regime, hung)
    assert "adjoint" in line or (hung and "adjoint" in str(hung))
    if "adjoint" in line:
        for mode in ("strong", "weak"):
            assert line["adjoint"][mode]["allreduce_calls"] == 1
    assert out is not None and line["extras_file"].endswith("bench_extras_n8.json")
    assert out["comm"]["comm_ranks"] == 8 and [d["rank"] for d in out["comm"]["devices"]] == list(range(8))
    assert [r_["rank"] for r_ in out["breakdown"]["per_rank"]] == list(range(8))
    print("bench.py --gpus 8 over gloo on one GPU: {:.1f} s".format(elapsed))
    assert elapsed < 300, elapsed


def test_bench_census_through_rccl_at_world_size_one(tmp_path):
    """bench.py's communicator census — the all-reduce of ones ON THE DEVICE and the gather of the ranks' GPU identities
    that every N > 1 run performs before timing anything — executed through RCCL itself: TDEQ_DIST_FORCE_INIT=1 creates
    the nccl process group (bound to the rank's GPU, as dist.init_from_env does for N ranks) at world size 1."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TDEQ_DIST_FORCE_INIT="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29723")
    env.pop("TDEQ_DIST_BACKEND", None)
    r, lines, out = _run_bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-extras",
                                "--no-cpu-baseline"], env, tmp_path, 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads(lines[-1])
    assert len(lines) == 1 and len(lines[0]) < 4096
    assert line["backend"] == "nccl" and line["rccl_ranks"] == 1 and line["value"] > 0
    assert out["backend"] == "nccl" and out["rccl_ranks"] == 1 and out["comm"]["comm_ranks"] == 1
    dev = out["comm"]["devices"][0]
    assert dev["rank"] == 0 and dev["device_index"] == 0 and dev["device_name"]
    assert out["value"] > 0 and out["n_gpus"] == 1


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="needs FEWER visible GPUs than ranks")
def test_bench_refuses_more_ranks_than_gpus_without_an_explicit_backend():
    """`--gpus 2` on a 1-GPU box with TDEQ_DIST_BACKEND unset: no silent gloo run — one JSON error line, status 2;
    the same under torch.distributed.run (the way the driver launches N > 1)."""
    import json
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("TDEQ_DIST_BACKEND", None)
    bench = os.path.join(os.path.dirname(HERE), "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--steps", "5", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["value"] is None and "RCCL needs one GPU per rank" in line["error"]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29717", bench, "--gpus", "2", "--steps", "5",
                        "--warmup", "1"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["value"] is None


def test_device_guard_switching_branch_runs_on_a_one_gpu_box(monkeypatch):
    """The two-GPU test below cannot run on the GPU box the suite gets (one MI355X).  What it protects is the guard's
    switching branch — `torch.cuda.device(state's device)` around every entry point — so that branch is made to run
    here: the guard is told that the caller's current device is cuda:1 (`_GuardProbe.pretend_current`), the state lives
    on cuda:0, and forward, fixed-grid, event, dense and adjoint (forward + backward, entered from the autograd engine's
    thread) solves must each pass through it and give the bits of an unguarded run."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd import _native
    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 16).cuda()
    y0 = torch.randn(64, 16, device="cuda:0")
    t = torch.tensor([0.0, 0.5, 1.0], device="cuda:0")

    def run():
        out = {}
        with torch.no_grad():
            out["dopri5"] = tda.odeint(lambda t_, y_: lin(y_), y0, t, method="dopri5")
            out["rk4"] = tda.odeint(lambda t_, y_: lin(y_), y0, t, method="rk4")
            et, ey = tda.odeint_event(lambda t_, y_: lin(y_), y0, t[0], event_fn=lambda t_, y_: t_ - 0.3, method="dopri5")
            out["event_t"], out["event_y"] = et, ey
            out["dense"] = tda.odeint_dense(lambda t_, y_: lin(y_), y0, t[0], t[-1])(torch.tensor(0.37))
        x = y0.clone().requires_grad_(True)
        lin.zero_grad()
        tda.odeint_adjoint(lambda t_, y_: lin(y_), x, t, adjoint_params=tuple(lin.parameters()))[-1].pow(2).sum().backward()
        out["grad_x"], out["grad_w"] = x.grad.clone(), lin.weight.grad.clone()
        return out
    plain = run()
    monkeypatch.setattr(_native._GuardProbe, "pretend_current", 1)
    monkeypatch.setattr(_native._GuardProbe, "switched", 0)
    guarded = run()
    assert _native._GuardProbe.switched >= 6, _native._GuardProbe.switched
    for k in plain:
        assert torch.equal(plain[k], guarded[k]), k
    assert torch.cuda.current_device() == 0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_state_on_a_non_current_device():
    """y0 on cuda:1 while cuda:0 is the current device: the kernels must go to cuda:1's stream (device guard)."""
    import torchdiffeq_amd as tda
    torch.cuda.set_device(0)
    A = (torch.randn(32, 32) / 6 - 0.1 * torch.eye(32))
    y0 = torch.randn(256, 32)
    t = torch.tensor([0.0, 1.0])
    outs = []
    for dev in ("cuda:0", "cuda:1"):
        Ad = A.to(dev)
        with torch.no_grad():
            outs.append(tda.odeint(lambda tt, y: y @ Ad.T, y0.to(dev), t.to(dev), rtol=1e-6, atol=1e-8).cpu())
        lin = torch.nn.Linear(32, 32).to(dev)
        x = y0.to(dev).requires_grad_(True)
        tda.odeint_adjoint(lambda tt, y: lin(y), x, t.to(dev), adjoint_params=tuple(lin.parameters()))[-1].sum().backward()
        assert torch.isfinite(x.grad).all()
    assert torch.cuda.current_device() == 0
    assert torch.equal(outs[0], outs[1])
