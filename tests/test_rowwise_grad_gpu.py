"""Gradients through `odeint_rowwise(..., differentiable=True)` on the HIP kernels: the two backward kernels
(`tdeq_row_scale_many`, `tdeq_row_multi_dot`) against torch, and the recorded solve against the reference's per-row
gradients, the host path, and itself at other batch sizes."""
import warnings

import pytest
import torch

from _rowwise_grad_cases import CASE_NAMES, METHODS, loss_weights, random_problem, row_bounds, solve_case

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        yield


def _rows(B, L, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(B, L, generator=g, dtype=torch.float64, device=DEV).to(dtype)


# -- kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("L", [1, 3, 4, 127, 128, 2048, 2049, (1 << 15) + 5])
def test_row_scale_many(L, dtype):
    """outs[m][r, :] = w[m, r] * g[r, :] with ONE rounding: equal to torch's product bit for bit; 16-byte and scalar
    elements, 1 and 14 outputs, weights with exact 0 and 1.  4096 rows of 2^15 + 5 elements (134M scalar-path items) is
    the one case with more items than the capped grid has threads (65536 x 256): only there does a lane walk on to a
    second element, in another row, and fetch that row's weights over the ones it holds."""
    kern = _native.get_kernels(DEV, dtype)
    for B in (1, 7, 4096):
        g = _rows(B, L, dtype, L + B)
        for n_out in (1, 14):
            w = _rows(n_out, B, dtype, 3 * L + n_out)
            w[0, ::2] = 0.0
            w[-1, ::3] = 1.0
            outs = [torch.full_like(g, float("nan")) for _ in range(n_out)]
            kern.row_scale_many(outs, g, w)
            torch.cuda.synchronize()
            for m in range(n_out):          # (one product at a time: the large case has 1 GiB per tensor)
                assert torch.equal(outs[m], w[m][:, None] * g), (B, L, n_out, m)
            del outs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("L", [1, 3, 4, 127, 128, 2048, 2049, (1 << 15) + 5, 1025, 1500, 2047, 4096, 4100, 8192])
def test_row_multi_dot(L, dtype):
    """out[m, r] = <g[r], x_m[r]> in fp64: within the bound of an fp64 accumulation of L terms (L * 2^-53 * sum|g x|),
    and the same bits for a row at B = 1 and inside a large batch."""
    kern = _native.get_kernels(DEV, dtype)
    B = 4096 if L <= 2049 else 64
    g = _rows(B, L, dtype, L)
    xs = [_rows(B, L, dtype, 100 + L + m) for m in range(3)]
    out = kern.row_multi_dot(g, xs)
    torch.cuda.synchronize()
    assert out.shape == (3, B) and out.dtype == torch.float64
    for m in range(3):
        prod = g.double() * xs[m].double()
        bound = (L + 1) * 2.0 ** -53 * prod.abs().sum(dim=1) + 1e-300
        assert bool(((out[m] - prod.sum(dim=1)).abs() <= bound).all()), (L, m)
    for r in (0, B // 2, B - 1):
        one = kern.row_multi_dot(g[r:r + 1].clone(), [x[r:r + 1].clone() for x in xs])
        assert torch.equal(one[:, 0], out[:, r]), (L, r)
    # 14 inputs in one launch, and 1: the most and the fewest the entry point takes
    many = [_rows(5, L, dtype, 200 + m) for m in range(14)]
    g5 = _rows(5, L, dtype, 7)
    for xs in (many, many[:1]):
        out = kern.row_multi_dot(g5, xs)
        for m in range(len(xs)):
            prod = g5.double() * xs[m].double()
            assert bool(((out[m] - prod.sum(dim=1)).abs() <= (L + 1) * 2.0 ** -53 * prod.abs().sum(dim=1) + 1e-300).all())


def test_row_kernels_empty_and_invalid():
    kern = _native.get_kernels(DEV, torch.float32)
    lib = kern.lib
    g = torch.zeros(4, 4, device=DEV)
    ptrs = (_native.ctypes.c_void_p * 1)(g.data_ptr())
    out = torch.ones(4, dtype=torch.float64, device=DEV)
    assert lib.tdeq_row_scale_many(ptrs, 1, g.data_ptr(), g.data_ptr(), 0, 4, 0, None) == 0
    assert lib.tdeq_row_scale_many(ptrs, 1, g.data_ptr(), g.data_ptr(), 4, 0, 0, None) == 0
    assert lib.tdeq_row_scale_many(ptrs, 15, g.data_ptr(), g.data_ptr(), 4, 4, 0, None) == -1
    assert lib.tdeq_row_scale_many(ptrs, 0, g.data_ptr(), g.data_ptr(), 4, 4, 0, None) == -1
    for n_x in (0, 15):
        assert lib.tdeq_row_multi_dot(g.data_ptr(), ptrs, n_x, 4, 4, out.data_ptr(), None, 0, 0, None) == -1
    assert lib.tdeq_row_multi_dot(g.data_ptr(), ptrs, 1, 0, 4, out.data_ptr(), None, 0, 0, None) == 0
    assert lib.tdeq_row_multi_dot(g.data_ptr(), ptrs, 1, 4, 0, out.data_ptr(), None, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0.0] * 4                       # row_len == 0: zeros
    assert lib.tdeq_row_multi_dot(g.data_ptr(), ptrs, 1, 4, 1 << 20, out.data_ptr(), None, 0, 0, None) == -2
    assert lib.tdeq_row_dots_workspace_bytes(4, 1 << 20, 3, 0) == 3 * 4 * 128 * 8


# -- solves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hip_reference_rows(name):
    """tests/test_rowwise_grad.py::test_reference_rows on the device: every row, a tenth of the reference's spread."""
    dev, spread, stats, counts = solve_case(tda, name, device=DEV)
    bounds = row_bounds(name)
    print(f"{name}: worst row deviation {float(dev.max()):.3e} (row {int(dev.argmax())}), case bound {0.1 * spread:.3e}")
    print("   per row deviation / bound: " + " ".join(f"{float(d):.1e}/{float(b):.1e}" for d, b in zip(dev, bounds)))
    if counts is not None:
        assert stats["n_accepted"].tolist() == counts[0]
        assert stats["n_rejected"].tolist() == counts[1]
    for r in range(len(dev)):
        assert float(dev[r]) < 0.1 * spread, (name, r, float(dev[r]), spread)
        assert float(dev[r]) < float(bounds[r]), (name, r, float(dev[r]), float(bounds[r]))


@pytest.mark.parametrize("kind", ["t1d", "t2d"])
@pytest.mark.parametrize("method", METHODS)
def test_hip_forward_bits(method, kind):
    y0, make = random_problem(37, 6, torch.float64, 11)
    t = torch.linspace(0, 1.5, 5, dtype=torch.float64)
    if kind == "t2d":
        t = t[:, None] * torch.linspace(0.4, 1.0, 37, dtype=torch.float64) + 0.05 * torch.arange(37)
    y0, t = y0.to(DEV), t.to(DEV)
    with torch.no_grad():
        plain, sp = tda.odeint_rowwise(make(DEV), y0, t, rtol=1e-6, atol=1e-8, method=method, return_stats=True)
    rec, sr = tda.odeint_rowwise(make(DEV), y0.clone().requires_grad_(True), t, rtol=1e-6, atol=1e-8, method=method,
                                 return_stats=True, differentiable=True)
    assert rec.requires_grad and torch.equal(rec, plain)
    assert sr["nfe"] == sp["nfe"]
    assert torch.equal(sr["n_accepted"], sp["n_accepted"]) and torch.equal(sr["n_rejected"], sp["n_rejected"])


def _grad_y0(make, y0, t, W, idx=None, device=DEV, **kw):
    y = (y0 if idx is None else y0[idx]).to(device).clone().requires_grad_(True)
    sol, stats = tda.odeint_rowwise(make(device, idx), y, t.to(device), return_stats=True, differentiable=True, **kw)
    Wd = (W if idx is None else W[:, idx]).to(device)
    return torch.autograd.grad((sol * Wd).sum(), y)[0], stats


def _row_rel(a, b):
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return (a - b).flatten(1).abs().amax(dim=1) / b.flatten(1).abs().amax(dim=1).clamp_min(1e-300)


@pytest.mark.parametrize("method", METHODS)
def test_hip_gradient_matches_host_path_fp64(method):
    """The bounds of tests/test_rowwise_gpu.py::test_hip_matches_host_path_fp64 for the solution, applied per row to the
    y0 gradient."""
    y0, make = random_problem(96, 5, torch.float64, 1)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    W = loss_weights((4, 96, 5), torch.float64)
    cpu, sc = _grad_y0(make, y0, t, W, device="cpu", rtol=1e-6, atol=1e-8, method=method)
    gpu, sg = _grad_y0(make, y0, t, W, rtol=1e-6, atol=1e-8, method=method)
    assert sg["n_accepted"].tolist() == sc["n_accepted"].tolist()
    assert sg["n_rejected"].tolist() == sc["n_rejected"].tolist()
    rel = _row_rel(gpu, cpu)
    print(f"{method}: worst row {float(rel.max()):.3e}")
    bound = 1e-7 if method == "dopri8" else 1e-12
    for r in range(96):
        assert float(rel[r]) < bound, (r, float(rel[r]))


def test_hip_gradient_matches_host_path_fp32():
    y0, make = random_problem(200, 8, torch.float32, 2)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float32)
    W = loss_weights((4, 200, 8), torch.float32)
    cpu, sc = _grad_y0(make, y0, t, W, device="cpu", rtol=1e-4, atol=1e-6)
    gpu, sg = _grad_y0(make, y0, t, W, rtol=1e-4, atol=1e-6)
    differ = (sg["n_accepted"] != sc["n_accepted"]) | (sg["n_rejected"] != sc["n_rejected"])
    assert int(differ.sum()) <= 2          # at most 1 % of the rows
    rel = _row_rel(gpu, cpu)
    print(f"fp32: worst row with equal counts {float(rel[~differ].max()):.3e}")
    for r in range(200):
        if not differ[r]:
            assert float(rel[r]) < 1e-5, (r, float(rel[r]))


@pytest.mark.parametrize("B", [1, 37, 4096])
def test_hip_gradient_batch_invariance(B):
    y0, make = random_problem(4096, 6, torch.float64, 3)
    t = torch.linspace(0, 1, 3, dtype=torch.float64)
    W = loss_weights((3, 4096, 6), torch.float64)
    full, _ = _grad_y0(make, y0, t, W, rtol=1e-6, atol=1e-8)
    idx = torch.randperm(4096, generator=torch.Generator().manual_seed(B))[:B]
    part, _ = _grad_y0(make, y0, t, W, idx=idx, rtol=1e-6, atol=1e-8)
    assert torch.equal(part, full[idx.to(DEV)])


def test_hip_shared_parameters_sum_over_rows():
    B, D = 64, 4
    g = torch.Generator().manual_seed(7)
    lin = torch.nn.Linear(D, D).double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(D, D, generator=g, dtype=torch.float64) * 0.5 - 0.3 * torch.eye(D))
    lin = lin.to(DEV)
    y0 = torch.randn(B, D, generator=g, dtype=torch.float64).to(DEV)
    t = torch.tensor([0.0, 0.4, 1.0], dtype=torch.float64, device=DEV)
    W = loss_weights((3, B, D), torch.float64, DEV)
    field = lambda t_, y: torch.tanh(lin(y)) * torch.cos(t_)[:, None]      # noqa: E731
    sol = tda.odeint_rowwise(field, y0, t, rtol=1e-6, atol=1e-8, differentiable=True)
    gw, gb = torch.autograd.grad((sol * W).sum(), [lin.weight, lin.bias])
    sw, sb = torch.zeros_like(gw), torch.zeros_like(gb)
    for r in range(B):
        one = tda.odeint_rowwise(field, y0[r:r + 1], t, rtol=1e-6, atol=1e-8, differentiable=True)
        a, b = torch.autograd.grad((one * W[:, r:r + 1]).sum(), [lin.weight, lin.bias])
        sw, sb = sw + a, sb + b
    rel = max(float((gw - sw).abs().max() / sw.abs().max()), float((gb - sb).abs().max() / sb.abs().max()))
    print(f"shared parameters: relative difference to the sum of single-row gradients {rel:.3e}")
    assert rel < 1e-10


def test_hip_finished_and_rejected_rows():
    B = 10
    y0, make = random_problem(B, 2, torch.float64, 21)
    tg = torch.linspace(0, 1, 5, dtype=torch.float64)[:, None] ** 1.5 * torch.linspace(0.3, 3.0, B, dtype=torch.float64)
    W = loss_weights((5, B, 2), torch.float64)
    full, stats = _grad_y0(make, y0, tg, W, rtol=1e-5, atol=1e-7, method="bosh3")
    n_rej = stats["n_rejected"]
    assert int((n_rej > 0).sum()) > 0 and int((n_rej == 0).sum()) > 0, n_rej.tolist()
    assert torch.isfinite(full).all()
    for r in range(B):
        idx = torch.tensor([r])
        one, _ = _grad_y0(make, y0, tg[:, r], W, idx=idx, rtol=1e-5, atol=1e-7, method="bosh3")
        assert torch.equal(one[0], full[r]), r


def test_hip_long_rows():
    """A state of 2^22 elements (2 rows of 2^21: the chunked row dots of the first step and the long-row scale walk),
    against the same rows solved alone."""
    B, L = 2, 1 << 21
    g = torch.Generator().manual_seed(4)
    k = torch.tensor([[0.5], [4.0]])
    y0 = torch.randn(B, L, generator=g, dtype=torch.float32)
    t = torch.tensor([0.0, 0.5, 1.0])
    W = torch.cos(torch.arange(L, dtype=torch.float32) * 1e-3).expand(3, B, L)

    def make(device, idx=None):
        kk = (k if idx is None else k[idx]).to(device)
        # (autonomous: a time term would put a sum over the 2^21 elements of a row into func's own backward, whose
        #  order ATen chooses by shape)
        return lambda t_, y: -kk * y + 0.25 * torch.roll(y, 1, dims=1)
    full, _ = _grad_y0(make, y0, t, W, rtol=1e-5, atol=1e-7)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    for r in range(B):
        one, _ = _grad_y0(make, y0, t, W, idx=torch.tensor([r]), rtol=1e-5, atol=1e-7)
        assert torch.equal(one[0], full[r])


@pytest.mark.parametrize("L", [4100, 1501])
def test_hip_one_chunk_long_rows(L):
    """`test_hip_long_rows` at long rows of ONE chunk (1024 < 16-byte or scalar elements <= 2048: the chunk kernels
    writing the row dots directly, no finalize pass), against the same rows solved alone and against the host path."""
    B = 3
    g = torch.Generator().manual_seed(L)
    k = torch.tensor([[0.5], [4.0], [1.5]])
    y0 = torch.randn(B, L, generator=g, dtype=torch.float32)
    t = torch.tensor([0.0, 0.5, 1.0])
    W = torch.cos(torch.arange(L, dtype=torch.float32) * 1e-3).expand(3, B, L)

    def make(device, idx=None):
        kk = (k if idx is None else k[idx]).to(device)
        return lambda t_, y: -kk * y + 0.25 * torch.roll(y, 1, dims=1)
    full, sg = _grad_y0(make, y0, t, W, rtol=1e-5, atol=1e-7)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    for r in range(B):
        one, _ = _grad_y0(make, y0, t, W, idx=torch.tensor([r]), rtol=1e-5, atol=1e-7)
        assert torch.equal(one[0], full[r])
    cpu, sc = _grad_y0(make, y0, t, W, device="cpu", rtol=1e-5, atol=1e-7)
    rel = _row_rel(full, cpu)
    for r in range(B):                     # (the fp32 bound of test_hip_gradient_matches_host_path_fp32, rows with equal counts)
        if int(sg["n_accepted"][r]) == int(sc["n_accepted"][r]) and int(sg["n_rejected"][r]) == int(sc["n_rejected"][r]):
            assert float(rel[r]) < 1e-5, (r, float(rel[r]))


def test_hip_second_order_is_refused():
    y = torch.ones(3, 2, dtype=torch.float64, device=DEV, requires_grad=True)
    sol = tda.odeint_rowwise(lambda t_, yy: -yy * yy, y, torch.tensor([0.0, 1.0], device=DEV), differentiable=True)
    with pytest.raises(NotImplementedError, match="second-order"):
        torch.autograd.grad(sol.pow(2).sum(), y, create_graph=True)
