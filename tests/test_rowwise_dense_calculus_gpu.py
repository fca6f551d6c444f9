"""`RowDenseOutput.derivative` / `.antiderivative` / `.integral` on the MI355X end to end: `odeint_rowwise_dense` on the device
against the host path, bit for bit — plain and with `compact`, ascending and descending, with `jump_dy` — and the NaN rows of
`check=False`.

The comparison has two parts.  The host path on the DEVICE's record (the record copied to the CPU) must give the bits of the
HIP kernels, always: that is the parity of the new kernels.  And against the host SOLVE of the same problem: the three
methods are functions of the record alone, so wherever that solve's record has the device record's bits its results must
have the device's bits too; where the two solves took different steps (this change does not touch the solve) the results
are compared to the accuracy of the solve instead."""
import copy

import pytest
import torch

from _rowwise_dense_calculus_oracle import same_bits
from _rowwise_dense_oracle import decay_problem, per_row_t1, random_queries, tolerances

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, L, SEED, Q = 12, 5, 3, 5


def _solve(device, dtype, t0, t1, **kw):
    y0, func, _ = decay_problem(B, L, dtype, SEED, device)
    t1 = t1.to(device) if isinstance(t1, torch.Tensor) else t1
    kw = {k: ({n: (v.to(device) if isinstance(v, torch.Tensor) else v) for n, v in opt.items()} if k == "options" else opt)
          for k, opt in kw.items()}
    with torch.no_grad():
        return tda.odeint_rowwise_dense(func, y0, t0, t1, method="dopri5", **tolerances("dopri5", dtype), **kw)


def _on_host(dense):
    """The same record on the CPU, evaluated by the host path."""
    twin = copy.copy(dense)
    for name in ("_t0", "_t1", "_ta", "_tb", "offsets", "coeffs", "t0", "t1", "seg_start", "seg_end"):
        setattr(twin, name, getattr(dense, name).cpu())
    twin._k, twin._prefix = None, None
    return twin


def _queries(dense):
    """[Q + 3, B] on the CPU: interior points, t0, t1 and an interior breakpoint per row."""
    off = dense.offsets.tolist()
    t0, t1, ends = dense.t0.cpu(), dense.t1.cpu(), dense.seg_end.cpu()
    sign = dense._sign
    brk = torch.stack([ends[off[r] + (off[r + 1] - off[r]) // 2 - 1] if off[r + 1] - off[r] > 1 else t1[r] for r in range(B)])
    return torch.cat([random_queries(Q, t0 * sign, t1 * sign, 17) * sign, t0[None], t1[None], brk[None]])


def _three(dense, q):
    q = q.to(dense.coeffs.device)
    return dense.derivative(q), dense.antiderivative(q), dense.integral(q, q.flip(0))


CASES = {
    "up": dict(t0=0.0, t1=per_row_t1(B)),
    "up-compact": dict(t0=0.0, t1=per_row_t1(B), compact=True),
    "down": dict(t0=0.3, t1=0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)),
    "down-compact": dict(t0=0.3, t1=0.3 - torch.linspace(0.1, 0.3, B, dtype=F64), compact=True),
    "doses": dict(t0=0.0, t1=per_row_t1(B), options={
        "jump_t": (0.4 * per_row_t1(B))[None],
        "jump_dy": 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64)}),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host(case, dtype):
    kw = dict(CASES[case])
    if "options" in kw:
        kw["options"] = {**kw["options"], "jump_dy": kw["options"]["jump_dy"].to(dtype)}
    dense = _solve(DEV, dtype, **kw)
    assert dense.coeffs.device.type == DEV.type and dense._k is not None
    q = _queries(dense)
    if case == "doses":                                                      # the dose time, the times next to it
        p = kw["options"]["jump_t"]
        q = torch.cat([q, p, torch.nextafter(p, torch.zeros_like(p)), torch.nextafter(p, torch.ones_like(p))])
    got = _three(dense, q)
    assert all(g.device.type == DEV.type and g.shape == (q.shape[0], B, L) and not bool(torch.isnan(g).any()) for g in got)
    assert dense._prefix.device.type == DEV.type and dense._prefix.dtype == F64
    # 1. the host path on the device's record
    twin = _on_host(dense)
    for a, b in zip(got, _three(twin, q)):
        assert same_bits(a, b)
    assert same_bits(dense._prefix, twin._prefix)
    assert bool((dense.antiderivative(dense.t0[None]) == 0).all())
    # 2. the host solve of the same problem
    host = _solve("cpu", dtype, **kw)
    same_record = all(torch.equal(getattr(dense, n).cpu(), getattr(host, n)) for n in ("offsets", "seg_start", "seg_end", "coeffs"))
    print(f"{case}: the host solve has the device's record: {same_record}")
    want = _three(host, q)
    if same_record:
        for a, b in zip(got, want):
            assert same_bits(a, b)
    else:
        # two valid step sequences under one tolerance: the interpolants agree to the solve's accuracy, the derivative (one
        # order lower, divided by the step) to a hundred times that; relative to |value| + 1 as the mixed tolerance is
        tol = 1e-4 if dtype == F32 else 1e-6
        for a, b, factor in zip(got, want, (100, 1, 1)):
            a, b = a.cpu().double(), b.double()
            assert float(((a - b).abs() / (b.abs() + 1)).max()) < factor * tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_compact_gives_the_same_bits(dtype):
    plain, packed = _solve(DEV, dtype, **CASES["up"]), _solve(DEV, dtype, **CASES["up-compact"])
    q = _queries(plain)
    for a, b in zip(_three(plain, q), _three(packed, q)):
        assert same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_false_gives_nan_rows_and_raises_nothing(dtype):
    dense = _solve(DEV, dtype, **CASES["up"])
    good = random_queries(3, dense.t0, dense.t1, seed=9)
    q = good.clone()
    q[2, 1], q[1, 9], q[1, 3] = float("nan"), 5.0, -2.0
    for fn in (dense.derivative, dense.antiderivative, lambda t, **kw: dense.integral(t, good, **kw),
               lambda t, **kw: dense.integral(good, t, **kw)):
        got = fn(q, check=False)
        bad = torch.isnan(got).all(dim=2)
        assert bad.nonzero().tolist() == [[1, 3], [1, 9], [2, 1]]
        assert same_bits(got[~bad], fn(good)[~bad])
        with pytest.raises(ValueError, match=r"query 1 of row 3 "):
            fn(q)
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(tb = "):
        dense.integral(good, q)
    dense.drop_integral_cache()
    assert dense._prefix is None and not bool(torch.isnan(dense.integral(dense.t0[None], dense.t1[None])).any())
