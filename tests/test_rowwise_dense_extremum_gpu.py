"""`RowDenseOutput.maximum` / `.minimum` on the MI355X: `odeint_rowwise_dense` on the device against the host path, bit for bit
— plain and with `compact`, ascending and descending, with `jump_dy`, on oscillators — in the two-part scheme of
tests/test_rowwise_dense_calculus_gpu.py; then `row_dense_extremum` itself on a synthetic record: the scalar instantiation for a
misaligned base, sentinel borders around both outputs, NaN rows for out-of-range ends; and a window of more than 64 steps."""
import copy

import numpy as np
import pytest
import torch

from _rowwise_dense_extremum_oracle import MAXIMUM, MINIMUM, oscillator_problem, same_bits, windows
from _rowwise_dense_oracle import NONE, decay_problem, per_row_t1, tolerances
from _rowwise_kernels import SENTINEL

import torchdiffeq_amd as tda
from torchdiffeq_amd.rowwise import HostRowKernels

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B, SEED = 12, 3
BORDER = 8                                                   # elements: the payload stays 16-byte aligned


def _solve(device, dtype, L, problem="decay", t0=0.0, t1=None, **kw):
    if problem == "decay":
        y0, func, _ = decay_problem(B, L, dtype, SEED, device)
        t1 = per_row_t1(B) if t1 is None else t1
    else:
        y0, func, _, t1 = oscillator_problem(B, L, dtype, device)
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
    twin._k = None
    return twin


def _both(dense, qa, qb):
    dev = dense.coeffs.device
    return dense.maximum(qa.to(dev), qb.to(dev)), dense.minimum(qa.to(dev), qb.to(dev))


DOWN = 0.3 - torch.linspace(0.1, 0.3, B, dtype=F64)
CASES = {
    "up": dict(),
    "down": dict(t0=0.3, t1=DOWN),
    "compact": dict(compact=True),
    "doses": dict(options={"jump_t": (0.4 * per_row_t1(B))[None]}),
    "oscillator": dict(problem="oscillator"),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host(case, L, dtype):
    """L = 5: scalar elements; L = 8: 16-byte elements for both dtypes.  Windows: see `windows` — the whole row and its reverse,
    inside one segment, across and from a breakpoint, a single point; with doses also around the dose time."""
    kw = dict(CASES[case])
    if case == "doses":
        dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64)
        kw["options"] = {**kw["options"], "jump_dy": dy.to(dtype)}
    dense = _solve(DEV, dtype, L, **kw)
    assert dense.coeffs.device.type == DEV.type and dense._k is not None
    qa, qb = windows(dense)
    if case == "doses":                                                      # inside, near end, far end, the dose time itself
        p, t1 = kw["options"]["jump_t"], per_row_t1(B)[None]
        qa, qb = torch.cat([qa, 0.35 * t1, p, 0.35 * t1, p]), torch.cat([qb, 0.6 * t1, 0.6 * t1, p, p])
    got = _both(dense, qa, qb)
    for g in got:
        assert g.values.device.type == g.times.device.type == DEV.type and g.values.dtype == dtype and g.times.dtype == F64
        assert g.values.shape == g.times.shape == (qa.shape[0], B, L)
        assert not bool(torch.isnan(g.values).any()) and not bool(torch.isnan(g.times).any())
    assert dense._prefix is None
    if case == "doses":                                                      # the right limit at p, at time p
        assert torch.equal(got[0].times[8:10].cpu(), p[:, :, None].expand(2, B, L))
        assert bool((got[0].values[8:10] > dense(p.to(DEV))).all())
    # 1. the host path on the device's record
    twin = _on_host(dense)
    for a, b in zip(got, _both(twin, qa, qb)):
        assert same_bits(a.values, b.values) and same_bits(a.times, b.times)
    # 2. the host solve of the same problem
    host = _solve("cpu", dtype, L, **kw)
    same_record = all(torch.equal(getattr(dense, n).cpu(), getattr(host, n)) for n in ("offsets", "seg_start", "seg_end", "coeffs"))
    print(f"{case}: the host solve has the device's record: {same_record}")
    want = _both(host, qa, qb)
    if same_record:
        for a, b in zip(got, want):
            assert same_bits(a.values, b.values) and same_bits(a.times, b.times)
    else:
        # two valid step sequences under one tolerance: the extreme VALUES agree to the solve's accuracy, relative to
        # |value| + 1 as the mixed tolerance is (a flat extremum's time does not)
        tol = 1e-4 if dtype == F32 else 1e-6
        for a, b in zip(got, want):
            a, b = a.values.cpu().double(), b.values.double()
            assert float(((a - b).abs() / (b.abs() + 1)).max()) < tol


def test_long_walk():
    """One row, one oscillator, tolerances that take more than 64 steps (chosen on the host: 1e-13 gives 166): the
    window over the whole row is walked by three lanes, one per element, through every segment."""
    y0, func, _, t1 = oscillator_problem(1, 3, F64, DEV)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", rtol=1e-13, atol=1e-13)
    assert dense.n_segments >= 64
    got = _both(dense, dense.t0[None], dense.t1[None])
    for a, b in zip(got, _both(_on_host(dense), dense.t0[None].cpu(), dense.t1[None].cpu())):
        assert same_bits(a.values, b.values) and same_bits(a.times, b.times)
    assert float(got[0].values[0, 0, 0]) == 1.0 and float(got[0].times[0, 0, 0]) == 0.0      # cos(t) peaks at t0
    assert abs(float(got[1].values[0, 0, 1]) + 1.0) < 1e-9                                    # -sin(t) at pi / 2
    assert abs(float(got[1].times[0, 0, 1]) - np.pi / 2) < 1e-4


# -- the kernel on a synthetic record ----------------------------------------------------------------------------------------------
def _bordered(shape, dtype, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER + shift,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[BORDER + shift:BORDER + shift + n].view(*shape)


def _payload_only(buf, shape, shift=0):
    n = int(np.prod(shape))
    host = buf.cpu()
    return bool((host[:BORDER + shift] == SENTINEL).all()) and bool((host[BORDER + shift + n:] == SENTINEL).all())


def _record(n_rows, L, dtype):
    """Rows of 1 .. 5 segments with coefficients of mixed sign and magnitude, and windows [6, n_rows]: the whole row, two
    interior pairs (one reversed), a single point, and two with an end out of range (beyond t1 / NaN)."""
    g = torch.Generator().manual_seed(100 * n_rows + L)
    counts = [1 + (r * 3) % 5 for r in range(n_rows)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_seg = int(off[-1])
    ta, tb, t0, t1 = np.empty(n_seg), np.empty(n_seg), np.empty(n_rows), np.empty(n_rows)
    for r, n in enumerate(counts):
        edges = 0.1 * r + np.concatenate([[0.0], np.cumsum(0.01 + 0.05 * torch.rand(n, generator=g, dtype=F64).numpy())])
        ta[off[r]:off[r + 1]], tb[off[r]:off[r + 1]] = edges[:-1], edges[1:]
        t0[r], t1[r] = edges[0], edges[-2] + 0.75 * (edges[-1] - edges[-2])
    scale = 10.0 ** (4 * torch.rand(5, n_seg, L, generator=g, dtype=F64) - 2)
    coeffs = (torch.randn(5, n_seg, L, generator=g, dtype=F64) * scale).to(dtype)
    span = t1 - t0
    qa = np.stack([t0, t0 + 0.2 * span, t0 + 0.9 * span, t0 + 0.5 * span, t0 + 0.1 * span, np.full(n_rows, np.nan)])
    qb = np.stack([t1, t0 + 0.7 * span, t0 + 0.3 * span, t0 + 0.5 * span, t1 + 1e-3, t0 + 0.4 * span])
    return dict(off=off, ta=ta, tb=tb, t0=t0, t1=t1, coeffs=coeffs, qa=qa, qb=qb)


def _search(hip_kernels, rec, q, dtype):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    seg = torch.empty(q.size, dtype=torch.int32, device=DEV)
    x = torch.empty(q.size, dtype=dtype, device=DEV)
    status = torch.tensor([NONE], dtype=torch.int32, device=DEV)
    hip_kernels.row_dense_search(dev(q), dev(rec["off"]), dev(rec["ta"]), dev(rec["tb"]), dev(rec["t0"]), dev(rec["t1"]), seg, x,
                                 status)
    return seg, x, dev(q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("n_rows", [3, 67])
def test_kernel_bounds_and_misaligned_bases(n_rows, L, dtype, hip_kernels):
    """`values` and `times` inside sentinel borders: nothing outside [n_idx, L] is written, a window with an out-of-range end
    holds NaN in both and no other does, and the bits are the host model's — also with `coeffs`, `values` or `times` one
    element off a 16-byte boundary, which takes scalar elements at L = 8.  67 rows: the last wave is partial."""
    rec = _record(n_rows, L, dtype)
    lists = [*_search(hip_kernels, rec, rec["qa"], dtype), *_search(hip_kernels, rec, rec["qb"], dtype)]
    ta, tb = torch.from_numpy(rec["ta"]), torch.from_numpy(rec["tb"])
    on_host = [t.cpu() for t in lists]
    n = rec["qa"].size
    bad = np.zeros((6, n_rows), dtype=bool)
    bad[4:] = True
    aligned = rec["coeffs"].to(DEV)
    off_by_one = torch.empty(aligned.numel() + 1, dtype=dtype, device=DEV)[1:].view_as(aligned).copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and off_by_one.data_ptr() % 16 != 0
    for which in (MAXIMUM, MINIMUM):
        for sign in (1.0, -1.0):
            want_v, want_t = HostRowKernels.quartic_extrema(rec["coeffs"], ta, tb, sign, *on_host, which == MAXIMUM)
            for shifted in (None, "coeffs", "values", "times"):
                if (shifted is not None and L != 8) or (shifted is not None and sign < 0):
                    continue
                v_shift, t_shift = int(shifted == "values"), int(shifted == "times")
                v_buf, values = _bordered((n, L), dtype, v_shift)
                t_buf, times = _bordered((n, L), F64, t_shift)
                assert (values.data_ptr() % 16 != 0) == bool(v_shift) and (times.data_ptr() % 16 != 0) == bool(t_shift)
                hip_kernels.row_dense_extremum(values, times, which, off_by_one if shifted == "coeffs" else aligned, ta.to(DEV),
                                               tb.to(DEV), sign, *lists)
                torch.cuda.synchronize()
                assert _payload_only(v_buf, (n, L), v_shift) and _payload_only(t_buf, (n, L), t_shift), (which, sign, shifted)
                assert same_bits(values, want_v) and same_bits(times, want_t), (which, sign, shifted)
                for out in (values, times):
                    nan_rows = torch.isnan(out.cpu()).view(6, n_rows, L)
                    assert np.array_equal(nan_rows.all(dim=2).numpy(), bad) and np.array_equal(nan_rows.any(dim=2).numpy(), bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_false_gives_nan_rows_and_raises_nothing(dtype):
    dense = _solve(DEV, dtype, 8)
    qa, qb = windows(dense)
    qa, qb = qa[:3].clone().to(DEV), qb[:3].to(DEV)
    good = dense.maximum(qa, qb)
    qa[2, 1], qa[1, 9], qa[1, 3] = float("nan"), 5.0, -2.0
    for fn in (dense.maximum, dense.minimum):
        for got in (fn(qa, qb, check=False), fn(qb, qa, check=False)):
            for out in got:
                assert torch.isnan(out).all(dim=2).nonzero().tolist() == torch.isnan(out).any(dim=2).nonzero().tolist() \
                    == [[1, 3], [1, 9], [2, 1]]
        with pytest.raises(ValueError, match=r"query 1 of row 3 \(ta = "):
            fn(qa, qb)
        with pytest.raises(ValueError, match=r"query 1 of row 3 \(tb = "):
            fn(qb, qa)
    ok = ~torch.isnan(dense.maximum(qa, qb, check=False).values)
    assert same_bits(dense.maximum(qa, qb, check=False).values[ok], good.values[ok])
