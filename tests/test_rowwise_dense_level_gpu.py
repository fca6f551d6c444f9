"""`RowDenseOutput.crossings` / `.time_above` on the MI355X: `odeint_rowwise_dense` on the device against the host path, bit for
bit — plain and with `compact`, ascending and descending, with `jump_dy`, on oscillators — in the two-part scheme of
tests/test_rowwise_dense_extremum_gpu.py; then `row_dense_level` itself on that file's synthetic record: the scalar
instantiation for a misaligned base, sentinel borders around the four outputs, -1 / NaN rows for out-of-range ends; a window
of more than 64 steps with the closed-form counts; and `check=False`."""
import copy

import numpy as np
import pytest
import torch

from _rowwise_dense_extremum_oracle import oscillator_problem, same_bits, windows
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
INT_SENTINEL = -77


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


def _levels(case, L, dtype):
    """A scalar level and a [B, L] level (one per row times one per element) that the elements pass (CPU tensors)."""
    if case == "oscillator":
        return [0.5, torch.linspace(0.5, 1.0, B, dtype=F64)[:, None] * torch.linspace(-0.9, 0.9, L, dtype=F64)]
    hi = 3.0 if case == "down" else 1.2
    return [0.9, (torch.linspace(0.5, 1.0, B, dtype=F64)[:, None] * torch.linspace(0.1, hi, L, dtype=F64)).to(dtype)]


def _same(got, want):
    return all(same_bits(a, b) for a, b in zip(got, want))


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
    """L = 5: scalar elements; L = 8: 16-byte elements for both dtypes.  Windows: see `windows` of the extremum oracle; with doses
    also around the dose time, against a level halfway up the dose."""
    kw = dict(CASES[case])
    if case == "doses":
        dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64)
        kw["options"] = {**kw["options"], "jump_dy": dy.to(dtype)}
    dense = _solve(DEV, dtype, L, **kw)
    assert dense.coeffs.device.type == DEV.type and dense._k is not None
    qa, qb = windows(dense)
    levels = _levels(case, L, dtype)
    if case == "doses":                                                      # inside, near end, far end, the dose time itself
        p, t1 = kw["options"]["jump_t"], per_row_t1(B)[None]
        qa, qb = torch.cat([qa, 0.35 * t1, p, 0.35 * t1, p]), torch.cat([qb, 0.6 * t1, 0.6 * t1, p, p])
        levels.append((dense(p.to(DEV))[0].cpu() + 0.5 * dy[0].to(dtype)))
    twin = _on_host(dense)
    host = _solve("cpu", dtype, L, **kw)
    same_record = all(torch.equal(getattr(dense, n).cpu(), getattr(host, n)) for n in ("offsets", "seg_start", "seg_end", "coeffs"))
    print(f"{case}: the host solve has the device's record: {same_record}")
    crossed = 0
    for level in levels:
        on_dev = level.to(DEV) if isinstance(level, torch.Tensor) else level
        got = dense.crossings(on_dev, qa.to(DEV), qb.to(DEV))
        assert all(v.device.type == DEV.type and v.shape == (qa.shape[0], B, L) for v in got)
        assert got.count.dtype == torch.int32 and got.first.dtype == got.last.dtype == got.time_above.dtype == F64
        assert bool((got.count >= 0).all()) and not bool(torch.isnan(got.time_above).any())
        assert same_bits(dense.time_above(on_dev, qa.to(DEV), qb.to(DEV)), got.time_above)
        crossed += int((got.count > 0).sum())
        # 1. the host path on the device's record
        assert _same(got, twin.crossings(level, qa, qb))
        # 2. the host solve of the same problem
        want = host.crossings(level, qa, qb)
        if same_record:
            assert _same(got, want)
        else:
            # two valid step sequences under one tolerance: away from a grazing contact the time above agrees to the solve's
            # accuracy (a count does not: a level inside the rounding gap of a breakpoint adds a pair of crossings)
            tol = 1e-4 if dtype == F32 else 1e-6
            agree = got.count.cpu() == want.count
            assert float((got.time_above.cpu() - want.time_above).abs()[agree].max()) < tol
    assert dense._prefix is None and crossed > 0
    if case == "doses":                                                      # the up-crossing at p, at time p, bit for bit
        at_p = p[:, :, None].expand(2, B, L)
        assert torch.equal(got.first[8:10].cpu(), at_p)
        assert bool((got.count[10:] == 0).all()) and bool((got.time_above[10:] == 0).all())


def test_long_walk():
    """One row, one oscillator, tolerances that take more than 64 steps (chosen on the host: 1e-13 gives 166): the window over
    the whole row is walked by three lanes, one per element, through every segment.  cos(t) on [0, t1 = 2] passes 0.5 once,
    at pi / 3, and is above it until then; -sin(t) passes -0.5 once, at pi / 6."""
    y0, func, _, t1 = oscillator_problem(1, 3, F64, DEV)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", rtol=1e-13, atol=1e-13)
    assert dense.n_segments >= 64 and float(t1[0]) == 2.0
    level = torch.tensor([0.5, -0.5, 0.5], dtype=F64)
    got = dense.crossings(level.to(DEV), dense.t0[None], dense.t1[None])
    assert _same(got, _on_host(dense).crossings(level, dense.t0[None].cpu(), dense.t1[None].cpu()))
    assert got.count[0, 0].tolist() == [1, 1, 1]                             # (exp(-t) passes 0.5 at log 2)
    want = torch.tensor([np.pi / 3, np.pi / 6, np.log(2.0)], dtype=F64)
    assert float((got.first[0, 0].cpu() - want).abs().max()) < 1e-9 and same_bits(got.first, got.last)
    above = torch.tensor([np.pi / 3, np.pi / 6, np.log(2.0)], dtype=F64)      # each starts above its level
    assert float((got.time_above[0, 0].cpu() - above).abs().max()) < 1e-9
    many = dense.crossings(torch.tensor([0.99999, 0.0, 0.2], dtype=F64, device=DEV), 0.0, 2.0)
    assert many.count[0].tolist() == [1, 0, 1]                               # -sin(t) < 0 on (0, 2]: never above 0


# -- the kernel on a synthetic record ----------------------------------------------------------------------------------------------
def _bordered(shape, dtype, shift=0):
    n = int(np.prod(shape))
    fill = INT_SENTINEL if dtype == torch.int32 else SENTINEL
    buf = torch.full((n + 2 * BORDER + shift,), fill, dtype=dtype, device=DEV)
    return buf, buf[BORDER + shift:BORDER + shift + n].view(*shape)


def _payload_only(buf, shape, shift=0):
    n = int(np.prod(shape))
    host = buf.cpu()
    fill = INT_SENTINEL if buf.dtype == torch.int32 else SENTINEL
    return bool((host[:BORDER + shift] == fill).all()) and bool((host[BORDER + shift + n:] == fill).all())


def _record(n_rows, L, dtype):
    """Rows of 1 .. 5 segments with coefficients of mixed sign and magnitude, and windows [6, n_rows]: the whole row, two
    interior pairs (one reversed), a single point, and two with an end out of range (beyond t1 / NaN); the record of
    tests/test_rowwise_dense_extremum_gpu.py, plus levels [n_rows, L] near the scale of the coefficients."""
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
    # the value of each row's first segment at a random x, and every fourth level exactly its e coefficient (phi == 0 at x = 0)
    x = torch.rand(n_rows, L, generator=g, dtype=F64)
    first = coeffs[:, torch.from_numpy(off[:-1])].double()
    level = first[0] + x * (first[1] + x * (first[2] + x * (first[3] + x * first[4])))
    level.view(-1)[::4] = first[0].reshape(-1)[::4]
    return dict(off=off, ta=ta, tb=tb, t0=t0, t1=t1, coeffs=coeffs, qa=qa, qb=qb, level=level.to(dtype).contiguous())


def _search(hip_kernels, rec, q, dtype):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    seg = torch.empty(q.size, dtype=torch.int32, device=DEV)
    x = torch.empty(q.size, dtype=dtype, device=DEV)
    status = torch.tensor([NONE], dtype=torch.int32, device=DEV)
    hip_kernels.row_dense_search(dev(q), dev(rec["off"]), dev(rec["ta"]), dev(rec["tb"]), dev(rec["t0"]), dev(rec["t1"]), seg, x,
                                 status)
    return seg, x, dev(q)


def _off_by_one(t):
    out = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view_as(t).copy_(t)
    assert t.data_ptr() % 16 == 0 and out.data_ptr() % 16 != 0
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("n_rows", [3, 67])
def test_kernel_bounds_and_misaligned_bases(n_rows, L, dtype, hip_kernels):
    """The four outputs inside sentinel borders: nothing outside [n_idx, L] is written, a window with an out-of-range end holds
    -1 / NaN in all four and no other does, and the bits are the host model's — also with `coeffs`, `level` or one of the outputs
    one element off a 16-byte boundary, which takes scalar elements at L = 8.  67 rows: the last wave is partial."""
    rec = _record(n_rows, L, dtype)
    lists = [*_search(hip_kernels, rec, rec["qa"], dtype), *_search(hip_kernels, rec, rec["qb"], dtype)]
    ta, tb = torch.from_numpy(rec["ta"]), torch.from_numpy(rec["tb"])
    on_host = [t.cpu() for t in lists]
    n = rec["qa"].size
    bad = np.zeros((6, n_rows), dtype=bool)
    bad[4:] = True
    coeffs, level = rec["coeffs"].to(DEV), rec["level"].to(DEV)
    shifted_in = {"coeffs": _off_by_one(coeffs), "level": _off_by_one(level)}
    names = ("count", "first", "last", "time_above")
    for sign in (1.0, -1.0):
        want = HostRowKernels.quartic_levels(rec["coeffs"], rec["level"], ta, tb, sign, *on_host)
        assert int((want[0] > 0).sum()) > n_rows and int((want[0] > 1).sum()) > 0
        for shifted in (None, "coeffs", "level", *names):
            if shifted is not None and (L != 8 or sign < 0):
                continue
            bufs, outs = zip(*(_bordered((n, L), torch.int32 if name == "count" else F64, int(shifted == name)) for name in names))
            for name, out in zip(names, outs):
                assert (out.data_ptr() % 16 != 0) == (shifted == name)
            hip_kernels.row_dense_level(*outs, shifted_in["level"] if shifted == "level" else level,
                                        shifted_in["coeffs"] if shifted == "coeffs" else coeffs, ta.to(DEV), tb.to(DEV), sign,
                                        *lists)
            torch.cuda.synchronize()
            for name, buf in zip(names, bufs):
                assert _payload_only(buf, (n, L), int(shifted == name)), (sign, shifted, name)
            assert _same(outs, want), (sign, shifted)
            minus = (outs[0].cpu() == -1).view(6, n_rows, L)
            assert np.array_equal(minus.all(dim=2).numpy(), bad) and np.array_equal(minus.any(dim=2).numpy(), bad)
            nan_rows = torch.isnan(outs[3].cpu()).view(6, n_rows, L)
            assert np.array_equal(nan_rows.all(dim=2).numpy(), bad) and np.array_equal(nan_rows.any(dim=2).numpy(), bad)
            for out in outs[1:3]:                                            # first, last: NaN also without a crossing
                assert torch.equal(torch.isnan(out.cpu()), outs[0].cpu() <= 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_false_reads_nothing_and_raises_nothing(dtype, monkeypatch):
    dense = _solve(DEV, dtype, 8)
    qa, qb = windows(dense)
    qa, qb = qa[:3].clone().to(DEV), qb[:3].to(DEV)
    good = dense.crossings(0.9, qa, qb)
    qa[2, 1], qa[1, 9], qa[1, 3] = float("nan"), 5.0, -2.0
    with monkeypatch.context() as m:
        def no_read(*a, **k):
            raise AssertionError("check=False read from the device")
        for name in ("tolist", "item", "cpu", "numpy"):
            m.setattr(torch.Tensor, name, no_read)
        outs = [dense.crossings(0.9, qa, qb, check=False), dense.crossings(0.9, qb, qa, check=False)]
        above = dense.time_above(0.9, qa, qb, check=False)
    assert same_bits(above, outs[0].time_above)
    for got in outs:
        assert (got.count == -1).all(dim=2).nonzero().tolist() == (got.count == -1).any(dim=2).nonzero().tolist() \
            == [[1, 3], [1, 9], [2, 1]]
        assert torch.isnan(got.time_above).all(dim=2).nonzero().tolist() == torch.isnan(got.time_above).any(dim=2).nonzero().tolist() \
            == [[1, 3], [1, 9], [2, 1]]
        for out in (got.first, got.last):                                    # NaN also without a crossing
            assert torch.equal(torch.isnan(out), got.count <= 0)
        ok = got.count != -1
        assert all(same_bits(a[ok], b[ok]) for a, b in zip(got, good))
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(ta = "):
        dense.crossings(0.9, qa, qb)
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(tb = "):
        dense.time_above(0.9, qb, qa)
