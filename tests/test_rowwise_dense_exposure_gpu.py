"""`RowDenseOutput.exposure` / `.area_above` / `.area_below` on the MI355X: `odeint_rowwise_dense` on the device against the host
path, bit for bit — plain and with `compact`, ascending and descending, with `jump_dy`, on oscillators — in the two-part scheme
of tests/test_rowwise_dense_level_gpu.py; then `row_dense_exposure` itself on that file's synthetic record: the scalar
instantiation for a misaligned base, sentinel borders around the three outputs, NaN rows for out-of-range ends; a window of
more than 64 steps with the closed-form areas; and `check=False`.  The solves, cases, levels and the record are that file's."""
import numpy as np
import pytest
import torch

from _rowwise_dense_extremum_oracle import oscillator_problem, same_bits, windows
from _rowwise_dense_oracle import per_row_t1
from _rowwise_kernels import SENTINEL
from test_rowwise_dense_level_gpu import (B, BORDER, CASES, DEV, DTYPES, F32, F64, _levels, _off_by_one, _on_host, _record,
                                          _same, _search, _solve)

import torchdiffeq_amd as tda
from torchdiffeq_amd.rowwise import HostRowKernels

pytestmark = pytest.mark.gpu


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
    over = under = 0
    for level in levels:
        on_dev = level.to(DEV) if isinstance(level, torch.Tensor) else level
        got = dense.exposure(on_dev, qa.to(DEV), qb.to(DEV))
        assert all(v.device.type == DEV.type and v.shape == (qa.shape[0], B, L) for v in got)
        assert got.area_above.dtype == got.area_below.dtype == dtype and got.time_above.dtype == F64
        assert not any(bool(torch.isnan(v).any()) for v in got)
        assert bool((got.area_above >= 0).all()) and bool((got.area_below >= 0).all())
        assert same_bits(dense.time_above(on_dev, qa.to(DEV), qb.to(DEV)), got.time_above)
        assert same_bits(dense.area_above(on_dev, qa.to(DEV), qb.to(DEV)), got.area_above)
        over, under = over + int((got.area_above > 0).sum()), under + int((got.area_below > 0).sum())
        # 1. the host path on the device's record
        assert _same(got, twin.exposure(level, qa, qb))
        # 2. the host solve of the same problem
        want = host.exposure(level, qa, qb)
        if same_record:
            assert _same(got, want)
        else:
            # two valid step sequences under one tolerance: where both solves count the same crossings the three outputs agree
            # to the solve's accuracy (the figures of tests/test_rowwise_dense_level_gpu.py for `time_above`)
            tol = 1e-4 if dtype == F32 else 1e-6
            agree = (dense.crossings(on_dev, qa.to(DEV), qb.to(DEV)).count.cpu() == host.crossings(level, qa, qb).count)
            for a, b in zip(got, want):
                assert float((a.cpu().to(F64) - b.to(F64)).abs()[agree].max()) < tol
    assert dense._prefix is None and over > 0 and under > 0
    if case == "doses":                                                      # the dose level: nothing above before the dose
        assert bool((got.area_above[10:] == 0).all()) and bool((got.time_above[10:] == 0).all())
        assert bool((got.area_above[8:10] > 0).all()) and same_bits(got.area_above[8], got.area_above[9])


def test_long_walk():
    """One row, one oscillator, tolerances that take more than 64 steps (1e-13 gives 166 on the host): the window over the whole
    row is walked by three lanes, one per element, through every segment.  On [0, t1 = 2]: cos(t) is above 0.5 until pi / 3,
    -sin(t) above -0.5 until pi / 6, exp(-t) above 0.5 until log 2."""
    y0, func, _, t1 = oscillator_problem(1, 3, F64, DEV)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", rtol=1e-13, atol=1e-13)
    assert dense.n_segments >= 64 and float(t1[0]) == 2.0
    level = torch.tensor([0.5, -0.5, 0.5], dtype=F64)
    got = dense.exposure(level.to(DEV), dense.t0[None], dense.t1[None])
    assert _same(got, _on_host(dense).exposure(level, dense.t0[None].cpu(), dense.t1[None].cpu()))
    z = [np.pi / 3, np.pi / 6, np.log(2.0)]
    F = [lambda t: np.sin(t) - 0.5 * t, lambda t: np.cos(t) + 0.5 * t, lambda t: -np.exp(-t) - 0.5 * t]      # of y - level
    above = torch.tensor([f(c) - f(0.0) for f, c in zip(F, z)], dtype=F64)
    below = torch.tensor([-(f(2.0) - f(c)) for f, c in zip(F, z)], dtype=F64)
    assert float((got.area_above[0, 0].cpu() - above).abs().max()) < 1e-9
    assert float((got.area_below[0, 0].cpu() - below).abs().max()) < 1e-9
    assert float((got.time_above[0, 0].cpu() - torch.tensor(z, dtype=F64)).abs().max()) < 1e-9


# -- the kernel on a synthetic record ----------------------------------------------------------------------------------------------
def _bordered(shape, dtype, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BORDER + shift,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[BORDER + shift:BORDER + shift + n].view(*shape)


def _payload_only(buf, shape, shift=0):
    n = int(np.prod(shape))
    host = buf.cpu()
    return bool((host[:BORDER + shift] == SENTINEL).all()) and bool((host[BORDER + shift + n:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("n_rows", [3, 67])
def test_kernel_bounds_and_misaligned_bases(n_rows, L, dtype, hip_kernels):
    """The three outputs inside sentinel borders: nothing outside [n_idx, L] is written, a window with an out-of-range end holds
    NaN in all three and no other does, and the bits are the host model's — also with `coeffs`, `level` or one of the outputs one
    element off a 16-byte boundary, which takes scalar elements at L = 8.  67 rows: the last wave is partial."""
    rec = _record(n_rows, L, dtype)
    lists = [*_search(hip_kernels, rec, rec["qa"], dtype), *_search(hip_kernels, rec, rec["qb"], dtype)]
    ta, tb = torch.from_numpy(rec["ta"]), torch.from_numpy(rec["tb"])
    on_host = [t.cpu() for t in lists]
    n = rec["qa"].size
    bad = np.zeros((6, n_rows), dtype=bool)
    bad[4:] = True
    coeffs, level = rec["coeffs"].to(DEV), rec["level"].to(DEV)
    shifted_in = {"coeffs": _off_by_one(coeffs), "level": _off_by_one(level)}
    names = ("area_above", "area_below", "time_above")
    for sign in (1.0, -1.0):
        want = HostRowKernels.quartic_exposure(rec["coeffs"], rec["level"], ta, tb, sign, *on_host)
        assert int((want[0] > 0).sum()) > n_rows and int((want[1] > 0).sum()) > n_rows
        for shifted in (None, "coeffs", "level", *names):
            if shifted is not None and (L != 8 or sign < 0):
                continue
            bufs, outs = zip(*(_bordered((n, L), F64 if name == "time_above" else dtype, int(shifted == name)) for name in names))
            for name, out in zip(names, outs):
                assert (out.data_ptr() % 16 != 0) == (shifted == name)
            hip_kernels.row_dense_exposure(*outs, shifted_in["level"] if shifted == "level" else level,
                                           shifted_in["coeffs"] if shifted == "coeffs" else coeffs, ta.to(DEV), tb.to(DEV), sign,
                                           *lists)
            torch.cuda.synchronize()
            for name, buf in zip(names, bufs):
                assert _payload_only(buf, (n, L), int(shifted == name)), (sign, shifted, name)
            assert _same(outs, want), (sign, shifted)
            for out in outs:
                nan_rows = torch.isnan(out.cpu()).view(6, n_rows, L)
                assert np.array_equal(nan_rows.all(dim=2).numpy(), bad) and np.array_equal(nan_rows.any(dim=2).numpy(), bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_false_reads_nothing_and_raises_nothing(dtype, monkeypatch):
    dense = _solve(DEV, dtype, 8)
    qa, qb = windows(dense)
    qa, qb = qa[:3].clone().to(DEV), qb[:3].to(DEV)
    good = dense.exposure(0.9, qa, qb)
    qa[2, 1], qa[1, 9], qa[1, 3] = float("nan"), 5.0, -2.0
    with monkeypatch.context() as m:
        def no_read(*a, **k):
            raise AssertionError("check=False read from the device")
        for name in ("tolist", "item", "cpu", "numpy"):
            m.setattr(torch.Tensor, name, no_read)
        outs = [dense.exposure(0.9, qa, qb, check=False), dense.exposure(0.9, qb, qa, check=False)]
        above, below = dense.area_above(0.9, qa, qb, check=False), dense.area_below(0.9, qa, qb, check=False)
    assert same_bits(above, outs[0].area_above) and same_bits(below, outs[0].area_below)
    for got in outs:
        for v in got:
            assert torch.isnan(v).all(dim=2).nonzero().tolist() == torch.isnan(v).any(dim=2).nonzero().tolist() \
                == [[1, 3], [1, 9], [2, 1]]
        ok = ~torch.isnan(got.time_above)
        assert all(same_bits(a[ok], b[ok]) for a, b in zip(got, good))
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(ta = "):
        dense.exposure(0.9, qa, qb)
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(tb = "):
        dense.area_below(0.9, qb, qa)
