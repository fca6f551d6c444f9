"""`RowDenseOutput.crossing_times` on the MI355X: `odeint_rowwise_dense` on the device against the host path on the device's
record, bit for bit, and against `dense.crossings` on the device (two kernels, one answer) — the cases of
tests/test_rowwise_dense_level_gpu.py plus the harmonic problem with its closed form; then `row_dense_level_times` itself on a
sawtooth record whose counts and times are known without any model: sentinel borders around the four outputs, every slot
written, the scalar instantiation for a misaligned base, both time signs, -1 / NaN rows for out-of-range ends; a window of
more than 64 steps whose lists overflow; and `check=False`."""
import numpy as np
import pytest
import torch

from _rowwise_dense_crossing_times_oracle import (HARMONIC_BOUND, HARMONIC_LEVEL, HARMONIC_TOL, check_identities,
                                                  harmonic_distance, harmonic_problem)
from _rowwise_dense_extremum_oracle import same_bits, windows
from _rowwise_dense_oracle import per_row_t1
from _rowwise_kernels import SENTINEL
from test_rowwise_dense_level_gpu import (B, BORDER, CASES, DEV, DTYPES, F32, F64, INT_SENTINEL, _bordered, _levels,  # noqa: F401
                                          _off_by_one, _on_host, _payload_only, _same, _search, _solve)

import torchdiffeq_amd as tda
from torchdiffeq_amd.rowwise import HostRowKernels
from torchdiffeq_amd.rowwise_dense import RowDenseCrossingTimes

pytestmark = pytest.mark.gpu

K = 4
HARM_B = 5
ALL_CASES = [*CASES, "harmonic", "harmonic_down"]


def _to_cpu(got):
    return RowDenseCrossingTimes(*(v.cpu() for v in got))


def _well_formed(got, shape):
    assert got.n_rising.dtype == got.n_falling.dtype == torch.int32 and got.rising.dtype == got.falling.dtype == F64
    assert got.n_rising.shape == got.n_falling.shape == shape and got.rising.shape == got.falling.shape == (K, *shape)
    slot = torch.arange(K).view(K, *([1] * len(shape)))
    for n, times in ((got.n_rising, got.rising), (got.n_falling, got.falling)):
        assert torch.equal(torch.isnan(times), slot >= n.clamp(min=0, max=K)[None])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("case", ALL_CASES)
def test_device_equals_host(case, L, dtype):
    """L = 5: scalar elements; L = 8: 16-byte elements for both dtypes (harmonic: P = 2 pairs plus the tail, and P = 4).
    Windows: see `windows` of the extremum oracle; with doses also around the dose time, against a level halfway up the dose;
    the harmonic rows also against the closed form on the whole row."""
    harmonic = case.startswith("harmonic")
    if harmonic:
        rows, P, down = HARM_B, L // 2, case == "harmonic_down"
        y0, func, w, t1 = harmonic_problem(rows, P, L % 2, dtype, DEV)
        with torch.no_grad():
            dense = tda.odeint_rowwise_dense(func, y0, 0.0, -t1 if down else t1, method="dopri5", **HARMONIC_TOL[dtype])
        levels = [HARMONIC_LEVEL, torch.linspace(0.5, 1.0, rows, dtype=F64)[:, None] * torch.linspace(-0.9, 0.9, L, dtype=F64)]
    else:
        rows = B
        kw = dict(CASES[case])
        if case == "doses":
            dy = 0.5 + torch.rand(1, B, L, generator=torch.Generator().manual_seed(6), dtype=F64)
            kw["options"] = {**kw["options"], "jump_dy": dy.to(dtype)}
        dense = _solve(DEV, dtype, L, **kw)
        levels = _levels(case, L, dtype)
    assert dense.coeffs.device.type == DEV.type and dense._k is not None
    qa, qb = windows(dense)
    if case == "doses":                                                      # inside, near end, far end, the dose time itself
        p, t1 = kw["options"]["jump_t"], per_row_t1(B)[None]
        qa, qb = torch.cat([qa, 0.35 * t1, p, 0.35 * t1, p]), torch.cat([qb, 0.6 * t1, 0.6 * t1, p, p])
        levels.append((dense(p.to(DEV))[0].cpu() + 0.5 * dy[0].to(dtype)))
    twin = _on_host(dense)
    crossed = rebuilt = 0
    for level in levels:
        on_dev = level.to(DEV) if isinstance(level, torch.Tensor) else level
        got = dense.crossing_times(on_dev, qa.to(DEV), qb.to(DEV), max_count=K)
        assert all(v.device.type == DEV.type for v in got)
        ref = dense.crossings(on_dev, qa.to(DEV), qb.to(DEV))                # the level kernel, on the device
        got, ref = _to_cpu(got), type(ref)(*(v.cpu() for v in ref))
        _well_formed(got, (qa.shape[0], rows, L))
        assert bool((got.n_rising >= 0).all()) and bool((got.n_falling >= 0).all())
        crossed += int((got.n_rising > 0).sum()) + int((got.n_falling > 0).sum())
        # 1. the host path on the device's record
        assert _same(got, twin.crossing_times(level, qa, qb, max_count=K))
        # 2. two kernels, one answer
        rebuilt += check_identities(got, ref, qa, qb, dense._sign, K)
    assert dense._prefix is None and crossed > 0 and rebuilt > 0
    if case == "doses":                                                      # the dose in `rising` at p, at time p, bit for bit
        at_p = p[:, :, None].expand(2, B, L)
        assert bool((got.n_rising[8:10] == 1).all()) and torch.equal(got.rising[0, 8:10], at_p)
        assert bool((got.n_rising[10:] == 0).all()) and bool((got.n_falling[10:] == 0).all())
    if harmonic:
        whole = _to_cpu(dense.crossing_times(HARMONIC_LEVEL, dense.t0[None], dense.t1[None], max_count=K))
        whole = RowDenseCrossingTimes(whole.n_rising[0], whole.n_falling[0], whole.rising[:, 0], whole.falling[:, 0])
        worst, fit, overflow = harmonic_distance(whole, w, t1.cpu(), down, K)
        print(f"{case}: largest distance from the closed form {worst:.3g} (bound {HARMONIC_BOUND[dtype]:.3g}); {fit} lists "
              f"fit, {overflow} overflow")
        assert fit > 0 and overflow > 0 and worst <= HARMONIC_BOUND[dtype]


def test_long_walk():
    """One harmonic row (w = 2 pi and 2.5 pi, t1 = 6) at tolerances that take more than 64 steps: the window over the whole row
    is walked by five lanes, one per element, through every segment; cos(w t) passes 0.3 six to eight times per direction, so
    both lists overflow `max_count` = 4 and hold the first four, all before t = 4: inside the span of the bound's solves."""
    y0, func, w, t1 = harmonic_problem(1, 2, True, F64, DEV)
    t1 = 2 * t1
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, t1, method="dopri5", **HARMONIC_TOL[F64])
    assert dense.n_segments >= 64 and float(t1[0]) == 6.0
    got = _to_cpu(dense.crossing_times(HARMONIC_LEVEL, dense.t0[None], dense.t1[None], max_count=K))
    assert _same(got, _on_host(dense).crossing_times(HARMONIC_LEVEL, dense.t0[None].cpu(), dense.t1[None].cpu(), max_count=K))
    whole = RowDenseCrossingTimes(got.n_rising[0], got.n_falling[0], got.rising[:, 0], got.falling[:, 0])
    worst, fit, overflow = harmonic_distance(whole, w, t1.cpu(), False, K)
    assert bool((whole.n_rising[0, :2] > K).all()) and bool((whole.n_falling[0, :2] > K).all()) and (fit, overflow) == (0, 4)
    assert not bool(torch.isnan(whole.rising[:, 0, :2]).any()) and not bool(torch.isnan(whole.falling[:, 0, :2]).any())
    assert worst <= HARMONIC_BOUND[F64]


# -- the kernel on a synthetic record ----------------------------------------------------------------------------------------------
def _sawtooth(n_rows, L, dtype, falls):
    """Row r: 1 + r % 11 segments of width 0.25 from t0 = r / 2, every element the same line per segment.  Without `falls` the
    lines alternate between -1 + 2 x and 1 - 2 x: continuous, one crossing of 0 per segment at x = 1 / 2, up and down in turn.
    With `falls` every segment is -1 + 2 x: an up-crossing inside each, and at each breakpoint the fall from 1 to -1 is a
    down-crossing at the stored start of the next segment.  Windows [4, n_rows]: the whole row, the whole row reversed, and
    two with an end out of range (NaN / beyond t1).  Times are exact binary fractions: ta + 0.125 is computed without rounding."""
    counts = [1 + r % 11 for r in range(n_rows)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_seg = int(off[-1])
    ta, t0, t1 = np.empty(n_seg), np.empty(n_rows), np.empty(n_rows)
    coeffs = torch.zeros(5, n_seg, L, dtype=dtype)
    for r, n in enumerate(counts):
        ta[off[r]:off[r + 1]] = 0.5 * r + 0.25 * np.arange(n)
        t0[r], t1[r] = 0.5 * r, 0.5 * r + 0.25 * n
        for k in range(n):
            up = falls or k % 2 == 0
            coeffs[0, off[r] + k], coeffs[1, off[r] + k] = (-1.0, 2.0) if up else (1.0, -2.0)
    tb = ta + 0.25
    nan = np.full(n_rows, np.nan)
    qa, qb = np.stack([t0, t1, nan, t0]), np.stack([t1, t0, t1, t1 + 1e-3])
    ups = [[ta[s] + 0.125 for s in range(off[r], off[r + 1]) if falls or (s - off[r]) % 2 == 0] for r in range(n_rows)]
    if falls:
        downs = [[ta[s] for s in range(off[r] + 1, off[r + 1])] for r in range(n_rows)]
    else:
        downs = [[ta[s] + 0.125 for s in range(off[r], off[r + 1]) if (s - off[r]) % 2 == 1] for r in range(n_rows)]
    return dict(off=off, ta=ta, tb=tb, t0=t0, t1=t1, coeffs=coeffs, qa=qa, qb=qb, level=torch.zeros(n_rows, L, dtype=dtype)), ups, downs


def _expected(ups, downs, n_rows, L, sign):
    """The four outputs [.., 4 * n_rows, L] from the known crossings in solver time: windows 0 and 1 hold them, 2 and 3 are out
    of range.  Solver time t is true time sign * t, and an up-crossing rises in true time for sign > 0 only."""
    n = 4 * n_rows
    counts = [torch.full((n, L), -1, dtype=torch.int32) for _ in range(2)]
    lists = [torch.full((K, n, L), float("nan"), dtype=F64) for _ in range(2)]
    for which, per_row in enumerate((ups, downs) if sign > 0 else (downs, ups)):
        for window in (0, 1):
            for r, times in enumerate(per_row):
                i = window * n_rows + r
                counts[which][i] = len(times)
                for slot, t in enumerate(times[:K]):
                    lists[which][slot, i] = sign * t
    return (*counts, *lists)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [5, 8])
@pytest.mark.parametrize("n_rows", [3, 67])
def test_kernel_bounds_and_misaligned_bases(n_rows, L, dtype, hip_kernels):
    """The four outputs inside sentinel borders: nothing outside the payload is written and every payload slot is; the counts
    and times are those of the sawtooth (known without a model; lists overflow and fit) and the host model's bits; a window with
    an out-of-range end holds -1 / NaN in all four and no other does — also with `coeffs`, `level` or a counter one element off
    its alignment, which takes scalar elements at L = 8, and with a list 8 bytes off, which does not.  67 rows: the last wave is
    partial."""
    names = ("n_rising", "n_falling", "rising", "falling")
    for falls in (False, True):
        rec, ups, downs = _sawtooth(n_rows, L, dtype, falls)
        lists = [*_search(hip_kernels, rec, rec["qa"], dtype), *_search(hip_kernels, rec, rec["qb"], dtype)]
        ta, tb = torch.from_numpy(rec["ta"]), torch.from_numpy(rec["tb"])
        on_host = [t.cpu() for t in lists]
        n = rec["qa"].size
        bad = np.zeros((4, n_rows), dtype=bool)
        bad[2:] = True
        coeffs, level = rec["coeffs"].to(DEV), rec["level"].to(DEV)
        shifted_in = {"coeffs": _off_by_one(coeffs), "level": _off_by_one(level)}
        for sign in (1.0, -1.0):
            want = _expected(ups, downs, n_rows, L, sign)
            assert _same(HostRowKernels.quartic_crossing_times(rec["coeffs"], rec["level"], ta, tb, sign, K, *on_host), want)
            assert int(((want[0] > 0) & (want[0] <= K)).sum()) > 0 and (n_rows < 11 or int((want[0] > K).sum()) > 0)
            for shifted in (None, "coeffs", "level", *names):
                if shifted is not None and (L != 8 or sign < 0 or falls):
                    continue
                shapes = [(n, L), (n, L), (K, n, L), (K, n, L)]
                bufs, outs = zip(*(_bordered(shape, torch.int32 if name.startswith("n_") else F64, int(shifted == name))
                                   for name, shape in zip(names, shapes)))
                for name, out in zip(names, outs):
                    assert (out.data_ptr() % 16 != 0) == (shifted == name)
                hip_kernels.row_dense_level_times(*outs, shifted_in["level"] if shifted == "level" else level,
                                                  shifted_in["coeffs"] if shifted == "coeffs" else coeffs, ta.to(DEV), tb.to(DEV),
                                                  sign, *lists)
                torch.cuda.synchronize()
                for name, buf, shape in zip(names, bufs, shapes):
                    assert _payload_only(buf, shape, int(shifted == name)), (falls, sign, shifted, name)
                got = [out.cpu() for out in outs]
                for name, out in zip(names, got):                            # every slot was written
                    assert not bool((out == (INT_SENTINEL if name.startswith("n_") else SENTINEL)).any()), (falls, sign, shifted, name)
                assert _same(got, want), (falls, sign, shifted)
                for out in got[:2]:
                    minus = (out == -1).view(4, n_rows, L)
                    assert np.array_equal(minus.all(dim=2).numpy(), bad) and np.array_equal(minus.any(dim=2).numpy(), bad)
                for out in got[2:]:
                    assert bool(torch.isnan(out.view(K, 4, n_rows, L)[:, 2:]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_false_reads_nothing_and_raises_nothing(dtype, monkeypatch):
    dense = _solve(DEV, dtype, 8)
    qa, qb = windows(dense)
    qa, qb = qa[:3].clone().to(DEV), qb[:3].to(DEV)
    good = dense.crossing_times(0.9, qa, qb)
    qa[2, 1], qa[1, 9], qa[1, 3] = float("nan"), 5.0, -2.0
    with monkeypatch.context() as m:
        def no_read(*a, **k):
            raise AssertionError("check=False read from the device")
        for name in ("tolist", "item", "cpu", "numpy"):
            m.setattr(torch.Tensor, name, no_read)
        outs = [dense.crossing_times(0.9, qa, qb, check=False), dense.crossing_times(0.9, qb, qa, check=False)]
    for got in outs:
        for n in got[:2]:
            assert (n == -1).all(dim=2).nonzero().tolist() == (n == -1).any(dim=2).nonzero().tolist() == [[1, 3], [1, 9], [2, 1]]
        ok = got.n_rising != -1
        for times in got[2:]:
            assert bool(torch.isnan(times[:, ~ok]).all())
        assert all(same_bits(a[..., ok], b[..., ok]) for a, b in zip(got, good))
    assert _same(outs[0], outs[1])
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(ta = "):
        dense.crossing_times(0.9, qa, qb)
    with pytest.raises(ValueError, match=r"query 1 of row 3 \(tb = "):
        dense.crossing_times(0.9, qb, qa)
