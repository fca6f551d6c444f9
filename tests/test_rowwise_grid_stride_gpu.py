"""The second grid pass of the rowwise entry points.  Row kernels launch over n_rows * row_len items through the same
`stream_grid` (csrc/tdeq_abi_rowwise.hpp), and several recompute a row index and per-row data inside the grid-stride loop.
B = 4099 rows with

    scalar form   L = 4099          fp32 16-byte form   L = 16388          fp64 16-byte form   L = 8194

exceed 2^24 items each; the second pass lies in the last few rows and crosses row boundaries.  Per-row inputs (masks,
`active`, `jumped`, maps, indices, weights, step sizes) differ from row to row, and the rows of the second pass hold taken
and untaken ones.  The record-based kernels get a small record (a handful of segments per row) and 4099 queries.

Checked as tests/_launch_forms.py describes: a few rows x a few elements at the start, around item 2^24 and at the end against
the row oracles (tests/_rowwise_*_oracle.py), the whole result against runs of whole rows below the cap, sentinel borders.
The row reductions and row_multi_dot have their own chunk geometry (not `stream_grid`) and are not in here."""
import numpy as np
import pytest
import torch

import _launch_forms as lf
from _launch_forms import ROWS, Rows
from _rowwise_dense_calculus_oracle import np_prefix
from _rowwise_dense_level_oracle import LevelOracle
from _rowwise_kernels import RowVectors

pytestmark = pytest.mark.gpu
I32, I64, F64 = torch.int32, torch.int64, torch.float64
COEF = (0.0371, -0.211, 0.5, 1.25, -0.0625, 0.33)
MID = (0.3, -0.45)


@pytest.fixture(autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def _state(dtype, B, L, count):
    """[B, L] randn tensors of the shared input pool."""
    return [t.view(B, L) for t in lf.streams(dtype, B * L, 0, count)]


def _per_row(B, fn, dtype):
    return torch.tensor([fn(r) for r in range(B)], dtype=torch.float64).to(dtype).cuda()


def _taken(B, shift=0):              # two rows in three; the last six rows hold both kinds
    return _per_row(B, lambda r: int((r + shift) % 3 != 1), I32)


def _perm(B, into, mult=1237):       # distinct rows of a table of `into` >= B rows, in no order
    assert into >= B and np.gcd(mult, into) == 1
    return [(r * mult + 5) % into for r in range(B)]


def _dts(B, dtype):
    return _per_row(B, lambda r: (0.01 + 0.001 * (r % 13)) * (-1) ** r, dtype)


def _rc(tensors, prefix):
    return {f"{prefix}{j}": (t, "rc") for j, t in enumerate(tensors)}


def _ks(t, prefix="k"):
    return [t[name] for name in sorted((n for n in t if n.startswith(prefix) and n[len(prefix):].isdigit()),
                                       key=lambda n: int(n[len(prefix):]))]


# ---- row_combine ----------------------------------------------------------------------------------------------------
COMBINE_ROWS = ((COEF, 0b111111, True), ((0.0, 0.7, 0.0, -0.3, 0.9, 0.0), 0b011010, False))


def _build_combine(dtype, B, L):
    y0, acc, *ks = _state(dtype, B, L, 8)
    ins = {"y0": (y0, "rc"), "acc": (acc, "rc"), **_rc(ks, "k"), "dts": (_dts(B, dtype), "r"), "active": (_taken(B), "r")}
    return ins, {"o0": ((B, L), dtype, "rc", None), "o1": ((B, L), dtype, "rc", None)}


def _call_combine(k, t):
    k.row_combine([t["o0"], t["o1"]], COMBINE_ROWS, t["y0"], t["acc"], _ks(t), t["dts"], t["active"])


# ---- row_select, row_impulse, row_gather, row_scale_many ------------------------------------------------------------
def _build_select(dtype, B, L):
    src, = _state(dtype, B, L, 1)
    return {"src": (src, "rc"), "mask": (_taken(B), "r")}, {"dst": ((B, L), dtype, "rc", None)}


def _build_impulse(dtype, B, L):
    y, d0, d1 = _state(dtype, B, L, 3)
    dy = torch.stack([d0, d1])                                       # [K = 2, B, L]: a dose per original row
    g = torch.Generator().manual_seed(5)
    dy_index = torch.randint(-1, 2, (3, B), generator=g, dtype=I32).cuda()        # position, original row -> k or -1
    ins = {"y_in": (y, "rc"), "dy": (dy, "..c"), "dy_index": (dy_index, ".."),
           "jump_hit": (_per_row(B, lambda r: r % 3, I32), "r"), "jumped": (_taken(B, 1), "r"),
           "row_map": (torch.tensor(_perm(B, B), dtype=I32).cuda(), "r")}
    return ins, {"y": ((B, L), dtype, "rc", "y_in")}


def _build_gather(dtype, B, L):
    a, b = _state(dtype, B, L, 2)
    ins = {"a": (a, ".c"), "b": (b, ".c"), "idx": (torch.tensor(_perm(B, B, 2003), dtype=I32).cuda(), "r")}
    return ins, {"o0": ((B, L), dtype, "rc", None), "o1": ((B, L), dtype, "rc", None)}


def _build_scale(dtype, B, L):
    g, = _state(dtype, B, L, 1)
    w = torch.stack([_per_row(B, lambda r, m=m: 0.3 + 0.01 * ((r * (m + 2)) % 17) - m, dtype) for m in range(3)])
    return {"g": (g, "rc"), "w": (w, ".r")}, {f"o{m}": ((B, L), dtype, "rc", None) for m in range(3)}


# ---- the quartic of a step: row_dense_commit[_mapped], row_event_fit[_mapped], row_event_eval[_mapped] --------------
N_OUT = 3


def _build_quartic(dtype, B, L):
    y0, y1, f0, f1, k0, k1 = _state(dtype, B, L, 6)
    return {"y0_in": (y0, "rc"), "y1": (y1, "rc"), "f0_in": (f0, "rc"), "f1": (f1, "rc"), "k0": (k0, "rc"), "k1": (k1, "rc"),
            "dts": (_dts(B, dtype), "r")}


def _commit_state(B):
    """Per row: not accepted, or accepted with 0, 1 (the step's end: x = 1) or 2 output times."""
    kind = np.arange(B) % 4
    lo = (np.arange(B) // 4) % 2
    hi = lo + np.array([0, 0, 1, 2])[kind]
    tprev, t1 = 0.25 + 0.001 * (np.arange(B) % 7), 0.75 + 0.001 * (np.arange(B) % 5)
    tgrid = np.full((N_OUT, B), 9.0)
    for r in range(B):
        for j in range(lo[r], hi[r]):
            tgrid[j, r] = t1[r] if kind[r] == 2 else tprev[r] + (t1[r] - tprev[r]) * (j - lo[r] + 1) / 4
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()      # noqa: E731
    return {"tgrid": (dev(tgrid, F64), ".r"), "tprev": (dev(tprev, F64), "r"), "t0": (dev(t1, F64), "r"),
            "accepted": (dev(kind > 0, I32), "r"), "out_lo": (dev(lo, I32), "r"), "out_hi": (dev(hi, I32), "r")}


def _row_vectors(t):
    n, L = t["y1"].shape
    return RowVectors(t["y1"].device.type, n, L, t["tgrid"].cpu(), **{name: t[name].cpu() for name in
                                                                      ("tprev", "t0", "accepted", "out_lo", "out_hi")})


def _build_commit(dtype, B, L):
    ins = {**_build_quartic(dtype, B, L), **_commit_state(B)}
    return ins, {"sol": ((N_OUT, B, L), dtype, ".rc", None), "y0": ((B, L), dtype, "rc", "y0_in"),
                 "f0": ((B, L), dtype, "rc", "f0_in")}


def _call_commit(k, t):
    rows = _row_vectors(t)
    k.row_dense_commit(t["sol"], t["y0"], t["y1"], t["f0"], t["f1"], _ks(t), MID, t["dts"], rows.st)


def _build_commit_mapped(dtype, B, L):
    ins, outs = _build_commit(dtype, B, L)
    ins["row_map"] = (torch.tensor(_perm(B, B + 5), dtype=I32).cuda(), "r")
    outs["sol"] = ((N_OUT, B + 5, L), dtype, "..c", None)
    return ins, outs


def _call_commit_mapped(k, t):
    rows = _row_vectors(t)
    k.row_dense_commit_mapped(t["sol"], t["row_map"], t["y0"], t["y1"], t["f0"], t["f1"], _ks(t), MID, t["dts"], rows.st)


def _build_fit(dtype, B, L):
    ins = {**_build_quartic(dtype, B, L), "fired": (_taken(B, 2), "r")}
    return ins, {"q": ((5, B, L), dtype, ".rc", None)}


def _call_fit(k, t):
    k.row_event_fit(t["q"], t["fired"], t["y0_in"], t["y1"], t["f0_in"], t["f1"], _ks(t), MID, t["dts"])


def _build_fit_mapped(dtype, B, L):
    ins, _ = _build_fit(dtype, B, L)
    ins["row_map"] = (torch.tensor(_perm(B, B + 3), dtype=I32).cuda(), "r")
    return ins, {"q": ((5, B + 3, L), dtype, "..c", None)}


def _call_fit_mapped(k, t):
    k.row_event_fit_mapped(t["q"], t["row_map"], t["fired"], t["y0_in"], t["y1"], t["f0_in"], t["f1"], _ks(t), MID, t["dts"])


def _build_eval(dtype, B, L):
    q = torch.stack(_state(dtype, B, L, 5))
    x = _per_row(B, lambda r: ((r * 37) % 101) / 100.0, dtype)
    return {"q": (q, ".rc"), "x": (x, "r"), "mask": (_taken(B), "r")}, {"out": ((B, L), dtype, "rc", None)}


Q_ROWS = 61


def _build_eval_mapped(dtype, B, L):
    g = torch.Generator(device="cuda").manual_seed(61)
    q = torch.randn(5, Q_ROWS, L, generator=g, dtype=dtype, device="cuda")       # [5, 61, L]: many queries read one row
    x = _per_row(B, lambda r: ((r * 37) % 101) / 100.0, dtype)
    ins = {"q": (q, "..c"), "x": (x, "r"), "src": (_per_row(B, lambda r: (r * 7) % Q_ROWS, I32), "r"),
           "dst": (torch.tensor(_perm(B, B + 2), dtype=I32).cuda(), "r")}
    return ins, {"mapped": ((B + 2, L), dtype, ".c", None), "plain": ((B, L), dtype, "rc", None)}


def _call_eval_mapped(k, t):
    k.row_event_eval_mapped(t["mapped"], t["dst"], t["q"], t["src"], t["x"])
    k.row_event_eval_mapped(t["plain"], None, t["q"], t["src"], t["x"])


# ---- the record: row_dense_pack, row_dense_prefix, row_dense_calc, row_dense_extremum, row_dense_level -----------------------
def _build_pack(dtype, B, L):
    src = torch.stack(_state(dtype, B, L, 5))
    dest = torch.tensor(_perm(B, B + 4), dtype=I64).cuda()
    return {"src": (src, ".rc"), "dest": (dest, "r")}, {"dst": ((5, B + 4, L), dtype, "..c", None)}


def _call_pack(k, t):
    k.row_dense_pack(t["dst"], t["src"], t["dest"], t["dest"].numel())


def _edges(n_rows, counts):
    """Per row `counts[r]` segments that follow each other in time -> (offsets, ta, tb) on the CPU, fp64."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ta, tb = np.empty(off[-1]), np.empty(off[-1])
    for r in range(n_rows):
        e = 0.1 * (r % 11) + 0.05 * np.arange(counts[r] + 1) * (1 + 0.1 * (r % 3))
        ta[off[r]:off[r + 1]], tb[off[r]:off[r + 1]] = e[:-1], e[1:]
    return torch.from_numpy(off), torch.from_numpy(ta), torch.from_numpy(tb)


def _build_prefix(dtype, B, L):
    """The launch walks B record rows (one lane per element): one or two segments each, so that the record stays small."""
    counts = [1 + r % 2 for r in range(B)]
    off, ta, tb = _edges(B, counts)
    n_seg = int(off[-1])
    g = torch.Generator(device="cuda").manual_seed(77)
    coeffs = torch.randn(5, n_seg, L, generator=g, dtype=dtype, device="cuda")
    ins = {"coeffs": (coeffs, "..c"), "off": (off.cuda(), "R"), "ta": (ta.cuda(), "."), "tb": (tb.cuda(), ".")}
    return ins, {"prefix": ((n_seg, L), F64, ".c", None)}


def _call_prefix(k, t):
    # (a slice run passes the offsets of its rows alone: they index the whole record, which the kernel is given in full)
    k.row_dense_prefix(t["prefix"], t["coeffs"], t["off"], t["ta"], t["tb"])


def _ref_prefix(k, t):
    """np_prefix on the rows of the window; only their segments are written."""
    off = t["off"].numpy()
    P = np_prefix(t["coeffs"].numpy(), off, t["ta"].numpy(), t["tb"].numpy())
    t["prefix"][off[0]:off[-1]] = torch.from_numpy(P[off[0]:off[-1]])


N_REC, PER = 7, 3


def _record_and_queries(dtype, B, L, hip):
    off, ta, tb = _edges(N_REC, [PER] * N_REC)
    n_seg = N_REC * PER
    g = torch.Generator(device="cuda").manual_seed(99)
    coeffs = torch.randn(5, n_seg, L, generator=g, dtype=dtype, device="cuda")
    prefix = torch.empty(n_seg, L, dtype=F64, device="cuda")
    hip.row_dense_prefix(prefix, coeffs, off.cuda(), ta.cuda(), tb.cuda())       # (one pass; tied to the oracle elsewhere)
    c = torch.Generator().manual_seed(3)
    row = torch.arange(B) % N_REC
    s = [row * PER + torch.randint(0, PER, (B,), generator=c) for _ in range(2)]
    tq = [ta[si] + torch.rand(B, generator=c, dtype=F64) * (tb[si] - ta[si]) for si in s]
    swap = tq[1] < tq[0]                                              # the window runs forward in time
    s = [torch.where(swap, s[1], s[0]), torch.where(swap, s[0], s[1])]
    tq = [torch.where(swap, tq[1], tq[0]), torch.where(swap, tq[0], tq[1])]
    x = [((tqi - ta[si]) / (tb[si] - ta[si])).to(dtype) for si, tqi in zip(s, tq)]         # as row_dense_search rounds it
    ins = {"coeffs": (coeffs, "..c"), "prefix": (prefix, ".c"), "ta": (ta.cuda(), "."), "tb": (tb.cuda(), ".")}
    for j in range(2):
        ins.update({f"seg{j}": (s[j].to(I32).cuda(), "r"), f"x{j}": (x[j].cuda(), "r"), f"tq{j}": (tq[j].cuda(), "r")})
    return ins


def _queries(t):
    return t["seg0"], t["x0"], t["tq0"], t["seg1"], t["x1"], t["tq1"]


def _build_calc(dtype, B, L, hip):
    return _record_and_queries(dtype, B, L, hip), {name: ((B, L), dtype, "rc", None) for name in ("d", "a", "i")}


def _call_calc(k, t):
    for mode, name in enumerate(("d", "a", "i")):
        k.row_dense_calc(t[name], mode, t["coeffs"], t["ta"], t["tb"], t["prefix"], 1.0, *_queries(t))


def _build_extremum(dtype, B, L, hip):
    ins = _record_and_queries(dtype, B, L, hip)
    outs = {}
    for which in ("max", "min"):
        outs[f"{which}_v"], outs[f"{which}_t"] = ((B, L), dtype, "rc", None), ((B, L), F64, "rc", None)
    return ins, outs


def _call_extremum(k, t):
    for which, name in enumerate(("max", "min")):
        k.row_dense_extremum(t[f"{name}_v"], t[f"{name}_t"], which, t["coeffs"], t["ta"], t["tb"], 1.0, *_queries(t))


def _build_level(dtype, B, L, hip):
    ins = _record_and_queries(dtype, B, L, hip)
    level, = _state(dtype, B, L, 1)                                  # a level per query and element, of the record's magnitude
    ins["level"] = (level, "rc")
    outs = {"count": ((B, L), I32, "rc", None)}
    outs.update({name: ((B, L), F64, "rc", None) for name in ("first", "last", "above")})
    return ins, outs


def _call_level(k, t):
    k.row_dense_level(t["count"], t["first"], t["last"], t["above"], t["level"], t["coeffs"], t["ta"], t["tb"], 1.0, *_queries(t))


CASES = [
    Rows("row_combine", _build_combine, _call_combine),
    Rows("row_select", _build_select, lambda k, t: k.row_select(t["dst"], t["src"], t["mask"])),
    Rows("row_impulse", _build_impulse,
         lambda k, t: k.row_impulse(t["y"], t["dy"], t["dy_index"], t["jump_hit"], t["jumped"], t["row_map"])),
    Rows("row_gather", _build_gather, lambda k, t: k.row_gather([t["o0"], t["o1"]], [t["a"], t["b"]], t["idx"])),
    Rows("row_scale_many", _build_scale, lambda k, t: k.row_scale_many([t["o0"], t["o1"], t["o2"]], t["g"], t["w"])),
    Rows("row_dense_commit", _build_commit, _call_commit),
    Rows("row_dense_commit_mapped", _build_commit_mapped, _call_commit_mapped),
    Rows("row_event_fit", _build_fit, _call_fit),
    Rows("row_event_fit_mapped", _build_fit_mapped, _call_fit_mapped),
    Rows("row_event_eval", _build_eval, lambda k, t: k.row_event_eval(t["out"], t["q"], t["x"], t["mask"])),
    Rows("row_event_eval_mapped", _build_eval_mapped, _call_eval_mapped),
    Rows("row_dense_pack", _build_pack, _call_pack),
    Rows("row_dense_prefix", _build_prefix, _call_prefix, _ref_prefix),
    Rows("row_dense_calc", _build_calc, _call_calc),
    Rows("row_dense_extremum", _build_extremum, _call_extremum),
    Rows("row_dense_level", _build_level, _call_level),
]
NEEDS_HIP = ("row_dense_calc", "row_dense_extremum", "row_dense_level")


@pytest.mark.parametrize("case,dtype,form", [pytest.param(c, d, f, id=f"{c.name}-{lf.NAME[d]}-{f}")
                                             for f in ("vec", "scalar") for d in lf.REAL for c in CASES])
def test_rows(hip_kernels, oracle_kernels, case, dtype, form):
    if case.name in NEEDS_HIP:        # (their record's prefix sums come from one small launch of the HIP kernel)
        build = case.build
        case = Rows(case.name, lambda dt, B, L: build(dt, B, L, hip_kernels), case.call, case.ref)
    lf.check_rows(case, dtype, form, hip_kernels, LevelOracle(oracle_kernels))


def test_shapes_exceed_the_cap_and_the_second_pass_crosses_rows():
    for form, lens in lf.ROW_LEN.items():
        for dtype, L in lens.items():
            le = L // (lf.LANE[dtype] if form == "vec" else 1)
            assert ROWS * le > lf.CAP and (ROWS * le - lf.CAP) > 3 * le          # the second pass crosses three row boundaries
