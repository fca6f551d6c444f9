"""Shared pieces of the launch-form tests (tests/test_launch_policy_gpu.py, test_grid_stride_gpu.py,
test_rowwise_grid_stride_gpu.py).  No test in here.

The streaming kernels choose an instantiation or a loop shape from the launch size alone: a cache policy
from the bytes the streams touch, and a grid-stride loop past `kMaxGrid` = 65536 workgroups of 256 lanes = 2^24 items.

  * `run_child`: one pytest child per setting of the two environment variables `stream_policy()` reads once per process.
  * `check_flat` / `check_rows`: one entry point past the grid cap, checked three ways, all bit for bit —
      1. windows (the start, the item where the second pass begins, the end) against the CPU oracle on copies;
      2. the whole result against launches of the same entry point on slices below the cap (the one-pass form is what
         the kernel tests tie to the oracle, and the operations are elementwise);
      3. a 64-element sentinel border on both sides of every output.
"""
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 24                    # items one grid pass covers (csrc/tdeq_abi.hip: kMaxGrid workgroups of kBlock lanes)
ITEMS = CAP + 773                # three full workgroups and five lanes of second pass
PAD = 64
REAL = (torch.float32, torch.float64)
LOW = (torch.bfloat16, torch.float16)
LANE = {torch.float32: 4, torch.float64: 2, torch.bfloat16: 8, torch.float16: 8}       # elements per 16-byte access
INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16,
       torch.int32: torch.int32}
# NaNs with a payload (no kernel result has these bits); for int32 outputs simply a value no count reaches
SENTINEL = {torch.int32: 0x7FA5A5A5, torch.int64: 0x7FF5A5A5A5A5A5A5, torch.int16: 0x7FA5}
NAME = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.float16: "f16"}


def bits(t):
    return t.view(INT[t.dtype])


def same_bits(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    if not torch.equal(bits(got), bits(ref)):
        bad = (bits(got) != bits(ref)).nonzero()
        raise AssertionError((what, "differs at", bad[0].tolist(), "and", bad.shape[0] - 1, "more"))


# ---------------------------------------------------------------------------------------------------------------------
# child processes
# ---------------------------------------------------------------------------------------------------------------------
POLICY_VARS = ("TDEQ_COMBINE_POLICY", "TDEQ_NT_THRESHOLD_MB")
CHILD_MARK = "TDEQ_LAUNCH_FORMS_CHILD"       # set in every child: a test that starts children refuses to run inside one
DIED = (134, 139, 124, 137)                  # abort, segmentation fault, time limits
_state = {"died": None}                      # the first child that ended by signal or time limit: nothing more is started
_collected = {}


def _child_env(setting):
    env = {k: v for k, v in os.environ.items() if k not in POLICY_VARS}
    env.update(setting)
    env[CHILD_MARK] = "1"
    return env


def _counts(text):
    """{'passed': 3, 'failed': 1, ...} of pytest's last summary line."""
    for line in reversed(text.strip().splitlines()):
        found = re.findall(r"(\d+) (passed|failed|skipped|error|errors|xfailed|xpassed|deselected)", line)
        if found:
            return {k.rstrip("s") if k.startswith("error") else k: int(v) for v, k in found}
    return {}


def collected_count(node_ids):
    """How many gpu tests the node list holds, collected by a child with neither variable set (no GPU is touched)."""
    key = tuple(node_ids)
    if key not in _collected:
        r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--collect-only", *node_ids], cwd=ROOT,
                           env=_child_env({}), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"(\d+)(?:/\d+)? tests? collected", r.stdout)
        assert m, r.stdout[-3000:]
        _collected[key] = int(m.group(1))
    return _collected[key]


def run_child(node_ids, setting, timeout):
    """Run the node list in one fresh pytest child under `setting`; every test of it must pass, none may be skipped.
    A child that ends by signal or time limit fails this case and every later one, without another process."""
    assert os.environ.get(CHILD_MARK) != "1", "a test that starts child processes was listed for a child"
    assert _state["died"] is None, f"not started: an earlier child ended by signal or time limit ({_state['died']})"
    want = collected_count(node_ids)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", *node_ids],
                           cwd=ROOT, env=_child_env(setting), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as exc:
        _state["died"] = f"{setting}: no end after {timeout} s"
        raise AssertionError(_state["died"] + "\n" + str(exc.stdout)[-2000:])
    tail = r.stdout[-4000:] + r.stderr[-2000:]
    if r.returncode < 0 or r.returncode in DIED:
        _state["died"] = f"{setting}: exit status {r.returncode}"
        raise AssertionError(_state["died"] + "\n" + tail)
    got = _counts(r.stdout)
    assert r.returncode == 0, (setting, r.returncode, got, tail)
    assert not got.get("failed") and not got.get("error") and not got.get("skipped"), (setting, got, tail)
    assert got.get("passed") == want, (setting, got, "collected without a variable:", want)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# outputs inside sentinel borders, inputs shared by the cases of one geometry
# ---------------------------------------------------------------------------------------------------------------------
class Window:
    """An output of `shape` inside an allocation filled with a sentinel bit pattern, `offset` elements past a 16-byte
    boundary.  `row_stride`: a [rows, n] output whose rows lie that far apart (the gaps are border too)."""

    def __init__(self, shape, dtype, offset=0, row_stride=None):
        shape = tuple(shape)
        numel = 1
        for s in shape:
            numel *= s
        self.n_row = shape[-1] if row_stride else numel
        self.stride = row_stride or numel
        self.rows = shape[0] if row_stride else 1
        span = (self.rows - 1) * self.stride + self.n_row
        self.raw = torch.full((PAD + offset + span + PAD,), SENTINEL[INT[dtype]], dtype=INT[dtype], device="cuda")
        self.lo = PAD + offset
        flat = self.raw.view(dtype)[self.lo:self.lo + span]
        self.t = flat.as_strided(shape, (row_stride, 1)) if row_stride else flat.view(shape)
        assert self.raw.data_ptr() % 16 == 0 and (self.t.data_ptr() % 16 == 0) == (offset == 0)

    def intact(self):
        s, raw = SENTINEL[self.raw.dtype], self.raw
        ok = bool((raw[:self.lo] == s).all())
        for r in range(self.rows):
            end = self.lo + r * self.stride + self.n_row
            nxt = self.lo + (r + 1) * self.stride if r + 1 < self.rows else raw.numel()
            ok = ok and bool((raw[end:nxt] == s).all())
        return ok


_pool = {}


def streams(dtype, n, offset, count, seed=0):
    """`count` randn streams of `n` elements of `dtype` on the GPU, `offset` elements past a 16-byte boundary; one pool is
    alive at a time and is shared by the cases that ask for the same geometry."""
    key = (dtype, n, offset, seed)
    if key not in _pool or _pool[key].shape[0] < count:
        _pool.clear()
        torch.cuda.empty_cache()
        g = torch.Generator(device="cuda").manual_seed(1234 + seed)
        buf = torch.empty(max(count, 14), -(-(n + offset) // 64) * 64 + 64, dtype=dtype, device="cuda")
        for row in buf:
            row.normal_(generator=g)
        _pool[key] = buf
    buf = _pool[key]
    assert bool(torch.isfinite(buf[0, :4096].float()).all())
    return [buf[j, offset:offset + n] for j in range(count)]


def release():
    _pool.clear()
    torch.cuda.empty_cache()


class Env:
    """What a case needs besides tensors, for the HIP kernels (device tensors) or the oracle (CPU tensors)."""

    def __init__(self, kern, dtype):
        self.kern, self.dtype = kern, dtype
        self.device = None if kern.name == "oracle" else torch.device("cuda:0")
        self._plan = None

    def tensor(self, data, dtype):
        return torch.tensor(data, dtype=dtype, device=self.device or "cpu")

    def plan(self, accept, dt):
        """A plan whose device-resident controller words say {accept, sign * T(dt)}."""
        if self._plan is None:
            self._plan = self.kern.make_plan([(0, 1024, 1e-5, 1e-7)], 1024, 1024, self.device)
        self._plan.ctrl_dev[:2].copy_(torch.tensor([accept, as_type(dt, self.dtype)], dtype=torch.float64))
        return self._plan


def as_type(x, dtype):
    """A host number rounded to the state's type (through float32 for the 16-bit types, as the package does)."""
    t = torch.tensor(float(x), dtype=torch.float64)
    if dtype in LOW:
        t = t.to(torch.float32)
    return float(t.to(dtype))


# ---------------------------------------------------------------------------------------------------------------------
# flat-state entry points
# ---------------------------------------------------------------------------------------------------------------------
class Flat:
    """One flat-state entry point.  `call(kern, x, o, env)` launches it on the input streams `x` into the outputs `o`;
    `outs` = per output (rows, init): rows > 1 a [rows, n] output, init = the index of the stream an in-place output
    starts from (None: nothing but the kernel writes it).  `ref`: the same on the oracle where its interface differs.
    `contiguous`: the rows of a [rows, n] output lie n apart (the 16-byte form then needs n % lane == 0).  `one_lane`: the
    entry point has no 16-byte form (one element per item at the 16-byte size too)."""

    def __init__(self, name, n_in, outs, call, ref=None, contiguous=False, one_lane=False):
        self.name, self.n_in, self.outs, self.call, self.ref = name, n_in, outs, call, ref or call
        self.contiguous, self.one_lane = contiguous, one_lane


def flat_size(dtype, form, whole_lanes=False):
    if form == "scalar":
        return ITEMS
    lane = LANE[dtype]
    return lane * ITEMS + (0 if whole_lanes else lane - 1)


def flat_windows(n, lane):
    """The start, where the second pass begins (up to 2048 elements of it: at fp64 and in the scalar form the tensor
    ends sooner), the partial workgroup and the scalar tail."""
    return [(0, 4096), (lane * CAP - 2048, min(lane * CAP + 2048, n)), (n - 4099, n)]


def flat_slices(n):
    step = (n // 5) // 64 * 64               # slice starts stay 16-byte aligned (or stay one element off, scalar form)
    cuts = [i * step for i in range(5)] + [n]
    return list(zip(cuts[:-1], cuts[1:]))


def _flat_outputs(case, x, lo, hi, dtype, offset):
    wins = []
    for rows, init in case.outs:
        m = hi - lo
        if rows == 1:
            w = Window((m,), dtype, offset)
        else:
            w = Window((rows, m), dtype, offset, row_stride=m if case.contiguous else -(-m // 16) * 16 + 16)
        if init is not None:
            w.t.copy_(x[init][lo:hi].expand_as(w.t))
        wins.append(w)
    return wins


def check_flat(case, dtype, form, hip, oracle):
    lane = LANE[dtype] if form == "vec" and not case.one_lane else 1
    offset = 0 if form == "vec" else 1
    n = flat_size(dtype, form, whole_lanes=case.contiguous)
    assert n // lane > CAP
    n_streams = max([case.n_in] + [i + 1 for _, i in case.outs if i is not None])
    x = [t[:n] for t in streams(dtype, flat_size(dtype, form), offset, n_streams)]
    env = Env(hip, dtype)
    whole = _flat_outputs(case, x, 0, n, dtype, offset)
    case.call(hip, x[:case.n_in], [w.t for w in whole], env)
    # 2. slice by slice, every slice below the cap
    for lo, hi in flat_slices(n):
        assert (hi - lo) // lane < CAP and lo % 64 == 0
        part = _flat_outputs(case, x, lo, hi, dtype, offset)
        case.call(hip, [t[lo:hi] for t in x[:case.n_in]], [p.t for p in part], env)
        for j, (w, p) in enumerate(zip(whole, part)):
            assert p.intact(), (case.name, "slice", lo, "output", j, "wrote outside its slice")
            same_bits(w.t[..., lo:hi], p.t, (case.name, "whole against the slice from", lo, "output", j))
        del part
    # 3. the borders of the whole launch
    for j, w in enumerate(whole):
        assert w.intact(), (case.name, "output", j, "wrote outside [0, n)")
    # 1. windows against the oracle
    oenv = Env(oracle, dtype)
    for lo, hi in flat_windows(n, lane):
        xc = [t[lo:hi].cpu().contiguous() for t in x]
        ref = _flat_ref_outputs(case, xc, hi - lo, dtype)
        case.ref(oracle, xc[:case.n_in], ref, oenv)
        for j, (w, r) in enumerate(zip(whole, ref)):
            same_bits(w.t[..., lo:hi].cpu().contiguous(), r, (case.name, "window", lo, hi, "output", j))


def _flat_ref_outputs(case, xc, m, dtype):
    outs = []
    for rows, init in case.outs:
        shape = (m,) if rows == 1 else (rows, m)
        if init is None:
            t = torch.full(shape, SENTINEL[INT[dtype]], dtype=INT[dtype]).view(dtype)
        else:
            t = xc[init].expand(shape).clone()
        outs.append(t)
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# rowwise entry points: launches over n_rows * row_len items
# ---------------------------------------------------------------------------------------------------------------------
ROWS = 4099
ROW_LEN = {"scalar": {torch.float32: 4099, torch.float64: 4099}, "vec": {torch.float32: 16388, torch.float64: 8194}}


class Rows:
    """One rowwise entry point.  `build(dtype, B, L)` -> (ins, outs): `ins` name -> (tensor on the GPU, spec), `outs`
    name -> (shape, dtype, spec, init).  A spec names each axis: 'r' the launch's row axis (what a slice run cuts), 'R' that
    axis with one more entry (offsets), 'c' the element axis (what an oracle window cuts besides), '.' anything else.  An
    output without 'r' is indexed through a map: the slice runs share one full-size copy of it.  `init`: the input an
    in-place output starts from.  `call(kern, t)` launches on the tensors `t` (inputs and outputs by name); `ref` the
    same on the oracle where that differs."""

    def __init__(self, name, build, call, ref=None):
        self.name, self.build, self.call, self.ref = name, build, call, ref or call


def _cut(t, spec, rows=None, cols=None):
    idx = []
    for ch in spec:
        if ch == "r" and rows is not None:
            idx.append(slice(rows[0], rows[1]))
        elif ch == "R" and rows is not None:
            idx.append(slice(rows[0], rows[1] + 1))
        elif ch == "c" and cols is not None:
            idx.append(slice(cols[0], cols[1]))
        else:
            idx.append(slice(None))
    return t[tuple(idx)]


def _cut_shape(shape, spec, rows=None, cols=None):
    return tuple(_cut(torch.empty(shape, device="meta"), spec, rows, cols).shape)


def row_slices(B):
    step = -(-B // 5)
    return [(lo, min(lo + step, B)) for lo in range(0, B, step)]


def row_windows(B, L, lane):
    """(rows, columns): the first rows, the rows around item 2^24 with the elements around it, the last rows."""
    le = L // lane
    r, c = CAP // le, (CAP % le) * lane
    return [((0, 3), (0, min(16, L))), ((r - 1, min(r + 2, B)), (max(c - 8, 0), min(c + 8, L))),
            ((B - 6, B), (0, min(8, L))), ((B - 3, B), (max(L - 16, 0), L))]


def check_rows(case, dtype, form, hip, oracle):
    B, L = ROWS, ROW_LEN[form][dtype]
    lane = LANE[dtype] if form == "vec" else 1
    assert (L % LANE[dtype] == 0) == (form == "vec")          # what decides the form of a row kernel (aligned bases given)
    assert B * (L // lane) > CAP
    ins, outs = case.build(dtype, B, L)

    def windows_for(rows):
        res = {}
        for name, (shape, odt, spec, init) in outs.items():
            if rows is not None and "r" not in spec:
                continue
            w = Window(_cut_shape(shape, spec, rows), odt)
            if init is not None:
                w.t.copy_(_cut(ins[init][0], ins[init][1], rows))
            res[name] = w
        return res

    whole = windows_for(None)
    case.call(hip, {**{k: v[0] for k, v in ins.items()}, **{k: w.t for k, w in whole.items()}})
    # 2. runs of whole rows below the cap
    joined = {name: Window(shape, odt) for name, (shape, odt, spec, init) in outs.items() if "r" not in spec}
    for rows in row_slices(B):
        assert (rows[1] - rows[0]) * (L // lane) < CAP
        part = windows_for(rows)
        t = {k: _cut(v, spec, rows).contiguous() for k, (v, spec) in ins.items()}
        t.update({k: w.t for k, w in part.items()})
        t.update({k: w.t for k, w in joined.items()})
        case.call(hip, t)
        for name, p in part.items():
            assert p.intact(), (case.name, "rows from", rows[0], name, "wrote outside its slice")
            same_bits(_cut(whole[name].t, outs[name][2], rows), p.t, (case.name, "whole against the rows from", rows[0], name))
        del part, t
    for name, j in joined.items():
        assert j.intact(), (case.name, name, "joined")
        same_bits(whole[name].t, j.t, (case.name, "whole against the joined slice runs", name))
    # 3. borders
    for name, w in whole.items():
        assert w.intact(), (case.name, name, "wrote outside the output")
    # 1. windows against the oracle
    for rows, cols in row_windows(B, L, lane):
        t = {k: _cut(v, spec, rows, cols).cpu().contiguous() for k, (v, spec) in ins.items()}
        ref = {}
        for name, (shape, odt, spec, init) in outs.items():
            if init is None:
                ref[name] = torch.full(_cut_shape(shape, spec, rows, cols), SENTINEL[INT[odt]], dtype=INT[odt]).view(odt)
            else:
                ref[name] = t[init].clone()
        case.ref(oracle, {**t, **ref})
        for name, r in ref.items():
            spec = outs[name][2]
            got = _cut(whole[name].t, spec, rows, cols).cpu().contiguous()
            what = (case.name, "rows", rows, "columns", cols, name)
            if "r" in spec:
                same_bits(got, r, what)
            else:                     # written through a map: what the oracle wrote for these rows
                wrote = bits(r) != SENTINEL[INT[r.dtype]]
                assert bool(wrote.any()), what
                same_bits(got[wrote], r[wrote], what)
