"""Recorder of tests/golden/rowwise_family_launch_log.json: what `odeint_rowwise`, `odeint_rowwise_event` and
`odeint_rowwise_dense` LAUNCH, call for call and argument for argument, on the CPU (no GPU needed).

The fixture was recorded from the tree of the commit BEFORE the three entry points got one driver loop, one step hook and
one bisection, and has not been edited since: it pins what that refactor had to keep.

The log and the proxy are those of make_odeint_launch_log.py (`Log`, `LoggedKernels`, `compact`, `dump`'s layout); `sig` is
extended here by an address-free signature of `_native.RowState` (its integer fields) and `_native.StepCtrl` (a constant).
Besides the kernel calls the log holds, in sequence, every call of `func` ("f") and of `event_fn` ("e") with `list(y.shape)`
and `rows.tolist()` (None without `compact`).

"dev" regimes: the device driver (`HipRowKernels`) on the CPU oracle of tests/_rowwise_dense_oracle.py, as the tests run it.
"host" regimes: the same calls on `HostRowKernels`, nothing patched — the log then holds the `func` / `event_fn` calls only.
Per regime the fixture keeps the call count, the SHA-256 of the whole log, the explicit log up to the end of the second trial
step (shared logs kept once), a byte digest of every returned tensor, every `stats` entry and the error message, if any.

    python tests/golden/make_rowwise_launch_log.py          # rewrites the fixture from the tree it runs in

tests/test_rowwise_launch_log.py re-runs every regime and compares all recorded fields."""
import collections
import contextlib
import functools
import hashlib
import importlib.util
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _path in (os.path.join(ROOT, "tests"), ROOT):
    if _path not in sys.path:
        sys.path.insert(0, _path)
FIXTURE = os.path.join(HERE, "rowwise_family_launch_log.json")

_spec = importlib.util.spec_from_file_location("make_odeint_launch_log", os.path.join(HERE, "make_odeint_launch_log.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

B, L = 7, 5
COMPACT = (None, 0.5, 1.0)
COUNTED = ("f", "e", "row_gather")      # counted per case: the calls of func, of event_fn and the repacks' gathers


class RowLog(base.Log):
    def sig(self, v):
        from torchdiffeq_amd import _native
        if isinstance(v, _native.RowState):      # (its other fields are addresses)
            return ["rowstate", int(v.n_rows), int(v.row_len), int(v.n_out), int(v.order), int(v.max_num_steps)]
        if isinstance(v, _native.StepCtrl):
            return "ctrl"
        return super().sig(v)

    def called(self, letter, fn):
        """`fn` (func or event_fn, taking `rows` or not) with every call logged."""
        def logged(t, y, rows=None):
            self.calls.append([letter, [list(y.shape), None if rows is None else rows.tolist()], {}])
            return fn(t, y) if rows is None else fn(t, y, rows)
        return logged


class Detaching:
    """Proxy of the oracle that detaches every tensor argument (the same storage): a recorded solve hands its launches
    graph tensors, which a HIP kernel takes by address and the oracle's numpy arithmetic refuses."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if name.startswith("_") or not callable(value):
            return value

        def strip(v):
            if isinstance(v, torch.Tensor):
                return v.detach()
            return type(v)(strip(x) for x in v) if type(v) in (list, tuple) else v
        return lambda *args, **kwargs: value(*strip(args), **{k: strip(v) for k, v in kwargs.items()})


@contextlib.contextmanager
def logged_backend(log, dev):
    """`dev`: `_native.get_kernels` answers with a logging proxy of the dense oracle and `HipRowKernels` stands in for
    `HostRowKernels` (the tests' `device_driver`).  Either way the start of every trial step is marked."""
    from _rowwise_dense_oracle import DenseOracle
    from oracle.kernels import OracleKernels
    from torchdiffeq_amd import _fallback, _native, rowwise
    orig_get, orig_host, warned = _native.get_kernels, rowwise.HostRowKernels, _fallback._warned
    steps = {cls: cls.trial_step for cls in (rowwise.HostRowKernels, rowwise.HipRowKernels)}

    def marking(step):
        def trial_step(self, *args, **kwargs):
            log.marks.append(len(log.calls))
            return step(self, *args, **kwargs)
        return trial_step
    for cls, step in steps.items():
        cls.trial_step = marking(step)
    if dev:
        proxy = base.LoggedKernels(Detaching(DenseOracle(OracleKernels())), log)
        _native.get_kernels = lambda device, dtype=None: proxy
        rowwise.HostRowKernels = rowwise.HipRowKernels
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            yield
    finally:
        _native.get_kernels, rowwise.HostRowKernels = orig_get, orig_host
        for cls, step in steps.items():
            cls.trial_step = step
        _fallback._warned = warned


# ---- the problem and the solves -------------------------------------------------------------------------------------
def _setup(dtype, method, tol):
    from _rowwise_dense_oracle import decay_problem, per_row_t1
    y0, func, _ = decay_problem(B, L, dtype, 3)
    kw = dict(rtol=1e-3, atol=1e-5) if method == "bosh3" else dict(rtol=1e-6, atol=1e-8)
    if tol == "rtol_rows":
        kw["rtol"] = torch.logspace(-4, -7, B, dtype=torch.float64)
    elif tol == "atol_rows":
        kw["atol"] = torch.logspace(-7, -9, B, dtype=torch.float64)
    return y0, func, per_row_t1(B), dict(kw, method=method)


def _plain(log, compact, method="dopri5", dtype=torch.float64, grid="TB", tol=None, options=None, differentiable=False):
    import torchdiffeq_amd as tda
    y0, func, t1, kw = _setup(dtype, method, tol)
    t = {"TB": torch.stack([torch.zeros(B, dtype=torch.float64), t1 / 2, t1]),
         "T": torch.tensor([0.0, 0.2, 0.45], dtype=torch.float64),
         "reverse": -torch.stack([torch.zeros(B, dtype=torch.float64), t1 / 2, t1]),
         # the stiffest row, row 0, has next to nothing to do: it leaves first and another row runs out of steps
         "short_row0": torch.stack([torch.zeros(B, dtype=torch.float64), torch.cat([t1.new_tensor([1e-3]), t1[1:]])])}[grid]
    if differentiable:
        y0 = y0.requires_grad_(True)
        with torch.enable_grad():
            sol, stats = tda.odeint_rowwise(log.called("f", func), y0, t, differentiable=True, return_stats=True, **kw)
            sol[-1].pow(2).sum().backward()
        return {"solution": sol, "y0_grad": y0.grad}, stats
    sol, stats = tda.odeint_rowwise(log.called("f", func), y0, t, compact=compact, options=options, return_stats=True, **kw)
    return {"solution": sol}, stats


@functools.lru_cache(maxsize=None)
def _crossing_t_end():
    """`t_end` with one row's end just before its event, inside the step the row fires in: that row's last step crosses
    `t_end` AND changes sign.  Found by two unlogged solves on the host backend (`run_case` asks before it patches)."""
    import torchdiffeq_amd as tda
    y0, func, t1, kw = _setup(torch.float64, "dopri5", None)

    def solve(t_end):
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            event_t, _, stats = tda.odeint_rowwise_event(func, y0, 0.0, event_fn=lambda t, y: y[:, 0] - 0.6, t_end=t_end,
                                                          return_stats=True, **kw)
        return event_t, stats
    event_t, st = solve(t1)
    r = int(torch.nonzero(st["fired"]).view(-1)[0])
    t_end = t1.clone()
    t_end[r] = event_t[r] - 1e-4
    _, st2 = solve(t_end)
    assert bool(st["fired"][r]) and not bool(st2["fired"][r]) and torch.equal(st2["n_accepted"], st["n_accepted"])
    return t_end


def _event(log, compact, variant="t_end", tol=None):
    import torchdiffeq_amd as tda
    y0, func, t1, kw = _setup(torch.float64, "dopri5", tol)
    level = torch.full((B,), 0.6, dtype=torch.float64)
    t_end = t1.clone()
    if variant == "reverse":
        t_end = -t1
    elif variant == "some_at_t0":
        level[[1, 4]] = y0[[1, 4], 0]
    elif variant == "all_at_t0":
        level = y0[:, 0].clone()
    elif variant == "crosses_t_end":
        t_end = _crossing_t_end()
    event_fn = lambda t, y, rows=None: y[:, 0] - (level if rows is None else level[rows])      # noqa: E731
    event_t, sol, stats = tda.odeint_rowwise_event(log.called("f", func), y0, 0.0, event_fn=log.called("e", event_fn),
                                                   t_end=t_end, compact=compact, return_stats=True, **kw)
    return {"event_t": event_t, "solution": sol}, stats


def _dense(log, compact, method="dopri5", dtype=torch.float64):
    import torchdiffeq_amd as tda
    y0, func, t1, kw = _setup(dtype, method, None)
    dense, stats = tda.odeint_rowwise_dense(log.called("f", func), y0, 0.0, t1, compact=compact, return_stats=True,
                                            options=dict(dense_chunk_rows=9), **kw)
    outside = t1 / 3
    outside[3] = 1.0
    out = {"coeffs": dense.coeffs, "offsets": dense.offsets, "seg_start": dense.seg_start, "seg_end": dense.seg_end,
           "dense_scalar": dense(0.1), "dense_Q": dense(torch.tensor([0.05, 0.25, 0.0], dtype=torch.float64)),
           "dense_QB": dense(torch.stack([t1 / 3, t1, t1 * 0.9])), "dense_unchecked": dense(outside, check=False)}
    assert bool(out["dense_unchecked"][3].isnan().all()) and not bool(out["dense_unchecked"][2].isnan().any())
    return out, stats


def _regimes():
    """name -> (solve, compact, its other keyword arguments); every one is run on both backends."""
    r = {}
    plain = {"TB": {}, "T": dict(grid="T"), "reverse": dict(grid="reverse"), "first_step": dict(options=dict(first_step=0.01)),
             "rtol_rows": dict(tol="rtol_rows"), "dopri8": dict(method="dopri8"), "bosh3": dict(method="bosh3"),
             "f32": dict(dtype=torch.float32)}
    event = {"t_end": {}, "reverse": dict(variant="reverse"), "some_at_t0": dict(variant="some_at_t0"),
             "all_at_t0": dict(variant="all_at_t0"), "crosses_t_end": dict(variant="crosses_t_end"),
             "atol_rows": dict(tol="atol_rows")}
    dense = {"chunks": {}, "bosh3_f32": dict(method="bosh3", dtype=torch.float32)}
    for family, solve, variants in (("plain", _plain, plain), ("event", _event, event), ("dense", _dense, dense)):
        for name, kw in variants.items():
            for c in COMPACT:
                r["{}/{}/compact={}".format(family, name, c)] = (solve, c, kw)
    for c in (None, 1.0):
        r["plain/max_num_steps/compact={}".format(c)] = (_plain, c, dict(grid="short_row0", options=dict(max_num_steps=6)))
    for m in ("dopri5", "tsit5"):
        r["recorded/{}".format(m)] = (_plain, None, dict(method=m, differentiable=True))
    return r


REGIMES = _regimes()
CASES = ["{}/{}".format(backend, name) for backend in ("dev", "host") for name in REGIMES]


def _plain_value(v):
    return v.tolist() if isinstance(v, torch.Tensor) else v


def run_case(case):
    backend, name = case.split("/", 1)
    solve, c, kw = REGIMES[name]
    if kw.get("variant") == "crosses_t_end":
        _crossing_t_end()
    log = RowLog()
    outs, stats, failed = {}, {}, None
    with logged_backend(log, backend == "dev"), torch.no_grad():
        try:
            outs, stats = solve(log, c, **kw)
        except AssertionError as exc:
            failed = str(exc)
    head = log.calls[:log.marks[2]] if len(log.marks) > 2 else log.calls
    return {"calls": len(log.calls), "trial_steps": len(log.marks), "sha256": log.digest(),
            "head": [base.compact(call) for call in head], "failed": failed,
            "counts": {k: n for k, n in collections.Counter(call[0] for call in log.calls).items() if k in COUNTED},
            "tensors": {k: base._bytes_digest(v)[:12] for k, v in outs.items()},
            "stats": {k: _plain_value(v) for k, v in stats.items()}}


def record():
    out = {}
    for case in CASES:
        rec = out[case] = run_case(case)
        print("{:44s} {:5d} calls {:4d} trial steps  {}".format(case, rec["calls"], rec["trial_steps"], rec["failed"] or ""))
    for case, rec in out.items():
        if "max_num_steps" in case:
            assert rec["failed"] is not None and "max_num_steps exceeded" in rec["failed"], case
            assert rec["failed"] == out["host/plain/max_num_steps/compact=None"]["failed"]      # the ORIGINAL row
            if case == "dev/plain/max_num_steps/compact=1.0":
                assert rec["counts"]["row_gather"] > 0, "no repack before the row failed"
        else:
            assert rec["failed"] is None, (case, rec["failed"])
        if "all_at_t0" in case:
            assert rec["trial_steps"] == 0 and "f" not in rec["counts"], case
        if case.startswith("dev/") and "compact=1.0" in case and "all_at_t0" not in case:
            assert rec["stats"].get("n_repacks", 1) > 0, case
        if "dense/" in case:
            assert rec["stats"]["n_chunks"] > 1, case
    return out


def dump(data, path):
    """The layout of make_odeint_launch_log.py's fixture: explicit logs that several cases share are kept once, in "logs",
    under the first 8 digits of their digest; one line per case."""
    logs = {}

    def key(lines):
        k = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:8]
        assert logs.setdefault(k, lines) == lines
        return k

    def row(d):
        return ",\n".join('  {}: {}'.format(json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in d.items())
    cases = {n: dict(r, head=key(r["head"])) for n, r in data.items()}
    with open(path, "w") as f:
        f.write('{{\n "cases": {{\n{}\n }},\n "logs": {{\n{}\n }}\n}}\n'.format(row(cases), row(logs)))


def load(path=FIXTURE):
    """The fixture with every case's explicit log in place again."""
    with open(path) as f:
        data = json.load(f)
    for r in data["cases"].values():
        r["head"] = data["logs"][r["head"]]
    return data["cases"]


if __name__ == "__main__":
    dump(record(), FIXTURE)
    load()
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
