"""Recorder of tests/golden/odeint_launch_log.json: what `odeint`'s adaptive trial step LAUNCHES, call for call and argument
for argument, on the CPU (no GPU needed).

Part "solves": whatever `_native.get_kernels` returns — the CPU oracle standing in for the HIP kernels, or the torch-op host
path — is wrapped in a proxy that logs every public kernel method with a signature of its arguments (tensors as a tag that
follows the data: the same buffer keeps its tag, so the log also pins which tensor goes where; coefficients and scalars as
`float.hex`).  Per regime the fixture keeps the call count, a SHA-256 of the whole log, the explicit log up to the end of the
second trial step (one short line per call, `compact`), the solution's byte digest, the number of func evaluations and the accept / reject record.

Part "graph_body": one `_GraphStep.body(s, side)` replayed on a logging stand-in for the kernels (no arithmetic), the
`_GraphStep` made without its constructor.

    python tests/golden/make_odeint_launch_log.py          # rewrites the fixture from the tree it runs in

tests/test_odeint_launch_log.py re-runs every regime and compares all recorded fields."""
import contextlib
import ctypes
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "odeint_launch_log.json")

METHODS = ("dopri5", "tsit5", "dopri8", "bosh3", "fehlberg2", "adaptive_heun")
# per method (rtol, atol) at which every solve of the problem below takes between 4 and 200 trial steps (the order-2 pairs
# need hundreds to thousands at the defaults)
TOL = {"dopri5": (1e-9, 1e-11), "tsit5": (1e-9, 1e-11), "dopri8": (1e-9, 1e-11), "bosh3": (1e-5, 1e-7),
       "fehlberg2": (1e-5, 1e-7), "adaptive_heun": (1e-3, 1e-5)}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---- the log --------------------------------------------------------------------------------------------------------
class Log:
    def __init__(self):
        self.calls, self.marks = [], []
        self._tags, self._alive = {}, []

    def tag(self, x: torch.Tensor) -> str:
        key = (x.data_ptr(), x.dtype, tuple(x.shape))
        if key not in self._tags:
            self._alive.append(x)         # a tagged buffer is never freed: its address cannot come back as another tensor
            self._tags[key] = "{}{}#{}".format(str(x.dtype).replace("torch.", ""), list(x.shape), len(self._tags))
        return self._tags[key]

    def sig(self, v):
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v).hex()
        if isinstance(v, torch.Tensor):
            return self.tag(v)
        if isinstance(v, (list, tuple)):
            return [self.sig(x) for x in v]
        if isinstance(v, ctypes.Structure) and hasattr(v, "t0") and hasattr(v, "dt"):
            return ["ctrl", float(v.t0).hex(), float(v.dt).hex()]      # the per-step words of the device controller
        return type(v).__name__

    def add(self, name, args, kwargs):
        self.calls.append([name, [self.sig(a) for a in args], {k: self.sig(kwargs[k]) for k in sorted(kwargs)}])

    def digest(self) -> str:
        return _digest(self.calls)


class LoggedKernels:
    """Proxy of a kernels object: flags and underscore attributes pass through, every public method is logged."""

    def __init__(self, inner, log):
        self.__dict__["_inner"], self.__dict__["_log"] = inner, log

    def __getattr__(self, name):
        value = getattr(self._inner, name)          # (AttributeError for what the backend does not have: `hasattr` holds)
        if name.startswith("_") or not callable(value):
            return value
        log = self._log

        def logged(*args, **kwargs):
            log.add(name, args, kwargs)
            return value(*args, **kwargs)
        return logged

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def logged_backend(log, oracle):
    """`_native.get_kernels` answers with a logging proxy: of the CPU oracle (`oracle` True: the product's host logic as it
    runs on the HIP kernels) or of what it returns by itself for a CPU state (the torch-op host path)."""
    from torchdiffeq_amd import _fallback, _native
    from torchdiffeq_amd.solvers.adaptive import RKAdaptiveStepsizeODESolver as Solver
    orig_get, orig_step, warned = _native.get_kernels, Solver._trial_step, _fallback._warned
    proxies = {}

    def get_kernels(device, dtype=None):
        if oracle:
            from oracle.kernels import OracleKernels
            inner = proxies.get("oracle") or proxies.setdefault("oracle", OracleKernels())
        else:
            inner = orig_get(device, dtype)
        if id(inner) not in proxies:
            proxies[id(inner)] = LoggedKernels(inner, log)
        return proxies[id(inner)]

    def trial_step(self):
        log.marks.append(len(log.calls))
        return orig_step(self)
    _native.get_kernels, Solver._trial_step = get_kernels, trial_step
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            yield
    finally:
        _native.get_kernels, Solver._trial_step = orig_get, orig_step
        _fallback._warned = warned      # (the once-per-process HostPathWarning was swallowed above: not this run's to spend)


# ---- the problem ----------------------------------------------------------------------------------------------------
def _bytes_digest(*tensors) -> str:
    h = hashlib.sha256()
    for x in tensors:
        x = x.detach().contiguous()
        h.update(x.view(_INT_VIEW[x.element_size()]).numpy().tobytes())
    return h.hexdigest()


def _problem(dtype=torch.float64):
    g = torch.Generator().manual_seed(11)
    A = torch.randn(6, 6, generator=g, dtype=torch.float64)
    y0 = torch.randn(8, 6, generator=g, dtype=torch.float64)
    return A.to(dtype), y0.to(dtype), torch.tensor([0.0, 0.3, 0.7], dtype=torch.float64)


class Field(torch.nn.Module):
    """tanh(y A^T); counts its evaluations.  `param`: A is an nn.Parameter (func's output requires grad)."""

    def __init__(self, A, param=False, callbacks=None):
        super().__init__()
        self.A = torch.nn.Parameter(A) if param else A
        self.nfe = 0
        if callbacks is not None:
            self.callback_step = lambda t0, y, dt: callbacks.append(["s", float(t0).hex(), float(dt).hex()])
            self.callback_accept_step = lambda t0, y, dt: callbacks.append(["a", float(t0).hex(), float(dt).hex()])
            self.callback_reject_step = lambda t0, y, dt: callbacks.append(["r", float(t0).hex(), float(dt).hex()])

    def forward(self, t, y):
        self.nfe += 1
        if isinstance(y, tuple):
            return tuple(torch.tanh(torch.cat(y, dim=1) @ self.A.T).split([c.shape[1] for c in y], dim=1))
        return torch.tanh(y @ self.A.T)


def _solve(method, dtype=torch.float64, grad="no_grad", y0_grad=False, param=False, adjoint=False, tuple_state=False,
           reverse=False, callbacks=False, env=None, tol=None, **kw):
    """One regime -> (digest of the solution [and gradients], nfe, accept / reject record)."""
    import torchdiffeq_amd as tda
    from torchdiffeq_amd.solvers.adaptive import RKAdaptiveStepsizeODESolver as Solver
    A, y0, t = _problem(dtype)
    if reverse:
        t = t.flip(0)
    steps = [] if callbacks else None
    f = Field(A, param=param or adjoint, callbacks=steps)
    if y0_grad or adjoint:
        y0 = y0.requires_grad_(True)
    state = (y0[:, :4], y0[:, 4:] * 1.0) if tuple_state else y0
    rtol, atol = tol or TOL[method]
    solvers, orig = [], Solver.integrate

    def integrate(self, t_):
        solvers.append(self)
        return orig(self, t_)
    Solver.integrate = integrate
    outs, failed = (), None
    try:
        with _env(**{"TDEQ_CARRY": None, "TDEQ_LOOKAHEAD": None, **(env or {})}), \
                (torch.no_grad() if grad == "no_grad" else torch.enable_grad()):
            try:
                y = (tda.odeint_adjoint if adjoint else tda.odeint)(f, state, t, method=method, rtol=rtol, atol=atol, **kw)
                outs = tuple(y) if isinstance(y, tuple) else (y,)
                if adjoint:
                    outs[0][-1].pow(2).sum().backward()
                    outs = outs + (y0.grad, f.A.grad)
            except AssertionError as exc:
                failed = str(exc)
    finally:
        Solver.integrate = orig
    fwd = solvers[0]
    record = steps if callbacks else {"n_accepted": fwd.n_accepted, "n_rejected": fwd.n_rejected}
    return (_bytes_digest(*outs) if failed is None else None), f.nfe, record, failed


def _regimes():
    """name -> (oracle backend?, keyword arguments of `_solve`)."""
    r = {}
    for m in METHODS:
        for grad in ("no_grad", "grad_on"):
            for carry in ("0", "1"):
                r["{}/f64/{}/carry{}".format(m, grad, carry)] = (True, dict(method=m, grad=grad, env={"TDEQ_CARRY": carry}))
        r[m + "/f64/y0_requires_grad"] = (True, dict(method=m, grad="grad_on", y0_grad=True))
        for carry in ("0", "1"):
            r["{}/f64/parameter/carry{}".format(m, carry)] = (True, dict(method=m, grad="grad_on", param=True,
                                                                         env={"TDEQ_CARRY": carry}))
    for m in ("dopri5", "tsit5", "dopri8"):
        r[m + "/f32/no_grad"] = (True, dict(method=m, dtype=torch.float32, tol=(1e-6, 1e-8)))
    r["dopri5/user_norm"] = (True, dict(method="dopri5", options=dict(norm=lambda x: x.abs().max())))
    r["dopri5/tensor_rtol"] = (True, dict(method="dopri5", tol=(torch.full((8, 6), 1e-9, dtype=torch.float64), 1e-11)))
    r["dopri5/step_t_jump_t"] = (True, dict(method="dopri5", options=dict(step_t=torch.tensor([0.11, 0.52]),
                                                                         jump_t=torch.tensor([0.4]))))
    r["dopri5/callbacks"] = (True, dict(method="dopri5", callbacks=True))
    r["dopri5/lookahead0"] = (True, dict(method="dopri5", env={"TDEQ_LOOKAHEAD": "0"}))
    r["dopri5/reverse"] = (True, dict(method="dopri5", reverse=True))
    r["dopri5/tuple_state"] = (True, dict(method="dopri5", tuple_state=True))
    r["dopri5/max_num_steps"] = (True, dict(method="dopri5", options=dict(max_num_steps=3)))
    for m in ("dopri5", "tsit5"):
        r[m + "/adjoint"] = (True, dict(method=m, grad="grad_on", adjoint=True))
    for m in ("dopri5", "tsit5", "fehlberg2"):
        r[m + "/hostpath/f64"] = (False, dict(method=m))
    r["dopri5/hostpath/bf16"] = (False, dict(method="dopri5", dtype=torch.bfloat16, tol=(2e-3, 2e-4)))
    return r


REGIMES = _regimes()


def compact(call) -> str:
    """One logged call as a short line for the fixture: tensors by their number, a list of coefficients or times by a
    6-digit digest (the SHA-256 of the whole log covers every digit), scalars as they are."""
    def fmt(v):
        if isinstance(v, list):
            if v and all(isinstance(x, str) and x.lstrip("-").startswith("0x") for x in v):
                return "c" + hashlib.sha256(",".join(v).encode()).hexdigest()[:6]
            return "[" + ",".join(fmt(x) for x in v) + "]"
        if isinstance(v, str) and "#" in v:
            return v[v.index("#"):]
        return {None: "-", True: "T", False: "F"}.get(v, str(v)) if not isinstance(v, (int, float)) or isinstance(v, bool) \
            else str(v)
    name, args, kwargs = call
    return "{}({})".format(name, ",".join([fmt(a) for a in args] + ["{}={}".format(k, fmt(v)) for k, v in kwargs.items()]))


def _digest(calls) -> str:
    return hashlib.sha256(json.dumps(calls, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def run_regime(name):
    oracle, kw = REGIMES[name]
    log = Log()
    with logged_backend(log, oracle):
        digest, nfe, steps, failed = _solve(**kw)
    head = log.calls[:log.marks[2]] if len(log.marks) > 2 else log.calls
    return {"calls": len(log.calls), "trial_steps": len(log.marks), "sha256": log.digest(),
            "head": [compact(c) for c in head], "solution": digest and digest[:16], "nfe": nfe, "steps": steps,
            "failed": failed}


# ---- _GraphStep.body ------------------------------------------------------------------------------------------------
class _Plan:
    numels = [48]
    n_seg = 1


class BodyKernels:
    """Logging stand-in for the HIP kernels as a captured step sees them (no arithmetic).  `low`: the 16-bit route — no
    multi-output launch that reads the step size on the device, rows never split."""
    name = "launch-log"
    _LAUNCHES = ("stage_combine_dev", "stage_combine_multi", "stage_combine_multi_dev", "stage_combine_err",
                 "error_norm_ctrl", "error_norm_partial_ctrl", "error_norm_vec_ctrl")

    def __init__(self, log, low):
        self._log, self._low = log, low
        self.split_row_sums = not low
        self.norm_copies_last_stage = not low
        self.whole_row_controller = True      # (a pair without the end-of-step fusion, fehlberg2, gets its controller words too)

    def make_plan(self, segments, total, chunk, device):
        return _Plan()

    def __getattr__(self, name):
        if name not in self._LAUNCHES or (self._low and name in ("stage_combine_multi", "stage_combine_multi_dev")):
            raise AttributeError(name)
        return lambda *args, **kwargs: self._log.add(name, args, kwargs)


def run_body(method, side, low, carry):
    """The launches of one `_GraphStep.body(s, side)` of a solver built by its own constructor on the stand-in."""
    from torchdiffeq_amd import _native, solvers
    from torchdiffeq_amd._graph import _GraphStep
    from torchdiffeq_amd.misc import OdeFunc, StateLayout, rms_norm
    from torchdiffeq_amd.solvers.adaptive import RKAdaptiveStepsizeODESolver
    cls = next(c for c in vars(solvers).values() if isinstance(c, type) and issubclass(c, RKAdaptiveStepsizeODESolver)
               and getattr(c, "tableau", None) is not None and c.tableau.name == method)
    log = Log()
    fake, orig, empty_like = BodyKernels(log, low), _native.get_kernels, torch.empty_like
    _native.get_kernels = lambda device, dtype=None: fake
    try:
        with _env(TDEQ_CARRY=carry), torch.no_grad():
            y0 = torch.ones(8, 6, dtype=torch.float64)
            func = OdeFunc(lambda t, y: y * 0.5, StateLayout([y0.shape], False), 1.0, y0.dtype, y0.device)
            s = cls(func=func, y0=y0.reshape(-1), rtol=1e-6, atol=1e-8, norm=rms_norm, hip_graph=False)
            g = object.__new__(_GraphStep)
            flat = y0.reshape(-1)
            g.y, g.epart, g.f0 = [flat.clone(), flat.clone()], [flat.clone(), flat.clone()], flat.clone()
            g.tbuf = torch.zeros(len(s._beta), dtype=torch.float64)
            g.ts, g.k, g.vec_tol = g.tbuf.unbind(0), [[flat.clone()] * (len(s._beta) + 1), None], None
            for x in (*g.y, *g.epart, g.f0, g.k[0][-1], g.tbuf):      # the static buffers first: stable, readable tags
                log.tag(x)
            g.f0.fill_(7.0)
            torch.empty_like = torch.zeros_like       # (no uninitialised memory in the evaluations: `f0` below is decidable)
            g.body(s, side)
            assert g.k[side] is not None and len(g.k[side]) == len(s._beta) + 1
            # side 1 hands its last evaluation to side 0's buffer: by the norm launch (`copy_last_to`) or by a copy of its own
            log.calls.append(["f0.copy_", [bool((g.f0 != 7.0).any())], {}])
    finally:
        _native.get_kernels, torch.empty_like = orig, empty_like
    return log.calls


def body_cases():
    return ["{}/side{}/{}/carry{}".format(m, side, "low" if low else "f64", carry) for m in METHODS for side in (0, 1)
            for low, carry in ((False, "0"), (False, "1"), (True, "1"))]


def run_body_case(case):
    m, side, kind, carry = case.split("/")
    calls = run_body(m, int(side[-1]), kind == "low", carry[-1])
    return {"sha256": _digest(calls), "log": [compact(c) for c in calls]}


def record():
    out = {"solves": {}, "graph_body": {}}
    for name in REGIMES:
        rec = out["solves"][name] = run_regime(name)
        n_rej = rec["steps"]["n_rejected"] if isinstance(rec["steps"], dict) else sum(1 for s in rec["steps"] if s[0] == "r")
        print("{:40s} {:5d} calls {:4d} trial steps ({} rejected) nfe {}".format(name, rec["calls"], rec["trial_steps"],
                                                                              n_rej, rec["nfe"]))
        if name != "dopri5/max_num_steps":
            assert 4 <= rec["trial_steps"] <= 200, (name, rec["trial_steps"])
    assert any(isinstance(r["steps"], dict) and r["steps"]["n_rejected"] > 0 for n, r in out["solves"].items()
               if n.startswith("dopri5/")), "no dopri5 regime with a rejected step"
    for case in body_cases():
        out["graph_body"][case] = run_body_case(case)
    return out


def dump(data, path):
    """Explicit logs that several cases share (grad mode on with nothing to record launches what `no_grad` does, ...) are
    kept once, in "logs", under the first 8 digits of their digest; one line per case."""
    logs = {}

    def key(lines):
        k = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:8]
        assert logs.setdefault(k, lines) == lines
        return k
    solves = {n: dict(r, head=key(r["head"])) for n, r in data["solves"].items()}
    bodies = {n: dict(r, log=key(r["log"])) for n, r in data["graph_body"].items()}
    row = lambda d: ",\n".join('  {}: {}'.format(json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in d.items())
    with open(path, "w") as f:
        f.write('{{\n "solves": {{\n{}\n }},\n "graph_body": {{\n{}\n }},\n "logs": {{\n{}\n }}\n}}\n'.format(
            row(solves), row(bodies), row(logs)))


def load(path=FIXTURE):
    """The fixture with every case's explicit log in place again."""
    with open(path) as f:
        data = json.load(f)
    logs = data.pop("logs")
    for r in data["solves"].values():
        r["head"] = logs[r["head"]]
    for r in data["graph_body"].values():
        r["log"] = logs[r["log"]]
    return data


if __name__ == "__main__":
    dump(record(), FIXTURE)
    load()
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
