"""`torchdiffeq_amd.autodiff.Ops` op by op against fp64 autograd of plain-torch twins (tests/_ops_twins.py).

Every elementwise kernel call of a differentiable `odeint` is ONE `_LinearOp` node with a hand-written backward; the
whole-solve gradient tests mix that calculus with the field's and with step selection, at one small size and one loss.
Here each `Ops` method is called directly — on the CPU oracle (fp32 / fp64), on the torch-op kernels (complex, 16-bit)
and on the HIP kernels (all six types) — and its forward bits, first-order and second-order gradients and the node's
mechanics are compared with `torch.autograd.grad` of the twin, a random `grad_output` standing for any loss.

Bounds.  With u the unit roundoff of the state's type (2^-53, 2^-24, 2^-11, 2^-8), S the absolute-value companion of
the compared quantity (the twin's module docstring) and gamma(c, u) = c u / (1 - c u):

  * gradient of a tensor input, per element: gamma(c, u) S + 32 * 2^-53 S.  c counts the rounded operations between the
    T-rounded scalars and the stored gradient, read from autodiff.py / _fallback.py / csrc/tdeq_kernels.hpp:
      - `scale_many` rounds the weight to T and the product w g once each;
      - a weight Ops forms in double from T-rounded scalars (fixed_stage, rk4_stage, lerp, dense_eval) is exact to
        2^-53 S there, so c = 2;
      - combine's weight T(T(c) T(dt)) is one rounding of the twin's exact product, already of type T: c = 2;
      - weighted_sum's weights are the twin's own constants: c = 1 (c = 2 where one tensor enters twice: two products,
        one addition of the two gradients);
      - adams_predict differentiated through (y, dy, delta) at once: c = 3 (g_y + g_dy, then T(cb_j) times that; T(dt)
        g_delta, then T(cm_j) times that; the sum of both); adams_correct: c = 2 (g_y + g_dy, times T(c));
      - Hermite: the basis values are formed on the host IN T (events.py): at most 5 roundings per weight, each
        relative to a sub-expression the companion dominates, plus the product: c = 6.
    32 * 2^-53 S covers the twin's own fp64 evaluation (a few dozen operations at most) and Ops' double arithmetic.
  * gradient of a scalar shadow: (N + 1 + 64) 2^-53 S with N the number of real elements of a dot: `tdeq_multi_dot`,
    the oracle and `_fallback.real_dot` (which the 16-bit kernels inherit) all accumulate in fp64 — the bound of
    test_row_multi_dot per dot, combined through |dw|, which is what the companion's gradient is.  64 covers dw formed
    in double, the sum over the terms and the twin's own sums.
  * second order (`_backward_with_graph` is torch ops in the state's type): tensors gamma(c2, u) S + 32 * 2^-53 S with
    c2 = c + 4 + 2 M (1 + n_scalars) (every one of the M inputs contributes one rounded product and one rounded addition
    per scalar and for g); scalars additionally N u_acc S for the sum over the elements that ATen's backward of
    `g * w` forms in the state's type — accumulated in that type for fp32 / fp64 and in float32 for the 16-bit types
    (ATen's accumulation type), any summation order.
  * every rounded operation of a T-valued result adds half the type's smallest subnormal (gradual underflow).
  * scalar gradients whose dw table or saved inputs are themselves T-rounded carry c_dw u S more (`Case.c_dw`): Hermite's
    d/d(dt) weights are the T-rounded h10, h11 (4 roundings); adams_predict's delta = T(dt) sm saves the RECORDED sm, a
    T-rounded sum of `order` products (2 order - 1 roundings), and autograd adds g_y + g_dy in T before the dots (1);
    adams_correct: that addition only (1).

Found by this file: `Ops.fixed_stage` and `Ops.rk4_stage` rounded the weights that the reference writes as SECOND operands
(`k * w`, `* _one_third`, the increment's `* dt`) to the state's type, where the 16-bit kernels and the torch-op path
take them at float32 (`_scalars.operand`).  The dt gradient of a bf16 fixed_stage was off by 2^-9 relative, 10^11 times
its bound (tensor gradients stayed inside theirs by luck of c).  Both now use `operand`; fp32 / fp64 / complex weights
are the same numbers as before.  test_first_order[*-bf16-fixed_stage*] and [*-f16-fixed_stage*] are the regression
tests; the rk4 stages run for the complex and 16-bit backends too for that reason.

Non-contiguous tensor INPUTS are out of scope: the kernels read data pointers and every caller of `Ops` hands them
contiguous tensors.  A non-contiguous `grad_output` is in scope (autograd produces expanded ones) and is tested.

The fused `tdeq_adams_predict` takes at most TDEQ_MAX_TERMS = 14 history terms, so the "same bits" claim is checked
against it for histories of 1, 8, 9 and 14; the recorded path alone goes further (`_long_sum`'s third link): histories
of 15 and 22 are checked bit for bit against the same chain of no-grad `weighted_sum` calls, and their gradients
against the twin.
"""
from __future__ import annotations

import functools
import types
import warnings
import zlib
from typing import Callable, Dict, Optional, Sequence, Tuple

import pytest
import torch

import _ops_twins as tw
from torchdiffeq_amd import _fallback, _native
from torchdiffeq_amd._scalars import operand, scalar_type
from torchdiffeq_amd.autodiff import Ops
from torchdiffeq_amd.solvers._common import _NO_SHADOW, _StepShadow
from torchdiffeq_amd.solvers.events import FixedGridEvents

F32, F64, C64, C128, BF16, F16 = (torch.float32, torch.float64, torch.complex64, torch.complex128, torch.bfloat16,
                                  torch.float16)
UNIT = {F64: 2.0 ** -53, C128: 2.0 ** -53, F32: 2.0 ** -24, C64: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
U_ACC = {F64: 2.0 ** -53, C128: 2.0 ** -53, F32: 2.0 ** -24, C64: 2.0 ** -24, F16: 2.0 ** -24, BF16: 2.0 ** -24}
U64 = 2.0 ** -53
# gradual underflow: a rounded result below the smallest normal number carries an ABSOLUTE error of half the smallest
# subnormal (fp16 gradients of small weights get there: 2.7e-3 * 1e-2 < 6.1e-5)
ETA = {F64: 0.0, C128: 0.0, F32: 2.0 ** -150, C64: 2.0 ** -150, F16: 2.0 ** -25, BF16: 2.0 ** -134}
NAMES = {F32: "f32", F64: "f64", C64: "c64", C128: "c128", BF16: "bf16", F16: "f16"}
N_ODD = 4099                 # odd, beyond one vector width and one block
N_BIG = (1 << 20) + 3        # `tdeq_multi_dot` reduces over many blocks


def gamma(c: int, u: float) -> float:
    return c * u / (1 - c * u)


# -- backends ------------------------------------------------------------------------------------------------------------
def _b(kind, dtype):
    return pytest.param((kind, dtype), id=f"{kind}-{NAMES[dtype]}", marks=[pytest.mark.gpu] if kind == "hip" else [])


REAL = [_b("oracle", F32), _b("oracle", F64), _b("hip", F32), _b("hip", F64)]
OTHER = [_b("host", C64), _b("host", C128), _b("host", BF16), _b("host", F16),
         _b("hip", C64), _b("hip", C128), _b("hip", BF16), _b("hip", F16)]
ALL = REAL + OTHER


class Backend:
    def __init__(self, kind, dtype, kernels, device):
        self.kind, self.dtype, self.device = kind, dtype, device
        self.ops = Ops(kernels, scalar_type(dtype))
        self.wide = torch.complex128 if dtype.is_complex else torch.float64


@pytest.fixture()
def be(request, monkeypatch):
    kind, dtype = request.param
    if kind == "oracle":
        from oracle.kernels import OracleKernels
        yield Backend(kind, dtype, OracleKernels(), torch.device("cpu"))
    elif kind == "host":
        cls = _fallback.LowPrecisionHostKernels if dtype in (BF16, F16) else _fallback.HostKernels
        yield Backend(kind, dtype, cls(), torch.device("cpu"))
    else:
        monkeypatch.setattr(_fallback, "_warned", False)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", category=_fallback.HostPathWarning)
            device = torch.device("cuda")
            yield Backend(kind, dtype, _native.get_kernels(device, dtype), device)


# -- cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """One call of an `Ops` method: input values (CPU, state dtype), the scalars that can carry a shadow (name -> the
    T-rounded value the kernel uses), `run(ops, X, sh, out=None)` and `twin(X, s, S)` -> tuples of outputs."""

    def __init__(self, key, tensors, scalars, run, twin, c, none=(), n_out=1, c_dw=0, extra=None):
        self.key, self.tensors, self.scalars, self.run, self.twin, self.c = key, tensors, scalars, run, twin, c
        self.c_dw = c_dw                  # T-roundings in the dw table (scalar gradients): 0 unless dw is built from T values
        self.extra = extra
        self.none = frozenset(none)       # inputs whose weight is exactly 0: no gradient from the node
        self.n_out = n_out
        self.dtype = next(iter(tensors.values())).dtype
        self.n = next(iter(tensors.values())).numel()
        self.census = None


def _draw(gen, n, dtype, scale=1.0):
    v = torch.randn(n, generator=gen, dtype=torch.float64) * scale
    if dtype.is_complex:
        v = torch.complex(v, torch.randn(n, generator=gen, dtype=torch.float64) * scale)
    return v.to(dtype)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()))


def _T(dtype):
    T = scalar_type(dtype)
    return lambda v: float(T(v))


_COEFS13 = (0.0371, -0.211, 0.5, 1.25, -0.0625, 0.33, -0.7071, 0.1234, 0.9, -0.45, 0.271828, -0.314159, 0.05)


def _combine(dtype, n, nk):
    gen, T = _gen("combine", dtype, n, nk), _T(dtype)
    coefs, dt = list(_COEFS13[:nk]), 0.0731
    X = {"y0": _draw(gen, n, dtype)}
    X.update({f"k{j}": _draw(gen, n, dtype, 1.0 + 0.5 * j) for j in range(nk)})
    ks = lambda Z: [Z[f"k{j}"] for j in range(nk)]
    cT = [T(c) for c in coefs]
    return Case(("combine", dtype, n, nk), X, {"dt": T(dt)},
                lambda ops, Z, sh, out=None: (ops.combine(Z["y0"], ks(Z), coefs, dt, sh["dt"], out=out),),
                lambda Z, s, S: (tw.combine(Z["y0"], ks(Z), cT, s["dt"], S),), c=2)


def _fixed_stage(dtype, n, mode, ws=(0.2113, -0.6431, 0.4477), dt=0.0731):
    gen = _gen("fixed", dtype, n, mode)
    ws = list(ws[:1] if mode == 1 else ws)
    X = {"y0": _draw(gen, n, dtype)}
    X.update({f"k{j}": _draw(gen, n, dtype, 1.0 + j) for j in range(len(ws))})
    ks = lambda Z: [Z[f"k{j}"] for j in range(len(ws))]
    T = scalar_type(dtype)
    wk = [operand(T, w) for w in ws]          # the weights as the kernels take them (second operands)
    return Case(("fixed_stage", dtype, n, mode, tuple(ws), dt), X, {"dt": float(T(dt))},
                lambda ops, Z, sh, out=None: (ops.fixed_stage(mode, Z["y0"], ks(Z), ws, dt, sh["dt"], out=out),),
                lambda Z, s, S: (tw.fixed_stage(mode, Z["y0"], ks(Z), wk, s["dt"], S),), c=2)


def _rk4(dtype, n, stage):
    gen, T = _gen("rk4", dtype, n, stage), scalar_type(dtype)
    dt = 0.0731
    X = {name: _draw(gen, n, dtype) for name in ("y0", "k1", "k2", "k3", "k4")}
    # 1/3 and the increment's dt are second operands of the reference's expressions, dt elsewhere a first operand
    third, dt_used = operand(T, 1.0 / 3.0), (operand(T, dt) if stage == 4 else float(T(dt)))
    return Case(("rk4", dtype, n, stage), X, {"dt": dt_used},
                lambda ops, Z, sh, out=None: (ops.rk4_stage(stage, Z["y0"], Z["k1"], Z["k2"], Z["k3"], Z["k4"], dt, sh["dt"],
                                                            out=out),),
                lambda Z, s, S: (tw.rk4_stage(stage, Z["y0"], Z["k1"], Z["k2"], Z["k3"], Z["k4"], s["dt"], third, S),), c=2)


def _lerp(dtype, n):
    gen, T = _gen("lerp", dtype, n), _T(dtype)
    slope = 0.3717
    X = {"y0": _draw(gen, n, dtype), "y1": _draw(gen, n, dtype, 2.0)}
    return Case(("lerp", dtype, n), X, {"slope": T(slope)},
                lambda ops, Z, sh, out=None: (ops.lerp(Z["y0"], Z["y1"], slope, sh["slope"], out=out),),
                lambda Z, s, S: (tw.lerp(Z["y0"], Z["y1"], s["slope"], S),), c=2)


def _weighted_sum(dtype, n):
    """Weights a s, b s (products exact in every type), a constant, exactly 1 and exactly 0."""
    gen, T = _gen("wsum", dtype, n), _T(dtype)
    s0, a, b, const = 0.375, 0.75, -1.25, T(0.3)
    X = {name: _draw(gen, n, dtype) for name in "abcde"}
    xs = lambda Z: [Z[name] for name in "abcde"]
    ws = [a * s0, b * s0, const, 1.0, 0.0]
    return Case(("weighted_sum", dtype, n), X, {"s": s0},
                lambda ops, Z, sh, out=None: (ops.weighted_sum(xs(Z), ws, [(sh["s"], [a, b, 0.0, 0.0, 0.0])], out=out),),
                lambda Z, s, S: (tw.weighted_sum(xs(Z), [a * s["s"], (abs(b) if S else b) * s["s"], const, 1.0, 0.0]),),
                c=1, none=("e",))


def _twice(dtype, n):
    gen, T = _gen("twice", dtype, n), _T(dtype)
    X = {"a": _draw(gen, n, dtype), "b": _draw(gen, n, dtype)}
    ws = [T(0.3), T(-0.7), T(0.55)]
    return Case(("twice", dtype, n), X, {},
                lambda ops, Z, sh, out=None: (ops.weighted_sum([Z["a"], Z["b"], Z["a"]], ws, out=out),),
                lambda Z, s, S: (tw.weighted_sum([Z["a"], Z["b"], Z["a"]], [abs(w) if S else w for w in ws]),), c=2)


_MID13 = (0.0431, -0.0217, 0.1093, 0.0871, -0.1312, 0.0659, 0.2113, -0.0933, 0.0127, 0.1571, -0.0389, 0.0743, 0.0299)


def _dense(dtype, n, shape, x=0.3717):
    """shape: "dopri5" (7 stages, k_1 without mid weight -> unused, f0 / f1 carry one: merged slots), "plain" (f0 / f1
    carry none), "dopri8" (13 stages, all with a mid weight: 15 inputs)."""
    n_k, mid_idx = {"dopri5": (7, [0, 2, 3, 4, 5, 6]), "plain": (5, [1, 2, 3]), "dopri8": (13, list(range(13)))}[shape]
    gen, T = _gen("dense", dtype, n, shape), _T(dtype)
    mid, dt = list(_MID13[:len(mid_idx)]), 0.0731
    X = {"y0": _draw(gen, n, dtype), "y1": _draw(gen, n, dtype)}
    X.update({f"k{j}": _draw(gen, n, dtype, 1.0 + 0.25 * j) for j in range(n_k)})
    ks = lambda Z: [Z[f"k{j}"] for j in range(n_k)]
    midT = [T(c) for c in mid]
    return Case(("dense", dtype, n, shape, x), X, {"dt": T(dt), "x": T(x)},
                lambda ops, Z, sh, out=None: (ops.dense_eval(Z["y0"], Z["y1"], ks(Z), mid_idx, mid, dt, x, sh["dt"], sh["x"],
                                                             out=out),),
                lambda Z, s, S: (tw.dense_eval(Z["y0"], Z["y1"], ks(Z), mid_idx, midT, s["dt"], s["x"], S),), c=2,
                none=[name for name in X if name != "y0"] if x == 0.0 else ())     # at x = 0 the output IS y0


def _grid(gen, m, bits=12):
    """m coefficients on a 2^-bits grid: their products with dt = 0.375 are exact in fp32."""
    return [float(v) / 2 ** bits for v in torch.randint(-2 ** bits + 1, 2 ** bits, (m,), generator=gen)]


def _adams_predict(dtype, n, order, implicit=True):
    gen = _gen("adams", dtype, n, order, implicit)
    dt = 0.375
    bash, moulton = _grid(gen, order), (_grid(gen, order) if implicit else None)
    cb = [b * dt for b in bash]
    X = {"y0": _draw(gen, n, dtype)}
    X.update({f"f{j}": _draw(gen, n, dtype, 1.0 + 0.1 * j) for j in range(order)})
    hist = lambda Z: [Z[f"f{j}"] for j in range(order)]
    some = lambda outs: tuple(o for o in outs if o is not None)
    return Case(("adams_predict", dtype, n, order, implicit), X, {"dt": dt},
                lambda ops, Z, sh, out=None: some(ops.adams_predict(Z["y0"], hist(Z), cb, moulton, dt, sh["dt"], db=bash,
                                                                    out=out)),
                lambda Z, s, S: some(tw.adams_predict(Z["y0"], hist(Z), bash, moulton, s["dt"], S)), c=3,
                n_out=3 if implicit else 1, c_dw=2 * order, extra=dict(bash=bash, moulton=moulton, dt=dt))


def _adams_correct(dtype, n):
    gen = _gen("correct", dtype, n)
    dt, m0 = 0.375, _grid(gen, 1)[0]
    c = m0 * dt
    X = {name: _draw(gen, n, dtype) for name in ("y0", "f", "delta")}
    dy = c * X["f"].double() + X["delta"].double()
    # half the elements within the corrector's tolerance of the new dy, half outside it: a census that is neither 0 nor n
    X["dy_old"] = (dy * (1 + 2e-3 * torch.randn(n, generator=gen, dtype=torch.float64))).to(dtype)
    case = Case(("adams_correct", dtype, n), X, {"dt": dt}, None,
                lambda Z, s, S: tw.adams_correct(Z["y0"], Z["f"], Z["delta"], m0, s["dt"], S), c=2, n_out=2, c_dw=1)

    def run(ops, Z, sh, out=None):
        dev = Z["y0"].device
        plan = ops.k.make_plan([(0, n, 1e-3, 1e-6)], n, _native.pick_chunk(n), dev)
        res = ops.adams_correct(plan, Z["y0"], Z["f"], Z["delta"], Z["dy_old"], c, sh["dt"], m0)
        case.census = list(ops.k.read_norms(plan)[0])
        return res
    case.run = run
    return case


def _hermite(dtype, n, sign):
    """t0, t1 and t such that h = 2741 / 8192 and dt = 1/2 are exact in fp32: the op and the twin are the same function."""
    gen = _gen("hermite", dtype, n, sign)
    T = scalar_type(dtype)
    t0, t1 = 0.25, 0.75
    t = t0 + 0.5 * 2741 / 8192
    X = {name: _draw(gen, n, dtype) for name in ("y0", "f0", "y1", "f1")}

    def run(ops, Z, sh, out=None):
        holder = types.SimpleNamespace(ops=ops, func=types.SimpleNamespace(sign=sign))
        if sh["t0"] is None and sh["t1"] is None and sh["t"] is None:
            step = _NO_SHADOW
        else:
            const = lambda v: torch.tensor(v, dtype=torch.float64, device=Z["y0"].device)
            step = _StepShadow(const(t0) if sh["t0"] is None else sh["t0"], const(t1) if sh["t1"] is None else sh["t1"],
                               sign)
        return (FixedGridEvents._cubic_hermite_interp(holder, T, T(t0), Z["y0"], Z["f0"], T(t1), Z["y1"], Z["f1"], T(t),
                                                      step, sh["t"], out=out),)
    return Case(("hermite", dtype, n, sign), X, {"t0": t0, "t1": t1, "t": t}, run,
                lambda Z, s, S: (tw.hermite(s["t0"], s["t1"], s["t"], Z["y0"], Z["f0"], Z["y1"], Z["f1"], sign, S),), c=6,
                c_dw=4)


_BUILDERS: Dict[str, Callable] = {
    "combine6": lambda d, n: _combine(d, n, 6),
    "combine13": lambda d, n: _combine(d, n, 13),
    "fixed_stage0": lambda d, n: _fixed_stage(d, n, 0),
    "fixed_stage1": lambda d, n: _fixed_stage(d, n, 1),
    "lerp": _lerp,
    "weighted_sum": _weighted_sum,
    "dense_dopri5": lambda d, n: _dense(d, n, "dopri5"),
    "dense_plain": lambda d, n: _dense(d, n, "plain"),
    "dense_dopri8": lambda d, n: _dense(d, n, "dopri8"),
    "rk4_1": lambda d, n: _rk4(d, n, 1),
    "rk4_2": lambda d, n: _rk4(d, n, 2),
    "rk4_3": lambda d, n: _rk4(d, n, 3),
    "rk4_4": lambda d, n: _rk4(d, n, 4),
    "adams_explicit3": lambda d, n: _adams_predict(d, n, 3, implicit=False),
    "adams_predict1": lambda d, n: _adams_predict(d, n, 1),
    "adams_predict8": lambda d, n: _adams_predict(d, n, 8),
    "adams_predict9": lambda d, n: _adams_predict(d, n, 9),
    "adams_predict14": lambda d, n: _adams_predict(d, n, 14),
    "adams_predict15": lambda d, n: _adams_predict(d, n, 15),
    "adams_predict22": lambda d, n: _adams_predict(d, n, 22),
    "adams_correct": _adams_correct,
    "hermite+": lambda d, n: _hermite(d, n, 1.0),
    "hermite-": lambda d, n: _hermite(d, n, -1.0),
    "twice": _twice,
    "dense_at_start": lambda d, n: _dense(d, n, "dopri5", x=0.0),
    # w = 1 + 0.99 * 2^-24 rounds to 1 in fp32 and dt's significand is just above 1.0101 (test_fixed_stage_weight_...)
    "fixed_stage1_rounding": lambda d, n: _fixed_stage(d, n, 1, ws=(1.0 + 0.99 * 2.0 ** -24,), dt=1.0102 / 16),
}
FIVE = ["combine6", "combine13", "fixed_stage0", "fixed_stage1", "lerp", "weighted_sum", "dense_dopri5", "dense_plain",
        "dense_dopri8"]
RK4 = ["rk4_1", "rk4_2", "rk4_3", "rk4_4"]       # (beyond the five: their scalars are operands of both kinds in 16 bits)
REAL_ONLY = ["adams_explicit3", "adams_predict1", "adams_predict8", "adams_predict9",
             "adams_predict14", "adams_predict15", "adams_predict22", "adams_correct", "hermite+", "hermite-"]
BEYOND_FUSED = ("adams_predict15", "adams_predict22")     # more history terms than tdeq_adams_predict takes


@functools.lru_cache(maxsize=None)
def case_of(name: str, dtype, n: int) -> Case:
    return _BUILDERS[name](dtype, n)


def _matrix(names_all, names_real):
    """(backend, case) pairs: the five shared ops for every backend, the rest for the real fp32 / fp64 backends."""
    out = []
    for b in ALL:
        for name in names_all:
            out.append(pytest.param(b.values[0], name, id=f"{b.id}-{name}", marks=b.marks))
    for b in REAL:
        for name in names_real:
            out.append(pytest.param(b.values[0], name, id=f"{b.id}-{name}", marks=b.marks))
    return out


# -- leaves, references, comparison --------------------------------------------------------------------------------------
def _leaves(case: Case, be: Backend, active: Sequence[str], offset_view=False, grad=True):
    X = {}
    for name, v in case.tensors.items():
        if offset_view:      # the tensor starts one element into a larger buffer: its base pointer is not vector-aligned
            buf = torch.zeros(case.n + 1, dtype=v.dtype, device=be.device)
            buf[1:].copy_(v)
            x = buf[1:].detach()
            assert x.storage_offset() == 1 and x.is_contiguous()
        else:
            x = v.to(be.device)
        X[name] = x.requires_grad_(grad)
    sh = {name: (torch.tensor(val, dtype=torch.float64, device=be.device, requires_grad=True) if name in active else None)
          for name, val in case.scalars.items()}
    return X, sh


def _contract(grads, vs, wide):
    """sum_i Re<v_i, grad_i> in the wide type."""
    total = None
    for gr, v in zip(grads, vs):
        if gr is None:
            continue
        term = (v.conj() * gr.to(wide)).real.sum() if wide.is_complex else (v * gr.to(wide)).sum()
        total = term if total is None else total + term
    return total


@functools.lru_cache(maxsize=None)
def _reference(name: str, dtype, n: int, active: Tuple[str, ...], order: int, const_g: bool = False):
    """The twin's gradients and their companions, computed once on the CPU and shared by every backend.
    order 1: d<g, out>/d(inputs).  order 2: first-order gradients with create_graph, contracted with fixed vectors `vs`,
    differentiated wrt (inputs, g)."""
    case = case_of(name, dtype, n)
    wide = torch.complex128 if dtype.is_complex else torch.float64
    gen = _gen("ref", name, dtype, n, active, order)
    if const_g:
        gs = [torch.full((n,), 0.7311 + 0.1 * i, dtype=torch.float64).to(dtype) for i in range(case.n_out)]
    else:
        gs = [_draw(gen, n, dtype) for _ in range(case.n_out)]
    vs = [_draw(gen, n, dtype) for _ in case.tensors] + \
         [torch.tensor(float(b), dtype=torch.float64) for b in (0.6180, -1.4142, 0.5772)[:len(active)]]

    def run(S: bool):
        mod = (lambda t: t.abs()) if S else (lambda t: t)      # (the modulus of a complex tensor is real)
        kind = torch.float64 if S else wide
        X = {k: mod(v.to(wide)).requires_grad_() for k, v in case.tensors.items()}
        s = {k: torch.tensor(abs(val) if S else val, dtype=torch.float64, requires_grad=k in active)
             for k, val in case.scalars.items()}
        g = [mod(t.to(wide)).requires_grad_(order == 2) for t in gs]
        inputs = list(X.values()) + [s[a] for a in active]
        outs = case.twin(X, s, S)
        g1 = torch.autograd.grad(outs, inputs, g, allow_unused=True, create_graph=order == 2)
        if order == 1:
            return list(g1)
        F = _contract(g1, [mod(v.to(wide) if v.dim() else v) for v in vs], kind)
        return list(torch.autograd.grad(F, inputs + g, allow_unused=True))
    names = list(case.tensors) + list(active) + ([f"g{i}" for i in range(case.n_out)] if order == 2 else [])
    return types.SimpleNamespace(gs=gs, vs=vs, names=names, ref=run(False), S=run(True))


def _compare(case: Case, be: Backend, label: str, names, got, ref, S, c: int, second: bool, strict_none=True) -> float:
    u, n_real = UNIT[case.dtype], case.n * (2 if case.dtype.is_complex else 1)
    worst = 0.0
    for name, a, r, s in zip(names, got, ref, S):
        if name in case.none and not second:
            assert a is None, f"{label}: {name} has weight 0 and must get no gradient"
            assert r is None or not bool(r.any())
            continue
        if a is None or r is None:
            if strict_none:
                assert a is None and r is None, f"{label}: {name}: op gives {type(a).__name__}, twin {type(r).__name__}"
            else:       # second order: autograd may hand back None for an all-zero gradient
                assert (a is None or not bool(a.any())) and (r is None or not bool(r.any())), f"{label}: {name}"
            continue
        is_scalar = r.dim() == 0
        if not is_scalar:
            assert a.dtype == case.dtype and a.shape == r.shape, f"{label}: {name}: {a.dtype} {tuple(a.shape)}"
        err = a.detach().cpu().to(r.dtype) - r
        err = torch.view_as_real(err).abs().amax(-1) if err.is_complex() else err.abs()
        if is_scalar and not second:
            bound = ((n_real + 1 + 64) * U64 + case.c_dw * u) * s
        elif is_scalar:
            bound = (gamma(c + case.c_dw, u) + n_real * U_ACC[case.dtype] + (n_real + 64) * U64) * s \
                + (c + n_real) * ETA[case.dtype]
        else:
            bound = (gamma(c, u) + 32 * U64) * s + c * ETA[case.dtype]
        bad = err > bound
        ratio = float((err / bound.clamp_min(1e-300)).max())
        assert not bool(bad.any()), (f"{label}: {name}: error / bound = {ratio:.3g} (max error {float(err.max()):.3e}, "
                                     f"{int(bad.sum())} of {bad.numel()} over)")
        worst = max(worst, ratio)
    print(f"OPS_RATIO {be.kind} {NAMES[case.dtype]} {'second' if second else 'first'} {label} {worst:.3e}")
    return worst


def _g_on_device(g: torch.Tensor, be: Backend, layout: str) -> torch.Tensor:
    if layout == "expanded":                 # what `.sum()` hands back: one element, stride 0
        return g[0].to(be.device).expand(g.shape)
    if layout == "strided":
        buf = torch.zeros(2 * g.numel(), dtype=g.dtype, device=be.device)
        buf[::2] = g.to(be.device)
        return buf[::2]
    return g.to(be.device)


def check_first_order(be: Backend, name: str, n: int, active: Optional[Sequence[str]] = None, layout="dense",
                      offset_view=False):
    case = case_of(name, be.dtype, n)
    active = tuple(case.scalars) if active is None else tuple(active)
    R = _reference(name, be.dtype, n, active, 1, layout == "expanded")
    X, sh = _leaves(case, be, active, offset_view)
    outs = case.run(be.ops, X, sh)
    gs = [_g_on_device(g, be, layout) for g in R.gs]
    if layout != "dense":
        assert not gs[0].is_contiguous()
    inputs = list(X.values()) + [sh[a] for a in active]
    got = torch.autograd.grad(outs, inputs, gs, allow_unused=True)
    label = f"{name}[n={n},{','.join(active) or '-'},{layout}{',view' if offset_view else ''}]"
    _compare(case, be, label, R.names, got, R.ref, R.S, case.c, second=False)
    return case, X, gs, got


def check_second_order(be: Backend, name: str, n: int, active: Optional[Sequence[str]] = None):
    case = case_of(name, be.dtype, n)
    active = tuple(case.scalars) if active is None else tuple(active)
    R = _reference(name, be.dtype, n, active, 2)
    X, sh = _leaves(case, be, active)
    outs = case.run(be.ops, X, sh)
    gs = [g.to(be.device).requires_grad_() for g in R.gs]
    inputs = list(X.values()) + [sh[a] for a in active]
    g1 = torch.autograd.grad(outs, inputs, gs, allow_unused=True, create_graph=True)
    F = _contract(g1, [v.to(be.device).to(be.wide if v.dim() else torch.float64) for v in R.vs], be.wide)
    got = torch.autograd.grad(F, inputs + gs, allow_unused=True)
    c2 = case.c + 4 + 2 * len(case.tensors) * (1 + len(active))
    label = f"{name}[n={n},{','.join(active) or '-'}]"
    _compare(case, be, label, R.names, got, R.ref, R.S, c2, second=True, strict_none=False)


# -- 1. forward bits -----------------------------------------------------------------------------------------------------
def _long_sum_by_hand(ops, xs, ws):
    """`_long_sum`'s chain with no-grad calls: 8 terms, then the running sum with weight 1 and 7 more per link."""
    acc = ops.weighted_sum(xs[:8], ws[:8])
    lo = 8
    while lo < len(xs):
        acc = ops.weighted_sum([acc, *xs[lo:lo + 7]], [1.0, *ws[lo:lo + 7]])
        lo += 7
    return acc


@pytest.mark.parametrize("be,name", _matrix(FIVE + RK4, REAL_ONLY), indirect=["be"])
def test_forward_bits(be, name):
    """A recorded call returns the bits of the no-grad call — recorded because a tensor requires grad, and recorded
    because only a shadow does.  For adams_predict that is the docstring's "same bits" as the fused kernel (histories of
    1, 8, 9, 14), for 15 and 22 terms the bits of the hand-made chain; adams_correct also leaves the same census."""
    case = case_of(name, be.dtype, N_ODD)
    X, none = _leaves(case, be, (), grad=False)
    with torch.no_grad():
        if name in BEYOND_FUSED:
            hist = [X[k] for k in case.tensors if k != "y0"]
            bash, moulton, dt = case.extra["bash"], case.extra["moulton"], case.extra["dt"]
            dy = _long_sum_by_hand(be.ops, hist, [b * dt for b in bash])
            plain = (be.ops.weighted_sum([X["y0"], dy], [1.0, 1.0]), dy,
                     be.ops.weighted_sum([_long_sum_by_hand(be.ops, hist, moulton)], [dt]))
        else:
            plain = case.run(be.ops, X, none)
    census = case.census
    assert all(not o.requires_grad for o in plain)
    first_scalar = tuple(case.scalars)[:1]
    for what, active, grad in (("tensor", (), True), ("shadow", first_scalar, False)):
        if what == "shadow" and not first_scalar:
            continue
        Z, sh = _leaves(case, be, active, grad=grad)
        rec = case.run(be.ops, Z, sh)
        assert len(rec) == len(plain)
        for i, (a, b) in enumerate(zip(rec, plain)):
            assert a.requires_grad and a.grad_fn is not None, f"{name}: output {i} was not recorded ({what})"
            assert a.dtype == b.dtype and torch.equal(a.detach(), b), f"{name}: output {i} differs from the no-grad call ({what})"
        if census is not None:
            assert case.census == census and 0 < census[0] < case.n, (case.census, census)


# -- 2. first order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, N_ODD])
@pytest.mark.parametrize("be,name", _matrix(FIVE + RK4 + ["twice"], REAL_ONLY), indirect=["be"])
def test_first_order(be, name, n):
    """Gradients wrt every tensor input and every shadow for a random grad_output, against the twin (module docstring
    for the bounds); inputs the op does not use come back None from both."""
    case, X, gs, got = check_first_order(be, name, n)
    if name.startswith(("combine", "fixed_stage", "rk4", "adams")):
        # y0 enters every stage combine with weight exactly 1: its gradient IS grad_output (of the outputs it reaches)
        g_y0 = gs[0]
        assert torch.equal(got[0], g_y0), f"{name}: a weight of exactly 1 must pass grad_output through"


@pytest.mark.parametrize("active", [("dt",), ("x",), ()], ids=["dt", "x", "none"])
@pytest.mark.parametrize("be", ALL, indirect=True)
def test_first_order_dense_eval_some_shadows(be, active):
    """dense_eval with a shadow for one scalar and None for the other, and with none at all."""
    check_first_order(be, "dense_dopri5", N_ODD, active)


@pytest.mark.parametrize("active", [("t",), ("t0", "t1"), ("t1",), ()], ids=["t", "t0t1", "t1", "none"])
@pytest.mark.parametrize("be", REAL, indirect=True)
def test_first_order_hermite_some_shadows(be, active):
    check_first_order(be, "hermite-", N_ODD, active)


@pytest.mark.parametrize("be", REAL, indirect=True)
def test_shadow_of_another_dtype(be):
    """A float32 shadow (the time grid of an fp32 solve) gets a float32 0-dim gradient: the fp64 sum, rounded once."""
    case = case_of("lerp", be.dtype, N_ODD)
    R = _reference("lerp", be.dtype, N_ODD, ("slope",), 1)
    X, _ = _leaves(case, be, ())
    shadow = torch.tensor(case.scalars["slope"], dtype=torch.float32, device=be.device, requires_grad=True)
    (out,) = case.run(be.ops, X, {"slope": shadow})
    (got,) = torch.autograd.grad(out, [shadow], [R.gs[0].to(be.device)])
    ref, S = float(R.ref[-1]), float(R.S[-1])
    assert got.dtype == torch.float32 and got.shape == ()
    assert abs(float(got) - ref) <= (N_ODD + 1 + 64) * U64 * S + 2.0 ** -24 * abs(ref)


# -- 3. second order -----------------------------------------------------------------------------------------------------
SECOND_FIVE = ["combine6", "fixed_stage0", "fixed_stage1", "lerp", "weighted_sum", "dense_dopri5", "dense_plain"]
SECOND_REAL = RK4 + ["adams_predict9", "adams_predict22", "adams_correct", "hermite+",
               "hermite-"]


@pytest.mark.parametrize("be,name", _matrix(SECOND_FIVE, SECOND_REAL), indirect=["be"])
def test_second_order(be, name):
    """create_graph=True with a grad_output that requires grad; the first-order gradients contracted with fixed vectors
    and differentiated again wrt inputs, shadows and grad_output.  dense_eval and Hermite go through `w_fn` (weights
    non-linear in their scalars), every other op through the constant-dw branch of `_backward_with_graph`."""
    check_second_order(be, name, N_ODD)


@pytest.mark.parametrize("active", [("dt",), ("x",)], ids=["dt", "x"])
@pytest.mark.parametrize("be", ALL, indirect=True)
def test_second_order_dense_eval_one_shadow(be, active):
    check_second_order(be, "dense_dopri5", N_ODD, active)


@pytest.mark.parametrize("active", [("t",), ("t0", "t1")], ids=["t", "t0t1"])
@pytest.mark.parametrize("be", REAL, indirect=True)
def test_second_order_hermite_some_shadows(be, active):
    check_second_order(be, "hermite+", N_ODD, active)


@pytest.mark.parametrize("be", REAL, indirect=True)
def test_second_order_single_element(be):
    check_second_order(be, "dense_dopri5", 1)
    check_second_order(be, "hermite-", 1)


# -- 4. node mechanics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", ALL, indirect=True)
def test_weights_of_exactly_one_and_zero(be):
    """weighted_sum with weights (.., 1.0, 0.0): 1.0 returns grad_output itself, 0.0 no gradient at all; dense_eval at
    x = 0 (the step's start): y1's weight is exactly 0."""
    case, X, gs, got = check_first_order(be, "weighted_sum", N_ODD)
    names = list(case.tensors)
    assert torch.equal(got[names.index("d")], gs[0])
    assert got[names.index("e")] is None
    for active in ((), ("dt", "x")):
        case, X, gs, got = check_first_order(be, "dense_at_start", N_ODD, active)
        assert all(g_ is None for g_ in got[1:len(case.tensors)])
        assert torch.equal(got[0], gs[0])       # y0's weight at x = 0 is exactly 1


@pytest.mark.parametrize("be", ALL, indirect=True)
def test_same_tensor_twice(be):
    """One tensor as two terms of a weighted_sum: autograd adds the two gradients of the node."""
    check_first_order(be, "twice", N_ODD)


@pytest.mark.parametrize("be,name", _matrix(["combine6", "fixed_stage0", "lerp", "weighted_sum", "dense_dopri5"],
                                            ["rk4_3", "hermite+"]), indirect=["be"])
def test_recorded_call_ignores_out(be, name):
    """`out=` is for no-grad calls: a recorded call returns a fresh tensor and leaves the buffer alone."""
    case = case_of(name, be.dtype, N_ODD)
    X, sh = _leaves(case, be, ())
    sentinel = torch.full((case.n,), 7.0, dtype=be.dtype, device=be.device)
    (res,) = case.run(be.ops, X, sh, out=sentinel)
    assert res.data_ptr() != sentinel.data_ptr() and res.requires_grad
    assert bool((sentinel == 7.0).all()), f"{name}: a recorded call wrote into out="
    with torch.no_grad():       # ... and the no-grad call does write there, the same bits
        Z, none = _leaves(case, be, (), grad=False)
        (plain,) = case.run(be.ops, Z, none, out=sentinel)
    assert plain.data_ptr() == sentinel.data_ptr() and torch.equal(plain, res.detach())


@pytest.mark.parametrize("layout", ["expanded", "strided"])
@pytest.mark.parametrize("be,name", _matrix(["combine6", "dense_dopri8", "weighted_sum"], ["adams_predict9", "hermite-"]),
                         indirect=["be"])
def test_grad_output_layouts(be, name, layout):
    """grad_output expanded from one element (stride 0: what `.sum()` produces) and as a stride-2 slice."""
    check_first_order(be, name, N_ODD, layout=layout)


@pytest.mark.parametrize("be,name", _matrix(["combine6", "fixed_stage0", "lerp", "weighted_sum", "dense_dopri8"],
                                            ["rk4_4", "adams_predict9", "adams_correct", "hermite+"]), indirect=["be"])
def test_inputs_one_element_into_a_buffer(be, name):
    """Every input is an offset-by-one view of a larger buffer: contiguous, but its base pointer is not aligned for
    vector loads (forward kernel, scale_many's g and multi_dot's x)."""
    check_first_order(be, name, N_ODD, offset_view=True)


@pytest.mark.parametrize("be", [_b("oracle", F32), _b("hip", F32)], indirect=True)
def test_fixed_stage_weight_is_the_rounded_one(be):
    """fixed_stage, mode 1, fp32: the gradient's weight is T(dt) * T(w), not T(dt) * w.  w = 1 + 0.99 * 2^-24 rounds
    to 1 (relative error 0.99 u) and dt's significand is just above 1.0101, so T(dt * w) is one ulp above T(dt) — an
    error of up to 1.98 u in the weight, 2.98 u with the product's rounding, against a bound of c = 2."""
    check_first_order(be, "fixed_stage1_rounding", N_ODD)


# -- 5. sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["combine6", "dense_dopri8"])
@pytest.mark.parametrize("be", ALL, indirect=True)
def test_first_order_many_blocks(be, name):
    """2^20 + 3 elements: `tdeq_multi_dot` reduces over many blocks, `tdeq_scale_many` runs a grid-stride loop plus tail."""
    check_first_order(be, name, N_BIG)
