"""`jump_dy`: per-row state impulses at the jump points of `odeint_rowwise` and `odeint_rowwise_dense`, without a GPU — the
host path against the closed form and the chained `odeint` solve, the closed rule for a step that lands on a point, the
bits of the `jump_t` solve for zero impulses, row independence, the equivalent forms, the left limits, compaction, the
device driver on the CPU row oracle, and the validation."""
import pytest
import torch

from _rowwise_impulse_oracle import (decay_problem, device_impulse_problem, doses, impulse_driver)  # noqa: F401
from _rowwise_steps_oracle import METHODS, assert_device_matches_host, device_tolerances, quiet  # noqa: F401

import torchdiffeq_amd as tda

NAN = float("nan")
F64 = torch.float64


def _same(a, b, with_nfe=True):
    (sa, ta), (sb, tb) = a, b
    assert torch.equal(sa, sb)
    for name in ("n_accepted", "n_rejected", "n_impulses"):
        assert torch.equal(ta[name], tb[name]), name
    if with_nfe:
        assert ta["nfe"] == tb["nfe"]


# -- 1. the closed form and the chained reference solve ------------------------------------------------------------------------
def test_bolus_doses_against_closed_form_and_chained_solve():
    """Depot -> central, dy/dt = A_r y with per-row ka, ke, three boluses into the depot per row at the row's own times (one
    NaN entry), fp64, rtol 1e-9, atol 1e-11, five output times per row, none a dose time.  Truth: matrix_exp propagation
    between doses.  Yardstick: per row, `odeint` from dose to dose with y += dose in between; its maximum error against the
    truth is e_ref, and the one batched solve with `jump_dy` must have e <= 4 e_ref (two valid step sequences under one local
    error control; a missed or doubled dose is an O(dose) error).

    Measured: e_ref = 4.27e-10, e = 5.90e-10."""
    B = 6
    ka = torch.tensor([1.2, 0.8, 2.0, 1.5, 0.6, 1.0], dtype=F64)
    ke = torch.tensor([0.3, 0.25, 0.5, 0.2, 0.4, 0.35], dtype=F64)
    A = torch.zeros(B, 2, 2, dtype=F64)
    A[:, 0, 0], A[:, 1, 0], A[:, 1, 1] = -ka, ka, -ke
    y0 = torch.tensor([[1.0, 0.1], [0.5, 0.0], [2.0, 0.3], [1.0, 1.0], [0.0, 0.5], [1.5, 0.2]], dtype=F64)
    t0 = torch.tensor([0.0, 0.1, 0.0, 0.2, 0.05, 0.0], dtype=F64)
    t_end = torch.tensor([4.0, 3.5, 5.0, 4.2, 3.0, 4.5], dtype=F64)
    frac = torch.tensor([0.0, 0.17, 0.39, 0.58, 0.81, 1.0], dtype=F64)
    t = t0[None, :] + frac[:, None] * (t_end - t0)[None, :]                       # [6, B]: t0 and five output times
    jump = torch.tensor([[1.0, 0.9, 2.5, NAN, 0.5, 3.1],
                         [2.0, 2.2, 0.7, 1.3, 2.9, 0.4],
                         [3.3, 1.6, 4.1, 3.0, 1.7, 1.9]], dtype=F64)              # (unsorted columns, one NaN)
    dose = torch.tensor([[1.0, 0.5, 2.0, 9.0, 0.7, 1.1],
                         [0.8, 1.5, 1.0, 0.6, 1.2, 0.9],
                         [1.3, 0.4, 0.5, 1.4, 1.0, 2.0]], dtype=F64)
    dy = torch.stack([dose, torch.zeros_like(dose)], dim=-1)                      # [3, B, 2]: into the depot
    assert not bool((t[1:, None, :] == jump[None]).any())
    tol = dict(rtol=1e-9, atol=1e-11)

    sol, st = tda.odeint_rowwise(lambda t_, y: torch.einsum("bij,bj->bi", A, y), y0, t,
                                 options={"jump_t": jump, "jump_dy": dy}, return_stats=True, **tol)
    truth, chained = torch.empty_like(sol), torch.empty_like(sol)
    n_doses = []
    for r in range(B):
        inside = sorted((float(jump[k, r]), k) for k in range(3) if float(t0[r]) < float(jump[k, r]) <= float(t_end[r]))
        n_doses.append(len(inside))
        cuts = [float(t0[r])] + [p for p, _ in inside] + [float(t_end[r])]
        y_true, y_ref = y0[r].clone(), y0[r].clone()
        truth[0, r] = chained[0, r] = y0[r]
        for s in range(len(cuts) - 1):
            a, b = cuts[s], cuts[s + 1]
            outs = [j for j in range(1, t.shape[0]) if a < float(t[j, r]) <= b]
            grid = torch.tensor([a] + [float(t[j, r]) for j in outs] + ([] if outs and float(t[outs[-1], r]) == b else [b]),
                                dtype=F64)
            seg = tda.odeint(lambda t_, y, Ar=A[r]: Ar @ y, y_ref, grid, **tol)
            for n, j in enumerate(outs):
                chained[j, r] = seg[n + 1]
                truth[j, r] = torch.linalg.matrix_exp(A[r] * (float(t[j, r]) - a)) @ y_true
            y_true = torch.linalg.matrix_exp(A[r] * (b - a)) @ y_true
            y_ref = seg[-1].clone()
            if s < len(inside):
                y_true = y_true + dy[inside[s][1], r]
                y_ref = y_ref + dy[inside[s][1], r]
    e_ref = float((chained - truth).abs().max())
    e = float((sol - truth).abs().max())
    print(f"bolus doses: e_ref = {e_ref:.3e}, e = {e:.3e}")
    assert e <= 4 * e_ref, (e, e_ref)
    assert st["n_impulses"].tolist() == n_doses and len(n_doses) == B and min(n_doses) >= 2


# -- 2. a step that lands on a point exactly ---------------------------------------------------------------------------------------
def test_exact_landing_applies_every_dose():
    """`first_step = 0.125` ends the first step on the first dose time exactly.  With `jump_dy` the closed rule makes that a
    step onto the point: all three doses are applied and all three points are breakpoints.  With `jump_t` alone the quirk of
    the reference stays (tests/test_rowwise_steps.py::test_point_hit_exactly_matches_odeint): the index sticks on 0.125 and
    0.6 and 1.1 are no breakpoints."""
    y0, make = decay_problem(1, 3, F64, 2)
    points = torch.tensor([0.125, 0.6, 1.1], dtype=F64)
    dy = doses(3, 1, 3, F64, 3)
    kw = dict(rtol=1e-6, atol=1e-8, return_stats=True)
    dense, st = tda.odeint_rowwise_dense(make(), y0, 0.0, 2.0, options={"jump_t": points, "jump_dy": dy,
                                                                        "first_step": 0.125}, **kw)
    plain, sp = tda.odeint_rowwise_dense(make(), y0, 0.0, 2.0, options={"jump_t": points, "first_step": 0.125}, **kw)
    assert st["n_impulses"].tolist() == [3]
    assert all(bool((dense.seg_end == p).any()) for p in (0.125, 0.6, 1.1))
    assert float(plain.seg_end[0]) == 0.125 and "n_impulses" not in sp
    assert not bool(((plain.seg_end == 0.6) | (plain.seg_end == 1.1)).any())
    # every dose arrived: behind the last point the two states differ by the doses, each decayed since its time
    assert float((dense(2.0) - plain(2.0)).abs().min()) > 0.01


# -- 3. zero impulses are the jump_t solve ------------------------------------------------------------------------------------------
JUMP7 = torch.tensor([[NAN, 0.0, 3.0, 0.5, 0.7, 0.55, 0.6],
                      [NAN, NAN, NAN, NAN, 0.25, 0.9, 0.15],
                      [NAN, NAN, NAN, NAN, NAN, NAN, 0.85]], dtype=F64)
FIRST7 = torch.tensor([0.05, 0.02, 0.03, 0.04, 0.01, 0.04, 0.02], dtype=F64)
B7 = 7


def _problem7(dtype, direction=1, L=3):
    """Columns: no point | a point at t0 (zero dy) | a point beyond the end | one, two, two and three doses."""
    y0, make = decay_problem(B7, L, dtype, 4)
    t = torch.linspace(0, 1, 4, dtype=F64) * direction
    dy = doses(3, B7, L, dtype, 6)
    dy[0, 1] = 0.0                                           # the point at t0: nothing to add
    return y0, make, t, JUMP7 * direction, dy


@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
def test_zero_impulses_are_the_jump_t_solve(direction):
    y0, make, t, jump, dy = _problem7(F64, direction)
    assert bool((y0 != 0).all())
    kw = dict(rtol=1e-6, atol=1e-8, return_stats=True)
    f = make(direction=direction)
    a, sa = tda.odeint_rowwise(f, y0, t, options={"jump_t": jump, "first_step": FIRST7}, **kw)
    b, sb = tda.odeint_rowwise(f, y0, t, options={"jump_t": jump, "jump_dy": torch.zeros_like(dy), "first_step": FIRST7},
                               **kw)
    assert torch.equal(a, b)
    assert torch.equal(sa["n_accepted"], sb["n_accepted"]) and torch.equal(sa["n_rejected"], sb["n_rejected"])
    assert sa["nfe"] == sb["nfe"]
    assert sb["n_impulses"].tolist() == [0, 0, 0, 1, 2, 2, 3]


# -- 4. row independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
def test_rows_are_independent(method, dtype, direction):
    y0, make, t, jump, dy = _problem7(dtype, direction)
    kw = dict(rtol=1e-5, atol=1e-7, method=method, return_stats=True)
    full, st = tda.odeint_rowwise(make(direction=direction), y0, t,
                                  options={"jump_t": jump, "jump_dy": dy, "first_step": FIRST7}, **kw)
    assert st["n_impulses"].tolist() == [0, 0, 0, 1, 2, 2, 3]
    for r in range(B7):
        one, s1 = tda.odeint_rowwise(make(rows_of=[r], direction=direction), y0[r:r + 1], t,
                                     options={"jump_t": jump[:, r:r + 1], "jump_dy": dy[:, r:r + 1],
                                              "first_step": FIRST7[r:r + 1]}, **kw)
        assert torch.equal(one[:, 0], full[:, r]), r
        for name in ("n_accepted", "n_rejected", "n_impulses"):
            assert int(s1[name]) == int(st[name][r]), (r, name)


# -- 5. equivalent forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
def test_equivalent_forms(direction):
    y0, make, t, jump, dy = _problem7(F64, direction)
    f = make(direction=direction)
    kw = dict(rtol=1e-6, atol=1e-8, return_stats=True)

    def run(jump_t, jump_dy):
        return tda.odeint_rowwise(f, y0, t, options={"jump_t": jump_t, "jump_dy": jump_dy}, **kw)
    # [K, L] shared against its [K, B, L] broadcast, with shared and per-row times
    shared_t = torch.tensor([0.7, 0.3], dtype=F64) * direction
    shared_dy = dy[:2, 0]
    ref = run(shared_t, shared_dy)
    assert ref[1]["n_impulses"].tolist() == [2] * B7
    _same(ref, run(shared_t, shared_dy[:, None].expand(-1, B7, -1)))
    _same(ref, run(shared_t[:, None].expand(-1, B7), shared_dy))
    _same(ref, run(shared_t.tolist(), shared_dy.numpy()))
    # the points permuted together with their dy
    ref = run(jump, dy)
    perm = [2, 0, 1]
    _same(ref, run(jump[perm], dy[perm]))
    # NaN-padded tables against the unpadded ones (the dy behind a NaN time is ignored, NaN included)
    pad_t = torch.cat([torch.full((1, B7), NAN, dtype=F64), jump, torch.full((2, B7), NAN, dtype=F64)])
    pad_dy = torch.cat([torch.full_like(dy[:1], NAN), dy, torch.full_like(dy[:2], 7.0)])
    _same(ref, run(pad_t, pad_dy))


# -- 6. left limits and the dense contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
def test_left_limits_and_dense_contract(direction):
    y0, make, _, jump, dy = _problem7(F64, direction)
    f = make(direction=direction)
    kw = dict(rtol=1e-6, atol=1e-8)
    first = torch.tensor([NAN, NAN, NAN, 0.5, 0.25, 0.55, 0.15], dtype=F64) * direction      # each row's first dose time
    rows = [3, 4, 5, 6]
    grid = torch.stack([torch.zeros(B7, dtype=F64), torch.where(first == first, first, 0.5 * direction),
                        torch.full((B7,), 1.0 * direction, dtype=F64)])
    sol = tda.odeint_rowwise(f, y0, grid, options={"jump_t": jump, "jump_dy": dy}, **kw)
    bare = tda.odeint_rowwise(f, y0, grid, options={"jump_t": jump}, **kw)
    dense = tda.odeint_rowwise_dense(f, y0, 0.0, 1.0 * direction, options={"jump_t": jump, "jump_dy": dy}, **kw)
    # an output time equal to a dose time holds the state before the impulse: up to its first dose a row is the jump_t solve
    assert torch.equal(sol[1, rows], bare[1, rows])
    at = dense(grid[1:2])[0]                                 # ([1, B]: a query per row)
    assert torch.equal(at[rows], sol[1, rows])               # dense(p): the left limit, a breakpoint belongs to the earlier step
    behind = dense(torch.nextafter(grid[1:2], grid[2:3]))[0]
    k_first = [int(torch.nonzero(jump[:, r] == first[r])[0]) for r in rows]
    want = torch.stack([dy[k, r] for k, r in zip(k_first, rows)])
    assert float((behind[rows] - at[rows] - want).abs().max()) < 1e-12      # ... and the first value behind it has the dose
    assert not bool((sol[2, rows] == bare[2, rows]).any())
    # the contract of the dense output: dense(q) is odeint_rowwise on the grid [t0, q, t1]
    q = torch.tensor([0.1, 0.3, 0.52, 0.77], dtype=F64) * direction
    on_grid = tda.odeint_rowwise(f, y0, torch.cat([grid[:1, 0], q, grid[-1:, 0]]),
                                 options={"jump_t": jump, "jump_dy": dy}, **kw)
    assert torch.equal(dense(q), on_grid[1:-1])


# -- 7. compaction -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.5, True])
def test_compaction_is_bit_exact(c):
    y0, make, t, jump, dy = _problem7(F64)
    tg = t[:, None] * torch.linspace(0.2, 1.0, B7, dtype=F64)          # rows finish at different times; row 6 last, at 1
    options = {"jump_t": jump, "jump_dy": dy, "max_step": 0.05}
    kw = dict(rtol=1e-6, atol=1e-8, options=options, return_stats=True)
    seen = []

    def by_rows(t_, y, rows, inner=make(by_rows=True)):
        last = rows == B7 - 1
        if bool(last.any()):
            seen.append((int(rows.numel()), float(t_[last][0])))
        return inner(t_, y, rows)
    plain = tda.odeint_rowwise(make(), y0, tg, **kw)
    packed = tda.odeint_rowwise(by_rows, y0, tg, compact=c, **kw)
    da, ta = tda.odeint_rowwise_dense(make(), y0, 0.0, tg[-1], **kw)
    db, tb = tda.odeint_rowwise_dense(make(by_rows=True), y0, 0.0, tg[-1], compact=c, **kw)
    _same(plain, packed, with_nfe=False)
    assert packed[1]["n_repacks"] > 0 and tb["n_repacks"] > 0
    # row 6 takes its dose at 0.85 in a batch that was repacked before
    assert any(n < B7 and tt < 0.85 for n, tt in seen) and int(packed[1]["n_impulses"][6]) == 3
    for name in ("offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(da, name), getattr(db, name)), name
    _same((da.coeffs, ta), (db.coeffs, tb), with_nfe=False)


# -- 8. the device driver on the row oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 129])
@pytest.mark.parametrize("method", METHODS)
def test_device_driver_matches_host_path(method, L, dtype, direction, impulse_driver):  # noqa: F811
    y0, f, t, options = device_impulse_problem(dtype, L, direction)
    kw = dict(method=method, options=options, return_stats=True, **device_tolerances(dtype))
    host, sh = tda.odeint_rowwise(f, y0, t, **kw)
    with impulse_driver():
        dev, sd = tda.odeint_rowwise(f, y0, t, **kw)
    assert_device_matches_host(dev, sd, host, sh, dtype, method)
    assert sd["n_impulses"].tolist() == sh["n_impulses"].tolist() == [2, 2, 1, 1, 2, 1]


def test_device_driver_exact_landing_dense_and_compaction(impulse_driver):  # noqa: F811
    """On the oracle's controller: the closed rule (a first step that lands on the first dose), the dense hook and a repack
    with `jump_hit` and the index table by original row."""
    y0, make, t, jump, dy = _problem7(F64)
    jump = jump.clone()
    jump[0, 3] = 0.04                                        # = FIRST7[3]: row 3's first step lands on it
    t_end = torch.linspace(0.2, 1.0, B7, dtype=F64)
    kw = dict(rtol=1e-6, atol=1e-8, options={"jump_t": jump, "jump_dy": dy, "first_step": FIRST7}, return_stats=True)
    q = torch.tensor([0.05, 0.15], dtype=F64)

    def run(compact):
        dense, st = tda.odeint_rowwise_dense(make(by_rows=compact is not None), y0, 0.0, t_end, compact=compact, **kw)
        return dense(q), st
    host, sh = run(None)
    with impulse_driver():
        dev, sd = run(None)
        devc, sdc = run(1.0)
    for name in ("n_accepted", "n_rejected", "n_impulses"):
        assert sd[name].tolist() == sh[name].tolist(), name
        assert torch.equal(sdc[name], sd[name]), name
    assert sd["nfe"] == sh["nfe"] and int(sh["n_impulses"][3]) == 1
    assert float((dev - host).abs().max() / host.abs().max()) < 1e-12
    assert torch.equal(devc, dev) and sdc["n_repacks"] > 0


# -- 9. validation ---------------------------------------------------------------------------------------------------------------------------
def test_validation():
    y0, make, t, jump, dy = _problem7(F64)
    f = make()

    def run(options, **kw):
        return tda.odeint_rowwise(f, y0, t, options=options, **kw)
    with pytest.raises(ValueError, match="jump_dy needs jump_t"):
        run({"jump_dy": dy})
    with pytest.raises(ValueError, match="jump_dy must be"):
        run({"jump_t": jump, "jump_dy": dy[:2]})                                 # another K
    with pytest.raises(ValueError, match="jump_dy must be"):
        run({"jump_t": jump, "jump_dy": dy[:, :, :2]})                           # another row shape
    with pytest.raises(ValueError, match="jump_dy must be"):
        run({"jump_t": jump, "jump_dy": dy[:, 0, 0]})
    bad = dy.clone()
    bad[1, 5, 2] = float("inf")
    with pytest.raises(ValueError, match=r"jump_dy\[1\] is not finite for row 5"):
        run({"jump_t": jump, "jump_dy": bad})
    bad = dy.clone()
    bad[0, 1, 1] = 0.5                                                           # row 1's point is its t0
    with pytest.raises(ValueError, match="row 1 is the row's start time.*add it to y0"):
        run({"jump_t": jump, "jump_dy": bad})
    with pytest.raises(ValueError, match="jump_dy must be real"):
        run({"jump_t": jump, "jump_dy": dy.to(torch.complex128)})
    with pytest.raises(NotImplementedError, match="jump_dy"):
        tda.odeint_rowwise_event(f, y0, 0.0, event_fn=lambda t_, y: y[:, 0] - 0.1, t_end=1.0,
                                 options={"jump_t": jump, "jump_dy": dy})
    with pytest.raises(NotImplementedError, match="jump_t, jump_dy are not supported for a recorded solve"):
        run({"jump_t": jump, "jump_dy": dy}, differentiable=True)
    # a NaN dy behind a NaN time and a point before t0 with any dy are fine
    ok = dy.clone()
    ok[0, 0] = NAN
    run({"jump_t": jump, "jump_dy": ok})
    run({"jump_t": torch.tensor([-1.0, 0.5], dtype=F64), "jump_dy": dy[:2]})
