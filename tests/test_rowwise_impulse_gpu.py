"""`jump_dy` on the MI355X: the HIP kernels against the host path on the problem of the device-driver test, batch
invariance, compaction bit for bit for both entry points, and a refresh whose unused rows and unused impulses are NaN."""
import warnings

import pytest
import torch

from _rowwise_impulse_oracle import decay_problem, device_impulse_problem, doses
from _rowwise_steps_oracle import METHODS, assert_device_matches_host, device_tolerances

import torchdiffeq_amd as tda

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
NAN = float("nan")


@pytest.mark.parametrize("direction", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [3, 129])
@pytest.mark.parametrize("method", METHODS)
def test_hip_matches_host_path(method, L, dtype, direction):
    y0, f, t, options = device_impulse_problem(dtype, L, direction)
    kw = dict(method=method, return_stats=True, **device_tolerances(dtype))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", tda.HostPathWarning)
        host, sh = tda.odeint_rowwise(f, y0, t, options=options, **kw)
    y0d, fd, td, options_d = device_impulse_problem(dtype, L, direction, DEV)
    dev, sd = tda.odeint_rowwise(fd, y0d, td, options=options_d, **kw)
    assert_device_matches_host(dev, sd, host, sh, dtype, method)
    assert sd["n_impulses"].tolist() == sh["n_impulses"].tolist() == [2, 2, 1, 1, 2, 1]


def _problem64(dtype, L=8):
    """B = 64 rows with their own end times and one to three doses each (the third column NaN for every other row)."""
    B = 64
    y0, make = decay_problem(B, L, dtype, 21, DEV)
    end = torch.linspace(0.25, 1.0, B, dtype=F64)
    jump = torch.stack([0.3 * end, 0.8 * end, torch.where(torch.arange(B) % 2 == 0, 0.55 * end, NAN)])
    jump = jump[:, torch.arange(B)].flip(0).contiguous()     # (unsorted columns)
    dy = doses(3, B, L, dtype, 22, DEV)
    return y0, make, end, jump, dy


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_batch_invariance(dtype):
    y0, make, end, jump, dy = _problem64(dtype)
    t = torch.stack([torch.zeros(64, dtype=F64), 0.5 * end, end])
    kw = dict(rtol=1e-5, atol=1e-7, return_stats=True)
    full, st = tda.odeint_rowwise(make(), y0, t.to(DEV), options={"jump_t": jump, "jump_dy": dy}, **kw)
    sub = list(range(3, 64, 4))
    part, sp = tda.odeint_rowwise(make(rows_of=sub), y0[sub], t[:, sub].to(DEV),
                                  options={"jump_t": jump[:, sub], "jump_dy": dy[:, sub]}, **kw)
    assert torch.equal(part, full[:, sub])
    for name in ("n_accepted", "n_rejected", "n_impulses"):
        assert torch.equal(sp[name], st[name][sub]), name
    assert st["n_impulses"].tolist() == [3 if r % 2 == 0 else 2 for r in range(64)]


@pytest.mark.parametrize("c", [0.5, True])
def test_compaction_is_bit_exact(c):
    y0, make, end, jump, dy = _problem64(F32)
    t = torch.stack([torch.zeros(64, dtype=F64), 0.5 * end, end]).to(DEV)
    kw = dict(rtol=1e-5, atol=1e-7, options={"jump_t": jump, "jump_dy": dy}, return_stats=True)
    plain, sa = tda.odeint_rowwise(make(), y0, t, **kw)
    slow = int((sa["n_accepted"] + sa["n_rejected"]).argmax())     # the row that takes the most trial steps
    seen = []

    def by_rows(t_, y, rows, inner=make(by_rows=True)):
        at = rows == slow
        if bool(at.any()):
            seen.append((int(rows.numel()), t_[at][0]))
        return inner(t_, y, rows)
    packed, sb = tda.odeint_rowwise(by_rows, y0, t, compact=c, **kw)
    assert torch.equal(plain, packed) and sb["n_repacks"] > 0
    # that row takes its last dose, at 0.8 of its interval, in a batch that was repacked before
    assert any(n < 64 and float(tt) < 0.8 * float(end[slow]) for n, tt in seen), slow
    assert int(sb["n_impulses"][slow]) >= 2
    for name in ("n_accepted", "n_rejected", "n_impulses"):
        assert torch.equal(sa[name], sb[name]), name
    da, ta = tda.odeint_rowwise_dense(make(), y0, 0.0, end, **kw)
    db, tb = tda.odeint_rowwise_dense(make(by_rows=True), y0, 0.0, end, compact=c, **kw)
    assert tb["n_repacks"] > 0 and torch.equal(ta["n_impulses"], tb["n_impulses"])
    for name in ("offsets", "seg_start", "seg_end", "coeffs"):
        assert torch.equal(getattr(da, name), getattr(db, name)), name


def test_poisoned_refresh():
    """The evaluation behind a jump returns NaN for every row that did not jump, and `jump_dy` holds NaN behind every NaN
    time: neither reaches the result."""
    y0, make, end, jump, dy = _problem64(F64)
    t = torch.stack([torch.zeros(64, dtype=F64), 0.5 * end, end]).to(DEV)
    kw = dict(rtol=1e-6, atol=1e-8, return_stats=True)
    clean, sc = tda.odeint_rowwise(make(), y0, t, options={"jump_t": jump, "jump_dy": dy}, **kw)
    poisoned_dy = torch.where(torch.isnan(jump).to(DEV)[:, :, None], torch.full_like(dy, NAN), dy)
    inner = make()
    points = torch.where(torch.isnan(jump), torch.full_like(jump, -1.0), jump).to(DEV)
    n_poisoned = [0]

    def f(t_, y):
        # a row is being refreshed iff its time is the next representable one behind one of its points
        behind = (t_[None, :] == torch.nextafter(points, points + 1)).any(dim=0)
        out = inner(t_, y)
        if bool(behind.any()):
            n_poisoned[0] += 1
            out = torch.where(behind[:, None], out, torch.full_like(out, NAN))
        return out
    got, sg = tda.odeint_rowwise(f, y0, t, options={"jump_t": jump, "jump_dy": poisoned_dy}, **kw)
    assert n_poisoned[0] > 0
    assert torch.equal(got, clean)
    for name in ("n_accepted", "n_rejected", "n_impulses"):
        assert torch.equal(sg[name], sc[name]), name
