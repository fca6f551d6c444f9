"""`weights=` of `RowDenseOutput.moments` / `.cross_covariance` on the MI355X: `row_dense_moments_weighted` and
`row_dense_cross_weighted` themselves on the hand-made record of the moments test against the two-pass numpy.longdouble
reference of tests/test_rowwise_dense_weighted.py (its docstring derives the bounds) on the values the `dense(t)` kernel gives
that record; the bit identities that pin the design (all-ones weights against the unweighted kernels, 0/1 weights against the
same rows out of range, the same call twice, sliced times); and the device against the reference and the host path on a real
solve.  Weights are 0.5 + rand, so the effective sample size stays well above `correction` (the reference asserts it); a
population that can hold a single row (B < 3) takes the weight 2.0, for which D = 0 exactly."""
import numpy as np
import pytest
import torch

from _rowwise_dense_oracle import decay_problem, per_row_t1, tolerances
from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_moments_gpu import _close, _record, _values
from test_rowwise_dense_weighted import check_moments, reference

import torchdiffeq_amd as tda
from torchdiffeq_amd._native import TDEQ_ROW_MOMENTS_SLAB_ROWS as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SENTINEL = 12345


def _weights(Q, B, per_time, took=None):
    """fp64 [Q, B] or [B] on the device; NaN for the rows that are in no time's population."""
    w = 0.5 + torch.rand(Q if per_time else 1, B, generator=torch.Generator().manual_seed(Q * 10 + B), dtype=F64)
    if B < 3:
        w[:] = 2.0
    if took is not None:
        w[:, torch.from_numpy(~took.any(axis=0))] = float("nan")
    return (w if per_time else w[0]).to(DEV)


def _run(k, coeffs, seg, x, Q, correction, w, covariance=False, z=None, bordered=False):
    """`row_dense_moments_weighted` (z None) or `row_dense_cross_weighted` into outputs with a border -> numpy arrays (count,
    mean, variance, covariance or None) or (out, count, ybar); the borders are intact."""
    L, B = coeffs.shape[2], seg.numel() // Q
    if z is None:
        shapes = [((Q,), torch.int64), ((Q, L), F64), ((Q, L), F64)] + ([((Q, L, L), F64)] if covariance else [])
    else:
        shapes = [((Q, L, z.shape[1]), F64), ((Q,), torch.int64), ((Q, L), F64)]
    pad = 8 if bordered else 0
    flats = [torch.full((int(np.prod(s)) + 2 * pad,), SENTINEL, dtype=t, device=DEV) for s, t in shapes]
    outs = [f[pad:f.numel() - pad].view(s) for f, (s, _) in zip(flats, shapes)]
    if z is None:
        work = torch.empty(k.row_dense_moments_weighted_workspace_bytes(covariance, Q, B, L, coeffs.dtype), dtype=torch.uint8,
                           device=DEV)
        k.row_dense_moments_weighted(*outs, *[None] * (not covariance), correction, coeffs, seg, x, work, w)
    else:
        work = torch.empty(k.row_dense_cross_weighted_workspace_bytes(Q, B, L, z.shape[1], coeffs.dtype), dtype=torch.uint8,
                           device=DEV)
        k.row_dense_cross_weighted(*outs, z, correction, coeffs, seg, x, work, w)
    for f in flats:
        assert not bordered or bool((torch.cat([f[:pad], f[-pad:]]) == SENTINEL).all())
    return [o.cpu().numpy() for o in outs] + [None] * (z is None and not covariance)


def _unweighted(k, coeffs, seg, x, Q, correction, covariance=False, z=None):
    """The same outputs from `row_dense_moments` / `row_dense_cross`."""
    L, B = coeffs.shape[2], seg.numel() // Q
    count, mean, var = torch.empty(Q, dtype=torch.int64, device=DEV), *torch.empty(2, Q, L, dtype=F64, device=DEV)
    if z is None:
        cov = torch.empty(Q, L, L, dtype=F64, device=DEV) if covariance else None
        work = torch.empty(k.row_dense_moments_workspace_bytes(covariance, Q, B, L, coeffs.dtype), dtype=torch.uint8, device=DEV)
        k.row_dense_moments(count, mean, var, cov, correction, coeffs, seg, x, work)
        return [None if o is None else o.cpu().numpy() for o in (count, mean, var, cov)]
    out = torch.empty(Q, L, z.shape[1], dtype=F64, device=DEV)
    work = torch.empty(k.row_dense_cross_workspace_bytes(Q, B, L, z.shape[1], coeffs.dtype), dtype=torch.uint8, device=DEV)
    k.row_dense_cross(out, count, mean, z, correction, coeffs, seg, x, work)
    return [o.cpu().numpy() for o in (out, count, mean)]


def _same_bits(a, b):
    return all((p is None and q is None) or np.array_equal(p.view(np.int64), q.view(np.int64)) for p, q in zip(a, b))


def _other(B, M):
    return (50 + torch.randn(B, M, generator=torch.Generator().manual_seed(B + M), dtype=F64)).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q,per_time", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("B", [1, 3, 67, R + 1])
@pytest.mark.parametrize("L", [5, 8, 70])
def test_kernels_against_longdouble(hip_kernels, L, B, Q, per_time, dtype):
    """L = 5: scalar loads; 8: 16-byte loads; 70: two element tiles, three pairs, a tail.  B = 1: an empty divisor with
    correction = 1; 3: fewer rows than a k-step; 67: several chunks and a partial one; R + 1: two slabs.  About one row in eight
    has left; where it has left every time its weight is NaN.  The cross kernel runs M = 1 (the 16-column block) and M = 17 (the
    64-column block); the outputs are bordered for B = 67."""
    coeffs, seg, x = _record(Q, B, L, dtype)
    y, took = _values(hip_kernels, coeffs, seg, x, Q)
    w = _weights(Q, B, per_time, took)
    wq = np.broadcast_to(w.cpu().numpy(), (Q, B))
    for correction in (0, 1):
        for covariance in (False, True):
            got = _run(hip_kernels, coeffs, seg, x, Q, correction, w, covariance, bordered=B == 67)
            for j in range(Q):
                check_moments([None if f is None else f[j] for f in got], y[j], wq[j], took[j], correction)
        for M in (1, 17):
            z = _other(B, M)
            out, count, ybar = _run(hip_kernels, coeffs, seg, x, Q, correction, w, z=z, bordered=B == 67)
            assert np.array_equal(count, got[0]) and _same_bits([ybar], [got[1]])
            for j in range(Q):
                _, _, ref, _, tol = reference(y[j], wq[j], took[j], correction, z.cpu().numpy())
                assert _close(out[j], ref, tol), (M, j)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [8, 70])
def test_bit_identities(hip_kernels, L, dtype):
    """Two slabs, Q = 3, every output: all-ones weights give the bits of the unweighted kernels; 0/1 weights give the bits of
    the same rows out of range under all-ones weights, `count` apart; the same call twice; Q = 3 against three calls of Q = 1."""
    Q, B = 3, R + 1
    coeffs, seg, x = _record(Q, B, L, dtype)
    ones = torch.ones(Q, B, dtype=F64, device=DEV)
    pick = (torch.rand(Q, B, generator=torch.Generator().manual_seed(3)) < 0.7).to(DEV)
    x_out = torch.where(pick.reshape(-1), x, torch.full_like(x, float("nan")))
    w = _weights(Q, B, True)
    for kw in (dict(covariance=False), dict(covariance=True), dict(z=_other(B, 3)), dict(z=_other(B, 17))):
        for correction in (0, 1):
            assert _same_bits(_run(hip_kernels, coeffs, seg, x, Q, correction, ones, **kw),
                              _unweighted(hip_kernels, coeffs, seg, x, Q, correction, **kw)), (kw.keys(), correction)
            assert _same_bits(_run(hip_kernels, coeffs, seg, x, Q, correction, ones[0].contiguous(), **kw),
                              _unweighted(hip_kernels, coeffs, seg, x, Q, correction, **kw))
        at = 1 if "z" in kw else 0                                                       # where `count` sits
        zero_one = _run(hip_kernels, coeffs, seg, x, Q, 1, pick.double(), **kw)
        left = _run(hip_kernels, coeffs, seg, x_out, Q, 1, ones, **kw)
        assert not np.array_equal(zero_one[at], left[at])
        assert _same_bits(zero_one[:at] + zero_one[at + 1:], left[:at] + left[at + 1:]), kw.keys()
        whole = _run(hip_kernels, coeffs, seg, x, Q, 1, w, **kw)
        assert _same_bits(whole, _run(hip_kernels, coeffs, seg, x, Q, 1, w, **kw))
        for j in range(Q):
            part = _run(hip_kernels, coeffs, seg[j * B:(j + 1) * B], x[j * B:(j + 1) * B], 1, 1, w[j:j + 1], **kw)
            assert _same_bits([None if a is None else a[j:j + 1] for a in whole], part), (kw.keys(), j)


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_solve_against_reference_and_host_path(dtype):
    """Per-row `t1`, B = 67, shared times beyond some rows' `t1` with `check=False` and `[Q, B]` weights: the device against
    the longdouble reference on its own `dense(t)` within the bound and against the host path within twice the bound."""
    B, L = 67, 8
    y0, func, k = decay_problem(B, L, dtype, 3, DEV)
    with torch.no_grad():
        dense = tda.odeint_rowwise_dense(func, y0, 0.0, per_row_t1(B).to(DEV), method="dopri5", **tolerances("dopri5", dtype))
    assert dense._k is not None
    twin = _on_host(dense)
    shared = torch.tensor([0.1, 0.45, 0.55], dtype=F64)
    y = dense(shared.to(DEV), check=False).cpu().numpy()
    took = ~np.isnan(y[:, :, 0])
    assert took[0].all() and 2 <= took[2].sum() < B
    w, z = _weights(3, B, True).cpu(), k.cpu().double()
    got = dense.moments(shared.to(DEV), covariance=True, weights=w, check=False)
    host = twin.moments(shared, covariance=True, weights=w, check=False)
    cross = dense.cross_covariance(shared.to(DEV), z, weights=w.to(DEV), check=False)
    cross_host = twin.cross_covariance(shared, z, weights=w, check=False)
    assert got.mean.device.type == DEV.type and torch.equal(got.count.cpu(), host.count)
    for j in range(3):
        check_moments([f[j].cpu().numpy() for f in got], y[j], w[j].numpy(), took[j], 1)
        _, _, ref, mean_tol, tol = reference(y[j], w[j].numpy(), took[j], 1)
        assert _close(got.mean[j].cpu().numpy(), host.mean[j].numpy().astype(np.longdouble), mean_tol, 2)
        assert _close(got.covariance[j].cpu().numpy(), host.covariance[j].numpy().astype(np.longdouble), tol, 2)
        _, _, ref, _, tol = reference(y[j], w[j].numpy(), took[j], 1, z.numpy())
        assert _close(cross[j].cpu().numpy(), ref, tol) and _close(cross[j].cpu().numpy(),
                                                                   cross_host[j].numpy().astype(np.longdouble), tol, 2), j
    with pytest.raises(ValueError, match=r"dense.moments\(t\): query 1 of row 0 \(t = 0.45"):
        dense.moments(shared.to(DEV), weights=w)
