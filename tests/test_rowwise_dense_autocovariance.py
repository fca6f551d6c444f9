"""`RowDenseOutput.autocovariance` on the host path: hand-made records with DYADIC breakpoints (multiples of 1/32 on [0, 1])
against a closed form in numpy.longdouble, worked in TRUE time (no quadrature: on every piece of the merged breakpoints both
quartics are re-expanded in the piece's own variable — well conditioned, where the base step's variable is not when the lead
step is 32 times shorter — and the product polynomial is integrated by monomials).

Tolerance (derived, not measured), in the notation of test_rowwise_dense_time_moments.py: u = 2^-53, N = 5 * (pieces of non-zero
length), Y the magnitude polynomial of a factor on its own step, m the reference mean, <f> the average over the overlap:
    |C_ij - ref| <= K u <(Y_i + |m_i|)(Y'_j + |m_j|)> + dm_i <Y'_j + |m_j|> + dm_j <Y_i + |m_i|>,      K = 2 (2 N + 219)
Per summed term (W_g v) v': a factor's Horner form 8; its node x_g = xlo + span * n_g with xlo = (p_lo - ta) / h and span =
(p_hi - p_lo) / h, eight roundings (h, the two differences, the two quotients, n_g's product and sum, h again), each relative to
a part of x, through x |p'| <= 4 Y: 32; its subtraction of the mean 1: 41 per factor, 82.  The lead factor alone: rounding p_lo +
tau perturbs its fraction by up to u |t + tau| / h', which enters through x |p'| <= 4 Y; breakpoints on multiples of 1/32 of [0,
1] keep |t + tau| / h' <= 32: 128.  The weight 3 (the difference, w_g, their product), the two products 2, the sum in any order
N, Wsum and the division N + 4: 2 N + 219, doubled for headroom as there.  dm = K_mean u <Y> is the bound of the INPUT mean (that
test's): over the overlap, unlike over the whole window, the deviations do not integrate to zero, so the mean's error enters at
first order.  Windows and lags here are dyadic too, so every p_lo + tau and breakpoint - tau is exact."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import torchdiffeq_amd as tda
from test_rowwise_dense_time_moments import DTYPES, F32, F64, LD, SIGNS, U, _moment
from test_rowwise_dense_time_moments import reference as moments_reference
from torchdiffeq_amd import _native, rowwise_dense

# 0; shorter than the shortest step; one that makes breakpoints coincide; one spanning several steps; one that leaves the whole
# row an overlap inside its first step
LAGS = torch.tensor([0.0, 1 / 64, 1 / 8, 23 / 64, 63 / 64], dtype=F64)


def make_record(dtype, L, counts, sign, kernels=None, device="cpu"):
    """A record of len(counts) rows on the solver-time interval [0, 1], row r with counts[r] steps at random multiples of
    1/32 and random coefficients of order 1 around 3 (the steps do not join: every breakpoint is a jump)."""
    g = torch.Generator().manual_seed(77 * L + sum(counts) + int(sign))
    B, n_seg = len(counts), sum(counts)
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
    cuts = [torch.cat([torch.zeros(1, dtype=F64), torch.sort(1 + torch.randperm(31, generator=g)[:n - 1])[0].to(F64) / 32,
                       torch.ones(1, dtype=F64)]) for n in counts]
    ta, tb = torch.cat([c[:-1] for c in cuts]), torch.cat([c[1:] for c in cuts])
    coeffs = torch.randn(5, n_seg, L, generator=g, dtype=F64)
    coeffs[0] += 3.0
    p = types.SimpleNamespace(sign=sign, shape=(B, L), device=torch.device(device),
                              tgrid=torch.stack([torch.zeros(B, dtype=F64), torch.ones(B, dtype=F64)]))
    return rowwise_dense.RowDenseOutput(p, kernels, offsets.to(device), ta.to(device), tb.to(device),
                                        coeffs.to(dtype).to(device).contiguous())


def windows(dense):
    """True-time ends (qa, qb), each [5, B]: inside the first step, several steps with both ends partial, the same reversed,
    zero length, the whole interval."""
    off, B = dense.offsets.tolist(), dense._shape[0]
    first = torch.stack([dense._tb[off[r]].cpu() for r in range(B)])                  # (solver time; the first step starts at 0)
    lo, hi, one = torch.full((B,), 9 / 64, dtype=F64), torch.full((B,), 55 / 64, dtype=F64), torch.ones(B, dtype=F64)
    qa = torch.stack([0.25 * first, lo, hi, 13 / 32 * one, 0.0 * one])
    qb = torch.stack([0.75 * first, hi, lo, 13 / 32 * one, one])
    return qa * dense._sign, qb * dense._sign


def _compose(c, al, be):
    """The coefficients in x of sum_k c[k] (al x + be)^k, c [5, L]."""
    out = np.zeros_like(c)
    for k in range(5):
        for m in range(k + 1):
            out[m] += c[k] * (math.comb(k, m) * al ** m * be ** (k - m))
    return out


def reference(dense, qa, qb, lags):
    """Per lag `lags` [K, B] and window of the true-time ends [Q, B] -> (C, tol), both longdouble [K, Q, B, L, L]; C[.., i, j]
    has i at t and j at t + lag, NaN where the lag is invalid for the window."""
    sg, co, off = LD(dense._sign), dense.coeffs.cpu().numpy().astype(LD), dense.offsets.tolist()
    ta, tb = dense._ta.cpu().numpy().astype(LD), dense._tb.cpu().numpy().astype(LD)
    (K, B), Q, L = lags.shape, qa.shape[0], co.shape[2]
    one = np.ones((5, 1), dtype=LD) * (np.arange(5) == 0)[:, None]
    C, tol = np.full((K, Q, B, L, L), np.nan, dtype=LD), np.zeros((K, Q, B, L, L), dtype=LD)
    for (j, r), (T, mean, _, mean_tol, _) in moments_reference(dense, qa, qb).items():
        a = min(LD(float(qa[j, r])), LD(float(qb[j, r])))
        spans = [(s, *sorted((sg * ta[s], sg * tb[s]))) for s in range(off[r], off[r + 1])]     # steps in true time
        find = lambda t: next(s for s, u0, u1 in spans if u0 <= t <= u1)                          # noqa: E731
        for k in range(K):
            tau = LD(lags[k, r])
            if not (tau == 0 or 0 < tau < T):
                continue
            if T == 0:
                C[k, j, r] = 0
                continue
            end = a + T - tau
            cuts = sorted({a, end} | {v for _, u0, u1 in spans for v in (u0, u1, u0 - tau, u1 - tau) if a < v < end})
            acc, big, wide_b, wide_l = 0, 0, 0, 0
            for p, q in zip(cuts[:-1], cuts[1:]):
                # both quartics in the piece's own variable z in [0, 1], t = p + (q - p) z: fractions x = x(p) + (x(q) - x(p)) z
                sb, sl = find((p + q) / 2), find((p + q) / 2 + tau)
                xb, xl = ((sg * v - ta[sb]) / (tb[sb] - ta[sb]) for v in (p, q)), \
                    ((sg * (v + tau) - ta[sl]) / (tb[sl] - ta[sl]) for v in (p, q))
                (b0, b1), (l0, l1) = xb, xl
                base, lead = _compose(co[:, sb], b1 - b0, b0), _compose(co[:, sl], l1 - l0, l0)
                wb, wl = _compose(np.abs(co[:, sb]), b1 - b0, b0), _compose(np.abs(co[:, sl]), l1 - l0, l0)
                base[0], lead[0], wb[0], wl[0] = base[0] - mean, lead[0] - mean, wb[0] + np.abs(mean), wl[0] + np.abs(mean)
                acc, big = acc + (q - p) * _moment(base, lead, 0, 1), big + (q - p) * _moment(wb, wl, 0, 1)
                wide_b, wide_l = wide_b + (q - p) * _moment(wb, one, 0, 1)[:, 0], wide_l + (q - p) * _moment(wl, one, 0, 1)[:, 0]
            W, k_lag = end - a, 2 * (2 * 5 * (len(cuts) - 1) + 219)
            C[k, j, r] = acc / W
            tol[k, j, r] = k_lag * U * big / W + np.outer(mean_tol, wide_l / W) + np.outer(wide_b / W, mean_tol)
    return C, tol


def check(got, C, tol, slack=1):
    """`got`: RowDenseAutocovariance with [K, Q, B, ...] fields (any device) against `reference`; NaN exactly where it has."""
    auto = got.autocovariance.cpu().numpy()
    diag, diag_tol = np.diagonal(C, axis1=-2, axis2=-1), np.diagonal(tol, axis1=-2, axis2=-1)
    assert np.array_equal(np.isnan(auto), np.isnan(diag))
    assert (np.isnan(diag) | (np.abs(auto.astype(LD) - diag) <= slack * diag_tol)).all()
    if got.covariance is not None:
        cov = got.covariance.cpu().numpy()
        assert np.array_equal(np.isnan(cov), np.isnan(C))
        assert (np.isnan(C) | (np.abs(cov.astype(LD) - C) <= slack * tol)).all()
        assert np.array_equal(np.diagonal(cov, axis1=-2, axis2=-1), auto, equal_nan=True)      # the diagonal rule, bit for bit


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_path_against_closed_form(dtype, sign):
    dense = make_record(dtype, 5, [1, 6, 3], sign)
    qa, qb = windows(dense)
    per_row = LAGS[:, None].expand(-1, 3).contiguous()
    C, tol = reference(dense, qa, qb, per_row.numpy())
    assert np.isfinite(C[:, 4].astype(np.float64)).all() and np.isnan(C[1:, 3].astype(np.float64)).all()   # whole row; zero length
    plain = dense.autocovariance(qa, qb, LAGS, check=False)
    full = dense.autocovariance(qa, qb, LAGS, covariance=True, check=False)
    assert plain.covariance is None and plain.autocovariance.shape == (5, 5, 3, 5) and plain.autocovariance.dtype == F64
    assert full.covariance.shape == (5, 5, 3, 5, 5) and full.covariance.dtype == F64
    check(plain, C, tol)
    check(full, C, tol)
    # duration and mean are those of time_moments; at lag 0 the covariance is its covariance within the sum of the bounds
    moments = dense.time_moments(qa, qb, covariance=True)
    assert all(torch.equal(v.duration, moments.duration) and torch.equal(v.mean, moments.mean) for v in (plain, full))
    for (j, r), (_, _, _, _, cov_tol) in moments_reference(dense, qa, qb).items():
        gap = np.abs(full.covariance[0, j, r].numpy().astype(LD) - moments.covariance[j, r].numpy())
        assert (gap <= tol[0, j, r] + cov_tol).all(), (j, r)
    assert not bool(full.covariance[0, 3].any()) and not bool(plain.autocovariance[0, 3].any())          # lag 0, zero length
    for a, b in zip(full[2:], dense.autocovariance(qb, qa, LAGS, covariance=True, check=False)[2:]):      # reversed ends
        assert torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))
    assert torch.equal(full.covariance[:, 1].nan_to_num(nan=7.0), full.covariance[:, 2].nan_to_num(nan=7.0))
    for a, b in zip(full[2:], dense.autocovariance(qa, qb, per_row, covariance=True, check=False)[2:]):   # [K] against [K, B]
        assert torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))
    one = dense.autocovariance(float(qa[1, 0]), float(qb[1, 0]), 1 / 8, covariance=True)
    assert one.duration.shape == (3,) and one.mean.shape == one.autocovariance.shape == (3, 5)
    assert torch.equal(one.covariance, full.covariance[2, 1])


def test_refusals_and_abi():
    dense = make_record(F32, 3, [2, 2], 1.0)
    what = r"dense.autocovariance\(ta, tb, lags\)"
    with pytest.raises(ValueError, match=what + ": lags must be >= 0"):
        dense.autocovariance(0.0, 1.0, -0.125)
    with pytest.raises(ValueError, match="lags must be >= 0 and not NaN"):
        dense.autocovariance(0.0, 1.0, torch.tensor([0.0, float("nan")]))
    ta, tb = torch.tensor([[0.0, 0.0], [0.0, 0.5]], dtype=F64), torch.tensor([[1.0, 1.0], [1.0, 0.75]], dtype=F64)
    lags = torch.tensor([0.0, 0.25])                                             # T = 0.25 for query 1 of row 1: 0.25 is no lag
    with pytest.raises(ValueError, match=what + r": lag 1 of query 1 of row 1 \(lag = 0.25\).*T = 0.25"):
        dense.autocovariance(ta, tb, lags)
    got = dense.autocovariance(ta, tb, lags, covariance=True, check=False)
    only = torch.zeros(2, 2, 2, dtype=torch.bool)
    only[1, 1, 1] = True
    assert torch.equal(got.autocovariance.isnan().all(-1), only) and torch.equal(got.autocovariance.isnan().any(-1), only)
    assert torch.equal(got.covariance.isnan().all(-1).all(-1), only) and not bool(got.mean.isnan().any())
    with pytest.raises(ValueError, match=r"query 0 of row 1 \(tb = 1.5\)"):      # the ends come first, as in time_moments
        dense.autocovariance(0.0, torch.tensor([[1.0, 1.5]], dtype=F64), 2.0)
    with pytest.raises(ValueError, match="covariance must be a bool"):
        dense.autocovariance(0.1, 0.2, 0.0, covariance=1)
    with pytest.raises(NotImplementedError, match="does not propagate gradients"):
        dense.autocovariance(torch.tensor(0.1, requires_grad=True), 0.2, 0.0)
    wide = make_record(F32, _native.TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN + 1, [1], 1.0)
    with pytest.raises(ValueError, match="covariance=True takes rows of at most 256 elements"):
        wide.autocovariance(0.1, 0.2, 0.0, covariance=True)
    assert wide.autocovariance(0.1, 0.2, 0.0).autocovariance.shape == (1, 257)
    # the ABI: additive within version 38; refusals before any launch (no GPU needed) and no-ops
    assert "RowDenseAutocovariance" in tda.__all__ and "RowDenseAutocovariance" in rowwise_dense.__all__
    assert tda.RowDenseAutocovariance._fields == ("duration", "mean", "autocovariance", "covariance")
    assert {"tdeq_row_dense_time_lagged", "tdeq_row_dense_time_lagged_gram"} <= set(_native.ABI_SIGNATURES)
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38
    p = ctypes.addressof(ctypes.create_string_buffer(64))
    tail = lambda sign, L, dtype=0, K=1, n=1: (p, p, p, K, p, 1, p, p, sign, p, p, p, p, p, p, n, L, dtype, None)   # noqa: E731
    lagged, gram = lib.tdeq_row_dense_time_lagged, lib.tdeq_row_dense_time_lagged_gram
    assert lagged(None, *tail(1.0, 1)) == -1 and gram(None, p, *tail(1.0, 1)) == -1 and gram(p, None, *tail(1.0, 1)) == -1
    assert lagged(p, *tail(2.0, 1)) == -1 and gram(p, p, *tail(0.0, 1)) == -1
    assert lagged(p, *tail(1.0, 1, 4)) == -1 and gram(p, p, *tail(1.0, 1, 4)) == -1 and gram(p, p, *tail(1.0, 257)) == -1
    for empty in (dict(L=0), dict(L=1, K=0), dict(L=1, n=0)):
        assert lagged(p, *tail(1.0, **empty)) == 0 and gram(p, p, *tail(1.0, **empty)) == 0
