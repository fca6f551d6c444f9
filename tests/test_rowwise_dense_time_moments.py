"""`RowDenseOutput.time_moments` on the host path: hand-made records against closed-form monomial integrals in numpy.longdouble
(no quadrature: the integral of x^m over the clipped step, of the product polynomial centred on the exact mean).

Tolerances (derived, not measured), with u = 2^-53, N = 5 * (segments of the window) summed terms, Y_i(x) = sum_k |c_k| x^k the
magnitude polynomial of element i (the bound of a Horner form), m_i the reference mean and <f> = (1/T) int f dt:
    |mean_i - ref|  <= K_mean u <Y_i>,                                             K_mean = 2 (N + 24)
    |cov_ij - ref|  <= K u <(Y_i + |m_i|)(Y_j + |m_j|)> + (K_mean u)^2 <Y_i> <Y_j>,  K      = 2 (2 N + 50)
K_mean: N - 1 additions of S, 8 operations of Horner, 8 u Y for the two roundings of the node x_g (x |p'| <= 4 Y), 6 for a
weight (h, xlo, xhi, u, h u, times w_g), the product and the division, N + 6 for Tsum: N + 24 with a factor 2 of headroom.
K: per factor v the 8 + 8 above and its subtraction (17, twice), 6 for the weight, 2 products, N for the sum in any order, N +
7 for Tsum and the division: 2 N + 49 <= 2 N + 50, doubled.  The mean's own error enters only through its square (deviations
from the exact mean integrate to zero).  `variance` takes the diagonal of the covariance bound."""
import ctypes
import types

import numpy as np
import pytest
import torch

import torchdiffeq_amd as tda
from torchdiffeq_amd import _native, rowwise_dense

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
SIGNS = [pytest.param(1.0, id="ascending"), pytest.param(-1.0, id="descending")]
LD = np.longdouble
U = LD(2.0) ** -53


def make_record(dtype, L, counts, sign, kernels=None, device="cpu", constant=False):
    """A record of len(counts) rows on the solver-time interval [0, 1], row r with counts[r] steps at random breakpoints and
    random coefficients of order 1 around 3 (`constant`: e a power of two per element, the other planes zero)."""
    g = torch.Generator().manual_seed(1000 * L + sum(counts) + int(sign))
    B, n_seg = len(counts), sum(counts)
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
    ta, tb = torch.empty(n_seg, dtype=F64), torch.empty(n_seg, dtype=F64)
    for r, n in enumerate(counts):
        cuts = torch.cat([torch.zeros(1, dtype=F64), torch.sort(0.05 + 0.9 * torch.rand(n - 1, generator=g, dtype=F64))[0],
                          torch.ones(1, dtype=F64)])
        ta[offsets[r]:offsets[r + 1]], tb[offsets[r]:offsets[r + 1]] = cuts[:-1], cuts[1:]
    coeffs = torch.randn(5, n_seg, L, generator=g, dtype=F64)
    coeffs[0] += 3.0
    if constant:
        coeffs[1:] = 0.0
        coeffs[0] = (2.0 ** torch.arange(L, dtype=F64).remainder(5)) * torch.where(torch.arange(L) % 2 == 0, 1.0, -1.0)
    p = types.SimpleNamespace(sign=sign, shape=(B, L), device=torch.device(device),
                              tgrid=torch.stack([torch.zeros(B, dtype=F64), torch.ones(B, dtype=F64)]))
    return rowwise_dense.RowDenseOutput(p, kernels, offsets.to(device), ta.to(device), tb.to(device),
                                        coeffs.to(dtype).to(device).contiguous())


def windows(dense):
    """True-time ends (qa, qb), each [5, B]: inside the first step, several steps with both ends partial, the same reversed,
    zero length, the whole interval."""
    off, B = dense.offsets.tolist(), dense._shape[0]
    first = torch.stack([dense._tb[off[r]].cpu() for r in range(B)])                  # (solver time; the first step starts at 0)
    lo, hi, one = torch.full((B,), 0.13, dtype=F64), torch.full((B,), 0.87, dtype=F64), torch.ones(B, dtype=F64)
    qa = torch.stack([0.25 * first, lo, hi, 0.4 * one, 0.0 * one])
    qb = torch.stack([0.75 * first, hi, lo, 0.4 * one, one])
    return qa * dense._sign, qb * dense._sign


def _moment(c1, c2, lo, hi):
    """int_lo^hi (sum_k c1[k] x^k)(sum_l c2[l] x^l) dx per pair of columns of c1 [5, L1], c2 [5, L2] -> [L1, L2]."""
    return sum(np.outer(c1[k], c2[l]) * ((hi ** (k + l + 1) - lo ** (k + l + 1)) / (k + l + 1)) for k in range(5) for l in range(5))


def reference(dense, qa, qb):
    """Per window (j, r) of the true-time ends [Q, B] -> {(j, r): (T, mean, cov, mean_tol, cov_tol)} in longdouble."""
    co, off = dense.coeffs.cpu().numpy().astype(LD), dense.offsets.tolist()
    ta, tb = dense._ta.cpu().numpy().astype(LD), dense._tb.cpu().numpy().astype(LD)
    one, out = np.ones((5, 1), dtype=LD) * (np.arange(5) == 0)[:, None], {}
    for j in range(qa.shape[0]):
        for r in range(qa.shape[1]):
            a, b = sorted((LD(float(qa[j, r]) * dense._sign), LD(float(qb[j, r]) * dense._sign)))
            sA, sB = (next(s for s in range(off[r], off[r + 1]) if t <= tb[s]) for t in (a, b))
            parts = [(co[:, s], tb[s] - ta[s], (a - ta[s]) / (tb[s] - ta[s]) if s == sA else LD(0),
                      (b - ta[s]) / (tb[s] - ta[s]) if s == sB else LD(1)) for s in range(sA, sB + 1)]
            T, N = b - a, 5 * len(parts)
            k_mean, k_cov = 2 * (N + 24), 2 * (2 * N + 50)
            if T == 0:
                c, _, x, _ = parts[0]
                pw = x ** np.arange(5)[:, None]
                out[j, r] = (T, (c * pw).sum(0), np.zeros((c.shape[1],) * 2, dtype=LD), k_mean * U * (np.abs(c) * pw).sum(0),
                             np.zeros((c.shape[1],) * 2, dtype=LD))
                continue
            mean = sum(h * _moment(c, one, lo, hi)[:, 0] for c, h, lo, hi in parts) / T
            size = sum(h * _moment(np.abs(c), one, lo, hi)[:, 0] for c, h, lo, hi in parts) / T
            cov, big = 0, 0
            for c, h, lo, hi in parts:
                centred, wide = c.copy(), np.abs(c)
                centred[0] -= mean
                wide[0] += np.abs(mean)
                cov, big = cov + h * _moment(centred, centred, lo, hi) / T, big + h * _moment(wide, wide, lo, hi) / T
            out[j, r] = (T, mean, cov, k_mean * U * size, k_cov * U * big + (k_mean * U) ** 2 * np.outer(size, size))
    return out


def check(got, ref, slack=1):
    """`got`: RowDenseTimeMoments with [Q, B, ...] fields (any device) against `reference`; the structure of the covariance."""
    dur, mean, var = (v.cpu().numpy() for v in got[:3])
    cov = None if got.covariance is None else got.covariance.cpu().numpy()
    for (j, r), (T, r_mean, r_cov, mean_tol, cov_tol) in ref.items():
        assert dur[j, r] == np.float64(T), ("duration", j, r)
        assert (np.abs(mean[j, r].astype(LD) - r_mean) <= slack * mean_tol).all(), ("mean", j, r)
        assert (np.abs(var[j, r].astype(LD) - np.diagonal(r_cov)) <= slack * np.diagonal(cov_tol)).all(), ("variance", j, r)
        assert (var[j, r] >= 0).all()
        if cov is not None:
            assert (np.abs(cov[j, r].astype(LD) - r_cov) <= slack * cov_tol).all(), ("covariance", j, r)
            assert np.array_equal(cov[j, r], cov[j, r].T) and np.array_equal(np.diagonal(cov[j, r]), var[j, r])


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_path_against_closed_form(dtype, sign):
    dense = make_record(dtype, 5, [1, 6, 3], sign)
    qa, qb = windows(dense)
    ref = reference(dense, qa, qb)
    plain, full = dense.time_moments(qa, qb), dense.time_moments(qa, qb, covariance=True)
    assert plain.covariance is None and full.covariance.shape == (5, 3, 5, 5) and full.covariance.dtype == F64
    assert plain.duration.shape == (5, 3) and plain.mean.shape == plain.variance.shape == (5, 3, 5)
    check(plain, ref)
    check(full, ref)
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], full[:3]))
    assert torch.equal(full.covariance[1], full.covariance[2]) and torch.equal(full.mean[1], full.mean[2])   # reversed ends
    assert bool((full.variance[3] == 0).all()) and bool((full.covariance[3] == 0).all()) and bool((full.duration[3] == 0).all())
    assert torch.equal(full.mean[3].to(dtype), dense.maximum(qa[3:4], qb[3:4]).values[0])     # p(xlo) in fp64
    # mean * duration is the integral over the window, ends ascending in true time
    lo, hi = torch.minimum(qa, qb), torch.maximum(qa, qb)
    area = dense.integral(lo, hi).double().numpy()
    eps = float(torch.finfo(dtype).eps)
    for (j, r), (T, _, _, mean_tol, _) in ref.items():
        tol = 2 * float(T) * mean_tol.astype(np.float64) + eps * np.abs(area[j, r])
        assert (np.abs((plain.mean[j, r] * plain.duration[j, r]).numpy() - area[j, r]) <= tol).all(), (j, r)
    one = dense.time_moments(float(qa[1, 0]), float(qb[1, 0]), covariance=True)
    assert one.duration.shape == (3,) and one.mean.shape == (3, 5) and one.covariance.shape == (3, 5, 5)
    assert torch.equal(one.covariance[0], full.covariance[1, 0])


def test_out_of_range_and_arguments():
    dense = make_record(F32, 3, [2, 2], 1.0)
    ok, out = torch.tensor([[0.2, 0.2]], dtype=F64), torch.tensor([[0.5, 1.5]], dtype=F64)         # [Q = 1, B = 2]
    with pytest.raises(ValueError, match=r"dense.time_moments\(ta, tb\): query 0 of row 1 \(tb = 1.5\)"):
        dense.time_moments(ok, out)
    with pytest.raises(ValueError, match=r"query 0 of row 1 \(ta = 1.5\)"):
        dense.time_moments(out, out)
    got = dense.time_moments(ok, out, covariance=True, check=False)
    assert all(bool(v[0, 1].isnan().all()) and not bool(v[0, 0].isnan().any()) for v in got)
    with pytest.raises(ValueError, match="covariance must be a bool"):
        dense.time_moments(0.1, 0.2, covariance=1)
    with pytest.raises(NotImplementedError, match="does not propagate gradients"):
        dense.time_moments(torch.tensor(0.1, requires_grad=True), 0.2)
    wide = make_record(F32, _native.TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN + 1, [1], 1.0)
    with pytest.raises(ValueError, match="covariance=True takes rows of at most 256 elements"):
        wide.time_moments(0.1, 0.2, covariance=True)
    assert wide.time_moments(0.1, 0.2).variance.shape == (1, 257)


def test_structure():
    assert "RowDenseTimeMoments" in tda.__all__ and "RowDenseTimeMoments" in rowwise_dense.__all__
    assert tda.RowDenseTimeMoments._fields == ("duration", "mean", "variance", "covariance")
    assert {"tdeq_row_dense_time_moments", "tdeq_row_dense_time_gram"} <= set(_native.ABI_SIGNATURES)
    lib = _native.load_library()
    assert lib.tdeq_abi_version() == _native.TDEQ_ABI_VERSION == 38 and _native.TDEQ_ROW_TIME_MOMENTS_MAX_COV_LEN == 256
    # refusals before any launch (no GPU needed): a NULL pointer, a time_sign other than +1 / -1, a row beyond the cap
    p = ctypes.addressof(ctypes.create_string_buffer(64))
    tail = lambda sign, L, dtype=0: (p, 1, p, p, sign, p, p, p, p, p, p, 1, L, dtype, None)       # noqa: E731
    assert lib.tdeq_row_dense_time_moments(None, p, p, *tail(1.0, 1)) == -1
    assert lib.tdeq_row_dense_time_gram(p, None, *tail(1.0, 1)) == -1
    assert lib.tdeq_row_dense_time_moments(p, p, p, *tail(2.0, 1)) == -1 and lib.tdeq_row_dense_time_gram(p, p, *tail(0.0, 1)) == -1
    assert lib.tdeq_row_dense_time_gram(p, p, *tail(1.0, 257)) == -1 and lib.tdeq_row_dense_time_gram(p, p, *tail(1.0, 1, 4)) == -1
    assert lib.tdeq_row_dense_time_gram(p, p, *tail(1.0, 0)) == 0 and lib.tdeq_row_dense_time_moments(p, p, p, *tail(1.0, 0)) == 0
