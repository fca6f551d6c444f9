"""`RowDenseOutput.time_moments` on the MI355X: `row_dense_time_moments` and `row_dense_time_gram` on hand-made records against
the closed-form longdouble reference and the bound of test_rowwise_dense_time_moments.py (K_mean = 2 (N + 24), K = 2 (2 N +
50), N = 5 * segments of the window), and against the host path: the same bits where the contract is the arithmetic
(`duration`, `mean`, the walk kernel's `variance`), twice the bound where it is an error bound (the matrix instruction's sums)."""
import numpy as np
import pytest
import torch

from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_time_moments import DTYPES, F64, check, make_record, reference, windows

from torchdiffeq_amd import rowwise_dense

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
COUNTS = [1, 5, 6, 7, 12]                                    # one step next to 4 k + 1, 4 k + 2, 4 k + 3 and whole stages


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 3, 16, 17, 64, 80])
def test_kernels_against_closed_form_and_host(hip_kernels, L, dtype, monkeypatch):
    """L = 1, 3, 16: a wave per window, padded columns; 17, 64: one 64-element block and both sides of the 16-wide instruction
    tile; 80: a second block, the off-diagonal pair and the mirror."""
    dense = make_record(dtype, L, COUNTS, 1.0, hip_kernels, DEV)
    qa, qb = windows(dense)
    ref = reference(dense, qa, qb)
    plain = dense.time_moments(qa.to(DEV), qb.to(DEV))
    full = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True)
    assert full.covariance.device.type == DEV.type and full.covariance.shape == (5, len(COUNTS), L, L)
    check(plain, ref)
    check(full, ref)                                                              # (symmetry and the diagonal rule too)
    host = _on_host(dense).time_moments(qa, qb, covariance=True)
    assert all(_bits(a, b) for a, b in zip(plain[:3], host[:3])) and _bits(full.mean, host.mean)
    check(host, ref)
    for (j, r), (_, _, _, _, cov_tol) in ref.items():
        gap = np.abs(full.covariance[j, r].cpu().numpy().astype(np.longdouble) - host.covariance[j, r].numpy())
        assert (gap <= 2 * cov_tol).all(), (j, r)
    assert _bits(full.covariance[1], full.covariance[2]) and _bits(full.variance[1], full.variance[2])    # reversed ends
    assert not bool(full.covariance[3].any()) and not bool(full.variance[3].any())                        # zero length
    again = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True)
    assert all(_bits(a, b) for a, b in zip(full, again))
    monkeypatch.setattr(rowwise_dense, "MOMENTS_WORKSPACE_BYTES", 1)              # one query time per launch
    sliced = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True)
    assert all(_bits(a, b) for a, b in zip(full, sliced))
    # the scalar form on a record one element off a 16-byte boundary: the bits of the 16-byte form
    flat = torch.empty(dense.coeffs.numel() + 1, dtype=dtype, device=DEV)
    twin = make_record(dtype, L, COUNTS, 1.0, hip_kernels, DEV)
    twin.coeffs = flat[1:].view_as(dense.coeffs).copy_(dense.coeffs)
    assert twin.coeffs.data_ptr() % 16 != 0
    assert all(_bits(a, b) for a, b in zip(plain[:3], twin.time_moments(qa.to(DEV), qb.to(DEV))[:3]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [3, 80])
def test_descending_and_out_of_range(hip_kernels, L, dtype):
    """A descending solve against the reference; `check=False` gives NaN rows and leaves the others their bits; `check=True`
    names the query."""
    dense = make_record(dtype, L, COUNTS, -1.0, hip_kernels, DEV)
    qa, qb = windows(dense)
    full = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True)
    check(full, reference(dense, qa, qb))
    qb[1, 2] = 0.5                                                               # (true time of a descending solve: <= 0)
    with pytest.raises(ValueError, match=r"dense.time_moments\(ta, tb\): query 1 of row 2 \(tb = 0.5\)"):
        dense.time_moments(qa.to(DEV), qb.to(DEV))
    nan = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True, check=False)
    keep = torch.ones(5, len(COUNTS), dtype=torch.bool)
    keep[1, 2] = False
    assert all(bool(v[1, 2].isnan().all()) and _bits(v[keep], w[keep]) for v, w in zip(nan, full))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [3, 80])
def test_constant_record(hip_kernels, L, dtype):
    """Planes d .. a zero and e a signed power of two (every W_g e is then exact, so S = e Tsum): mean exactly e, variance and
    covariance exactly 0."""
    dense = make_record(dtype, L, COUNTS, 1.0, hip_kernels, DEV, constant=True)
    qa, qb = windows(dense)
    got = dense.time_moments(qa.to(DEV), qb.to(DEV), covariance=True)
    e = dense.coeffs[0, dense.offsets[:-1]].to(F64)
    assert _bits(got.mean, e.expand(5, -1, -1).contiguous()) and not bool(got.variance.any()) and not bool(got.covariance.any())
    assert not bool(dense.time_moments(qa.to(DEV), qb.to(DEV)).variance.any())
