"""`RowDenseOutput.autocovariance` on the MI355X: `row_dense_time_lagged` and `row_dense_time_lagged_gram` on the hand-made
dyadic records, windows and lags of test_rowwise_dense_autocovariance.py against its closed-form longdouble reference and
bound (K = 2 (2 N + 219), N = 5 * pieces), and against the host path: the same bits where the contract is the arithmetic
(`duration`, `mean`, the walk kernel's `autocovariance`), twice the bound where it is an error bound (the matrix instruction's
sums)."""
import numpy as np
import pytest
import torch

from test_rowwise_dense_autocovariance import LAGS, check, make_record, reference, windows
from test_rowwise_dense_level_gpu import _on_host
from test_rowwise_dense_time_moments import DTYPES

from torchdiffeq_amd import rowwise_dense

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
COUNTS = [1, 5, 6, 7, 12]                # B = 5: four windows of a TW = 16 workgroup and a remainder; 4 k .. 4 k + 3 pieces


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


def _ask(dense, qa, qb, **kw):
    return dense.autocovariance(qa.to(DEV), qb.to(DEV), LAGS.to(DEV), check=False, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 3, 4, 16, 17, 80])
def test_kernels_against_closed_form_and_host(hip_kernels, L, dtype, monkeypatch):
    """L = 1, 3: the scalar lane, TW = 16 with padded columns; 4: one 16-byte lane of fp32; 16, 17: both sides of the TW = 16 /
    TW = 64 switch, a partial tile; 80: two tiles, so both off-diagonal block pairs (0, 1) and (1, 0) exist and differ."""
    dense = make_record(dtype, L, COUNTS, 1.0, hip_kernels, DEV)
    qa, qb = windows(dense)
    C, tol = reference(dense, qa, qb, LAGS[:, None].expand(-1, len(COUNTS)).numpy())
    plain, full = _ask(dense, qa, qb), _ask(dense, qa, qb, covariance=True)
    assert full.covariance.device.type == DEV.type and full.covariance.shape == (5, 5, len(COUNTS), L, L)
    check(plain, C, tol)
    check(full, C, tol)                                                           # (the NaN pattern and the diagonal rule too)
    host = _on_host(dense)
    host_plain, host_full = (host.autocovariance(qa, qb, LAGS, check=False, covariance=c) for c in (False, True))
    assert all(_bits(a, b) for a, b in zip(plain[:3], host_plain[:3]))
    assert all(_bits(a, b) for a, b in zip(full[:2], host_full[:2]))
    gap = np.abs(full.covariance.cpu().numpy().astype(np.longdouble) - host_full.covariance.numpy())
    assert (np.isnan(C) | (gap <= 2 * tol)).all()
    assert _bits(full.covariance[:, 1], full.covariance[:, 2])                    # reversed ends
    assert all(_bits(a, b) for a, b in zip(full, _ask(dense, qa, qb, covariance=True)))                   # a second call
    monkeypatch.setattr(rowwise_dense, "MOMENTS_WORKSPACE_BYTES", 1)              # one lag and query time per launch
    assert all(_bits(a, b) for a, b in zip(full, _ask(dense, qa, qb, covariance=True)))
    # the scalar form on a record one element off a 16-byte boundary: the bits of the 16-byte form
    flat = torch.empty(dense.coeffs.numel() + 1, dtype=dtype, device=DEV)
    twin = make_record(dtype, L, COUNTS, 1.0, hip_kernels, DEV)
    twin.coeffs = flat[1:].view_as(dense.coeffs).copy_(dense.coeffs)
    assert twin.coeffs.data_ptr() % 16 != 0
    assert all(_bits(a, b) for a, b in zip(plain[:3], _ask(twin, qa, qb)[:3]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [3, 80])
def test_descending_and_out_of_range(hip_kernels, L, dtype):
    """A descending solve against the true-time reference; `check=True` names an out-of-range end; `check=False` gives that
    row NaN and leaves the others their bits."""
    dense = make_record(dtype, L, COUNTS, -1.0, hip_kernels, DEV)
    qa, qb = windows(dense)
    C, tol = reference(dense, qa, qb, LAGS[:, None].expand(-1, len(COUNTS)).numpy())
    full = _ask(dense, qa, qb, covariance=True)
    check(full, C, tol)
    qb[1, 2] = 0.5                                                               # (true time of a descending solve: <= 0)
    with pytest.raises(ValueError, match=r"dense.autocovariance\(ta, tb, lags\): query 1 of row 2 \(tb = 0.5\)"):
        dense.autocovariance(qa.to(DEV), qb.to(DEV), LAGS[:1].to(DEV))
    nan = _ask(dense, qa, qb, covariance=True)
    keep = torch.ones(5, len(COUNTS), dtype=torch.bool)
    keep[1, 2] = False
    assert all(bool(v[1, 2].isnan().all()) and _bits(v[keep], w[keep]) for v, w in zip(nan[:2], full[:2]))
    assert all(bool(v[:, 1, 2].isnan().all()) and _bits(v[:, keep], w[:, keep]) for v, w in zip(nan[2:], full[2:]))
