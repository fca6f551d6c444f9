"""Shared pieces of the per-row tolerance tests of `odeint_rowwise` (rtol / atol as [B] vectors): the CPU row oracle
extended by `row_reduce_tol`, the device driver on it, and the mixed-tolerance problem.

`row_reduce_tol` is stated through what the oracle already has: the inner `row_reduce` on each one-row slice with that
row's two tolerances as floats, written into that row's slot of `part`."""
import contextlib

import pytest
import torch

from _rowwise_compact_oracle import CompactOracle, quiet, random_problem  # noqa: F401

from torchdiffeq_amd import _native, rowwise


class TolOracle(CompactOracle):
    """The compaction oracle (`row_gather`, `row_dense_commit_mapped`) plus `row_reduce_tol`."""

    def row_reduce_tol(self, mode, part, y0, y1, partial, ks, coefs, dts, active, rtol_rows, atol_rows) -> None:
        B, L = y0.shape
        assert rtol_rows.shape == atol_rows.shape == (B,) and rtol_rows.dtype == atol_rows.dtype == y0.dtype
        nch = self._inner.row_partials(L, y0.dtype)
        out = part.view(-1)[:3 * B * nch].view(3, B, nch)
        one = torch.empty(3 * nch, dtype=torch.float64)
        for r in range(B):
            row = slice(r, r + 1)
            self._inner.row_reduce(mode, one, y0[row], y1[row], None if partial is None else partial[row],
                                   [k[row] for k in ks], coefs, None if dts is None else dts[row],
                                   None if active is None else active[row], float(rtol_rows[r]), float(atol_rows[r]))
            out[:, r, :] = one.view(3, nch)


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_compact_oracle.py's fixture with the extended oracle: inside `with device_driver():` a CPU state is
    solved by `HipRowKernels` on the oracle's row operations."""
    wrapped = TolOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


MIXED_B, MIXED_L = 12, 5


def mixed_tolerances(dtype, B=MIXED_B):
    """Per-row tolerances over six (fp64) or three (fp32) decades, in a seeded order unrelated to the rows' stiffness:
    (rtol [B], atol [B]) as fp64 CPU tensors."""
    lo, hi = (-3, -9) if dtype == torch.float64 else (-2, -5)
    g = torch.Generator().manual_seed(11)
    rtol = torch.logspace(lo, hi, B, dtype=torch.float64)[torch.randperm(B, generator=g)]
    return rtol, rtol * 1e-2


def mixed_problem(dtype, device="cpu"):
    """-> (y0 [12, 5], t [4], rtol [12], atol [12], plain func, func taking `rows`, maker of a subset's plain func)."""
    y0, plain, by_rows, subset = random_problem(MIXED_B, MIXED_L, dtype, 3, device)
    t = torch.linspace(0, 1.5, 4, dtype=torch.float64)
    rtol, atol = mixed_tolerances(dtype)
    return y0, t, rtol, atol, plain, by_rows, subset
