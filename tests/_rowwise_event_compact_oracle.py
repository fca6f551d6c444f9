"""Shared pieces of the `odeint_rowwise_event(compact=...)` tests: the event oracle extended by the two mapped entry
points, stated through the expressions it already has (`row_event_fit` / `row_event_eval` on gathered rows), the device
driver on it, and `decay_event_problem` with `func` and `event_fn` taking `rows`."""
import contextlib

import pytest
import torch

from _rowwise_event_oracle import METHODS, EventOracle, quiet  # noqa: F401

from torchdiffeq_amd import _native, rowwise


class EventCompactOracle(EventOracle):
    """The event oracle plus `row_event_fit_mapped` and `row_event_eval_mapped`."""

    def row_event_fit_mapped(self, q, row_map, fired_now, y0, y1, f0, f1, ks, coefs, dts) -> None:
        n = y0.shape[0]
        assert row_map.shape == fired_now.shape == dts.shape == (n,) and q.shape[0] == 5 and q.shape[2] == y0.shape[1]
        rows = row_map.to(torch.int64)
        assert int(rows.min()) >= 0 and int(rows.max()) < q.shape[1] and rows.unique().numel() == n
        tmp = q[:, rows].contiguous()                        # the compact view of q: row r of it is q[:, row_map[r]]
        self.row_event_fit(tmp, fired_now, y0, y1, f0, f1, ks, coefs, dts)
        now = fired_now != 0
        q[:, rows[now]] = tmp[:, now]                        # (the rows that did not fire are not written)

    def row_event_eval_mapped(self, out, dst_map, q, src_map, x) -> None:
        n = src_map.numel()
        if n == 0:
            return
        assert x.shape == (n,) and (dst_map is None or dst_map.shape == (n,))
        src = src_map.to(torch.int64)
        assert int(src.min()) >= 0 and int(src.max()) < q.shape[1]
        tmp = torch.empty(n, out.shape[1], dtype=out.dtype)
        self.row_event_eval(tmp, q[:, src].contiguous(), x, torch.ones(n, dtype=torch.int32))
        if dst_map is None:
            out[:n] = tmp
        else:
            out[dst_map.to(torch.int64)] = tmp


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_event_oracle.py's fixture with the extended oracle: inside `with device_driver():` a CPU state is
    solved by `HipRowKernels` on the oracle's row operations."""
    wrapped = EventCompactOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def decay_event_problem_rows(B, L, dtype, seed, device="cpu"):
    """`decay_event_problem` of tests/_rowwise_event_oracle.py — the same draws in the same order — with `func` and
    `event_fn` taking the original indices `rows` of the rows of a call; without `rows` (or with None) they are the
    two-argument problem, bit for bit.  -> (y0, func, event_fn, k, level)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(0, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None]
    q = torch.linspace(0.9, 0.2, B, dtype=torch.float64)[torch.randperm(B, generator=g)]
    y0 = 1 + torch.rand(B, L, generator=g, dtype=torch.float64)
    k, y0 = k.to(device, dtype), y0.to(device, dtype)
    level = (y0[:, 0] * q.to(device, dtype)).clone()

    def func(t, y, rows=None):
        return -(k if rows is None else k[rows]) * y * (1 + t)[:, None]

    def event_fn(t, y, rows=None):
        return y[:, 0] - (level if rows is None else level[rows])
    return y0, func, event_fn, k, level
