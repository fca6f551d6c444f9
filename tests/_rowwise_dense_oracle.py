"""Shared pieces of the `odeint_rowwise_dense` tests: the event oracle extended by the three dense operations, stated in
torch from the text of include/tdeq_hip.h (slots in ascending row order, the pack as an indexed copy, the search as explicit
comparisons against every segment end of the row — no bisection, no searchsorted), the device driver on it, and the decay
problem with `rows` support."""
import contextlib

import pytest
import torch

from _rowwise_event_compact_oracle import METHODS, EventCompactOracle, quiet  # noqa: F401

from torchdiffeq_amd import _native, rowwise

NONE = 0x7FFFFFFF
LOW_ORDER = ("bosh3", "fehlberg2", "adaptive_heun")


class DenseOracle(EventCompactOracle):
    """The event oracle plus `row_dense_slots`, `row_dense_pack` and `row_dense_search`."""

    def row_dense_slots(self, st, row_map, cap, counter, slot_row, slot_ord, slot_ta, slot_tb, slot, mask) -> None:
        v = {name: torch.from_numpy(a) for name, a in self._inner._state_views(st).items()}
        n = int(st.n_rows)
        assert counter.shape == (2,) and slot.shape == mask.shape == (n,) and (row_map is None or row_map.shape == (n,))
        assert slot_row.shape == slot_ord.shape == slot_ta.shape == slot_tb.shape == (cap,)
        slot.fill_(-1)
        mask.zero_()
        for r in torch.nonzero(v["accepted"]).view(-1).tolist():          # ascending: one of the orders the kernel may take
            s = int(counter[0])
            counter[0] = s + 1
            if s >= cap:
                counter[1] = 1
                continue
            slot_row[s] = r if row_map is None else int(row_map[r])
            slot_ord[s] = int(v["n_acc"][r]) - 1
            slot_ta[s] = v["tprev"][r]
            slot_tb[s] = v["t0"][r]
            slot[r] = s
            mask[r] = 1

    def row_event_fit_mapped(self, q, row_map, fired_now, y0, y1, f0, f1, ks, coefs, dts) -> None:
        """The parent's operation on the rows with `fired_now` only: a dense solve passes the slots as `row_map`, and the
        rows without a slot hold -1 there (the kernel reads row_map[r] of the rows with fired_now[r] only)."""
        idx = torch.nonzero(fired_now).view(-1)
        if idx.numel() == 0:
            return
        super().row_event_fit_mapped(q, row_map[idx], fired_now[idx], y0[idx], y1[idx], f0[idx], f1[idx],
                                     [k[idx] for k in ks], coefs, dts[idx])

    @staticmethod
    def row_dense_pack(dst, src, dest, n_used) -> None:
        if n_used == 0:
            return
        assert dest.shape == (n_used,) and dest.dtype == torch.int64 and n_used <= src.shape[1]
        assert int(dest.min()) >= 0 and int(dest.max()) < dst.shape[1] and dest.unique().numel() == n_used
        dst[:, dest] = src[:, :n_used]

    @staticmethod
    def row_dense_search(tq, offsets, seg_ta, seg_tb, t0, t1, seg, x, status) -> None:
        Q, B = tq.shape
        n_seg = seg_ta.numel()
        for j in range(Q):
            for r in range(B):
                i, t = j * B + r, float(tq[j, r])
                lo, hi = int(offsets[r]), int(offsets[r + 1])
                if t >= float(t0[r]) and t <= float(t1[r]) and hi > lo:
                    hits = [s for s in range(lo, hi) if t <= float(seg_tb[s])]
                    s = hits[0] if hits else hi - 1
                    seg[i] = s
                    x[i] = ((tq[j, r] - seg_ta[s]) / (seg_tb[s] - seg_ta[s])).to(x.dtype)      # fp64 quotient, then T
                else:
                    seg[i] = min(lo, n_seg - 1)
                    x[i] = float("nan")
                    status[0] = min(int(status[0]), i)


@pytest.fixture()
def device_driver(monkeypatch, oracle_kernels):
    """tests/_rowwise_event_compact_oracle.py's fixture with the extended oracle: inside `with device_driver():` a CPU
    state is solved by `HipRowKernels` on the oracle's row operations (and the dense object it returns evaluates on them)."""
    wrapped = DenseOracle(oracle_kernels)

    @contextlib.contextmanager
    def patched():
        with monkeypatch.context() as m:
            m.setattr(_native, "get_kernels", lambda device, dtype=None: wrapped)
            m.setattr(rowwise, "HostRowKernels", rowwise.HipRowKernels)
            yield
    return patched


def decay_problem(B, L, dtype, seed, device="cpu"):
    """Rows y' = -k_r (1 + t) y with k_r from 1 to 30 in a shuffled order and y0 in (1, 2): elementwise, no transcendental
    (the same func bits on every backend); exact solution y0 exp(-k (t + t^2 / 2)).  `func(t, y, rows=None)` serves the
    calls with and without `compact`.  -> (y0, func, k [B, 1])."""
    g = torch.Generator().manual_seed(seed)
    k = torch.logspace(0, 1.5, B, dtype=torch.float64)[torch.randperm(B, generator=g)][:, None]
    y0 = 1 + torch.rand(B, L, generator=g, dtype=torch.float64)
    k, y0 = k.to(device, dtype), y0.to(device, dtype)

    def func(t, y, rows=None):
        return -(k if rows is None else k[rows]) * y * (1 + t)[:, None]
    return y0, func, k


def tolerances(method, dtype):
    """Settings that keep the step counts small (at the defaults fp64 adaptive_heun takes thousands of steps per row here)."""
    if method in LOW_ORDER:
        return dict(rtol=1e-3, atol=1e-5)
    return dict(rtol=1e-6, atol=1e-8) if dtype == torch.float32 else {}


def per_row_t1(B, device="cpu"):
    return torch.linspace(0.3, 0.6, B, dtype=torch.float64, device=device)


def random_queries(Q, t0, t1, seed):
    """[Q, B] fp64 times strictly inside (t0_r, t1_r), unsorted (t0, t1: fp64 [B] on any device)."""
    g = torch.Generator().manual_seed(seed)
    u = 0.02 + 0.96 * torch.rand(Q, t0.numel(), generator=g, dtype=torch.float64)
    return t0[None] + u.to(t0.device) * (t1 - t0)[None]


def grid_reference(solve, q, t0, t1):
    """`dense(q)` as `odeint_rowwise` gives it: `solve(grid)` on the per-row grid [t0, the distinct queries sorted in the
    direction of the solve, t1] -> [Q, B, ...], row (j, r) the grid solution of row r at q[j, r].  Queries equal to t0 or t1
    take the grid's ends."""
    Q, B = q.shape
    sign = 1.0 if bool((t1 > t0).all()) else -1.0
    cols, pos = [], torch.empty(Q, B, dtype=torch.int64)
    for r in range(B):
        inner = sorted({float(v) for v in q[:, r].tolist()} - {float(t0[r]), float(t1[r])}, key=lambda v: sign * v)
        col = [float(t0[r])] + inner + [float(t1[r])]
        cols.append(col)
        for j in range(Q):
            pos[j, r] = col.index(float(q[j, r]))
    T = max(len(c) for c in cols)
    # rows with fewer distinct queries: pad with extra interior times just before t1 (they change no step sequence)
    grid = torch.empty(T, B, dtype=torch.float64)
    for r, col in enumerate(cols):
        pad = T - len(col)
        last, end = col[-2], col[-1]
        extra = [last + (end - last) * (i + 1) / (pad + 1) for i in range(pad)]
        full = col[:-1] + extra + [end]
        grid[:, r] = torch.tensor(full, dtype=torch.float64)
        pos[:, r] = torch.where(pos[:, r] == len(col) - 1, torch.tensor(T - 1), pos[:, r])
    ref = solve(grid.to(t0.device))
    idx = pos.to(ref.device)
    return torch.gather(ref, 0, idx.view(Q, B, *([1] * (ref.dim() - 2))).expand(Q, B, *ref.shape[2:]))
