"""Shared pieces of the row-kernel tests (tests/test_rowwise_oracle.py, tests/test_rowwise_kernels_gpu.py): the per-row
vectors of a `RowState` on either device, and the row lengths that name every reduction geometry."""
import math

import numpy as np
import torch

from torchdiffeq_amd import _native

F64_VECTORS = ("t0", "tprev", "dt", "h0", "ratio")
I32_VECTORS = ("active", "accepted", "out_lo", "out_hi", "next_out", "since", "bad_y", "code")
I64_VECTORS = ("n_acc", "n_rej")
SENTINEL = -77.0


class RowVectors:
    """The vectors a `_native.RowState` points to, as tensors on `device`, built from CPU values (`init`: name -> list
    or tensor; what is not given starts as a recognisable non-zero filler, so a vector the kernel should not touch is
    seen to keep it)."""

    def __init__(self, device, B, L, tgrid, order=4, max_num_steps=2 ** 31 - 1, **init):
        self.B = B
        tgrid = torch.as_tensor(tgrid, dtype=torch.float64).reshape(-1, B).contiguous()
        self.v = {"tgrid": tgrid.to(device)}
        for names, dtype, filler in ((F64_VECTORS, torch.float64, -3.25), (I32_VECTORS, torch.int32, 0),
                                     (I64_VECTORS, torch.int64, 5)):
            for name in names:
                val = init.get(name)
                t = torch.full((B,), filler, dtype=dtype) if val is None else torch.as_tensor(val).to(dtype).reshape(B).clone()
                self.v[name] = t.to(device)
        self.v["status"] = torch.tensor([-1, -1], dtype=torch.int32).to(device)
        st = _native.RowState()
        for name, t in self.v.items():
            setattr(st, name, t.data_ptr())
        st.n_rows, st.row_len, st.max_num_steps = B, L, max_num_steps
        st.n_out, st.order = tgrid.shape[0], order
        self.st = st

    def cpu(self):
        return {name: t.cpu() for name, t in self.v.items()}


def ctrl_for(alpha, order, sign, np_dtype, safety=0.9, ifactor=10.0, dfactor=0.2):
    """The StepCtrl `HipRowKernels` builds: the abscissae rounded to T, no step bounds."""
    alpha_T = [np_dtype(a) for a in alpha]
    return _native.step_ctrl(alpha_T, [a == 1.0 for a in alpha], order, safety, ifactor, dfactor, 0.0, math.inf, sign,
                             n_norm_seg=1)


def lane_elems(dtype):
    return 4 if dtype == torch.float32 else 2


# nv (16-byte or scalar elements per row) of every geometry class: one lane per row, group growth, the 64-lane cap, the
# top of the short rows, the one-chunk long rows, the first two-chunk row, a chunk tail, and more than 64 partials
SHORT_NV = (1, 2, 3, 4, 5, 16, 17, 256, 257, 1023, 1024)
BAND_NV = (1025, 1500, 2048)
LONG_NV = (2049, 3 * 2048 + 1)
MANY_PARTIALS_NV = (64 * 2048 + 1, 127 * 2048 + 5)        # 65 and 128 partials per row


def row_lengths(dtype, nvs):
    """For each nv: the 16-byte-element L (nv * lanes) and the scalar L (nv itself, where it is no multiple of lanes)."""
    lv = lane_elems(dtype)
    out = []
    for nv in nvs:
        out.append(nv * lv)
        if nv % lv:
            out.append(nv)
    return sorted(set(out))


def seeded(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def np_type(dtype):
    return np.float32 if dtype == torch.float32 else np.float64
