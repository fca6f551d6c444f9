"""Shared pieces of the bfloat16 / float16 kernel tests (tests/test_lowp_kernels_gpu.py): inputs, device placement at
aligned and unaligned offsets, the bit-for-bit comparison, sentinel-bordered output windows.  No test in here."""
import math

import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
COEFS = (0.0371, -0.211, 0.5, 1.25, -0.0625, 0.33, 0.9, -0.7, 0.0123, 2.5, -1.0, 0.125, 0.77, -0.31)
SENTINEL_BITS = 0x7FA5      # a NaN with a payload in both types: no kernel result has these bits (a kernel's own NaN is 0x7FC0 / 0x7E00)
PAD = 64


def kernels(dtype):
    from torchdiffeq_amd import _lowp, _native
    k = _native.get_kernels(torch.device("cuda:0"), dtype)
    assert isinstance(k, _lowp.LowPrecisionHipKernels) and k.name == "hip-low"
    return k


def to_type(x, dtype):
    """A host number as a 0-dim tensor of `dtype` holds it (fp64 -> the type)."""
    return torch.tensor(float(x), dtype=torch.float64).to(dtype)


def draw(n, seed, dtype, count, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn(n, generator=g, dtype=torch.float64)).to(dtype) for _ in range(count)]


def draw_edge(n, seed, dtype, count):
    """`count` tensors of the values at which a 16-bit kernel can round differently from ATen.  The kind of value is
    chosen per POSITION, for all tensors alike, so that sums and products of them stay in that range:
      0  ordinary (randn),
      1  magnitudes 2^-24 .. 2^-14 — the float16 subnormal range (normal numbers for bfloat16),
      2  a quarter of the type's largest value up to that value: products and sums overflow to inf,
      3  per tensor one of +0, -0, +inf, -inf, NaN or an ordinary value.
    bfloat16 subnormals (= float32 subnormals, below 2^-126) are out of scope: products and squares of the magnitudes
    above stay far from them."""
    g = torch.Generator().manual_seed(seed)
    kind = (torch.arange(n) + seed) % 4
    big = float(torch.finfo(dtype).max)
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan], dtype=torch.float64)
    out = []
    for _ in range(count):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        sgn = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
        tiny = sgn * torch.exp2(-24.0 + 10.0 * torch.rand(n, generator=g, dtype=torch.float64))
        large = sgn * big * (0.25 + 0.75 * torch.rand(n, generator=g, dtype=torch.float64))
        pick = torch.randint(0, 8, (n,), generator=g)
        spec = torch.where(pick < 5, special[pick.clamp(max=4)], x)
        v = torch.where(kind == 1, tiny, torch.where(kind == 2, large, torch.where(kind == 3, spec, x)))
        out.append(v.to(dtype))
    return out


def dev(ts, offset=0):
    """On the GPU; offset > 0: a view that starts `offset` elements into its buffer (not 16-byte aligned)."""
    out = []
    for t in ts:
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
        buf[offset:].copy_(t)
        out.append(buf[offset:])
    return out


def same(got, ref_cpu, what=""):
    """Bit-identical where the oracle's value is finite or infinite (the sign of a zero included); where it is NaN the
    kernel's must be NaN too — the payload is not compared (csrc/tdeq_kernels_lp.hpp claims bit identity for finite
    inputs and inf only)."""
    got = got.cpu()
    assert got.dtype == ref_cpu.dtype and got.shape == ref_cpu.shape, what
    nan_got, nan_ref = torch.isnan(got), torch.isnan(ref_cpu)
    assert torch.equal(nan_got, nan_ref), (what, "NaN at other positions", int((nan_got != nan_ref).sum()))
    diff = (got.view(torch.int16) != ref_cpu.view(torch.int16)) & ~nan_ref
    assert not bool(diff.any()), (what, int(diff.sum()), int(diff.nonzero()[0]))


def bits(t):
    return t.view(torch.int16)


class Window:
    """An output tensor of `n` elements carved out of a larger allocation filled with a sentinel bit pattern, starting
    `offset` elements past a 16-byte boundary."""

    def __init__(self, n, dtype, offset, rows=1):
        self.big = torch.full((PAD + offset + rows * n + PAD,), SENTINEL_BITS, dtype=torch.int16, device="cuda").view(dtype)
        self.lo, self.hi = PAD + offset, PAD + offset + rows * n
        assert self.big.data_ptr() % 16 == 0 and PAD % 8 == 0
        self.t = self.big[self.lo:self.hi]
        if rows > 1:
            self.t = self.t.view(rows, n)

    def intact(self):
        b = bits(self.big)
        return bool((b[:self.lo] == SENTINEL_BITS).all()) and bool((b[self.hi:] == SENTINEL_BITS).all())

    def written(self):
        return not bool((bits(self.big)[self.lo:self.hi] == SENTINEL_BITS).any())
