"""fp64 reference, derived bound and inputs for the skinny GEMM (csrc/kernels/skinny_gemm.hip,
ops/skinny.py): y[M, N] = x[M, K] . w[N, K]^T, bf16 in and out, fp32 inside.  Plain PyTorch on the CPU.

    |y - y64| <= BF16_O |y64| + e sum_k |x_k w_k|,    e = roundings(K) * 2^-24

The chain: x and w are bf16, so every product is exact in fp32.  A wave owns ceil(S / nw) of the S = K // 64
steps, two MFMAs each, and wave 0 one more MFMA where K % 64 == 32; an MFMA adds 32 products to the
accumulator, at most one fp32 rounding per added term (the assumption the issue states); wave 0 then adds the
nw - 1 other partials in order.  Longest path: 32 * (2 ceil(S / nw) + [K % 64 > 0]) + nw - 1 roundings, never
more than K, the any-order worst case.  Each rounding is relative to a partial sum, itself at most
sum_k |x_k w_k|.  The store rounds once to bf16: BF16_O |y64|.
"""
import functools

import torch

from llm_refs import BF16_O


def waves(K):
    """Waves per workgroup at this K: waves_for() of the kernel file (the GPU test checks the library's)."""
    return 16 if K >= 2048 else (8 if K >= 1024 else 4)


def roundings(K):
    nw, S = waves(K), K // 64
    return min(K, 32 * (2 * -(-S // nw) + (K % 64 > 0)) + nw - 1)


@functools.lru_cache(maxsize=None)
def inputs(M, K, N, seed=0):
    """bf16 x [M, K] ~ N(0, 1) and w [N, K] ~ N(0, 1 / K) from a seeded CPU generator.  Not to be modified."""
    g = torch.Generator(device="cpu").manual_seed(5000 + seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    return x, w


@functools.lru_cache(maxsize=None)
def linear_fp64(M, K, N, seed=0):
    """The reference of inputs(M, K, N): o = y64 and its bound b_o."""
    x, w = inputs(M, K, N, seed)
    y = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    return dict(o=y, b_o=BF16_O * y.abs() + roundings(K) * 2.0 ** -24 * mag)
