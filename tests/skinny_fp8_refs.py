"""fp64 reference, derived bound and inputs for the FP8-weight skinny GEMM (csrc/kernels/skinny_gemm_fp8.hip,
ops/skinny.py): y[M, N] = (x[M, K] . q[N, K]^T) * scale[N], x bf16, q e4m3, scale a power of two, fp32 inside,
bf16 out.  Plain PyTorch on the CPU.

    |y - y64| <= BF16_O |y64| + e scale sum_k |x_k q_k|,    e = roundings(K) * 2^-24

The chain: e4m3 -> bf16 is exact, so every product is exact in fp32, and the multiply by the scale is exact.  A
wave owns at most ceil(S / nw) of the S = K // 128 steps, four MFMAs each, and wave 0 two more MFMAs where
K % 128 == 64; an MFMA adds 32 products to the accumulator, at most one fp32 rounding per added term; wave 0 then
adds the nw - 1 other partials in order.  Longest path: 32 * (4 ceil(S / nw) + 2 [K % 128 > 0]) + nw - 1
roundings, never more than K, the any-order worst case.  Each rounding is relative to a partial sum, itself at
most sum_k |x_k q_k|.  The store rounds once to bf16: BF16_O |y64|.
"""
import functools

import torch

from llm_refs import BF16_O


def waves(K):
    """Waves per workgroup at this K: waves_for() of the kernel file (the GPU test checks the library's)."""
    return 16 if K >= 2048 else (8 if K >= 1024 else 4)


def roundings(K):
    nw, S = waves(K), K // 128
    return min(K, 32 * (4 * -(-S // nw) + 2 * (K % 128 > 0)) + nw - 1)


@functools.lru_cache(maxsize=None)
def inputs(M, K, N, seed=0):
    """bf16 x [M, K] ~ N(0, 1); w [N, K] ~ N(0, 1 / K) times a row gain 4^(n % 4), so that neighbouring rows
    carry different scales; (q, scale) = quantize_rows(w).  Seeded CPU generator.  Not to be modified."""
    from pytorch_operator_amd.ops.skinny import quantize_rows
    g = torch.Generator(device="cpu").manual_seed(6000 + seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) / K ** 0.5 * (4.0 ** (torch.arange(N) % 4))[:, None]
    q, scale = quantize_rows(w)
    return x, w, q, scale


@functools.lru_cache(maxsize=None)
def linear_fp64(M, K, N, seed=0):
    """The reference of inputs(M, K, N): o = y64 and its bound b_o."""
    x, _, q, scale = inputs(M, K, N, seed)
    s = scale.double()[None, :]
    y = s * (x.double() @ q.double().t())
    mag = s * (x.double().abs() @ q.double().abs().t())
    return dict(o=y, b_o=BF16_O * y.abs() + roundings(K) * 2.0 ** -24 * mag)
