"""fp64 reference, derived bound and inputs for the MXFP4-weight skinny GEMM (csrc/kernels/skinny_gemm_fp4.hip,
ops/skinny.py): y[M, N] = x[M, K] . w[N, K]^T, x bf16, w = dequantize_rows_fp4(q, scale), fp32 inside, bf16 out.
Plain PyTorch on the CPU.

    |y - y64| <= BF16_O |y64| + e sum_k |x_k w_k|,    e = roundings(K) * 2^-24

The chain: an e2m1 code times its block's power of two is exact in bf16 (the conversion applies the scale), so
every product is exact in fp32.  A wave owns at most ceil(S / nw) of the S = K // 256 steps, eight MFMAs each, and
wave 0 four more MFMAs where K % 256 == 128; an MFMA adds 32 products to the accumulator, at most one fp32 rounding
per added term; wave 0 then adds the nw - 1 other partials in order.  Longest path:
32 * (8 ceil(S / nw) + 4 [K % 256 > 0]) + nw - 1 roundings, never more than K, the any-order worst case.  Each
rounding is relative to a partial sum, itself at most sum_k |x_k w_k|.  The store rounds once to bf16: BF16_O |y64|.
"""
import functools

import torch

from llm_refs import BF16_O


def waves(K):
    """Waves per workgroup at this K: waves_for() of the kernel file (the GPU test checks the library's)."""
    return 16 if K >= 2048 else (8 if K >= 1024 else 4)


def roundings(K):
    nw, S = waves(K), K // 256
    return min(K, 32 * (8 * -(-S // nw) + 4 * (K % 256 > 0)) + nw - 1)


@functools.lru_cache(maxsize=None)
def inputs(M, K, N, seed=0):
    """bf16 x [M, K] ~ N(0, 1); w [N, K] ~ N(0, 1 / K) times a gain 4^((n + 3 block) % 5 - 2) per row n and 32-block
    along K, so that neighbouring rows and neighbouring blocks carry different exponents; (q, scale) =
    quantize_rows_fp4(w).  Seeded CPU generator.  Not to be modified."""
    from pytorch_operator_amd.ops.skinny import quantize_rows_fp4
    g = torch.Generator(device="cpu").manual_seed(7000 + seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    gain = 4.0 ** ((torch.arange(N)[:, None] + 3 * torch.arange(K // 32)[None, :]) % 5 - 2)
    w = torch.randn(N, K, generator=g) / K ** 0.5 * gain.repeat_interleave(32, dim=1)
    q, scale = quantize_rows_fp4(w)
    return x, w, q, scale


@functools.lru_cache(maxsize=None)
def linear_fp64(M, K, N, seed=0):
    """The reference of inputs(M, K, N): o = y64 and its bound b_o."""
    from pytorch_operator_amd.ops.skinny import dequantize_rows_fp4
    x, _, q, scale = inputs(M, K, N, seed)
    w = dequantize_rows_fp4(q, scale, torch.float64)
    y = x.double() @ w.t()
    mag = x.double().abs() @ w.abs().t()
    return dict(o=y, b_o=BF16_O * y.abs() + roundings(K) * 2.0 ** -24 * mag)
