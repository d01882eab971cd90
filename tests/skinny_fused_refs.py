"""Inputs, fp64 references and derived bounds for the skinny GEMMs with the residual add and RMSNorm folded in
(csrc/kernels/skinny_gemm_fused.hip, ops/skinny.py).  Plain PyTorch on the CPU.  u = 2^-24 (one fp32 rounding).

Residual epilogue.  h and a have no bound: they are bits (resid + d and its product with gamma, d the plain
GEMM's output).  ss[m][t] sums 16 squares of fp32 values hf: every square is rounded (u), then a square passes
through at most 3 additions inside its lane and 3 across the lane groups, 15 additions in all, each rounding a
partial sum of non-negative terms:

    |ss - ss64| <= ((1 + u)^7 - 1) ss64

Row-scale epilogue.  y = bf16(rstd32 * acc), acc the plain GEMM's fp32 accumulator of a . W^T (times the e4m3
scale: exact).  skinny_refs' chain bounds |acc - acc64| <= e(K) sum_k |a_k w_k|, and every term of it is scaled
by rstd.  rstd32 = rsqrtf(sum_t ss_t / K + eps): the K / 16 non-negative partials are added in CHAINS = 16
chains of n = ceil(K / 256) terms in ascending order (n - 1 roundings: the first add to zero is exact), the
chains in order (15), then one division and one addition, (n + 16) u relative in all on the argument, which
the inverse square root halves; rsqrtf itself is within 1 ulp (HIP's documented accuracy), 2 u relative.  The
product rstd32 * acc rounds once more (u), the store once to bf16:

    |y - y64| <= BF16_O |y64| + rstd64 e(K) sum_k |a_k w_k| + ((n + 16) / 2 + 3) u |y64|

Chain (residual epilogue into row-scale epilogue, against fp64 add + RMSNorm + linear of the original inputs).
Beside the row-scale bound with a64 = h64 g in place of a, the operand is rounded once to bf16 (and its product
h g once in fp32), and h itself carries the first GEMM's error b_d (skinny_refs' bound: d is rounded to bf16
as the plain kernel stores it), which reaches y through the operand and through rstd (d rstd / rstd =
-sum h dh / sum h^2):

    + (BF16_O + u) rstd64 sum_k |h_k g_k w_k| + rstd64 sum_k b_d,k |g_k w_k| + |y64| sum_k |h_k| b_d,k / sum_k h_k^2
"""
import functools

import torch

import skinny_fp8_refs
import skinny_refs
from llm_refs import BF16_O

U = 2.0 ** -24
CHAINS = 16       # the GPU test checks it against the library
EPS = 1e-5
# (K, N): one tile and one ss column, 4 partials per row as the consumer's K; 5 tiles (e4m3: a ragged last
# workgroup at 2 and 4 tiles per wave); 8 waves, the e4m3 half step, 68 partials; 16 waves, 17 tiles, 128
# partials; bf16 weights alone: their half step.  K = 224 is outside the e4m3 kernels' K % 64 == 0: that format
# takes its own tests' 192 (a step and the half step) for the same 5 tiles.
SHAPES = {"bf16": [(64, 16), (224, 80), (1088, 48), (2048, 272), (1056, 48)],
          "e4m3": [(64, 16), (192, 80), (1088, 48), (2048, 272)]}
CASES = [(f, K, N) for f in SHAPES for K, N in SHAPES[f]]


@functools.lru_cache(maxsize=None)
def gemm(fmt, M, K, N, seed=0):
    """(x bf16 [M, K], the weight arguments of the wrappers -- (w,) or (q, scale) --, the weight as fp64 [N, K],
    e(K)) from skinny_refs.inputs / skinny_fp8_refs.inputs.  Not to be modified."""
    if fmt == "bf16":
        x, w = skinny_refs.inputs(M, K, N, seed)
        return x, (w,), w.double(), skinny_refs.roundings(K) * U
    x, _, q, scale = skinny_fp8_refs.inputs(M, K, N, seed)
    return x, (q, scale), q.double() * scale.double()[:, None], skinny_fp8_refs.roundings(K) * U


@functools.lru_cache(maxsize=None)
def extras(M, N, seed=0):
    """resid fp32 [M, N] ~ N(0, 1) and gamma fp32 [N] ~ 1 + 0.1 N(0, 1), seeded.  Not to be modified."""
    g = torch.Generator(device="cpu").manual_seed(7000 + seed)
    return torch.randn(M, N, generator=g), 1 + 0.1 * torch.randn(N, generator=g)


def tile_sums(h):
    return h.reshape(*h.shape[:-1], -1, 16).pow(2).sum(-1)


def add_norm_ref(d, resid, gamma):
    """From the plain GEMM's output d (bf16) and resid in the stream's dtype: h and a as PyTorch rounds them, and
    the fp64 ss of the fp32 sums hf with its bound."""
    hf = resid.float() + d.float()
    ss = tile_sums(hf.double())
    return hf.to(resid.dtype), (hf * gamma).to(torch.bfloat16), dict(o=ss, b_o=((1 + U) ** 7 - 1) * ss)


def rstd_terms(K):
    return (-(-K // (16 * CHAINS)) + CHAINS) / 2 + 3


def scaled_ref(a, w64, e, ss, eps=EPS):
    """fp64 rsqrt(sum ss / K + eps) * (a . w^T) from the same a, ss and weights, and its bound."""
    K = a.shape[-1]
    rstd = torch.rsqrt(ss.double().sum(-1, keepdim=True) / K + eps)
    y = rstd * (a.double() @ w64.t())
    mag = a.double().abs() @ w64.abs().t()
    return dict(o=y, b_o=BF16_O * y.abs() + rstd * e * mag + rstd_terms(K) * U * y.abs())


def chain_ref(x, wp64, ep, resid, gamma, wc64, ec, eps=EPS):
    """fp64 add + RMSNorm + linear of the original inputs: h = resid + x . wp^T, y = norm(h) gamma . wc^T."""
    N = wp64.shape[0]
    d = x.double() @ wp64.t()
    b_d = BF16_O * d.abs() + ep * (x.double().abs() @ wp64.abs().t())
    h = resid.double() + d
    rstd = torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    gw = gamma.double()[:, None] * wc64.t()                                  # [N, Nc]
    y = rstd * (h @ gw)
    mag = h.abs() @ gw.abs()
    b = BF16_O * y.abs() + rstd * ec * mag + rstd_terms(N) * U * y.abs()
    b = b + (BF16_O + U) * rstd * mag + rstd * (b_d @ gw.abs()) + y.abs() * (h.abs() * b_d).sum(-1, keepdim=True) \
        / h.pow(2).sum(-1, keepdim=True)
    return dict(o=y, b_o=b)
