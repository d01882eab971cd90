"""Skinny bf16 GEMM (``csrc/kernels/skinny_gemm.hip``): the projections of a decode step, where the
"batch" of the GEMM is the B <= 16 sequences being continued and the operation streams the weights.

``linear_rows(x, w, swiglu=False)``: ``x`` [..., K] with at most ``MAX_ROWS`` rows in all, ``w`` [N, K]
as ``nn.Linear`` holds it (neither copied nor transposed) -> ``F.linear(x, w)`` [..., N] in bf16 with fp32
accumulation; with ``swiglu``, ``w`` is the packed [W1 | W3] of ``FeedForward.w13`` and the result is
``swiglu_packed(F.linear(x, w))`` [..., N / 2] from one launch, bit for bit what the two launches give.
Inference only.  On a GPU the HIP kernel runs, and a shape or dtype outside its contract
(``hip_supported``) is a ``ValueError``, never a silent fallback; on CPU the same math runs in PyTorch.

``quantize_rows`` / ``linear_rows_fp8(x, q, scale, swiglu=False, tiles=0)``: the same on e4m3 weights with a
power-of-two scale per output row (``csrc/kernels/skinny_gemm_fp8.hip``), under the same rules; see below.

``quantize_rows_fp4`` / ``linear_rows_fp4(x, q, scale, swiglu=False, tiles=0)``: the same on OCP MXFP4 weights, e2m1
codes with an e8m0 scale per 32 along K (``csrc/kernels/skinny_gemm_fp4.hip``), under the same rules; see below.

``linear_rows_add_norm`` / ``linear_rows_scaled`` and their ``_fp8`` forms: the decode step's residual add and
RMSNorm folded into the projections around them (``csrc/kernels/skinny_gemm_fused.hip``); see the end of the file.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from . import _native
from .llm import _aligned, _stream, swiglu_packed_reference


@functools.lru_cache(maxsize=None)
def max_rows() -> int:
    """The most rows of ``x`` the kernel takes (``MAX_ROWS``), read from the library."""
    return int(_native.load().pto_skinny_max_rows())


def __getattr__(name):
    if name == "MAX_ROWS":
        return max_rows()
    raise AttributeError(name)


def _rows(x: torch.Tensor) -> int:
    return x.numel() // x.shape[-1] if x.dim() >= 1 and x.shape[-1] else 0


def hip_supported(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False) -> bool:
    """The kernel's contract: bf16 CUDA operands, 1..MAX_ROWS rows, N % 16 == 0 (N % 32 == 0 with
    ``swiglu``: both halves in whole tiles), K % 32 == 0, ``w`` contiguous and 16-byte aligned."""
    if not (x.is_cuda and w.is_cuda) or x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        return False
    if w.dim() != 2 or x.dim() < 1 or x.shape[-1] != w.shape[1]:
        return False
    N, K = w.shape
    return (1 <= _rows(x) <= max_rows() and N > 0 and N % (32 if swiglu else 16) == 0 and K % 32 == 0
            and w.is_contiguous() and w.data_ptr() % 16 == 0)


def linear_rows_reference(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False) -> torch.Tensor:
    y = F.linear(x, w)
    return swiglu_packed_reference(y) if swiglu else y


def linear_rows(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False) -> torch.Tensor:
    if w.dim() != 2 or x.dim() < 1 or x.shape[-1] != w.shape[1]:
        raise ValueError(f"linear_rows: x [..., K] and w [N, K]; got {tuple(x.shape)}, {tuple(w.shape)}")
    if not 1 <= _rows(x) <= max_rows():
        raise ValueError(f"linear_rows: 1 to {max_rows()} rows (larger batches are the library GEMM's); got "
                         f"{tuple(x.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        raise ValueError("linear_rows: inference only (no backward); call it under torch.no_grad()")
    if swiglu and w.shape[0] % 2:
        raise ValueError(f"linear_rows: swiglu needs the packed [W1 | W3], an even N; got {tuple(w.shape)}")
    if not x.is_cuda:
        return linear_rows_reference(x, w, swiglu)
    if not hip_supported(x, w, swiglu):
        raise ValueError(f"linear_rows: the HIP kernel needs bf16 operands, N % {32 if swiglu else 16} == 0, "
                         f"K % 32 == 0 and a contiguous, 16-byte aligned w; got x {tuple(x.shape)} {x.dtype}, "
                         f"w {tuple(w.shape)} {w.dtype} stride {w.stride()}")
    N, K = w.shape
    x2 = _aligned(x.reshape(-1, K))
    y = x.new_empty(*x.shape[:-1], N // 2 if swiglu else N)
    _native.check(_native.load().pto_skinny_gemm(x2.data_ptr(), w.data_ptr(), y.data_ptr(), x2.shape[0], N, K,
                                                 int(swiglu), _stream(x)), "skinny_gemm")
    return y


# ---------------------------------------------------------------------------------------------------------
# FP8 weights (``csrc/kernels/skinny_gemm_fp8.hip``): OCP e4m3 with one power-of-two scale per output row,
# bf16 activations, fp32 accumulation -- half the weight bytes of a decode step.  e4m3 -> bf16 is exact and
# so is the multiply by a power of two: ``dequantize_rows(q, scale)`` is a bf16 matrix, and
# ``linear_rows_fp8(x, q, scale)`` is ``linear_rows`` on it.

E4M3_MAX = 448.0
FP8_TILES = (0, 1, 2, 4)  # accumulators per wave a caller may force; 0: the library picks from (M, N)


def quantize_rows(w: torch.Tensor):
    """``w`` [N, K] -> (``q`` e4m3 [N, K] contiguous, ``scale`` fp32 [N]) with ``scale[n] =
    2^ceil(log2(amax_n / 448))`` (1 for a zero row) and ``q = w / scale`` rounded to e4m3: the quotient is
    inside +-448 by construction, and the largest of a row lands in (224, 448]."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows: w [N, K]; got {tuple(w.shape)}")
    amax = w.detach().abs().amax(dim=1).double()
    m, e = torch.frexp(amax / E4M3_MAX)               # amax / 448 = m 2^e, m in [0.5, 1)
    e = torch.where(m == 0.5, e - 1, e)               # ceil(log2(.)): e, but e - 1 at an exact power of two
    scale = torch.ldexp(torch.ones_like(amax), e.clamp(-126, 127)).float()
    scale = torch.where(amax > 0, scale, torch.ones_like(scale))
    q = (w.detach().float() / scale[:, None]).to(torch.float8_e4m3fn).contiguous()
    return q, scale


def dequantize_rows(q: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """``scale[:, None] * q`` in ``dtype``: exact in bf16 (and anything wider) for a power-of-two scale."""
    return (q.float() * scale.float()[:, None]).to(dtype)


def _fp8_contract(x, q, scale, swiglu, tiles) -> bool:
    """What both devices ask: shapes, dtypes of q and scale, tiles."""
    if q.dim() != 2 or x.dim() < 1 or x.shape[-1] != q.shape[1] or scale.shape != (q.shape[0],):
        return False
    if q.dtype != torch.float8_e4m3fn or scale.dtype != torch.float32 or tiles not in FP8_TILES:
        return False
    N, K = q.shape
    return (1 <= _rows(x) <= max_rows() and N > 0 and N % (32 if swiglu else 16) == 0 and K % 64 == 0
            and q.is_contiguous() and scale.is_contiguous())


def hip_supported_fp8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                      tiles: int = 0) -> bool:
    """The kernel's contract: bf16 CUDA ``x``, 1..MAX_ROWS rows; ``q`` e4m3 [N, K], contiguous and 16-byte
    aligned; ``scale`` fp32 [N]; N % 16 == 0 (N % 32 == 0 with ``swiglu``), K % 64 == 0; ``tiles`` in
    ``FP8_TILES``; no gradient asked for."""
    if not (x.is_cuda and q.is_cuda and scale.is_cuda) or x.dtype != torch.bfloat16:
        return False
    if torch.is_grad_enabled() and x.requires_grad:
        return False
    return _fp8_contract(x, q, scale, swiglu, tiles) and q.data_ptr() % 16 == 0


def linear_rows_fp8_reference(x, q, scale, swiglu: bool = False) -> torch.Tensor:
    y = F.linear(x, dequantize_rows(q, scale, x.dtype))
    return swiglu_packed_reference(y) if swiglu else y


def linear_rows_fp8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                    tiles: int = 0) -> torch.Tensor:
    """``linear_rows(x, dequantize_rows(q, scale), swiglu)`` from the e4m3 bytes.  ``tiles`` forces the
    accumulators per wave (tests, benchmarks); the result does not depend on it."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise ValueError("linear_rows_fp8: inference only (no backward); call it under torch.no_grad()")
    ok = hip_supported_fp8(x, q, scale, swiglu, tiles) if x.is_cuda else _fp8_contract(x, q, scale, swiglu, tiles)
    if not ok:
        raise ValueError(f"linear_rows_fp8: x [..., K] of 1 to {max_rows()} rows (bf16 on a GPU), q [N, K] e4m3, "
                         f"contiguous and 16-byte aligned, scale [N] fp32, N % {32 if swiglu else 16} == 0, "
                         f"K % 64 == 0, tiles in {FP8_TILES}; got x {tuple(x.shape)} {x.dtype}, q {tuple(q.shape)} "
                         f"{q.dtype} stride {q.stride()}, scale {tuple(scale.shape)} {scale.dtype}, tiles {tiles}")
    if not x.is_cuda:
        return linear_rows_fp8_reference(x, q, scale, swiglu)
    return launch_rows_fp8(x, q, scale, swiglu, tiles)


def launch_rows_fp8(x, q, scale, swiglu: bool = False, tiles: int = 0) -> torch.Tensor:
    """The launch alone, for a caller that has just asked ``hip_supported_fp8`` about these very arguments
    (``models.llama.rows_linear``: a decode step is bound by the host, and the checks are most of a call)."""
    N, K = q.shape
    x2 = _aligned(x.reshape(-1, K))
    y = x.new_empty(*x.shape[:-1], N // 2 if swiglu else N)
    _native.check(_native.load().pto_skinny_fp8_gemm(x2.data_ptr(), q.data_ptr(), scale.data_ptr(), y.data_ptr(),
                                                     x2.shape[0], N, K, int(swiglu), tiles, _stream(x)),
                  "skinny_fp8_gemm")
    return y


# ---------------------------------------------------------------------------------------------------------
# MXFP4 weights (``csrc/kernels/skinny_gemm_fp4.hip``): OCP e2m1 codes, two to a byte, in blocks of 32 along K with
# one e8m0 power-of-two scale per block, bf16 activations, fp32 accumulation -- 17 / 32 of a byte per weight.  An
# e2m1 value times a power of two is exact in bf16: ``dequantize_rows_fp4(q, scale)`` is a bf16 matrix, and
# ``linear_rows_fp4(x, q, scale)`` is ``linear_rows`` on it.

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitudes of a code's bits 0-2; bit 3 is the sign
FP4_BLOCK = 32


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e in fp32 for integer ``e`` in [-126, 127], from the bits."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_rows_fp4(w: torch.Tensor):
    """``w`` [N, K], K % 32 == 0 -> (``q`` uint8 [N, K / 2], ``scale`` uint8 [N, K / 32]), both contiguous.  Byte j
    of a row of ``q`` holds the code of k = 2 j in its low nibble and of k = 2 j + 1 in its high one.  ``scale`` is
    e8m0: byte b means 2^(b - 127), with b - 127 = e = ceil(log2(amax / 6)) of the block clamped to [-125, 125]
    (0 for a zero block), so that the quotient is inside +-6 and every non-zero dequantised value is a normal bf16.
    A code is ``w / 2^e`` rounded to the nearest magnitude, ties to the even index, sign kept; 0x8 is never emitted."""
    if w.dim() != 2 or w.shape[1] % FP4_BLOCK or not w.is_floating_point():
        raise ValueError(f"quantize_rows_fp4: w [N, K] with K % {FP4_BLOCK} == 0; got {tuple(w.shape)} {w.dtype}")
    N, K = w.shape
    wf = w.detach()
    wf = (wf if wf.dtype == torch.float64 else wf.float()).reshape(N, K // FP4_BLOCK, FP4_BLOCK)
    amax = wf.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                          # amax = m 2^ex, m in [0.5, 1)
    e = torch.where(m <= 0.75, ex - 3, ex - 2)         # the least e with amax <= 6 * 2^e = 0.75 * 2^(e + 3)
    e = torch.where(amax > 0, e.clamp(-125, 125), torch.zeros_like(e))
    a = (wf * _pow2(-e).to(wf.dtype)[..., None]).abs()  # exact: at worst a value under 2^-126 in fp32, a zero code
    idx = torch.zeros_like(a, dtype=torch.uint8)
    for i in range(7):                                  # past the midpoint to the next magnitude; a tie goes to even
        mid = (E2M1[i] + E2M1[i + 1]) / 2
        idx += (a >= mid) if i % 2 else (a > mid)
    code = (idx | (((wf < 0) & (idx > 0)).to(torch.uint8) << 3)).reshape(N, K)
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return q, (e + 127).to(torch.uint8).contiguous()


def dequantize_rows_fp4(q: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """The [N, K] matrix that ``(q, scale)`` means, in ``dtype``: exact in bf16 and anything wider.  Code 0x8 reads
    as zero.  A table lookup and a multiply by a power of two built from its bits."""
    if q.dim() != 2 or q.dtype != torch.uint8 or scale.dtype != torch.uint8 \
            or scale.shape != (q.shape[0], q.shape[1] * 2 // FP4_BLOCK) or q.shape[1] * 2 % FP4_BLOCK:
        raise ValueError(f"dequantize_rows_fp4: q uint8 [N, K / 2] and scale uint8 [N, K / {FP4_BLOCK}]; got "
                         f"{tuple(q.shape)} {q.dtype}, {tuple(scale.shape)} {scale.dtype}")
    N, K = q.shape[0], q.shape[1] * 2
    lut = torch.tensor(E2M1 + (0.0,) + tuple(-v for v in E2M1[1:]), dtype=torch.float32, device=q.device)
    v = lut[torch.stack((q & 15, q >> 4), dim=-1).reshape(N, K // FP4_BLOCK, FP4_BLOCK).long()]
    return (v * _pow2(scale.to(torch.int32) - 127)[..., None]).reshape(N, K).to(dtype)


def _fp4_contract(x, q, scale, swiglu, tiles) -> bool:
    """What both devices ask: shapes, dtypes of q and scale, tiles."""
    if q.dim() != 2 or x.dim() < 1 or x.shape[-1] != 2 * q.shape[1] or q.dtype != torch.uint8 \
            or scale.dtype != torch.uint8 or tiles not in FP8_TILES:
        return False
    N, K = q.shape[0], 2 * q.shape[1]
    return (1 <= _rows(x) <= max_rows() and N > 0 and N % (32 if swiglu else 16) == 0 and K % 128 == 0
            and scale.shape == (N, K // FP4_BLOCK) and q.is_contiguous() and scale.is_contiguous())


def hip_supported_fp4(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                      tiles: int = 0) -> bool:
    """The kernel's contract: bf16 CUDA ``x``, 1..MAX_ROWS rows; ``q`` uint8 [N, K / 2], contiguous and 16-byte
    aligned; ``scale`` uint8 [N, K / 32], contiguous and 2-byte aligned (the kernel loads a step's two scale bytes at
    once; the rows are multiples of 4 bytes); N % 16 == 0 (N % 32 == 0 with ``swiglu``), K % 128 == 0; ``tiles`` in
    ``FP8_TILES``; no gradient asked for."""
    if not (x.is_cuda and q.is_cuda and scale.is_cuda) or x.dtype != torch.bfloat16:
        return False
    if torch.is_grad_enabled() and x.requires_grad:
        return False
    return _fp4_contract(x, q, scale, swiglu, tiles) and q.data_ptr() % 16 == 0 and scale.data_ptr() % 2 == 0


def linear_rows_fp4_reference(x, q, scale, swiglu: bool = False) -> torch.Tensor:
    y = F.linear(x, dequantize_rows_fp4(q, scale, x.dtype))
    return swiglu_packed_reference(y) if swiglu else y


def linear_rows_fp4(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                    tiles: int = 0) -> torch.Tensor:
    """``linear_rows(x, dequantize_rows_fp4(q, scale), swiglu)`` from the packed bytes.  ``tiles`` forces the
    accumulators per wave (tests, benchmarks); the result does not depend on it."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise ValueError("linear_rows_fp4: inference only (no backward); call it under torch.no_grad()")
    ok = hip_supported_fp4(x, q, scale, swiglu, tiles) if x.is_cuda else _fp4_contract(x, q, scale, swiglu, tiles)
    if not ok:
        raise ValueError(f"linear_rows_fp4: x [..., K] of 1 to {max_rows()} rows (bf16 on a GPU), q [N, K / 2] uint8, "
                         f"contiguous and 16-byte aligned, scale [N, K / {FP4_BLOCK}] uint8, contiguous and 2-byte "
                         f"aligned, N % {32 if swiglu else 16} == 0, K % 128 == 0, tiles in {FP8_TILES}; got x "
                         f"{tuple(x.shape)} {x.dtype}, q {tuple(q.shape)} {q.dtype} stride {q.stride()}, scale "
                         f"{tuple(scale.shape)} {scale.dtype}, tiles {tiles}")
    if not x.is_cuda:
        return linear_rows_fp4_reference(x, q, scale, swiglu)
    return launch_rows_fp4(x, q, scale, swiglu, tiles)


def launch_rows_fp4(x, q, scale, swiglu: bool = False, tiles: int = 0) -> torch.Tensor:
    """The launch alone, for a caller that has just asked ``hip_supported_fp4`` about these very arguments."""
    N, K = q.shape[0], 2 * q.shape[1]
    x2 = _aligned(x.reshape(-1, K))
    y = x.new_empty(*x.shape[:-1], N // 2 if swiglu else N)
    _native.check(_native.load().pto_skinny_fp4_gemm(x2.data_ptr(), q.data_ptr(), scale.data_ptr(), y.data_ptr(),
                                                     x2.shape[0], N, K, int(swiglu), tiles, _stream(x)),
                  "skinny_fp4_gemm")
    return y


# ---------------------------------------------------------------------------------------------------------
# The residual add and RMSNorm of a decode step folded into the projections around them
# (``csrc/kernels/skinny_gemm_fused.hip``).  RMSNorm's row scale commutes with the projection after it, so
# the GEMM that produces a branch output adds the residual and leaves the next GEMM's operand and the
# partial sums of squares, and the GEMM that consumes them scales its accumulators by rstd:
#
#   h, a, ss = linear_rows_add_norm(x, w, resid, gamma)     h = resid + linear_rows(x, w)   (resid's dtype)
#                                                           a = bf16(h * gamma), ss[..., t] = sum of h^2 over
#                                                           the columns 16 t .. 16 t + 15 (fp32)
#   y = linear_rows_scaled(a, w, ss, eps, swiglu)           rsqrt(ss.sum(-1) / K + eps) * linear_rows(a, w)
#
# which is ``linear_rows(rms_norm(h, gamma, eps), w)`` up to the roundings.  The ``_fp8`` forms take
# ``(q, scale)`` and ``tiles`` as ``linear_rows_fp8`` does.  Same rules as above: HIP on a GPU, ``ValueError``
# outside the contract, PyTorch on the CPU.

SS_TILE = 16  # columns per partial sum of squares: one MFMA tile


def _no_grad(name, *tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise ValueError(f"{name}: inference only (no backward); call it under torch.no_grad()")


def _add_norm_contract(x, N, resid, gamma) -> bool:
    """What both devices ask of the residual epilogue's own operands."""
    return (resid.dim() == x.dim() and resid.shape[:-1] == x.shape[:-1] and resid.shape[-1] == N
            and resid.dtype in (torch.float32, torch.bfloat16) and gamma.shape == (N,)
            and gamma.dtype == torch.float32 and N % SS_TILE == 0)


def _add_norm_hip(resid, gamma) -> bool:
    return (resid.is_cuda and gamma.is_cuda and resid.is_contiguous() and resid.data_ptr() % 16 == 0
            and gamma.is_contiguous())


def _scaled_contract(a, K, ss) -> bool:
    return (ss.dtype == torch.float32 and K % SS_TILE == 0 and ss.shape == (*a.shape[:-1], K // SS_TILE)
            and ss.is_contiguous() and ss.device == a.device)


def hip_supported_add_norm(x, w, resid, gamma) -> bool:
    """``hip_supported(x, w)``, and ``resid`` [..., N] fp32 or bf16 with ``x``'s leading shape, contiguous and
    16-byte aligned; ``gamma`` fp32 [N], contiguous."""
    return (hip_supported(x, w) and _add_norm_contract(x, w.shape[0], resid, gamma) and _add_norm_hip(resid, gamma))


def hip_supported_add_norm_fp8(x, q, scale, resid, gamma, tiles: int = 0) -> bool:
    return (hip_supported_fp8(x, q, scale, False, tiles) and _add_norm_contract(x, q.shape[0], resid, gamma)
            and _add_norm_hip(resid, gamma))


def hip_supported_scaled(a, w, ss, swiglu: bool = False) -> bool:
    """``hip_supported(a, w, swiglu)``, and ``ss`` fp32 [..., K / 16] with ``a``'s leading shape, contiguous."""
    return hip_supported(a, w, swiglu) and _scaled_contract(a, w.shape[1], ss)


def hip_supported_scaled_fp8(a, q, scale, ss, swiglu: bool = False, tiles: int = 0) -> bool:
    return hip_supported_fp8(a, q, scale, swiglu, tiles) and _scaled_contract(a, q.shape[1], ss)


def add_norm_reference(d: torch.Tensor, resid: torch.Tensor, gamma: torch.Tensor):
    """(h, a, ss) of a branch output ``d``: the residual epilogue after the GEMM, in PyTorch."""
    hf = resid.float() + d.float()
    ss = hf.reshape(*hf.shape[:-1], -1, SS_TILE).pow(2).sum(-1)
    return hf.to(resid.dtype), (hf * gamma.float()).to(d.dtype), ss


def scaled_reference(a, w, ss, eps: float, swiglu: bool = False) -> torch.Tensor:
    rstd = torch.rsqrt(ss.sum(-1, keepdim=True) / a.shape[-1] + eps)
    y = (rstd * F.linear(a.float(), w.float())).to(a.dtype)
    return swiglu_packed_reference(y) if swiglu else y


def _refuse(name, **got):
    desc = ", ".join(f"{k} {tuple(v.shape)} {v.dtype}" if isinstance(v, torch.Tensor) else f"{k} {v}"
                     for k, v in got.items())
    raise ValueError(f"{name}: outside the contract: the plain GEMM's (1 to {max_rows()} rows, bf16 on a GPU), resid "
                     f"fp32 / bf16 [..., N] contiguous and 16-byte aligned, gamma fp32 [N], ss fp32 "
                     f"[..., K / {SS_TILE}] contiguous; got {desc}")


def linear_rows_add_norm(x, w, resid, gamma):
    _no_grad("linear_rows_add_norm", x, w, resid, gamma)
    if not x.is_cuda:
        if w.dim() != 2 or x.dim() < 1 or x.shape[-1] != w.shape[1] or not 1 <= _rows(x) <= max_rows() \
                or not _add_norm_contract(x, w.shape[0], resid, gamma):
            _refuse("linear_rows_add_norm", x=x, w=w, resid=resid, gamma=gamma)
        return add_norm_reference(linear_rows_reference(x, w), resid, gamma)
    if not hip_supported_add_norm(x, w, resid, gamma):
        _refuse("linear_rows_add_norm", x=x, w=w, resid=resid, gamma=gamma, resid_stride=resid.stride())
    return launch_add_norm(x, w, None, resid, gamma)


def linear_rows_add_norm_fp8(x, q, scale, resid, gamma, tiles: int = 0):
    _no_grad("linear_rows_add_norm_fp8", x, resid, gamma)
    if not x.is_cuda:
        if not (_fp8_contract(x, q, scale, False, tiles) and _add_norm_contract(x, q.shape[0], resid, gamma)):
            _refuse("linear_rows_add_norm_fp8", x=x, q=q, scale=scale, resid=resid, gamma=gamma, tiles=tiles)
        return add_norm_reference(linear_rows_fp8_reference(x, q, scale), resid, gamma)
    if not hip_supported_add_norm_fp8(x, q, scale, resid, gamma, tiles):
        _refuse("linear_rows_add_norm_fp8", x=x, q=q, scale=scale, resid=resid, gamma=gamma, tiles=tiles,
                resid_stride=resid.stride())
    return launch_add_norm(x, q, scale, resid, gamma, tiles)


def linear_rows_scaled(a, w, ss, eps: float, swiglu: bool = False) -> torch.Tensor:
    _no_grad("linear_rows_scaled", a, w, ss)
    if not a.is_cuda:
        if w.dim() != 2 or a.dim() < 1 or a.shape[-1] != w.shape[1] or not 1 <= _rows(a) <= max_rows() \
                or (swiglu and w.shape[0] % 2) or not _scaled_contract(a, w.shape[1], ss):
            _refuse("linear_rows_scaled", a=a, w=w, ss=ss)
        return scaled_reference(a, w, ss, eps, swiglu)
    if not hip_supported_scaled(a, w, ss, swiglu):
        _refuse("linear_rows_scaled", a=a, w=w, ss=ss, swiglu=swiglu)
    return launch_scaled(a, w, None, ss, eps, swiglu)


def linear_rows_scaled_fp8(a, q, scale, ss, eps: float, swiglu: bool = False, tiles: int = 0) -> torch.Tensor:
    _no_grad("linear_rows_scaled_fp8", a, ss)
    if not a.is_cuda:
        if not (_fp8_contract(a, q, scale, swiglu, tiles) and _scaled_contract(a, q.shape[1], ss)):
            _refuse("linear_rows_scaled_fp8", a=a, q=q, scale=scale, ss=ss, tiles=tiles)
        return scaled_reference(a, dequantize_rows(q, scale, a.dtype), ss, eps, swiglu)
    if not hip_supported_scaled_fp8(a, q, scale, ss, swiglu, tiles):
        _refuse("linear_rows_scaled_fp8", a=a, q=q, scale=scale, ss=ss, swiglu=swiglu, tiles=tiles)
    return launch_scaled(a, q, scale, ss, eps, swiglu, tiles)


def launch_add_norm(x, w, scale, resid, gamma, tiles: int = 0):
    """The residual-epilogue launch alone (``scale`` None: bf16 weights), for a caller that has just asked the
    matching ``hip_supported_add_norm*`` about these very arguments."""
    N, K = w.shape
    x2 = _aligned(x.reshape(-1, K))
    h = torch.empty_like(resid)
    a = torch.empty(resid.shape, dtype=torch.bfloat16, device=resid.device)
    ss = torch.empty(*resid.shape[:-1], N // SS_TILE, dtype=torch.float32, device=resid.device)
    lib, bf = _native.load(), int(resid.dtype == torch.bfloat16)
    if scale is None:
        rc = lib.pto_skinny_add_norm(x2.data_ptr(), w.data_ptr(), resid.data_ptr(), gamma.data_ptr(), h.data_ptr(),
                                     a.data_ptr(), ss.data_ptr(), x2.shape[0], N, K, bf, _stream(x))
    else:
        rc = lib.pto_skinny_fp8_add_norm(x2.data_ptr(), w.data_ptr(), scale.data_ptr(), resid.data_ptr(),
                                         gamma.data_ptr(), h.data_ptr(), a.data_ptr(), ss.data_ptr(), x2.shape[0],
                                         N, K, bf, tiles, _stream(x))
    _native.check(rc, "skinny_add_norm")
    return h, a, ss


def launch_scaled(a, w, scale, ss, eps: float, swiglu: bool = False, tiles: int = 0) -> torch.Tensor:
    """The row-scale launch alone, as ``launch_add_norm``."""
    N, K = w.shape
    a2 = _aligned(a.reshape(-1, K))
    y = a.new_empty(*a.shape[:-1], N // 2 if swiglu else N)
    lib = _native.load()
    if scale is None:
        rc = lib.pto_skinny_scaled(a2.data_ptr(), w.data_ptr(), ss.data_ptr(), float(eps), y.data_ptr(), a2.shape[0],
                                   N, K, int(swiglu), _stream(a))
    else:
        rc = lib.pto_skinny_fp8_scaled(a2.data_ptr(), w.data_ptr(), scale.data_ptr(), ss.data_ptr(), float(eps),
                                       y.data_ptr(), a2.shape[0], N, K, int(swiglu), tiles, _stream(a))
    _native.check(rc, "skinny_scaled")
    return y
