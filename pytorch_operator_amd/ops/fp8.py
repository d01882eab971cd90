"""FP8 (OCP e4m3fn / e5m2) projection GEMMs for the Llama worker, off by default.

``quantize`` turns a bf16 matrix into per-tensor-scaled FP8 operands with the gfx950 kernels of
``csrc/kernels/fp8_cast.hip``: one pass for max |x|, one pass that casts and writes the matrix
and / or its transpose, so all three GEMMs of a linear layer get K-contiguous operands (the
layout ``linear_tn`` established as fastest) from one read of each tensor.  The scale is computed
just in time from the tensor itself: no amax history, no state, checkpoints are untouched.

``fp8_linear`` is ``linear_tn``'s contract (bf16 in and out, no bias) on ``torch._scaled_mm``
(hipBLASLt's FP8 GEMM): x and w in e4m3, the output gradient in ``grad_format``.  It saves the
FP8 transpose of x instead of the bf16 x.  Nothing is cached across steps: the optimizers write
the weights through raw pointers without bumping their version counters.

On CPU the same arithmetic runs in PyTorch (``quantize_reference`` and fp32 matmuls of the
dequantised operands).  On a GPU a missing kernel or an unsupported shape is an error.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _native

FORMATS = {"e4m3": (0, 448.0, torch.float8_e4m3fn), "e5m2": (1, 57344.0, torch.float8_e5m2)}

# How the backward gets the transposed FP8 weight for dX: True keeps it from the forward (one read
# of w makes both layouts; N*K bytes saved per layer until its backward), False quantizes w again
# in the backward (two more launches and one more read of w, nothing saved).  The choice and both
# measurements: profiles/fp8/README.md.  PTO_FP8_W8T=requant selects the other one (A/B runs).
KEEP_W8T = os.environ.get("PTO_FP8_W8T", "keep") != "requant"


def _fmt(fmt: str):
    try:
        return FORMATS[fmt]
    except KeyError:
        raise ValueError(f"fp8: format must be one of {sorted(FORMATS)}, got {fmt!r}") from None


def quantize_reference(x2d: torch.Tensor, fmt: str, scale=None):
    """(q [R, C], qT [C, R], scale_inv) of a 2-D tensor, in PyTorch: the kernels' arithmetic.

    ``amax`` is taken over the finite elements and a NaN or Inf element becomes NaN, so a
    non-finite input is never hidden and never spoils the scale of the rest."""
    _, fmax, dt = _fmt(fmt)
    xf = x2d.float()
    finite = torch.isfinite(xf)
    if scale is None:
        amax = torch.where(finite, xf.abs(), torch.zeros_like(xf)).max()
        one = torch.ones_like(amax)
        scale_t = torch.where(amax > 0, fmax / amax, one)
        scale_inv = torch.where(amax > 0, amax / fmax, one)
    else:
        scale_t = torch.as_tensor(scale, dtype=torch.float32, device=x2d.device).reshape(())
        scale_inv = 1.0 / scale_t
    qf = (xf * scale_t).clamp(-fmax, fmax)
    q = torch.where(finite, qf, torch.full_like(qf, float("nan"))).to(dt)
    return q, q.t().contiguous(), scale_inv


def hip_supported(x2d: torch.Tensor) -> bool:
    return (x2d.is_cuda and x2d.dim() == 2 and x2d.dtype == torch.bfloat16 and x2d.shape[0] % 64 == 0
            and x2d.shape[1] % 64 == 0 and x2d.numel() > 0)


def quantize(x2d: torch.Tensor, fmt: str, normal: bool = True, transposed: bool = True, scale=None):
    """(q or None, qT or None, scale_inv): FP8 tensors of ``x2d`` [R, C] (bf16) and the 0-d fp32
    dequantisation factor ``amax / fmax``.  GPU: the HIP kernels (R and C multiples of 64, else
    ``ValueError``); CPU: ``quantize_reference``.  ``scale`` fixes the scale instead of amax."""
    code, _, dt = _fmt(fmt)
    if not (normal or transposed):
        raise ValueError("fp8.quantize: nothing requested")
    if not x2d.is_cuda:
        q, qT, inv = quantize_reference(x2d, fmt, scale)
        return (q if normal else None), (qT if transposed else None), inv
    if not hip_supported(x2d):
        raise ValueError(f"fp8.quantize: needs a 2-D bf16 matrix with both dims multiples of 64, got "
                         f"{tuple(x2d.shape)} {x2d.dtype}")
    x2d = x2d.contiguous()
    if x2d.data_ptr() % 16:
        x2d = x2d.clone()
    R, C = x2d.shape
    dev = x2d.device
    lib = _native.load()
    stream = ctypes.c_void_p(_native.current_stream_ptr(dev))
    q = torch.empty((R, C), device=dev, dtype=dt) if normal else None
    qT = torch.empty((C, R), device=dev, dtype=dt) if transposed else None
    inv = torch.empty((), device=dev, dtype=torch.float32)
    if scale is None:
        nparts = lib.pto_fp8_amax_parts(R * C)
        ws = torch.empty(nparts, device=dev, dtype=torch.float32)
        _native.check(lib.pto_fp8_amax(x2d.data_ptr(), R, C, ws.data_ptr(), nparts, stream), "fp8_amax")
        ws_ptr, fixed_ptr = ws.data_ptr(), None
    else:
        fixed = torch.as_tensor(scale, dtype=torch.float32).reshape(1).to(dev)
        nparts, ws_ptr, fixed_ptr = 0, None, fixed.data_ptr()
    _native.check(lib.pto_fp8_cast(x2d.data_ptr(), R, C, code, ws_ptr, nparts, fixed_ptr,
                                   q.data_ptr() if normal else None, qT.data_ptr() if transposed else None,
                                   inv.data_ptr(), stream), "fp8_cast")
    return q, qT, inv


# ------------------------------------------------------------------------------- fp8_linear
def _quant(ref: bool, t: torch.Tensor, fmt: str, normal: bool, transposed: bool):
    if not ref:
        return quantize(t, fmt, normal, transposed)
    q, qT, inv = quantize_reference(t, fmt)
    return (q if normal else None), (qT if transposed else None), inv


def _mm(a8: torch.Tensor, b8t: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, ref: bool, out=None):
    """bf16 (a8 . b8t^T) * sa * sb for FP8 a8 [M, K] and b8t [N, K], both K-contiguous."""
    if ref:
        y = ((a8.float() @ b8t.float().t()) * (sa.float() * sb.float())).to(torch.bfloat16)
        return y if out is None else out.copy_(y)
    if out is not None:
        return torch._scaled_mm(a8, b8t.t(), scale_a=sa, scale_b=sb, out_dtype=torch.bfloat16,
                                use_fast_accum=False, out=out)
    return torch._scaled_mm(a8, b8t.t(), scale_a=sa, scale_b=sb, out_dtype=torch.bfloat16, use_fast_accum=False)


class _FP8Linear(torch.autograd.Function):
    """y = x.W^T with all three GEMMs in FP8, every operand K-contiguous: forward x8.(w8)^T,
    dX = dy8.(w8T)^T, dW = dy8T.(x8T)^T.  ``ref``: PyTorch quantisation and fp32 matmuls."""

    @staticmethod
    def forward(ctx, x, w, grad_format, ref):
        x2 = x.reshape(-1, x.shape[-1])
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        x8, x8T, sx = _quant(ref, x2, "e4m3", True, need_dw)
        keep = KEEP_W8T and need_dx
        w8, w8T, sw = _quant(ref, w, "e4m3", True, keep)
        ctx.save_for_backward(x8T if need_dw else None, sx, w8T if keep else None, sw, None if keep else w)
        ctx.xshape, ctx.wshape, ctx.grad_format, ctx.ref = x.shape, tuple(w.shape), grad_format, ref
        # gradient sink (parallel/zero.py): dW is written by the GEMM into the optimizer's bucket
        ctx.sink = getattr(w, "_pto_grad_sink", None)
        return _mm(x8, w8, sx, sw, ref).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x8T, sx, w8T, sw, w = ctx.saved_tensors
        ref = ctx.ref
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy2 = dy.reshape(-1, ctx.wshape[0]).to(torch.bfloat16)
        dy8, dy8T, sd = _quant(ref, dy2, ctx.grad_format, need_dx, need_dw)
        dx = dw = None
        if need_dx:
            if w8T is None:  # the scale is the forward's: w has not changed in between
                w8T = _quant(ref, w, "e4m3", False, True)[1]
            dx = _mm(dy8, w8T, sd, sw, ref).view(ctx.xshape)
        if need_dw:
            sink = ctx.sink
            if sink is not None and sink.dtype == torch.bfloat16 and sink.shape == ctx.wshape:
                _mm(dy8T, x8T, sd, sx, ref, out=sink.view)
                sink.ready()
            else:
                dw = _mm(dy8T, x8T, sd, sx, ref)
        return dx, dw, None, None


def _apply(x: torch.Tensor, w: torch.Tensor, grad_format: str, ref: bool) -> torch.Tensor:
    _fmt(grad_format)
    if w.dim() != 2 or x.shape[-1] != w.shape[1]:
        raise ValueError(f"fp8_linear: x {tuple(x.shape)} does not match w {tuple(w.shape)}")
    dev = x.device.type
    autocast = torch.is_autocast_enabled(dev)
    out_dtype = torch.bfloat16 if autocast or x.dtype == torch.bfloat16 else x.dtype
    if not ref:
        if not autocast and (x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16):
            raise ValueError(f"fp8_linear: bf16 operands (or bf16 autocast) on a GPU, got {x.dtype} and {w.dtype}")
        M, (N, K) = x.numel() // x.shape[-1], w.shape
        if M % 64 or N % 64 or K % 64 or M == 0:
            raise ValueError(f"fp8_linear: M, N and K must be multiples of 64 on a GPU, got x {tuple(x.shape)} "
                             f"(M = {M}) and w {tuple(w.shape)} (N = {N}, K = {K})")
    with torch.autocast(device_type=dev, enabled=False):
        return _FP8Linear.apply(x.to(torch.bfloat16), w.to(torch.bfloat16), grad_format, ref).to(out_dtype)


def fp8_linear_reference(x: torch.Tensor, w: torch.Tensor, grad_format: str = "e5m2") -> torch.Tensor:
    """``fp8_linear`` built on ``quantize_reference`` and fp32 matmuls of the dequantised operands,
    results rounded to bf16; any device, any shape."""
    return _apply(x, w, grad_format, True)


def fp8_linear(x: torch.Tensor, w: torch.Tensor, grad_format: str = "e5m2") -> torch.Tensor:
    """``F.linear(x, w)`` (no bias) with the forward and both backward GEMMs in per-tensor-scaled
    FP8: x and w in e4m3, the output gradient in ``grad_format``.  bf16 in and out (under
    autocast both operands are taken in bf16, as ``linear_tn`` does).  GPU: HIP cast kernels and
    ``torch._scaled_mm``; M, N or K not a multiple of 64 raises ``ValueError``.  CPU:
    ``fp8_linear_reference``."""
    return _apply(x, w, grad_format, not x.is_cuda)
