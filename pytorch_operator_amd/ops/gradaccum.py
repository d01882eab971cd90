"""Fold a micro-batch's gradient into an fp32 accumulator (``csrc/kernels/gradaccum.hip``).

Gradient accumulation (``--grad-accum N``: N forward/backward passes per optimizer step) sums the
micro-batches' gradients in fp32, sequentially, one rounding per add: ``A = ((g_1 + g_2) + ... +
g_N)``, each ``g_k`` in the parameter's dtype and widened.  ``MasterAdamW(grad_accum=N)`` folds
per parameter, ``ZeroAdamW(grad_accum=N)`` per bucket; both then hand ``A`` to the norm pass and
the AdamW kernel with ``1/(N*W)`` as the gradient scale, so nothing here scales.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _native


def fold(acc: torch.Tensor, g: torch.Tensor, first: bool, out: Optional[torch.Tensor] = None) -> None:
    """``acc = g`` (``first``: ``acc`` is not read, it may be uninitialised) or ``acc += g``, in
    fp32; ``out`` (bf16, optional) also receives the new ``acc`` rounded to nearest even.  ``out``
    may be ``g`` itself (a bf16 bucket reduced in place).  On the GPU one launch on the current
    stream: the package's only call of ``pto_grad_accum``; on the CPU the same math in PyTorch."""
    n = acc.numel()
    if acc.dtype != torch.float32 or not acc.is_contiguous():
        raise TypeError("gradient accumulator: a contiguous fp32 tensor")
    if g.numel() != n or g.device != acc.device or g.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("gradient fold: an fp32/bf16 gradient of the accumulator's size, on its device")
    if out is not None and (out.dtype != torch.bfloat16 or out.numel() != n or not out.is_contiguous()
                            or out.device != acc.device):
        raise TypeError("gradient fold: out is a contiguous bf16 tensor of the accumulator's size")
    if n == 0:
        return
    if not acc.is_cuda:
        if first:
            acc.copy_(g.reshape(acc.shape))
        else:
            acc.add_(g.reshape(acc.shape).float())
        if out is not None:
            out.view(-1).copy_(acc.view(-1))
        return
    lib = _native.load()  # a missing library is an error: there is no PyTorch path on the GPU
    if not g.is_contiguous() or g.data_ptr() % 16:
        g = g.contiguous().clone()  # fix-up copy, as MasterAdamW._hip_grad
    stream = ctypes.c_void_p(torch.cuda.current_stream(acc.device).cuda_stream)
    _native.check(lib.pto_grad_accum(acc.data_ptr(), g.data_ptr(), None if out is None else out.data_ptr(), n,
                                     1 if g.dtype == torch.bfloat16 else 0, 1 if first else 0, stream), "grad_accum")


def sweep() -> int:
    """Elements one sweep of the kernel's capped grid covers (a longer buffer loops)."""
    return int(_native.load().pto_grad_accum_sweep())
