"""Skinny bf16 GEMM (``csrc/kernels/skinny_gemm.hip``): the projections of a decode step, where the
"batch" of the GEMM is the B <= 16 sequences being continued and the operation streams the weights.

``linear_rows(x, w, swiglu=False)``: ``x`` [..., K] with at most ``MAX_ROWS`` rows in all, ``w`` [N, K]
as ``nn.Linear`` holds it (neither copied nor transposed) -> ``F.linear(x, w)`` [..., N] in bf16 with fp32
accumulation; with ``swiglu``, ``w`` is the packed [W1 | W3] of ``FeedForward.w13`` and the result is
``swiglu_packed(F.linear(x, w))`` [..., N / 2] from one launch, bit for bit what the two launches give.
Inference only.  On a GPU the HIP kernel runs, and a shape or dtype outside its contract
(``hip_supported``) is a ``ValueError``, never a silent fallback; on CPU the same math runs in PyTorch.
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
