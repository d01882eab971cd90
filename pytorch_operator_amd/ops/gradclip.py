"""Global L2 norm of a set of gradient buffers, on device (``csrc/kernels/gradclip.hip``).

The norm pass of ``MasterAdamW(max_grad_norm=...)`` and ``ZeroAdamW(max_grad_norm=...)``: one
``pto_grad_sumsq`` launch per buffer, each writing its per-block partials into its own
consecutive region of one workspace, then one ``pto_grad_sumsq_finish`` launch that leaves
``sum(g^2)`` and the norm in two device floats.  ``pto_adamw_step_clipped`` reads the sum on the
device; nothing here reads it on the host.

No float atomics: the number of partials and the order of every sum depend on the buffer
lengths alone, so the norm is bitwise reproducible and the same on every replica.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Tuple

import torch

from . import _native

_EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s


def clip_coef(norm: torch.Tensor, max_norm: float) -> torch.Tensor:
    """``clip_grad_norm_``'s factor, min(1, max_norm / (norm + 1e-6)), as an fp32 tensor (a
    non-finite norm propagates, as with ``error_if_nonfinite=False``)."""
    return torch.clamp(max_norm / (norm.float() + _EPS), max=1.0)


class DeviceGradNorm:
    """Workspace + the two result floats (``out[0]`` = sum of squares, ``out[1]`` = norm),
    allocated once and reused (the workspace only grows)."""

    def __init__(self):
        self.ws = None
        self.out = None
        self._parts: Dict[Tuple[int, bool], int] = {}

    def parts(self, n: int, bf16: bool) -> int:
        k = self._parts.get((n, bf16))
        if k is None:
            k = self._parts[(n, bf16)] = int(_native.load().pto_grad_sumsq_parts(n, 1 if bf16 else 0))
        return k

    def run(self, items: Sequence[Tuple[torch.Tensor, float]]) -> torch.Tensor:
        """Enqueue the norm of ``scale * g`` over every ``(g, scale)`` on the current stream;
        returns the two-float device tensor.  Buffers: contiguous, 16-byte aligned, fp32/bf16."""
        lib = _native.load()
        dev = items[0][0].device
        counts: List[int] = []
        for g, _ in items:
            if g.dtype not in (torch.float32, torch.bfloat16) or not g.is_contiguous():
                raise TypeError("gradient norm: contiguous fp32/bf16 buffers only")
            counts.append(self.parts(g.numel(), g.dtype == torch.bfloat16))
        total = sum(counts)
        if self.out is None or self.out.device != dev:
            self.out = torch.zeros(2, dtype=torch.float32, device=dev)
            self.ws = None
        if self.ws is None or self.ws.numel() < total:
            self.ws = torch.empty(total, dtype=torch.float32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        base, off = self.ws.data_ptr(), 0
        for (g, scale), k in zip(items, counts):
            _native.check(lib.pto_grad_sumsq(g.data_ptr(), g.numel(), 1 if g.dtype == torch.bfloat16 else 0,
                                             scale, base + 4 * off, self.ws.numel() - off, stream), "grad_sumsq")
            off += k
        _native.check(lib.pto_grad_sumsq_finish(base, total, self.out.data_ptr(), stream), "grad_sumsq_finish")
        return self.out
