"""Global L2 norm of a set of gradient buffers, on device (``csrc/kernels/gradclip.hip``).

The norm pass of ``MasterAdamW(max_grad_norm=...)`` and ``ZeroAdamW(max_grad_norm=...)``: one
``pto_grad_sumsq`` launch per buffer, each writing its per-block partials into its own
consecutive region of one workspace, then one ``pto_grad_sumsq_finish`` launch that leaves
``sum(g^2)`` and the norm in two device floats.  ``pto_adamw_step_clipped`` reads the sum on the
device; nothing here reads it on the host.  ``GlobalGradNorm`` is what the optimizers hold: that
pass (or, on the CPU, the same sum in PyTorch), the all-reduce across ranks, and the result.

No float atomics: the number of partials and the order of every sum depend on the buffer
lengths alone, so the norm is bitwise reproducible and the same on every replica.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence, Tuple

import torch
import torch.distributed as dist

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


class GlobalGradNorm:
    """The ``max_grad_norm`` state of one optimizer (``MasterAdamW``, ``ZeroAdamW``): the norm pass
    over the step's gradient buffers, its two-float result and, on the CPU, the clip factor.
    ``group`` / ``world``: each rank passes its own shards and the sum of squares is all-reduced."""

    def __init__(self, max_norm, group=None, world: int = 1):
        if not max_norm > 0:
            raise ValueError("max_grad_norm: a positive number, or None for no clipping")
        self.max_norm, self.group, self.world = float(max_norm), group, world
        self.out = None      # [sum of squares, norm] of the last run, on the gradients' device
        self.coef = None     # CPU: clip_coef of the last run (on the GPU, AdamW derives it from out)
        self._device = None  # DeviceGradNorm, created by the first GPU run

    def run(self, items: Sequence[Tuple[torch.Tensor, float]]) -> torch.Tensor:
        """Norm of ``scale * g`` over every ``(g, scale)``; on the GPU enqueued on the current
        stream and never read by the host."""
        if items[0][0].is_cuda:
            if self._device is None:
                self._device = DeviceGradNorm()
            out = self.out = self._device.run(items)
            if self.world > 1:
                dist.all_reduce(out[:1], op=dist.ReduceOp.SUM, group=self.group)
                torch.sqrt(out[:1], out=out[1:])
        else:
            sumsq = torch.zeros(1, dtype=torch.float32)
            for g, scale in items:
                sumsq += (g.float() * scale).pow(2).sum()
            if self.world > 1:
                dist.all_reduce(sumsq, op=dist.ReduceOp.SUM, group=self.group)
            self.out = torch.cat([sumsq, sumsq.sqrt()])
            self.coef = clip_coef(self.out[1], self.max_norm)
        return self.out

    def last_grad_norm(self):
        """The global norm of the last run, before clipping, as a 0-dim tensor on the gradients'
        device (``None`` before the first run).  Does not synchronise."""
        return None if self.out is None else self.out[1]
