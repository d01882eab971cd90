"""Micro-batches of a ``TokenStream`` on the training device, one ahead of the compute stream.

``TokenFeed.take(t, m)`` returns the expanded batch (``ops.token_batch.expand``) of optimizer step
``t``, micro-batch ``m`` for this rank and queues the host-to-device copy of the batch named by
``then``.  Only the narrow tokens cross the bus (2 or 4 bytes per token).

On a GPU a span is copied into one of two pinned host buffers and from there, on a side stream,
into that slot's device buffer.  A pinned buffer is rewritten only after its last copy's event has
completed (a host wait on an event two micro-batches old); a device buffer only after the ``expand``
that read it (the side stream waits for an event recorded behind that launch); ``expand`` runs on
the compute stream behind the copy's event.  On the CPU it is a plain copy.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..ops import token_batch
from .tokens import TokenStream


class TokenFeed:
    def __init__(self, stream: TokenStream, rank: int, device: torch.device, eos: Optional[int] = None):
        self.stream, self.rank, self.device = stream, rank, device
        self.eos = eos
        self.B, self.S = stream.batch_size, stream.seq_len
        self.gpu = device.type == "cuda"
        self._tdt = torch.int16 if stream.dtype.itemsize == 2 else torch.int32  # the ids' bits
        self._sdt = np.int16 if stream.dtype.itemsize == 2 else np.int32
        # running sums of expand's stats over every batch taken: valid targets, document starts, ids >= vocab
        self.total = torch.zeros(3, dtype=torch.int64, device=device)
        self.batches = 0
        self._pending = None  # (key, slot, src tensor or token count, row_stride)
        if self.gpu:
            n = self.B * (self.S + 1)
            self._pin = [torch.empty(n, dtype=self._tdt).pin_memory() for _ in range(2)]
            self._pin_np = [p.numpy() for p in self._pin]
            self._dev = [torch.empty(n, dtype=self._tdt, device=device) for _ in range(2)]
            self._copied = [torch.cuda.Event() for _ in range(2)]
            self._consumed = [torch.cuda.Event() for _ in range(2)]
            self._used = [False, False]
            self._side = torch.cuda.Stream(device)
            self._slot = 0

    def prefetch(self, t: int, m: int) -> None:
        span, row_stride = self.stream.span(t, m, self.rank)
        span = span.view(self._sdt)
        if not self.gpu:
            self._pending = ((t, m), 0, torch.from_numpy(np.array(span)), row_stride)
            return
        s, n = self._slot, span.shape[0]
        self._slot ^= 1
        if self._used[s]:
            self._copied[s].synchronize()  # the pinned buffer's last copy has left it
        self._pin_np[s][:n] = span
        with torch.cuda.stream(self._side):
            if self._used[s]:
                self._side.wait_event(self._consumed[s])  # the device buffer's last reader is done
            self._dev[s][:n].copy_(self._pin[s][:n], non_blocking=True)
            self._copied[s].record(self._side)
        self._used[s] = True
        self._pending = ((t, m), s, n, row_stride)

    def take(self, t: int, m: int, then: Optional[Tuple[int, int]] = None):
        """``(x, y, doc_start, doc_end, stats)`` of step ``t``, micro-batch ``m``; ``then``: the
        ``(t, m)`` to copy ahead."""
        if self._pending is None or self._pending[0] != (t, m):
            self.prefetch(t, m)
        _, s, src, row_stride = self._pending
        self._pending = None
        if self.gpu:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._copied[s])
            out = token_batch.expand(self._dev[s][:src], row_stride, self.B, self.S, self.stream.vocab_size,
                                     self.eos)
            self._consumed[s].record(cur)
        else:
            out = token_batch.expand(src, row_stride, self.B, self.S, self.stream.vocab_size, self.eos)
        self.total += out[4]
        self.batches += 1
        if then is not None:
            self.prefetch(*then)
        return out
