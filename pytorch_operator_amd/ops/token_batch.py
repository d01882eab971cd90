"""One micro-batch of token-file training data from its narrow tokens (``csrc/kernels/token_batch.hip``).

``expand(src, row_stride, B, S, vocab, eos)`` takes the span ``data.tokens.TokenStream.span`` returns
(16- or 32-bit ids; row ``b`` is ``src[b*row_stride : b*row_stride + S + 1]``) and returns
``(x, y, doc_start, doc_end, stats)``:

- ``x``, ``y`` int64 [B, S]: the tokens and the next tokens.  An id ``>= vocab`` becomes ``vocab - 1``
  (it must never reach the embedding gather) and is counted; everything else is computed from the
  clamped ids.  With ``eos``, ``y`` is ``-100`` where ``x == eos``.
- ``doc_start``, ``doc_end`` int32 [B, S] with ``eos`` (else ``None``): exactly
  ``attention.doc_starts_from_tokens(x, eos)`` and ``attention.doc_ends(doc_start)``.
- ``stats`` int64 [3]: targets that are not ignored, document starts in ``x`` (``B`` without ``eos``),
  ids ``>= vocab`` among the ``S + 1`` tokens of every row.

On the GPU it is one launch on the current stream and the package's only call of ``pto_token_batch``
(a missing library is an error); on the CPU it is the PyTorch composition, the kernel's reference.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _native
from .attention import doc_ends, doc_starts_from_tokens

_WIDTH = {torch.int16: 2, torch.int32: 4}
for _name, _w in (("uint16", 2), ("uint32", 4)):
    if hasattr(torch, _name):
        _WIDTH[getattr(torch, _name)] = _w


def _signed(src: torch.Tensor) -> torch.Tensor:
    """The same bits in a signed dtype (every torch op takes those)."""
    return src.view(torch.int16 if _WIDTH[src.dtype] == 2 else torch.int32)


def expand_reference(src: torch.Tensor, row_stride: int, B: int, S: int, vocab: int, eos: int):
    w = _WIDTH[src.dtype]
    tok = _signed(src).to(torch.int64) & (0xffff if w == 2 else 0xffffffff)
    idx = (torch.arange(B, device=src.device).view(B, 1) * row_stride
           + torch.arange(S + 1, device=src.device).view(1, S + 1))
    t = tok[idx]
    bad = t >= vocab
    t = torch.where(bad, torch.full_like(t, vocab - 1), t)
    x, y = t[:, :-1].contiguous(), t[:, 1:].contiguous()
    ds = de = None
    starts = B
    if eos >= 0:
        ds = doc_starts_from_tokens(x, eos)
        de = doc_ends(ds)
        y = y.masked_fill(x == eos, -100)  # that target would be the next document's first token
        starts = int((ds == torch.arange(S, device=src.device, dtype=torch.int32)).sum())
    stats = torch.tensor([int((y != -100).sum()), starts, int(bad.sum())], dtype=torch.int64, device=src.device)
    return x, y, ds, de, stats


def expand(src: torch.Tensor, row_stride: int, B: int, S: int, vocab: int, eos: Optional[int] = None
           ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    eos = -1 if eos is None or eos < 0 else int(eos)
    if src.dtype not in _WIDTH or src.dim() != 1 or not src.is_contiguous():
        raise TypeError(f"token span: a contiguous 1-D tensor of 16- or 32-bit ids; got {tuple(src.shape)} {src.dtype}")
    if B < 1 or S < 1 or row_stride < S or src.numel() < (B - 1) * row_stride + S + 1:
        raise ValueError(f"token span of {src.numel()} ids does not hold {B} rows of {S} + 1 at stride {row_stride}")
    if not 0 < vocab < 2 ** 31 or eos >= vocab:
        raise ValueError(f"vocab {vocab} / eos {eos}: 0 < vocab < 2^31 and eos < vocab")
    if not src.is_cuda:
        return expand_reference(src, row_stride, B, S, vocab, eos)
    lib = _native.load()  # a missing library is an error: there is no PyTorch path on the GPU
    dev = src.device
    x = torch.empty(B, S, dtype=torch.int64, device=dev)
    y = torch.empty(B, S, dtype=torch.int64, device=dev)
    ds = de = None
    if eos >= 0:
        ds = torch.empty(B, S, dtype=torch.int32, device=dev)
        de = torch.empty(B, S, dtype=torch.int32, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(_native.current_stream_ptr(dev))
    _native.check(lib.pto_token_batch(src.data_ptr(), _WIDTH[src.dtype], row_stride, B, S, vocab, eos,
                                      x.data_ptr(), y.data_ptr(), None if ds is None else ds.data_ptr(),
                                      None if de is None else de.data_ptr(), stats.data_ptr(), stream),
                  "token_batch")
    return x, y, ds, de, stats


def chunk() -> int:
    """Positions of a row one workgroup of the kernel owns (longer rows are split)."""
    return int(_native.load().pto_token_batch_chunk())
