"""Flash attention (``csrc/kernels/attention.hip``, ``attention_d64.hip``) as an autograd op for the
Llama worker.

``flash_attention(q, k, v, causal=True)``: q [B, S, Hq, D], k/v [B, S, Hkv, D] (GQA when
Hkv < Hq), token-major like the projections that produce them, so no transposes or copies
surround the kernels; returns o [B, S, Hq, D] (``o.reshape(B, S, Hq * D)`` feeds the output
projection).  Scale 1/sqrt(D).

The HIP path covers the Llama-3 attention shapes: bf16, D = 128 (8B / 70B) or 64 (Llama-3.2 1B),
S a multiple of 128 (``hip_supported``).  D = 64 runs the 4-wave kernels only: the 8-wave forward,
the pipelined backward and the variant setters are D = 128.  The forward keeps lse2 = log2-sum-exp of the scaled scores per query
row; the backward is two launches (dQ with delta = rowsum(dO * O), then dK/dV), both
deterministic.  On CPU the same math runs in PyTorch (``attention_reference``); a GPU call
with an unsupported shape raises instead of falling back silently.

``flash_attention(q, k, v, doc_start=ds)`` is the document mask of packed-sequence training
(the ``attn_doc_*`` kernels of ``attention.hip``, siblings of the plain 4-wave kernels; the two
backward passes share one templated body each with them): ``ds`` [B, S] holds, per token, the
index of the first token of its document, and query i sees key j iff ``ds[b, i] <= j <= i``.
``doc_starts_from_tokens`` builds it from an end-of-text id, ``validate_doc_start`` checks it where
a batch is built.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn.functional as F

from . import _native

HEAD_DIM = 128         # the 8B model's
HEAD_DIMS = (64, 128)  # every head dim the HIP kernels are built for
SEQ_MULTIPLE = 128


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(_native.current_stream_ptr(t.device))


def _c(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def hip_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    if not (q.is_cuda and k.is_cuda and v.is_cuda) or q.dim() != 4:
        return False
    B, S, Hq, D = q.shape
    return (q.dtype == k.dtype == v.dtype == torch.bfloat16 and D in HEAD_DIMS and S % SEQ_MULTIPLE == 0
            and k.shape == v.shape and k.shape[0] == B and k.shape[1] == S and k.shape[3] == D
            and Hq % k.shape[2] == 0)


def doc_starts_from_tokens(tokens: torch.Tensor, eos_id: int) -> torch.Tensor:
    """[B, S] int32: per token, the index of the first token of its document.  A token starts a
    document iff it is at position 0 or the token before it is ``eos_id`` (the end-of-text token
    closes its own document); the start index is the running maximum of those positions."""
    B, S = tokens.shape
    idx = torch.arange(S, device=tokens.device, dtype=torch.int64).expand(B, S)
    first = torch.ones(B, S, dtype=torch.bool, device=tokens.device)
    first[:, 1:] = tokens[:, :-1] == eos_id
    return torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), dim=1).values.to(torch.int32)


def doc_ends(doc_start: torch.Tensor) -> torch.Tensor:
    """[B, S] int32: per token, one past the last token of its document (no host sync)."""
    B, S = doc_start.shape
    idx = torch.arange(S, device=doc_start.device, dtype=torch.int64).expand(B, S)
    # the next document start after position i, or S: a reverse running minimum
    nxt = torch.full((B, S + 1), S, dtype=torch.int64, device=doc_start.device)
    nxt[:, :S] = torch.where(doc_start.to(torch.int64) == idx, idx, nxt[:, :S])
    return torch.cummin(nxt.flip(1), dim=1).values.flip(1)[:, 1:].to(torch.int32).contiguous()


def validate_doc_start(doc_start: torch.Tensor) -> None:
    """Raise ValueError unless every row is a document layout: ``doc_start[i] <= i``, and each
    value is the previous one (same document) or ``i`` (a new one).  Reads the tensor on the host:
    call it where a batch is built, not per step."""
    if doc_start.dim() != 2 or doc_start.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"doc_start must be int32/int64 [B, S]; got {tuple(doc_start.shape)} {doc_start.dtype}")
    d = doc_start.detach().to("cpu", torch.int64)
    idx = torch.arange(d.shape[1]).expand_as(d)
    if bool((d > idx).any()) or bool((d < 0).any()):
        raise ValueError("doc_start: a document start lies after its token (or is negative)")
    if bool(((d[:, 1:] != d[:, :-1]) & (d[:, 1:] != idx[:, 1:])).any()):
        raise ValueError("doc_start: each value must be the previous value or its own index")


def _doc_mask(doc_start: torch.Tensor, S: int) -> torch.Tensor:
    """bool [B, 1, S, S]: True where query i may see key j (doc_start[b, i] <= j <= i)."""
    j = torch.arange(S, device=doc_start.device)
    return ((j.view(1, 1, S) <= j.view(1, S, 1)) & (j.view(1, 1, S) >= doc_start.view(-1, S, 1))).unsqueeze(1)


def _check_doc_start(q: torch.Tensor, doc_start: torch.Tensor, causal: bool) -> None:
    if not causal:
        raise ValueError("a document mask is causal: doc_start needs causal=True")
    if (not isinstance(doc_start, torch.Tensor) or doc_start.dtype not in (torch.int32, torch.int64)
            or tuple(doc_start.shape) != (q.shape[0], q.shape[1]) or doc_start.device != q.device):
        raise ValueError(f"doc_start must be int32/int64 [B, S] = {(q.shape[0], q.shape[1])} on {q.device}; got "
                         f"{tuple(doc_start.shape) if isinstance(doc_start, torch.Tensor) else type(doc_start)} "
                         f"{getattr(doc_start, 'dtype', None)} on {getattr(doc_start, 'device', None)}")


def attention_reference(q, k, v, causal: bool = True, return_lse: bool = False, doc_start=None):
    """fp32 math on [B, S, H, D] tensors; lse in natural-log units of the scaled scores.
    ``doc_start`` [B, S]: the document mask (query i sees key j iff doc_start[b, i] <= j <= i)."""
    if doc_start is not None:
        _check_doc_start(q, doc_start, causal)
    B, S, Hq, D = q.shape
    G = Hq // k.shape[2]
    qf = q.float().transpose(1, 2)
    kf = k.float().repeat_interleave(G, dim=2).transpose(1, 2)
    vf = v.float().repeat_interleave(G, dim=2).transpose(1, 2)
    s = (qf @ kf.transpose(-1, -2)) / math.sqrt(D)
    if doc_start is not None:
        s = s.masked_fill(~_doc_mask(doc_start, S), float("-inf"))
    elif causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    o = (torch.softmax(s, dim=-1) @ vf).transpose(1, 2).to(q.dtype)
    return (o, lse) if return_lse else o


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal):
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        o = torch.empty_like(q)
        lse2 = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        scale = 1.0 / math.sqrt(D)
        _native.check(_native.load().pto_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                                  lse2.data_ptr(), B, S, Hq, Hkv, D, scale, int(causal),
                                                  _stream(q)), "attn_fwd")
        ctx.save_for_backward(q, k, v, o, lse2)
        ctx.causal = causal
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse2 = ctx.saved_tensors
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        do = _c(do.to(q.dtype))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse2)
        _native.check(_native.load().pto_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                                  do.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                                  dk.data_ptr(), dv.data_ptr(), B, S, Hq, Hkv, D,
                                                  1.0 / math.sqrt(D), int(ctx.causal), _stream(q)), "attn_bwd")
        return dq, dk, dv, None


class _FlashAttentionDoc(torch.autograd.Function):
    """The document-masked passes (the attn_doc_* kernels of attention.hip): doc_start / doc_end int32 [B, S]."""

    @staticmethod
    def forward(ctx, q, k, v, doc_start, doc_end):
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        o = torch.empty_like(q)
        lse2 = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        _native.check(_native.load().pto_attn_doc_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                                      lse2.data_ptr(), doc_start.data_ptr(), B, S, Hq, Hkv, D,
                                                      1.0 / math.sqrt(D), _stream(q)), "attn_doc_fwd")
        ctx.save_for_backward(q, k, v, o, lse2, doc_start, doc_end)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse2, doc_start, doc_end = ctx.saved_tensors
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        do = _c(do.to(q.dtype))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse2)
        _native.check(_native.load().pto_attn_doc_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                                      do.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                                      dk.data_ptr(), dv.data_ptr(), doc_start.data_ptr(),
                                                      doc_end.data_ptr(), B, S, Hq, Hkv, D, 1.0 / math.sqrt(D),
                                                      _stream(q)), "attn_doc_bwd")
        return dq, dk, dv, None, None


# The int32 bounds of the doc_start tensor seen last: every layer of a step passes the same tensor,
# so the conversion and doc_end run once per batch.  The entry holds the source tensor (its storage
# cannot be reused while it is cached) and its version counter (an in-place edit invalidates it).
_doc_bounds_cache = None


def _doc_bounds(doc_start: torch.Tensor):
    global _doc_bounds_cache
    c = _doc_bounds_cache
    if c is not None and c[0] is doc_start and c[1] == doc_start._version:
        return c[2], c[3]
    ds = doc_start.to(torch.int32).contiguous()
    de = doc_ends(ds)
    _doc_bounds_cache = (doc_start, doc_start._version, ds, de)
    return ds, de


def set_doc_bounds(doc_start: torch.Tensor, doc_end: torch.Tensor) -> None:
    """Prime the one-entry bounds cache with bounds that are correct by construction (the batch
    kernel of ``ops/token_batch.py`` writes both): ``flash_attention(..., doc_start=doc_start)`` with
    this very tensor, unedited, then uses ``doc_end`` as given and calls neither ``doc_ends`` nor
    ``validate_doc_start``."""
    global _doc_bounds_cache
    if (doc_start.dtype != torch.int32 or doc_end.dtype != torch.int32 or doc_start.dim() != 2
            or doc_start.shape != doc_end.shape or doc_start.device != doc_end.device
            or not doc_start.is_contiguous() or not doc_end.is_contiguous()):
        raise ValueError("set_doc_bounds: two contiguous int32 [B, S] tensors on one device")
    _doc_bounds_cache = (doc_start, doc_start._version, doc_start, doc_end)


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                    doc_start: torch.Tensor = None) -> torch.Tensor:
    if doc_start is not None:
        _check_doc_start(q, doc_start, causal)
    if not q.is_cuda:
        return attention_reference(q, k, v, causal, doc_start=doc_start)
    if not hip_supported(q, k, v):
        raise ValueError(f"flash_attention: HIP path needs bf16 [B,S,H,D] with D in {HEAD_DIMS}, S % {SEQ_MULTIPLE} == 0 "
                         f"and Hq % Hkv == 0; got q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}")
    if doc_start is not None:
        return _FlashAttentionDoc.apply(_c(q), _c(k), _c(v), *_doc_bounds(doc_start))
    return _FlashAttention.apply(_c(q), _c(k), _c(v), bool(causal))


def sdpa_bshd(q, k, v, causal: bool = True, doc_start=None) -> torch.Tensor:
    """The library path on the same [B, S, H, D] layout (A/B baseline and non-HIP shapes).
    ``doc_start``: the document mask as a dense boolean [B, 1, S, S] ``attn_mask``."""
    if doc_start is not None:
        _check_doc_start(q, doc_start, causal)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                           attn_mask=_doc_mask(doc_start, q.shape[1]),
                                           enable_gqa=k.shape[2] != q.shape[2])
        return o.transpose(1, 2)
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=causal,
                                       enable_gqa=k.shape[2] != q.shape[2])
    return o.transpose(1, 2)
