"""KV cache, RoPE-and-append and single-query attention over the cache
(``csrc/kernels/decode_attention.hip``): the decode step of ``models.llama.Llama.generate``.

``KVCache`` holds every layer's keys and values, token-major like the attention kernels
([L, B, max_len, Hkv, D]), and the number of valid rows per batch row (``lens``, int32, on the
device: the decode loop never reads it on the host).

``rope_append(qkv, cos, sin, k_layer, v_layer, pos, hq, hkv)``: the decode step's packed
projection [B, (hq + 2 hkv) * D] -> q [B, hq, D] rotated at ``pos[b]``; the rotated k and v are
stored at cache row ``pos[b]`` (a ``pos`` outside the cache stores nothing).

``decode_attention(q, k_layer, v_layer, lens, max_keys, impl)``: o [B, hq, D] =
softmax(q . K[:n]^T / sqrt(D)) . V[:n] per batch row, n = min(lens[b], max_keys); cache rows at or
past n never reach the result, whatever they hold.  ``impl``: "auto" = the HIP kernels on a GPU (an
unsupported shape is an error, never a silent fallback) and the PyTorch math on CPU; "sdpa" = the
library path (``scaled_dot_product_attention`` over the cache with a length mask): the A/B baseline,
and the path for shapes the kernel does not cover (fp32 caches, other head dims).

An FP8 cache (``KVCache(..., dtype=torch.float8_e4m3fn)``, ``csrc/kernels/decode_attention_fp8.hip``):
``k`` / ``v`` hold e4m3 codes in the same layout and ``k_scale`` / ``v_scale`` [L, B, Hkv, max_len_pad]
one fp32 power-of-two scale per (token, kv head), by the rule of ``ops.skinny.quantize_rows`` applied to
the bf16 row the bf16 cache would hold.  ``rope_append`` and ``decode_attention`` take the layer's scales as
``k_scale`` / ``v_scale``; ``quantize_kv(k, v, ...)`` is the prefill's copy.  Dequantisation is exact in
bf16: the attention is the bf16 attention on the dequantised cache.  q stays bf16; ``impl="sdpa"`` does not
serve an FP8 cache.

``append_rows`` / ``attend_rows`` (``csrc/kernels/decode_attention_multi.hip``, and
``decode_attention_multi_fp8.hip`` on an FP8 cache) are the same two steps for S tokens per sequence; see the end
of this file.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import _native
from .llm import _DT, _aligned, _stream, rope_reference
from .skinny import dequantize_rows, quantize_rows

HEAD_DIMS = (64, 128)
GROUPS = (1, 2, 4, 8)
FP8 = torch.float8_e4m3fn


class KVCache:
    """Keys and values of ``n_layers`` layers, ``k`` / ``v`` [L, B, max_len, Hkv, D], and ``lens``
    int32 [B] (valid rows per batch row) on the same device.  With ``dtype=torch.float8_e4m3fn`` also
    ``k_scale`` / ``v_scale`` fp32 [L, B, Hkv, max_len rounded up to a multiple of 4] (else None)."""

    def __init__(self, n_layers: int, B: int, max_len: int, Hkv: int, D: int, dtype=torch.bfloat16, device=None):
        if min(n_layers, B, max_len, Hkv, D) <= 0:
            raise ValueError(f"KVCache: sizes must be positive, got {(n_layers, B, max_len, Hkv, D)}")
        self.k = torch.zeros(n_layers, B, max_len, Hkv, D, dtype=dtype, device=device)
        self.v = torch.zeros_like(self.k)
        self.k_scale = self.v_scale = None
        if dtype == FP8:
            self.k_scale = torch.ones(n_layers, B, Hkv, -(-max_len // 4) * 4, dtype=torch.float32, device=device)
            self.v_scale = torch.ones_like(self.k_scale)
        self.lens = torch.zeros(B, dtype=torch.int32, device=device)
        self.max_len = max_len
        self.rope = None  # (cos, sin) tables of the model that fills the cache, built on first use

    def layer(self, i: int):
        return self.k[i], self.v[i]


def _check_cache(name, k_layer, v_layer, B, hkv, D):
    if k_layer.dim() != 4 or k_layer.shape != v_layer.shape or k_layer.dtype != v_layer.dtype or \
            k_layer.shape[0] != B or k_layer.shape[2] != hkv or k_layer.shape[3] != D:
        raise ValueError(f"{name}: caches must both be [B={B}, max_len, Hkv={hkv}, D={D}] of one dtype; got "
                         f"{tuple(k_layer.shape)} {k_layer.dtype}, {tuple(v_layer.shape)} {v_layer.dtype}")
    if not (k_layer.is_contiguous() and v_layer.is_contiguous()):
        raise ValueError(f"{name}: the cache layers must be contiguous (they are written in place)")


def _check_scales(name, k_layer, k_scale, v_scale) -> bool:
    """True for an FP8 cache with its scales; a ``ValueError`` where cache and scales do not go together."""
    if k_layer.dtype != FP8:
        if k_scale is not None or v_scale is not None:
            raise ValueError(f"{name}: k_scale / v_scale go with an e4m3 cache; the caches are {k_layer.dtype}")
        return False
    B, max_len, hkv, _ = k_layer.shape
    for what, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is None:
            raise ValueError(f"{name}: an e4m3 cache needs k_scale and v_scale (KVCache allocates them)")
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[:2] != (B, hkv) or t.shape[2] < max_len or \
                t.shape[2] % 4 or t.device != k_layer.device or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous fp32 [B={B}, Hkv={hkv}, >= {max_len} and a multiple "
                             f"of 4] on {k_layer.device}; got {t.dtype} {tuple(t.shape)} {t.device}")
    if k_scale.shape != v_scale.shape:
        raise ValueError(f"{name}: k_scale and v_scale differ in shape: {tuple(k_scale.shape)}, {tuple(v_scale.shape)}")
    return True


def _fp8_hip_ok(name, x, k_layer, v_layer, k_scale, v_scale, D):
    if x.dtype != torch.bfloat16 or D not in HEAD_DIMS or any(
            t.data_ptr() % 16 for t in (k_layer, v_layer, k_scale, v_scale)):
        raise ValueError(f"{name}: the HIP path on an e4m3 cache needs bf16 input, D in {HEAD_DIMS} and 16-byte "
                         f"aligned caches and scales; got {x.dtype}, D {D}")


def _quantize_heads(x: torch.Tensor):
    """[..., D] -> e4m3 codes of the bf16-rounded rows and their scales [...] (the PyTorch path)."""
    q, s = quantize_rows(x.to(torch.bfloat16).reshape(-1, x.shape[-1]))
    return q.view(x.shape), s.view(x.shape[:-1])


def dequantize_cache(layer: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """An e4m3 cache layer [B, max_len, Hkv, D] and its scales [B, Hkv, >= max_len] -> the cache in ``dtype``
    (exact in bf16 and wider)."""
    s = scale[:, :, :layer.shape[1]].transpose(1, 2)
    return dequantize_rows(layer.reshape(-1, layer.shape[-1]), s.reshape(-1), dtype).view(layer.shape)


def _check_index(name, what, t, B, device):
    if t.dtype != torch.int32 or t.shape != (B,) or t.device != device:
        raise ValueError(f"{name}: {what} must be int32 [{B}] on {device}; got {t.dtype} {tuple(t.shape)} {t.device}")


# ------------------------------------------------------------------------------ rope_append
def rope_append_reference(qkv, cos, sin, k_layer, v_layer, pos, hq: int, hkv: int, k_scale=None, v_scale=None):
    B, W = qkv.shape
    D = W // (hq + 2 * hkv)
    max_len = k_layer.shape[1]
    q, k, v = qkv.split([hq * D, hkv * D, hkv * D], dim=-1)
    p = pos.long()
    pt = p.clamp(0, cos.shape[0] - 1)
    # rope_reference takes [B, S, H, D] with tables [S, D/2]: one "sequence" of B rows, each at its own position
    c, s = cos[pt], sin[pt]
    qr = rope_reference(q.reshape(1, B, hq, D), c, s)[0]
    kr = rope_reference(k.reshape(1, B, hkv, D), c, s)[0]
    ok = ((p >= 0) & (p < max_len)).view(B, 1, 1)
    bi, row = torch.arange(B, device=qkv.device), p.clamp(0, max_len - 1)
    # a position outside the cache rewrites row 0 / max_len - 1 with what it already holds
    if k_layer.dtype == FP8:
        hi = torch.arange(hkv, device=qkv.device)
        for layer, scale, new in ((k_layer, k_scale, kr), (v_layer, v_scale, v.reshape(B, hkv, D))):
            code, sc = _quantize_heads(new)
            bytes_, at = layer.view(torch.uint8), (bi[:, None], hi[None, :], row[:, None])
            bytes_[bi, row] = torch.where(ok, code.view(torch.uint8), bytes_[bi, row])
            scale[at] = torch.where(ok.view(B, 1), sc, scale[at])
        return qr
    k_layer[bi, row] = torch.where(ok, kr.to(k_layer.dtype), k_layer[bi, row])
    v_layer[bi, row] = torch.where(ok, v.reshape(B, hkv, D).to(v_layer.dtype), v_layer[bi, row])
    return qr


def rope_append(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_layer: torch.Tensor,
                v_layer: torch.Tensor, pos: torch.Tensor, hq: int, hkv: int,
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B, hq, D] rotated at ``pos``; k (rotated) and v go to cache row ``pos[b]`` in place -- quantised,
    with their scales to ``k_scale`` / ``v_scale`` [B, hkv, max_len_pad], when the cache is e4m3."""
    if qkv.dim() != 2 or hq <= 0 or hkv <= 0 or qkv.shape[1] % (hq + 2 * hkv):
        raise ValueError(f"rope_append: qkv must be [B, (hq + 2 hkv) * D]; got {tuple(qkv.shape)} hq {hq} hkv {hkv}")
    B, W = qkv.shape
    D = W // (hq + 2 * hkv)
    _check_cache("rope_append", k_layer, v_layer, B, hkv, D)
    _check_index("rope_append", "pos", pos, B, qkv.device)
    if D % 8 or cos.dim() != 2 or cos.shape[1] != D // 2 or cos.shape != sin.shape or cos.shape[0] < 1:
        raise ValueError(f"rope_append: D % 8 == 0 and tables [rows, D/2]; got D {D}, cos {tuple(cos.shape)}")
    fp8 = _check_scales("rope_append", k_layer, k_scale, v_scale)
    if not qkv.is_cuda:
        return rope_append_reference(qkv, cos, sin, k_layer, v_layer, pos, hq, hkv, k_scale, v_scale)
    if fp8:
        _fp8_hip_ok("rope_append", qkv, k_layer, v_layer, k_scale, v_scale, D)
        qkv, cos, sin = _aligned(qkv), _aligned(cos.float()), _aligned(sin.float())
        q = qkv.new_empty(B, hq, D)
        _native.check(_native.load().pto_rope_append_fp8(
            qkv.data_ptr(), q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), k_scale.data_ptr(),
            v_scale.data_ptr(), k_scale.shape[2], cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), B, k_layer.shape[1],
            cos.shape[0], hq, hkv, D, _DT[qkv.dtype], _stream(qkv)), "rope_append_fp8")
        return q
    if qkv.dtype not in _DT or k_layer.dtype != qkv.dtype or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"rope_append: qkv and the caches must share fp32 or bf16 and be 16-byte aligned; got "
                         f"{qkv.dtype}, {k_layer.dtype}")
    qkv, cos, sin = _aligned(qkv), _aligned(cos.float()), _aligned(sin.float())
    q = qkv.new_empty(B, hq, D)
    _native.check(_native.load().pto_rope_append(
        qkv.data_ptr(), q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), cos.data_ptr(), sin.data_ptr(),
        pos.data_ptr(), B, k_layer.shape[1], cos.shape[0], hq, hkv, D, _DT[qkv.dtype], _stream(qkv)), "rope_append")
    return q


# ------------------------------------------------------------------------------ quantize_kv
def quantize_kv(k: torch.Tensor, v: torch.Tensor, k_layer: torch.Tensor, v_layer: torch.Tensor,
                k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
    """The prefill's copy into an e4m3 cache: rows [0, n), n = min(S, max_len), of ``k`` / ``v`` [B, S, Hkv, D]
    (as ``rope_qkv`` returns them) are rounded to bf16, quantised per (token, head) and stored with their
    scales: byte for byte what ``rope_append`` stores for the same token at the same position."""
    if k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype or k.device != k_layer.device:
        raise ValueError(f"quantize_kv: k and v must be [B, S, Hkv, D] of one dtype on the cache's device; got "
                         f"{tuple(k.shape)} {k.dtype}, {tuple(v.shape)} {v.dtype}")
    B, S, hkv, D = k.shape
    _check_cache("quantize_kv", k_layer, v_layer, B, hkv, D)
    if not _check_scales("quantize_kv", k_layer, k_scale, v_scale):
        raise ValueError(f"quantize_kv: the caches must be e4m3; got {k_layer.dtype}")
    max_len = k_layer.shape[1]
    n = min(S, max_len)
    if not k.is_cuda:
        for src, layer, scale in ((k, k_layer, k_scale), (v, v_layer, v_scale)):
            code, sc = _quantize_heads(src[:, :n])
            layer.view(torch.uint8)[:, :n] = code.view(torch.uint8)
            scale[:, :, :n] = sc.transpose(1, 2)
        return
    _fp8_hip_ok("quantize_kv", k, k_layer, v_layer, k_scale, v_scale, D)
    k, v = _aligned(k), _aligned(v)
    _native.check(_native.load().pto_kv_quantize(
        k.data_ptr(), v.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
        k_scale.shape[2], B, S, max_len, hkv, D, _stream(k)), "kv_quantize")


# -------------------------------------------------------------------------- decode_attention
def _valid(lens: torch.Tensor, max_keys: int) -> torch.Tensor:
    """bool [B, max_keys]: key j of row b is one of the first min(lens[b], max_keys)."""
    return torch.arange(max_keys, device=lens.device).view(1, -1) < lens.view(-1, 1)


def decode_attention_reference(q, k_layer, v_layer, lens, max_keys: Optional[int] = None) -> torch.Tensor:
    """The same math in PyTorch, fp32 inside, masked by selection (the CPU path)."""
    B, hq, D = q.shape
    hkv = k_layer.shape[2]
    mk = k_layer.shape[1] if max_keys is None else max_keys
    valid = _valid(lens, mk)                                                   # [B, mk]
    sel = valid.view(B, mk, 1, 1)
    with torch.autocast(device_type=q.device.type, enabled=False):            # the products stay fp32
        k = torch.where(sel, k_layer[:, :mk].float(), 0.0).repeat_interleave(hq // hkv, dim=2)   # [B, mk, hq, D]
        v = torch.where(sel, v_layer[:, :mk].float(), 0.0).repeat_interleave(hq // hkv, dim=2)
        s = torch.einsum("bhd,bjhd->bhj", q.float(), k) / math.sqrt(D)
        s = torch.where(valid.view(B, 1, mk), s, -math.inf)
        p = torch.softmax(s, dim=-1)
        p = torch.where(valid.view(B, 1, mk), p, 0.0)                         # lens 0: softmax of all -inf is NaN
        return torch.einsum("bhj,bjhd->bhd", p, v).to(q.dtype)


def decode_attention_sdpa(q, k_layer, v_layer, lens, max_keys: Optional[int] = None) -> torch.Tensor:
    """The library path.  The G = hq / hkv query heads of a kv head are the "sequence" of an SDPA
    call with hkv heads, so K and V are not expanded; invalid rows are replaced by zeros first (a
    masked score does not stop 0 * NaN in P.V) and rows without a key give zeros."""
    B, hq, D = q.shape
    hkv = k_layer.shape[2]
    mk = k_layer.shape[1] if max_keys is None else max_keys
    valid = _valid(lens, mk)
    sel = valid.view(B, mk, 1, 1)
    k = torch.where(sel, k_layer[:, :mk], 0.0).transpose(1, 2)                 # [B, hkv, mk, D]
    v = torch.where(sel, v_layer[:, :mk], 0.0).transpose(1, 2)
    o = F.scaled_dot_product_attention(q.reshape(B, hkv, hq // hkv, D), k, v, attn_mask=valid.view(B, 1, 1, mk))
    o = torch.where((lens > 0).view(B, 1, 1, 1), o, 0.0)
    return o.reshape(B, hq, D)


def hip_supported(q: torch.Tensor, k_layer: torch.Tensor, v_layer: torch.Tensor) -> bool:
    if not (q.is_cuda and k_layer.is_cuda and v_layer.is_cuda) or q.dim() != 3 or k_layer.dim() != 4:
        return False
    B, hq, D = q.shape
    hkv = k_layer.shape[2]
    return (q.dtype == torch.bfloat16 and k_layer.dtype == v_layer.dtype and k_layer.dtype in (torch.bfloat16, FP8)
            and D in HEAD_DIMS and hkv > 0
            and hq % hkv == 0 and hq // hkv in GROUPS and B <= 65535 and hkv <= 65535)


# fp32 partials of the key chunks, per (device, stream): grown on demand, reused by every call on that
# stream (calls on one stream run in order; two streams never share a buffer).  The combine kernel
# reads only the chunks that this call's lens make valid, all written by this call.
_workspace = {}


def _partials(device, floats: int) -> torch.Tensor:
    key = (device, _native.current_stream_ptr(device))
    ws = _workspace.get(key)
    if ws is None or ws.numel() < floats:
        ws = _workspace[key] = torch.empty(floats, dtype=torch.float32, device=device)
    return ws


def decode_attention(q: torch.Tensor, k_layer: torch.Tensor, v_layer: torch.Tensor, lens: torch.Tensor,
                     max_keys: Optional[int] = None, impl: str = "auto",
                     k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    if impl not in ("auto", "sdpa"):
        raise ValueError(f"decode_attention: impl must be 'auto' or 'sdpa', got {impl!r}")
    if q.dim() != 3 or k_layer.dim() != 4 or k_layer.shape[2] <= 0 or q.shape[1] % max(k_layer.shape[2], 1):
        raise ValueError(f"decode_attention: q [B, Hq, D] and caches [B, max_len, Hkv, D] with Hq % Hkv == 0; got "
                         f"{tuple(q.shape)}, {tuple(k_layer.shape)}")
    B, hq, D = q.shape
    _check_cache("decode_attention", k_layer, v_layer, B, k_layer.shape[2], D)
    _check_index("decode_attention", "lens", lens, B, q.device)
    max_len = k_layer.shape[1]
    if max_keys is None:
        max_keys = max_len
    if not isinstance(max_keys, int) or not 1 <= max_keys <= max_len:
        raise ValueError(f"decode_attention: max_keys must be an int in [1, max_len = {max_len}], got {max_keys!r}")
    fp8 = _check_scales("decode_attention", k_layer, k_scale, v_scale)
    if fp8 and impl == "sdpa":
        raise ValueError("decode_attention: impl='sdpa' does not serve an e4m3 cache (the library path needs q and "
                         "the cache in one dtype)")
    if not fp8 and q.dtype != k_layer.dtype:
        raise ValueError(f"decode_attention: q and the caches must share a dtype; got {q.dtype}, {k_layer.dtype}")
    if not q.is_cuda:
        if fp8:  # rows past the lengths may hold anything, NaN codes and scales included: selection hides them
            k_layer, v_layer = dequantize_cache(k_layer, k_scale, q.dtype), dequantize_cache(v_layer, v_scale, q.dtype)
        return decode_attention_reference(q, k_layer, v_layer, lens, max_keys)
    if impl == "sdpa":
        return decode_attention_sdpa(q, k_layer, v_layer, lens, max_keys)
    if not hip_supported(q, k_layer, v_layer) or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"decode_attention: the HIP path needs bf16 (or a bf16 q with e4m3 caches), D in {HEAD_DIMS}, "
                         f"Hq / Hkv in {GROUPS} and 16-byte aligned caches (impl='sdpa' serves other shapes); got q "
                         f"{tuple(q.shape)} {q.dtype}, caches {tuple(k_layer.shape)} {k_layer.dtype}")
    if fp8:
        _fp8_hip_ok("decode_attention", q, k_layer, v_layer, k_scale, v_scale, D)
    lib = _native.load()
    q = _aligned(q)
    nchunks = -(-max_keys // int(lib.pto_decode_chunk()))
    rows = B * hq * nchunks
    ws = _partials(q.device, rows * (D + 2))
    po, pm, pl = ws[:rows * D], ws[rows * D:rows * (D + 1)], ws[rows * (D + 1):rows * (D + 2)]
    o = torch.empty_like(q)
    if fp8:
        _native.check(lib.pto_decode_attn_fp8(q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), k_scale.data_ptr(),
                                              v_scale.data_ptr(), k_scale.shape[2], lens.data_ptr(), o.data_ptr(),
                                              po.data_ptr(), pm.data_ptr(), pl.data_ptr(), B, max_len, max_keys, hq,
                                              k_layer.shape[2], D, nchunks, _stream(q)), "decode_attn_fp8")
        return o
    _native.check(lib.pto_decode_attn(q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), lens.data_ptr(),
                                      o.data_ptr(), po.data_ptr(), pm.data_ptr(), pl.data_ptr(), B, max_len,
                                      max_keys, hq, k_layer.shape[2], D, nchunks, _stream(q)), "decode_attn")
    return o


# ------------------------------------------------------------- S tokens per sequence in one step
# csrc/kernels/decode_attention_multi.hip: a step over S tokens per sequence (the verification step of
# speculative decoding, or a few tokens appended to an existing cache).  ``append_rows`` is ``rope_append`` for
# qkv [B, S, W]: token s of sequence b is rotated at ``pos[b] + s`` and stored at that cache row (a row outside
# the cache stores nothing, token by token).  ``attend_rows`` is ``decode_attention`` for q [B, S, Hq, D]: query s
# sees the keys j < n_s, n_s = min(lens[b], max_keys) - (S - 1 - s), ``lens`` counting the rows after the append;
# n_s <= 0 gives a zero row.  The HIP kernel takes the S * Hq / Hkv query rows of a kv head as the 16 columns of
# one MFMA tile: bf16, D in HEAD_DIMS, S * Hq / Hkv <= MAX_QUERY_ROWS; ``impl="sdpa"`` serves the rest.
# An e4m3 cache (csrc/kernels/decode_attention_multi_fp8.hip) takes the layer's scales as ``k_scale`` / ``v_scale``,
# as ``rope_append`` and ``decode_attention`` do: the append stores byte for byte what S calls of ``rope_append``
# store, the attention is the bf16 one on the dequantised cache with both products on the MFMA, under the same
# shape limits; ``impl="sdpa"`` does not serve it.
MAX_QUERY_ROWS = 16


def _row_lens(lens, max_keys: int, S: int, s: int) -> torch.Tensor:
    return lens.clamp(max=max_keys) - (S - 1 - s)


def append_rows(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_layer: torch.Tensor,
                v_layer: torch.Tensor, pos: torch.Tensor, hq: int, hkv: int,
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B, S, hq, D], token s rotated at ``pos[b] + s``; its k (rotated) and v go to that cache row in place --
    quantised, with their scales to ``k_scale`` / ``v_scale`` [B, hkv, max_len_pad], when the cache is e4m3."""
    if qkv.dim() != 3 or hq <= 0 or hkv <= 0 or qkv.shape[1] < 1 or qkv.shape[2] % (hq + 2 * hkv):
        raise ValueError(f"append_rows: qkv must be [B, S, (hq + 2 hkv) * D]; got {tuple(qkv.shape)} hq {hq} hkv {hkv}")
    B, S, W = qkv.shape
    D = W // (hq + 2 * hkv)
    _check_cache("append_rows", k_layer, v_layer, B, hkv, D)
    _check_index("append_rows", "pos", pos, B, qkv.device)
    if D % 8 or cos.dim() != 2 or cos.shape[1] != D // 2 or cos.shape != sin.shape or cos.shape[0] < 1:
        raise ValueError(f"append_rows: D % 8 == 0 and tables [rows, D/2]; got D {D}, cos {tuple(cos.shape)}")
    fp8 = _check_scales("append_rows", k_layer, k_scale, v_scale)
    if not qkv.is_cuda:
        return torch.stack([rope_append_reference(qkv[:, s], cos, sin, k_layer, v_layer, pos + s, hq, hkv,
                                                  k_scale, v_scale) for s in range(S)], dim=1)
    if fp8:
        _fp8_hip_ok("append_rows", qkv, k_layer, v_layer, k_scale, v_scale, D)
        qkv, cos, sin = _aligned(qkv), _aligned(cos.float()), _aligned(sin.float())
        q = qkv.new_empty(B, S, hq, D)
        _native.check(_native.load().pto_rope_append_multi_fp8(
            qkv.data_ptr(), q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), k_scale.data_ptr(),
            v_scale.data_ptr(), k_scale.shape[2], cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), B, S,
            k_layer.shape[1], cos.shape[0], hq, hkv, D, _DT[qkv.dtype], _stream(qkv)), "rope_append_multi_fp8")
        return q
    if qkv.dtype not in _DT or k_layer.dtype != qkv.dtype or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"append_rows: qkv and the caches must share fp32 or bf16 and be 16-byte aligned; got "
                         f"{qkv.dtype}, {k_layer.dtype}")
    qkv, cos, sin = _aligned(qkv), _aligned(cos.float()), _aligned(sin.float())
    q = qkv.new_empty(B, S, hq, D)
    _native.check(_native.load().pto_rope_append_multi(
        qkv.data_ptr(), q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), cos.data_ptr(), sin.data_ptr(),
        pos.data_ptr(), B, S, k_layer.shape[1], cos.shape[0], hq, hkv, D, _DT[qkv.dtype], _stream(qkv)),
        "rope_append_multi")
    return q


def attend_rows_sdpa(q, k_layer, v_layer, lens, max_keys: int) -> torch.Tensor:
    """The library path: the S * G query rows of a kv head are the "sequence" of one SDPA call with a mask per
    row; rows past the lengths are replaced by zeros first and rows without a key give zeros."""
    B, S, hq, D = q.shape
    hkv = k_layer.shape[2]
    G = hq // hkv
    n = torch.stack([_row_lens(lens, max_keys, S, s) for s in range(S)], dim=1)            # [B, S]
    keys = torch.arange(max_keys, device=q.device).view(1, 1, -1)
    mask = (keys < n.view(B, S, 1)).view(B, 1, S, 1, max_keys).expand(B, 1, S, G, max_keys)
    sel = _valid(lens, max_keys).view(B, max_keys, 1, 1)
    k = torch.where(sel, k_layer[:, :max_keys], 0.0).transpose(1, 2)                       # [B, hkv, mk, D]
    v = torch.where(sel, v_layer[:, :max_keys], 0.0).transpose(1, 2)
    qs = q.view(B, S, hkv, G, D).permute(0, 2, 1, 3, 4).reshape(B, hkv, S * G, D)
    o = F.scaled_dot_product_attention(qs, k, v, attn_mask=mask.reshape(B, 1, S * G, max_keys))
    o = o.view(B, hkv, S, G, D).permute(0, 2, 1, 3, 4).reshape(B, S, hq, D)
    return torch.where((n > 0).view(B, S, 1, 1), o, 0.0)


def rows_supported(q: torch.Tensor, k_layer: torch.Tensor, v_layer: torch.Tensor) -> bool:
    """The HIP ``attend_rows`` serves q [B, S, Hq, D] over these caches."""
    if not (q.is_cuda and k_layer.is_cuda and v_layer.is_cuda) or q.dim() != 4 or k_layer.dim() != 4:
        return False
    B, S, hq, D = q.shape
    hkv = k_layer.shape[2]
    return (q.dtype == torch.bfloat16 and k_layer.dtype == v_layer.dtype and k_layer.dtype in (torch.bfloat16, FP8)
            and D in HEAD_DIMS and hkv > 0 and S >= 1 and hq % hkv == 0 and S * (hq // hkv) <= MAX_QUERY_ROWS
            and B <= 65535 and hkv <= 65535)


def attend_rows(q: torch.Tensor, k_layer: torch.Tensor, v_layer: torch.Tensor, lens: torch.Tensor,
                max_keys: Optional[int] = None, impl: str = "auto",
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """o [B, S, Hq, D]: query s of sequence b over the first n_s = min(lens[b], max_keys) - (S - 1 - s) cache rows;
    ``k_scale`` / ``v_scale`` are the layer's scales when the cache is e4m3."""
    if impl not in ("auto", "sdpa"):
        raise ValueError(f"attend_rows: impl must be 'auto' or 'sdpa', got {impl!r}")
    if q.dim() != 4 or k_layer.dim() != 4 or k_layer.shape[2] <= 0 or q.shape[1] < 1 or \
            q.shape[2] % max(k_layer.shape[2], 1):
        raise ValueError(f"attend_rows: q [B, S, Hq, D] and caches [B, max_len, Hkv, D] with Hq % Hkv == 0; got "
                         f"{tuple(q.shape)}, {tuple(k_layer.shape)}")
    B, S, hq, D = q.shape
    _check_cache("attend_rows", k_layer, v_layer, B, k_layer.shape[2], D)
    _check_index("attend_rows", "lens", lens, B, q.device)
    max_len = k_layer.shape[1]
    if max_keys is None:
        max_keys = max_len
    if not isinstance(max_keys, int) or not 1 <= max_keys <= max_len:
        raise ValueError(f"attend_rows: max_keys must be an int in [1, max_len = {max_len}], got {max_keys!r}")
    fp8 = _check_scales("attend_rows", k_layer, k_scale, v_scale)
    if fp8 and impl == "sdpa":
        raise ValueError("attend_rows: impl='sdpa' does not serve an e4m3 cache (the library path needs q and the "
                         "cache in one dtype)")
    if not fp8 and q.dtype != k_layer.dtype:
        raise ValueError(f"attend_rows: q and the caches must share a dtype; got {q.dtype}, {k_layer.dtype}")
    if not q.is_cuda:
        if fp8:  # rows past the lengths may hold anything, NaN codes and scales included: selection hides them
            k_layer, v_layer = dequantize_cache(k_layer, k_scale, q.dtype), dequantize_cache(v_layer, v_scale, q.dtype)
        return torch.stack([decode_attention_reference(q[:, s], k_layer, v_layer, _row_lens(lens, max_keys, S, s),
                                                       max_keys) for s in range(S)], dim=1)
    if impl == "sdpa":
        return attend_rows_sdpa(q, k_layer, v_layer, lens, max_keys)
    if not rows_supported(q, k_layer, v_layer) or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"attend_rows: the HIP path needs bf16 (or a bf16 q with e4m3 caches), D in {HEAD_DIMS}, "
                         f"S * Hq / Hkv <= {MAX_QUERY_ROWS} and 16-byte aligned caches (impl='sdpa' serves other "
                         f"bf16 shapes); got q {tuple(q.shape)} {q.dtype}, caches {tuple(k_layer.shape)} {k_layer.dtype}")
    if fp8:
        _fp8_hip_ok("attend_rows", q, k_layer, v_layer, k_scale, v_scale, D)
    lib = _native.load()
    q = _aligned(q)
    nchunks = -(-max_keys // int(lib.pto_decode_chunk()))
    rows = B * S * hq * nchunks
    ws = _partials(q.device, rows * (D + 2))
    po, pm, pl = ws[:rows * D], ws[rows * D:rows * (D + 1)], ws[rows * (D + 1):rows * (D + 2)]
    o = torch.empty_like(q)
    if fp8:
        _native.check(lib.pto_decode_attn_multi_fp8(
            q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
            k_scale.shape[2], lens.data_ptr(), o.data_ptr(), po.data_ptr(), pm.data_ptr(), pl.data_ptr(), B, S,
            max_len, max_keys, hq, k_layer.shape[2], D, nchunks, _stream(q)), "decode_attn_multi_fp8")
        return o
    _native.check(lib.pto_decode_attn_multi(q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), lens.data_ptr(),
                                            o.data_ptr(), po.data_ptr(), pm.data_ptr(), pl.data_ptr(), B, S, max_len,
                                            max_keys, hq, k_layer.shape[2], D, nchunks, _stream(q)),
                  "decode_attn_multi")
    return o
