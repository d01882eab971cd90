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
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import _native
from .llm import _DT, _aligned, _stream, rope_reference

HEAD_DIMS = (64, 128)
GROUPS = (1, 2, 4, 8)


class KVCache:
    """Keys and values of ``n_layers`` layers, ``k`` / ``v`` [L, B, max_len, Hkv, D], and ``lens``
    int32 [B] (valid rows per batch row) on the same device."""

    def __init__(self, n_layers: int, B: int, max_len: int, Hkv: int, D: int, dtype=torch.bfloat16, device=None):
        if min(n_layers, B, max_len, Hkv, D) <= 0:
            raise ValueError(f"KVCache: sizes must be positive, got {(n_layers, B, max_len, Hkv, D)}")
        self.k = torch.zeros(n_layers, B, max_len, Hkv, D, dtype=dtype, device=device)
        self.v = torch.zeros_like(self.k)
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


def _check_index(name, what, t, B, device):
    if t.dtype != torch.int32 or t.shape != (B,) or t.device != device:
        raise ValueError(f"{name}: {what} must be int32 [{B}] on {device}; got {t.dtype} {tuple(t.shape)} {t.device}")


# ------------------------------------------------------------------------------ rope_append
def rope_append_reference(qkv, cos, sin, k_layer, v_layer, pos, hq: int, hkv: int):
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
    k_layer[bi, row] = torch.where(ok, kr.to(k_layer.dtype), k_layer[bi, row])
    v_layer[bi, row] = torch.where(ok, v.reshape(B, hkv, D).to(v_layer.dtype), v_layer[bi, row])
    return qr


def rope_append(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, k_layer: torch.Tensor,
                v_layer: torch.Tensor, pos: torch.Tensor, hq: int, hkv: int) -> torch.Tensor:
    """q [B, hq, D] rotated at ``pos``; k (rotated) and v go to cache row ``pos[b]`` in place."""
    if qkv.dim() != 2 or hq <= 0 or hkv <= 0 or qkv.shape[1] % (hq + 2 * hkv):
        raise ValueError(f"rope_append: qkv must be [B, (hq + 2 hkv) * D]; got {tuple(qkv.shape)} hq {hq} hkv {hkv}")
    B, W = qkv.shape
    D = W // (hq + 2 * hkv)
    _check_cache("rope_append", k_layer, v_layer, B, hkv, D)
    _check_index("rope_append", "pos", pos, B, qkv.device)
    if D % 8 or cos.dim() != 2 or cos.shape[1] != D // 2 or cos.shape != sin.shape or cos.shape[0] < 1:
        raise ValueError(f"rope_append: D % 8 == 0 and tables [rows, D/2]; got D {D}, cos {tuple(cos.shape)}")
    if not qkv.is_cuda:
        return rope_append_reference(qkv, cos, sin, k_layer, v_layer, pos, hq, hkv)
    if qkv.dtype not in _DT or k_layer.dtype != qkv.dtype or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"rope_append: qkv and the caches must share fp32 or bf16 and be 16-byte aligned; got "
                         f"{qkv.dtype}, {k_layer.dtype}")
    qkv, cos, sin = _aligned(qkv), _aligned(cos.float()), _aligned(sin.float())
    q = qkv.new_empty(B, hq, D)
    _native.check(_native.load().pto_rope_append(
        qkv.data_ptr(), q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), cos.data_ptr(), sin.data_ptr(),
        pos.data_ptr(), B, k_layer.shape[1], cos.shape[0], hq, hkv, D, _DT[qkv.dtype], _stream(qkv)), "rope_append")
    return q


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
    return (q.dtype == k_layer.dtype == v_layer.dtype == torch.bfloat16 and D in HEAD_DIMS and hkv > 0
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
                     max_keys: Optional[int] = None, impl: str = "auto") -> torch.Tensor:
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
    if q.dtype != k_layer.dtype:
        raise ValueError(f"decode_attention: q and the caches must share a dtype; got {q.dtype}, {k_layer.dtype}")
    if not q.is_cuda:
        return decode_attention_reference(q, k_layer, v_layer, lens, max_keys)
    if impl == "sdpa":
        return decode_attention_sdpa(q, k_layer, v_layer, lens, max_keys)
    if not hip_supported(q, k_layer, v_layer) or k_layer.data_ptr() % 16 or v_layer.data_ptr() % 16:
        raise ValueError(f"decode_attention: the HIP path needs bf16, D in {HEAD_DIMS}, Hq / Hkv in {GROUPS} and "
                         f"16-byte aligned caches (impl='sdpa' serves other shapes); got q {tuple(q.shape)} "
                         f"{q.dtype}, caches {tuple(k_layer.shape)}")
    lib = _native.load()
    q = _aligned(q)
    nchunks = -(-max_keys // int(lib.pto_decode_chunk()))
    rows = B * hq * nchunks
    ws = _partials(q.device, rows * (D + 2))
    po, pm, pl = ws[:rows * D], ws[rows * D:rows * (D + 1)], ws[rows * (D + 1):rows * (D + 2)]
    o = torch.empty_like(q)
    _native.check(lib.pto_decode_attn(q.data_ptr(), k_layer.data_ptr(), v_layer.data_ptr(), lens.data_ptr(),
                                      o.data_ptr(), po.data_ptr(), pm.data_ptr(), pl.data_ptr(), B, max_len,
                                      max_keys, hq, k_layer.shape[2], D, nchunks, _stream(q)), "decode_attn")
    return o
