"""Llama-3 decoder for the BASELINE "Llama-3 8B DDP bf16" PyTorchJob config.

Not part of the reference (MNIST only); BASELINE.json names it as the large-model job
shape: Master=1 Worker=7, 288 GB HBM sizing, OnFailure restarts + gang scheduling.
Plain DDP fits on MI355X: 8.0 B parameters in fp32 (32 GB) + fp32 grads (32 GB) + AdamW
moments (64 GB) + bf16 activations for a 2 k-token sequence stay well inside 288 GB, so
no sharding is needed -- every rank keeps the whole model and only gradients cross xGMI.

Architecture (Meta's reference layout): token embedding, ``n_layers`` x [RMSNorm ->
GQA attention with RoPE (theta 500 000) -> residual, RMSNorm -> SwiGLU FFN -> residual],
final RMSNorm, untied output projection.  Matmuls run in bf16 under autocast
(hipBLASLt); attention runs the hand-written HIP flash attention (``ops.attention``, forward
and backward on MFMA, token-major [B, S, H, D] in and out, so no transposes around it) for
bf16 head_dim-128 and head_dim-64 shapes and ``scaled_dot_product_attention`` otherwise (``impl`` = "sdpa"
forces the library path for A/B runs).
The elementwise work between the matmuls runs as hand-written HIP kernels on a GPU:
RMSNorm (``ops.norm``, fp32 statistics over the fp32 residual stream, bf16 output under
autocast so the next matmul reads it directly), RoPE and SwiGLU (``ops.llm``, one HBM pass
each, fwd and bwd).  On CPU the same math runs in PyTorch.

``Llama.generate`` writes text: ``prefill`` fills a KV cache from the prompts, ``decode_step`` appends
one token per sequence and attends over the cache with the single-query HIP kernels of ``ops.decode``.
``decode_steps`` appends several tokens per sequence in one step (the multi-query MFMA kernel); with a
``draft`` model ``generate`` uses it to verify the draft's tokens (greedy speculative decoding).
"""
from __future__ import annotations

import collections
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class LlamaConfig:
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    vocab_size: int = 128256
    ffn_hidden: int = 14336
    norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    max_seq_len: int = 8192

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    def num_params(self) -> int:
        d, f, v, L = self.dim, self.ffn_hidden, self.vocab_size, self.n_layers
        kv = self.n_kv_heads * self.head_dim
        per_layer = d * d * 2 + d * kv * 2 + 3 * d * f + 2 * d
        return L * per_layer + 2 * v * d + d


CONFIGS = {
    "llama3-8b": LlamaConfig(),
    "llama3-1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_hidden=8192),
    "llama-tiny": LlamaConfig(dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=256, ffn_hidden=128,
                              max_seq_len=256),
    # smallest config with the 8B model's head_dim (128): exercises the HIP flash attention
    "llama-mini": LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, ffn_hidden=1024,
                              max_seq_len=1024),
    # the same at the 1B model's head_dim (64)
    "llama-mini64": LlamaConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, ffn_hidden=512,
                                max_seq_len=1024),
}


def rope_tables(head_dim: int, seq_len: int, theta: float, device=None):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device, dtype=torch.float32) / head_dim))
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    ang = torch.outer(t, inv)  # [S, D/2]
    return torch.cos(ang), torch.sin(ang)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [B, S, H, D]; rotates adjacent pairs (x0, x1) like Meta's complex formulation."""
    from ..ops.llm import rope
    return rope(x, cos, sin)


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ..ops.norm import rms_norm
        out_dtype = None
        if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
            out_dtype = torch.get_autocast_dtype("cuda")  # consumed by a bf16 matmul next
        return rms_norm(x, self.weight, self.eps, out_dtype)

    fuse_residual = True  # False: plain add + norm (A/B of the residual-fused kernels)

    def add_forward(self, x: torch.Tensor, delta: Optional[torch.Tensor]):
        """(x + delta, norm(x + delta)) -- the residual add fused into this norm."""
        if delta is None:
            return x, self(x)
        if not self.fuse_residual:
            s = x + delta
            return s, self(s)
        from ..ops.norm import add_rms_norm
        out_dtype = None
        if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
            out_dtype = torch.get_autocast_dtype("cuda")
        return add_rms_norm(x, delta, self.weight, self.eps, out_dtype)


class TNLinear(nn.Linear):
    """Bias-free projection whose backward GEMMs take K-contiguous operands (``ops.llm.linear_tn``)
    when ``impl == "tn"``; ``"autograd"`` is the plain ``nn.Linear`` backward (A/B); ``"fp8"`` runs the
    forward and both backward GEMMs in per-tensor-scaled FP8 (``ops.fp8.fp8_linear``, GPU and CPU)."""

    impl = "tn"
    fp8_grad_format = "e5m2"  # impl "fp8": the output gradient's format (x and w are e4m3)
    # calls with at most ops.skinny.MAX_ROWS rows (a decode step's): "hip" sends them to the skinny
    # GEMM (ops.skinny.linear_rows) where rows_linear() allows, "hip-fp8" to the one on e4m3 weights
    # (ops.skinny.linear_rows_fp8) for the modules Llama.quantize_decode_weights() has prepared, "hip-fp4" to
    # the one on MXFP4 weights (ops.skinny.linear_rows_fp4) after quantize_decode_weights(fmt="fp4"), "lib"
    # leaves every call where it was
    rows_impl = "lib"
    rows_calls = collections.Counter()  # such calls per path ("hip", "hip-fp8", "hip-fp4", "lib") on a GPU
    # True, with rows_impl "hip" or "hip-fp8": a decode step on a GPU folds its residual adds and RMSNorms
    # into the projections around them (Llama._decode_fused; ops.skinny.linear_rows_add_norm /
    # linear_rows_scaled), counted in rows_calls under rows_impl + "-add-norm" and + "-scaled", and the one
    # norm launch left per step under "rms-norm".  A step outside those kernels' contract runs as before.
    rows_fuse_norm = False

    def __init__(self, fin: int, fout: int):
        super().__init__(fin, fout, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            y = rows_linear(x, self.weight, mod=self)
            if y is not None:
                return y
        if self.impl == "fp8":
            from ..ops import fp8
            return fp8.fp8_linear(x, self.weight, self.fp8_grad_format)
        if self.impl == "tn" and x.is_cuda:
            from ..ops.llm import linear_tn
            return linear_tn(x, self.weight)
        return super().forward(x)


def rows_linear(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False, count_lib: bool = True, mod=None):
    """The decode step's choice for one CUDA projection.  A call of at most ``ops.skinny.MAX_ROWS`` rows
    is counted in ``TNLinear.rows_calls``.  It goes to the skinny HIP GEMM (``ops.skinny.linear_rows``),
    and its result is returned, when ``TNLinear.rows_impl == "hip"``, gradients are off, the input is
    bf16 (or bf16 autocast is on), the weight is bf16 already (casting an fp32 weight per call costs more
    than the GEMM: that case stays where it was) and the shape is inside ``ops.skinny.hip_supported``.
    With ``rows_impl == "hip-fp8"`` it goes to ``ops.skinny.linear_rows_fp8`` under the same conditions on
    ``x``, when ``mod`` (the module that owns ``w``) carries the ``rows_q`` and ``rows_scale`` of
    ``Llama.quantize_decode_weights`` and the shape is inside ``ops.skinny.hip_supported_fp8``; with
    ``"hip-fp4"`` to ``ops.skinny.linear_rows_fp4`` in the same way, on ``rows_q4`` and ``rows_scale4``.
    Otherwise None: the caller runs the path it always ran.  ``count_lib=False``: that path counts itself."""
    from ..ops import skinny
    if x.numel() > skinny.max_rows() * x.shape[-1]:
        return None
    impl = TNLinear.rows_impl
    hip = (impl in ("hip", "hip-fp8", "hip-fp4") and not torch.is_grad_enabled() and
           (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled("cuda") and
                                          torch.get_autocast_dtype("cuda") == torch.bfloat16)))
    if hip and impl == "hip":
        x = x.to(torch.bfloat16)
        hip = w.dtype == torch.bfloat16 and skinny.hip_supported(x, w, swiglu)
    elif hip and impl == "hip-fp4":
        hip = getattr(mod, "rows_q4", None) is not None
        if hip:
            if mod.rows_q4.device != x.device:  # plain attributes do not follow Module.to(): once, here
                mod.rows_q4, mod.rows_scale4 = mod.rows_q4.to(x.device), mod.rows_scale4.to(x.device)
            x = x.to(torch.bfloat16)
            hip = skinny.hip_supported_fp4(x, mod.rows_q4, mod.rows_scale4, swiglu)
    elif hip:
        hip = getattr(mod, "rows_q", None) is not None
        if hip:
            if mod.rows_q.device != x.device:  # plain attributes do not follow Module.to(): once, here
                mod.rows_q, mod.rows_scale = mod.rows_q.to(x.device), mod.rows_scale.to(x.device)
            x = x.to(torch.bfloat16)
            hip = skinny.hip_supported_fp8(x, mod.rows_q, mod.rows_scale, swiglu)
    if not hip:
        TNLinear.rows_calls["lib"] += int(count_lib)
        return None
    TNLinear.rows_calls[impl] += 1
    if impl == "hip":
        return skinny.linear_rows(x, w, swiglu)
    if impl == "hip-fp4":
        return skinny.launch_rows_fp4(x, mod.rows_q4, mod.rows_scale4, swiglu)
    return skinny.launch_rows_fp8(x, mod.rows_q, mod.rows_scale, swiglu)


class LayerCache(NamedTuple):
    """One layer's view of an ``ops.decode.KVCache`` for one forward: ``k``, ``v`` [B, max_len, Hkv, D];
    a decode step also needs ``pos`` (the row to append at), ``lens`` (valid rows after the append),
    both int32 [B] on the device, and the host-known bound ``max_keys``.  A prefill leaves them None.
    ``k_scale``, ``v_scale`` [B, Hkv, max_len_pad]: the layer's scales when the cache is e4m3, else None."""
    k: torch.Tensor
    v: torch.Tensor
    pos: Optional[torch.Tensor]
    lens: Optional[torch.Tensor]
    max_keys: Optional[int]
    k_scale: Optional[torch.Tensor] = None
    v_scale: Optional[torch.Tensor] = None


class Attention(nn.Module):
    """GQA attention with RoPE.  Which kernels run is chosen per call, for the prefill / training path
    and for the decode step alike: the hand-written HIP ones where the shape and dtype are theirs (bf16,
    head dim 64 or 128, ...), the library's ``scaled_dot_product_attention`` otherwise -- an fp32 model
    called without autocast, for instance, runs the library path on a GPU without an error (the
    ``ops`` wrappers themselves never fall back).  ``decode_calls`` counts the decode steps per path
    ("hip", "hip-fp8" on an e4m3 cache, "hip-rows" / "hip-rows-fp8" for a multi-token step, "sdpa", "cpu"), so that a benchmark
    or a test can assert which one it ran."""

    impl = "auto"  # "auto": HIP flash attention where it applies; "sdpa": library kernels
    decode_impl = None  # the decode step alone: None follows impl; "sdpa" / "auto" for A/B runs (tools/decode_bench.py)
    decode_calls = collections.Counter()

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.nh, self.nkv, self.hd = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        # one fused Q|K|V projection: one GEMM (N = (Hq + 2 Hkv) * D) forward and one for
        # the input gradient backward, instead of three plus a gradient sum
        self.wqkv = TNLinear(cfg.dim, (self.nh + 2 * self.nkv) * self.hd)
        self.wo = TNLinear(self.nh * self.hd, cfg.dim)

    def forward(self, x, cos, sin, doc_start=None, cache=None):
        """``cache`` (a ``LayerCache``): S > 1 is a prefill -- the rotated k and v also go to the layer's
        cache rows [0, S); S == 1 is a decode step -- k and v are appended at row ``cache.pos[b]`` and
        the one query attends to the ``cache.lens[b]`` rows of the cache (``ops.decode``); S > 1 with
        ``cache.pos`` set is a multi-token step -- rows ``pos[b]`` .. ``pos[b] + S - 1`` are appended and query s
        attends to ``cache.lens[b] - (S - 1 - s)`` rows (``ops.decode.append_rows`` / ``attend_rows``)."""
        B, S, _ = x.shape
        from ..ops import attention as A
        from ..ops.llm import rope_qkv
        if cache is not None and (S == 1 or cache.pos is not None):
            return self.wo(self.decode_heads(self.wqkv(x), cos, sin, cache))
        q, k, v = rope_qkv(self.wqkv(x), cos, sin, self.nh, self.nkv)
        if cache is not None:
            n = min(S, cache.k.shape[1])  # a prompt padded to the attention kernels' multiple may end past the cache
            if cache.k_scale is not None:
                from ..ops.decode import quantize_kv
                quantize_kv(k, v, cache.k, cache.v, cache.k_scale, cache.v_scale)
            else:
                cache.k[:, :n].copy_(k[:, :n])
                cache.v[:, :n].copy_(v[:, :n])
        if doc_start is not None:
            # packed documents: attention stays inside each one; RoPE positions stay absolute
            # (it is relative, so restarting them per document would change nothing)
            if self.impl != "sdpa" and A.hip_supported(q, k, v):
                o = A.flash_attention(q, k, v, causal=True, doc_start=doc_start)
            else:
                o = A.sdpa_bshd(q, k, v, causal=True, doc_start=doc_start)
        elif self.impl != "sdpa" and A.hip_supported(q, k, v):
            o = A.flash_attention(q, k, v, causal=True)  # [B, S, H, D], no transposes
        else:
            o = A.sdpa_bshd(q, k, v, causal=True)
        return self.wo(o.reshape(B, S, self.nh * self.hd))

    def decode_heads(self, qkv, cos, sin, cache):
        """A decode step between the two projections: ``qkv`` [B, S, (Hq + 2 Hkv) D] (``wqkv``'s output) is
        rotated, k and v are appended to the cache and the queries attend; returns [B, S, Hq D] for ``wo``."""
        from ..ops import decode as Dc
        B, S, _ = qkv.shape
        fp8 = cache.k.dtype == Dc.FP8  # the e4m3 cache has one path per device: no library side to fall to
        if S == 1:
            q = Dc.rope_append(qkv.reshape(B, -1), cos, sin, cache.k, cache.v, cache.pos, self.nh, self.nkv,
                               cache.k_scale, cache.v_scale)
            hip = fp8 or ((self.decode_impl or self.impl) != "sdpa"
                          and (not q.is_cuda or Dc.hip_supported(q, cache.k, cache.v)))
            Attention.decode_calls["cpu" if not q.is_cuda else (("hip-fp8" if fp8 else "hip") if hip else "sdpa")] += 1
            o = Dc.decode_attention(q, cache.k, cache.v, cache.lens, cache.max_keys, "auto" if hip else "sdpa",
                                    cache.k_scale, cache.v_scale)
        else:
            # S tokens per sequence appended at pos .. pos + S - 1, each attending to the rows up to its own
            q = Dc.append_rows(qkv, cos, sin, cache.k, cache.v, cache.pos, self.nh, self.nkv,
                               cache.k_scale, cache.v_scale)
            hip = fp8 or ((self.decode_impl or self.impl) != "sdpa"
                          and (not q.is_cuda or Dc.rows_supported(q, cache.k, cache.v)))
            Attention.decode_calls["cpu" if not q.is_cuda else
                                   (("hip-rows-fp8" if fp8 else "hip-rows") if hip else "sdpa")] += 1
            o = Dc.attend_rows(q, cache.k, cache.v, cache.lens, cache.max_keys, "auto" if hip else "sdpa",
                               cache.k_scale, cache.v_scale)
        return o.reshape(B, S, self.nh * self.hd)


class FeedForward(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        # fused W1|W3 (gate | up) projection: one GEMM each way, packed SwiGLU between
        self.w13 = TNLinear(cfg.dim, 2 * cfg.ffn_hidden)
        self.w2 = TNLinear(cfg.ffn_hidden, cfg.dim)

    def forward(self, x):
        from ..ops.llm import swiglu_packed
        # a decode step: the projection and SwiGLU in one launch
        if x.is_cuda and TNLinear.rows_impl in ("hip", "hip-fp8", "hip-fp4"):
            y = rows_linear(x, self.w13.weight, swiglu=True, count_lib=False, mod=self.w13)
            if y is not None:
                return self.w2(y)
        return self.w2(swiglu_packed(self.w13(x)))


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attention_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.attention = Attention(cfg)
        self.ffn_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.feed_forward = FeedForward(cfg)

    def forward(self, x, delta, cos, sin, doc_start=None, cache=None):
        """x: residual stream entering the block minus the previous block's FFN output
        ``delta`` (None for the first block): each residual add happens inside the next
        RMSNorm.  Returns (residual stream before the FFN add, FFN output)."""
        h, y = self.attention_norm.add_forward(x, delta)
        h, y = self.ffn_norm.add_forward(h, self.attention(y, cos, sin, doc_start, cache))
        return h, self.feed_forward(y)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig, checkpoint_layers: bool = False):
        super().__init__()
        self.cfg = cfg
        self.checkpoint_layers = checkpoint_layers
        self.tok_embeddings = nn.Embedding(cfg.vocab_size, cfg.dim)
        self.layers = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layers))
        self.norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.output = nn.Linear(cfg.dim, cfg.vocab_size, bias=False)
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self, std: float = 0.02):
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=std)
        # scaled init of the residual projections (GPT-2 / Llama practice)
        for blk in self.layers:
            nn.init.normal_(blk.attention.wo.weight, std=std / math.sqrt(2 * self.cfg.n_layers))
            nn.init.normal_(blk.feed_forward.w2.weight, std=std / math.sqrt(2 * self.cfg.n_layers))

    def forward(self, tokens: torch.Tensor, targets: Optional[torch.Tensor] = None,
                doc_start: Optional[torch.Tensor] = None):
        """``doc_start`` [B, S] (``ops.attention.doc_starts_from_tokens``): packed documents, attention
        does not cross their boundaries."""
        B, S = tokens.shape
        cos, sin = rope_tables(self.cfg.head_dim, S, self.cfg.rope_theta, tokens.device)
        h, d = self.tok_embeddings(tokens), None
        for blk in self.layers:
            if self.checkpoint_layers and self.training:
                h, d = torch.utils.checkpoint.checkpoint(blk, h, d, cos, sin, doc_start, use_reentrant=False)
            else:
                h, d = blk(h, d, cos, sin, doc_start)
        logits = self.output(self.norm.add_forward(h, d)[1])
        if targets is None:
            return logits
        from ..ops.llm import cross_entropy
        # the logits are this op's own intermediate: d(logits) may overwrite them
        return cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1), overwrite_logits=True)

    # ------------------------------------------------------------------ generation (ops.decode)
    def _lm_head(self, y: torch.Tensor) -> torch.Tensor:
        """``self.output`` for the few rows of a decode step, by TNLinear's ``rows_impl`` choice (``output``
        stays a plain ``nn.Linear``: the state-dict keys are the checkpoints')."""
        out = rows_linear(y, self.output.weight, mod=self.output) if y.is_cuda else None
        return self.output(y) if out is None else out

    @torch.no_grad()
    def quantize_decode_weights(self, snap: bool = True, fmt: str = "fp8") -> int:
        """Prepare ``TNLinear.rows_impl = "hip-fp8"``: every ``TNLinear`` and ``output`` gets ``rows_q`` (e4m3
        [N, K]) and ``rows_scale`` (fp32 [N], powers of two) of ``ops.skinny.quantize_rows`` as plain
        attributes -- neither parameters nor buffers, so state-dict keys and checkpoints do not change.
        ``snap``: the weight itself is overwritten in place with the dequantised value (exact in bf16), so
        the prefill (library GEMM on the weight) and the decode step (the kernel on ``rows_q``) run the same
        model.  The weights are kept: memory goes up by a byte per weight.  Returns the number of modules.
        ``fmt="fp4"`` prepares ``rows_impl = "hip-fp4"`` instead: ``rows_q4`` (uint8 [N, K / 2]) and
        ``rows_scale4`` (e8m0 [N, K / 32]) of ``ops.skinny.quantize_rows_fp4``, beside the e4m3 attributes if
        they are there, and ``snap`` overwrites the weight with their dequantised value; memory goes up by 17 / 32
        of a byte per weight."""
        from ..ops.skinny import dequantize_rows, dequantize_rows_fp4, quantize_rows, quantize_rows_fp4
        if fmt not in ("fp8", "fp4"):
            raise ValueError(f"quantize_decode_weights: fmt is 'fp8' or 'fp4'; got {fmt!r}")
        mods = [m for m in self.modules() if isinstance(m, TNLinear)] + [self.output]
        for m in mods:
            if fmt == "fp4":
                m.rows_q4, m.rows_scale4 = quantize_rows_fp4(m.weight)
                if snap:
                    m.weight.copy_(dequantize_rows_fp4(m.rows_q4, m.rows_scale4, m.weight.dtype))
                continue
            m.rows_q, m.rows_scale = quantize_rows(m.weight)
            if snap:
                m.weight.copy_(dequantize_rows(m.rows_q, m.rows_scale, m.weight.dtype))
        return len(mods)

    def _low_precision(self, device) -> bool:
        """The projections run in bf16: under autocast, or with bf16 matmul weights."""
        return torch.is_autocast_enabled(device.type) or self.layers[0].attention.wqkv.weight.dtype == torch.bfloat16

    def new_cache(self, B: int, max_len: int, dtype=None):
        """An empty ``ops.decode.KVCache`` for ``B`` sequences of up to ``max_len`` tokens, in the dtype
        the projections write (bf16 under autocast or with bf16 weights, else the weights' own), or in
        ``dtype``: ``torch.float8_e4m3fn`` is the quantised cache of ``ops.decode``."""
        from ..ops.decode import KVCache
        w = self.layers[0].attention.wqkv.weight
        if dtype is None:
            dtype = torch.bfloat16 if self._low_precision(w.device) else w.dtype
        return KVCache(self.cfg.n_layers, B, max_len, self.cfg.n_kv_heads, self.cfg.head_dim, dtype, w.device)

    @staticmethod
    def _layer_cache(cache, i: int, pos=None, lens=None, max_keys=None) -> LayerCache:
        if cache.k_scale is None:
            return LayerCache(cache.k[i], cache.v[i], pos, lens, max_keys)
        return LayerCache(cache.k[i], cache.v[i], pos, lens, max_keys, cache.k_scale[i], cache.v_scale[i])

    def _rope(self, cache, rows: int):
        if cache.rope is None or cache.rope[0].shape[0] < rows:
            cache.rope = rope_tables(self.cfg.head_dim, rows, self.cfg.rope_theta, cache.k.device)
        return cache.rope

    def _prefill_len(self, P: int, device) -> int:
        """The length a prompt of P tokens is run at: on a GPU with the HIP attention on, the next multiple
        of its tile (it takes whole tiles; causal masking hides the padding from every prompt token)."""
        from ..ops import attention as A
        if device.type == "cuda" and Attention.impl != "sdpa" and self.cfg.head_dim in A.HEAD_DIMS:
            return -(-P // A.SEQ_MULTIPLE) * A.SEQ_MULTIPLE
        return P

    def prefill(self, tokens: torch.Tensor, prompt_lens: torch.Tensor, cache) -> torch.Tensor:
        """Run the right-padded prompts ``tokens`` [B, P] (row b holds ``prompt_lens[b]`` >= 1 tokens),
        fill the cache and return the logits [B, V] after each row's last prompt token.  The hidden state
        is gathered at ``prompt_lens - 1`` before the final norm, so no [B, P, V] logits exist.  Cache
        rows at and past ``prompt_lens[b]`` hold padding; they are masked by ``cache.lens`` and
        overwritten by later appends."""
        B, P = tokens.shape
        S = self._prefill_len(P, tokens.device)
        if S > P:
            tokens = F.pad(tokens, (0, S - P))
        cos, sin = self._rope(cache, max(S, cache.max_len))
        cos, sin = cos[:S], sin[:S]
        h, d = self.tok_embeddings(tokens), None
        for i, blk in enumerate(self.layers):
            h, d = blk(h, d, cos, sin, None, self._layer_cache(cache, i))
        rows, last = torch.arange(B, device=tokens.device), prompt_lens.to(tokens.device).long() - 1
        logits = self._lm_head(self.norm.add_forward(h[rows, last].unsqueeze(1), d[rows, last].unsqueeze(1))[1])
        cache.lens = prompt_lens.to(device=tokens.device, dtype=torch.int32).clone()
        return logits[:, 0]

    def decode_step(self, tokens: torch.Tensor, cache, max_keys: Optional[int] = None) -> torch.Tensor:
        """Append one token per row (``tokens`` [B]) at position ``cache.lens`` and return the logits
        [B, V] of the next one.  ``max_keys``: a host-known upper bound of the lengths after the append
        (default: the cache's size); it alone sets the attention grid, nothing is read from the device."""
        pos = cache.lens
        lens = pos + 1
        mk = cache.max_len if max_keys is None else max_keys
        cos, sin = self._rope(cache, cache.max_len)
        h, d = self.tok_embeddings(tokens).unsqueeze(1), None
        if self._fuse_norm(h):
            logits = self._decode_fused(h, cos, sin, cache, pos, lens, mk)
            cache.lens = lens
            return logits[:, 0]
        for i, blk in enumerate(self.layers):
            h, d = blk(h, d, cos, sin, None, self._layer_cache(cache, i, pos, lens, mk))
        logits = self._lm_head(self.norm.add_forward(h, d)[1])
        cache.lens = lens
        return logits[:, 0]

    def decode_steps(self, tokens: torch.Tensor, cache, max_keys: Optional[int] = None) -> torch.Tensor:
        """Append S tokens per row (``tokens`` [B, S]) at positions ``cache.lens`` .. ``+ S - 1`` in one step
        and return the logits [B, S, V] after each of them: token s attends to the cache rows up to its own.
        ``cache.lens`` grows by S; ``max_keys`` bounds the lengths after the append, as in ``decode_step``.
        The multi-query kernels of ``ops.decode`` take S * n_heads / n_kv_heads <= 16 on a bf16 or an e4m3 cache
        (the library path serves the rest on a bf16 cache; on an e4m3 cache a larger S is an error); the
        projections take ``rows_linear``'s choice for B * S rows."""
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError(f"decode_steps: tokens must be [B, S] with S >= 1, got {tuple(tokens.shape)}")
        pos = cache.lens
        lens = pos + tokens.shape[1]
        mk = cache.max_len if max_keys is None else max_keys
        cos, sin = self._rope(cache, cache.max_len)
        h, d = self.tok_embeddings(tokens), None
        if self._fuse_norm(h):
            logits = self._decode_fused(h, cos, sin, cache, pos, lens, mk)
            cache.lens = lens
            return logits
        for i, blk in enumerate(self.layers):
            h, d = blk(h, d, cos, sin, None, self._layer_cache(cache, i, pos, lens, mk))
        logits = self._lm_head(self.norm.add_forward(h, d)[1])
        cache.lens = lens
        return logits

    # ------------------------------------------------------------------ decode step with the norms folded in
    def _fuse_norm(self, h: torch.Tensor) -> bool:
        """Whether a decode step whose embedded tokens are ``h`` [B, S, dim] takes ``_decode_fused``: the switch
        is on, ``rows_linear`` would send its projections to the skinny GEMMs, and every projection and norm of
        the model is inside the fused kernels' contract (asked once per weight format and device, not per
        step: the checks cost what the fusion saves).  Otherwise the step runs the existing path whole."""
        from ..ops import skinny
        impl = TNLinear.rows_impl
        if not (TNLinear.rows_fuse_norm and h.is_cuda and impl in ("hip", "hip-fp8") and not torch.is_grad_enabled()
                and h.numel() <= skinny.max_rows() * h.shape[-1]):
            return False
        if h.dtype != torch.bfloat16 and not (h.dtype == torch.float32 and torch.is_autocast_enabled("cuda")
                                              and torch.get_autocast_dtype("cuda") == torch.bfloat16):
            return False
        key = (impl, h.device, self.output.weight.dtype, getattr(self.output, "rows_q", None) is not None)
        known = self.__dict__.setdefault("_fuse_norm_ok", {})
        if key not in known:
            known[key] = self._fuse_norm_contract(h.device)
        return known[key]

    def _fuse_norm_contract(self, device) -> bool:
        from ..ops import skinny
        fp8 = TNLinear.rows_impl == "hip-fp8"
        probe = {}
        mods = [(self.output, False)]
        for blk in self.layers:
            mods += [(blk.attention.wqkv, False), (blk.attention.wo, False), (blk.feed_forward.w13, True),
                     (blk.feed_forward.w2, False)]
        for mod, swiglu in mods:
            K = mod.weight.shape[1]
            x = probe.setdefault(K, torch.empty(1, K, dtype=torch.bfloat16, device=device))
            if fp8:
                if getattr(mod, "rows_q", None) is None:
                    return False
                if mod.rows_q.device != device:  # plain attributes do not follow Module.to(): once, here
                    mod.rows_q, mod.rows_scale = mod.rows_q.to(device), mod.rows_scale.to(device)
                if not skinny.hip_supported_fp8(x, mod.rows_q, mod.rows_scale, swiglu):
                    return False
            elif mod.weight.dtype != torch.bfloat16 or not skinny.hip_supported(x, mod.weight, swiglu):
                return False
        norms = [self.norm] + [n for blk in self.layers for n in (blk.attention_norm, blk.ffn_norm)]
        return self.cfg.dim % skinny.SS_TILE == 0 and all(
            n.weight.dtype == torch.float32 and n.weight.is_cuda and n.weight.is_contiguous() for n in norms)

    def _decode_fused(self, h, cos, sin, cache, pos, lens, mk):
        """The blocks and the lm-head of a decode step, carrying (h, a, ss) from one projection to the next:
        h the residual stream, a = bf16(h * gamma) the next projection's operand, ss the partial sums of h^2
        from which that projection takes rstd.  Each wo adds the residual and takes its block's ffn_norm
        weight, each w2 the next block's attention_norm weight (the model's norm after the last block); wqkv,
        w13 + SwiGLU and the lm-head scale by rstd.  The first block's attention_norm has no producer: a plain
        norm and the plain GEMM.  7 launches per layer and 2 per step, against 9 and 2."""
        from ..ops import skinny
        from ..ops.llm import _aligned
        impl, calls = TNLinear.rows_impl, TNLinear.rows_calls
        L = len(self.layers)

        def weight(mod):
            return (mod.rows_q, mod.rows_scale) if impl == "hip-fp8" else (mod.weight, None)

        h = _aligned(h)
        a = self.layers[0].attention_norm(h).to(torch.bfloat16)
        ss = None
        calls["rms-norm"] += 1
        for i, blk in enumerate(self.layers):
            att, ffn = blk.attention, blk.feed_forward
            if ss is None:
                qkv = rows_linear(a, att.wqkv.weight, mod=att.wqkv)
            else:
                qkv = skinny.launch_scaled(a, *weight(att.wqkv), ss, blk.attention_norm.eps)
            o = att.decode_heads(qkv, cos, sin, self._layer_cache(cache, i, pos, lens, mk))
            h, a, ss = skinny.launch_add_norm(o, *weight(att.wo), h, blk.ffn_norm.weight)
            y = skinny.launch_scaled(a, *weight(ffn.w13), ss, blk.ffn_norm.eps, swiglu=True)
            nxt = self.layers[i + 1].attention_norm if i + 1 < L else self.norm
            h, a, ss = skinny.launch_add_norm(y, *weight(ffn.w2), h, nxt.weight)
        calls[impl + "-scaled"] += 2 * L
        calls[impl + "-add-norm"] += 2 * L
        return skinny.launch_scaled(a, *weight(self.output), ss, self.norm.eps)

    def _speculate(self, draft, k: int, prompts, lens, cache, T: int, eos_id, return_logits: bool):
        """The token loop of ``generate`` with a draft model (greedy).  A round: the draft takes k + 1 single
        steps from the last emitted token (its cache then holds all k drafts), the target verifies
        [last, d_1 .. d_k] in one ``decode_steps``, and a sequence emits the target's tokens t_1 .. t_(a+1),
        a = the length of the prefix on which drafts and target agree.  Both caches' ``lens`` go back to
        base + a + 1 on the device: the rows past that are dead and the next round overwrites them.  The
        sequences advance raggedly; the one host read per round is the smallest emitted count."""
        B, P = prompts.shape
        dev, V = prompts.device, self.cfg.vocab_size
        dcache = draft.new_cache(B, cache.max_len, cache.k.dtype)
        draft._rope(dcache, max(cache.max_len, draft._prefill_len(P, dev)))
        draft.prefill(prompts, lens, dcache)
        logits = self.prefill(prompts, lens, cache).float()
        width = T + k + 1                                    # a round may run k tokens past T; the last column is a dump
        out = torch.zeros(B, width, dtype=torch.long, device=dev)
        kept = torch.zeros(B * width, V, dtype=torch.float32, device=dev) if return_logits else None
        ar = torch.arange(k + 1, device=dev).view(1, -1)
        rows = torch.arange(B, device=dev).view(-1, 1) * width
        last = logits.argmax(-1)                             # emitted, not yet in either cache
        done = last == eos_id if eos_id is not None else None
        out[:, 0] = last
        if return_logits:
            kept.index_copy_(0, rows[:, 0], logits)
        cnt = torch.ones(B, dtype=torch.long, device=dev)   # tokens emitted per sequence
        r = 0
        while int(cnt.min()) < T:
            base, seen = cache.lens, P + r * (k + 1)         # every length is at most `seen` before this round
            toks, cur = [last], last
            for j in range(k + 1):
                dl = draft.decode_step(cur, dcache, max_keys=min(seen + j + 1, cache.max_len))
                if j < k:
                    cur = dl.argmax(-1)
                    toks.append(cur)
            toks = torch.stack(toks, dim=1)                  # [B, k + 1]: last, d_1 .. d_k
            logits = self.decode_steps(toks, cache, max_keys=min(seen + k + 1, cache.max_len)).float()
            t = logits.argmax(-1)                            # t_1 .. t_(k+1)
            if eos_id is not None:                           # after an eos, emitted now or earlier, only eos
                hit = (t == eos_id).long().cumsum(1)
                t = torch.where(done.view(-1, 1) | (hit - (t == eos_id).long() > 0), eos_id, t)
            a = (toks[:, 1:] == t[:, :k]).long().cumprod(1).sum(1)
            a = torch.where(cnt < T, a, -1)                  # a sequence that has its tokens stands still
            keep = ar <= a.view(-1, 1)
            idx = torch.where(keep, cnt.view(-1, 1) + ar, width - 1)
            out.scatter_(1, idx, t)
            if return_logits:
                kept.index_copy_(0, (rows + idx).view(-1), logits.reshape(-1, V))
            if eos_id is not None:
                done = done | ((t == eos_id) & keep).any(1)
            last = torch.where(a >= 0, t.gather(1, a.clamp(min=0).view(-1, 1))[:, 0], last)
            cnt = cnt + a + 1
            cache.lens = dcache.lens = base + (a + 1).to(torch.int32)
            r += 1
        return out[:, :T], (kept.view(B, width, V)[:, :T] if return_logits else None)

    def generate(self, prompts: torch.Tensor, prompt_lens=None, max_new_tokens: int = 32, temperature: float = 0.0,
                 top_k: int = 0, eos_id: Optional[int] = None, generator: Optional[torch.Generator] = None,
                 return_logits: bool = False, max_len: Optional[int] = None, kv_dtype=None,
                 draft: Optional["Llama"] = None, draft_tokens: int = 0):
        """Continue ``prompts`` [B, P] (right-padded; ``prompt_lens`` [B], default all P) by
        ``max_new_tokens`` tokens: LongTensor [B, max_new_tokens] (and the fp32 logits [B, T, V] each was
        chosen from, with ``return_logits``).  Greedy at temperature 0, else temperature / top-k sampling
        with ``torch.multinomial`` from ``generator``; a row that has emitted ``eos_id`` keeps emitting it.
        Runs without gradients in eval mode with bf16 projections on a GPU (never FP8).  ``kv_dtype``: the
        cache's dtype; ``torch.float8_e4m3fn`` halves its bytes and changes the numbers.  The token loop
        reads nothing back from the device; the one synchronisation is the caller's use of the result.

        ``draft`` (another ``Llama`` with the same vocabulary, on the same device) and ``draft_tokens`` = k >= 1:
        greedy speculative decoding, see ``_speculate``.  The tokens are the target's own greedy choices, each
        the argmax of the logits returned for it; a round costs one multi-token target step and k + 1 draft
        steps, and one host read.  The caches hold up to P + max_new_tokens + k rows.  With
        ``kv_dtype=torch.float8_e4m3fn`` both caches are e4m3 and the verification step runs ``ops.decode``'s
        e4m3 multi-token kernels ((k + 1) * n_heads / n_kv_heads <= 16); a rolled-back row's codes and scales
        are dead like the row itself and are overwritten together."""
        V = self.cfg.vocab_size
        if not isinstance(prompts, torch.Tensor) or prompts.dim() != 2 or prompts.dtype != torch.long or \
                prompts.shape[1] < 1:
            raise ValueError("generate: prompts must be a LongTensor [B, P] with P >= 1")
        B, P = prompts.shape
        T = max_new_tokens
        if not isinstance(T, int) or T < 1:
            raise ValueError(f"generate: max_new_tokens must be a positive int, got {T!r}")
        if not temperature >= 0.0 or not math.isfinite(temperature):
            raise ValueError(f"generate: temperature must be finite and >= 0, got {temperature!r}")
        if not isinstance(top_k, int) or not 0 <= top_k <= V:
            raise ValueError(f"generate: top_k must be in [0, {V}] (0 = off), got {top_k!r}")
        if eos_id is not None and not 0 <= eos_id < V:
            raise ValueError(f"generate: eos_id {eos_id} is not an id of the {V}-token vocabulary")
        k = draft_tokens
        if draft is None and k != 0:
            raise ValueError(f"generate: draft_tokens = {k!r} needs a draft model")
        if draft is not None:
            if not isinstance(draft, Llama) or draft.cfg.vocab_size != V or not isinstance(k, int) or k < 1:
                raise ValueError(f"generate: draft must be a Llama with the same {V}-token vocabulary and "
                                 f"draft_tokens >= 1, got {type(draft).__name__} and {k!r}")
            if temperature > 0.0:
                raise ValueError("generate: a draft model goes with greedy decoding (temperature 0)")
            if draft.tok_embeddings.weight.device != self.tok_embeddings.weight.device:
                raise ValueError("generate: draft and target must be on one device")
        max_len = P + T + k if max_len is None else max_len  # a draft round may write k rows past the last token
        if not P + T + k <= max_len <= min(self.cfg.max_seq_len, draft.cfg.max_seq_len if draft else max_len):
            raise ValueError(f"generate: need P + max_new_tokens + draft_tokens = {P + T + k} <= max_len = {max_len} "
                             f"<= max_seq_len = {self.cfg.max_seq_len}" +
                             (f" and the draft's {draft.cfg.max_seq_len}" if draft else ""))
        # host-side checks of the prompt, before the loop
        host_lens = [P] * B if prompt_lens is None else [int(n) for n in torch.as_tensor(prompt_lens).cpu().tolist()]
        if len(host_lens) != B or min(host_lens) < 1 or max(host_lens) > P:
            raise ValueError(f"generate: prompt_lens must be {B} lengths in [1, {P}], got {host_lens}")
        pc = prompts.cpu()
        if int(pc.min()) < 0 or int(pc.max()) >= V:
            raise ValueError(f"generate: prompt ids must be in [0, {V})")
        dev = self.tok_embeddings.weight.device
        prompts = prompts.to(dev)
        lens = torch.tensor(host_lens, dtype=torch.int32, device=dev)
        amp_on = dev.type == "cuda" or self._low_precision(dev)
        was_training, linear_impl = self.training, TNLinear.impl
        draft_training = draft.training if draft is not None else False
        self.eval()
        if draft is not None:
            draft.eval()
        if TNLinear.impl == "fp8":
            TNLinear.impl = "tn"
        try:
            with torch.no_grad(), torch.autocast(device_type=dev.type, dtype=torch.bfloat16, enabled=amp_on):
                cache = self.new_cache(B, max_len, kv_dtype or (torch.bfloat16 if amp_on else None))
                self._rope(cache, max(max_len, self._prefill_len(P, dev)))  # the tables, once: the padded prompt's too
                if draft is not None:
                    tokens, kept = self._speculate(draft, k, prompts, lens, cache, T, eos_id, return_logits)
                    return (tokens, kept) if return_logits else tokens
                logits = self.prefill(prompts, lens, cache).float()
                out, kept = [], []
                done = torch.zeros(B, dtype=torch.bool, device=dev)
                for t in range(T):
                    if temperature == 0.0:
                        nxt = logits.argmax(-1)
                    else:
                        z = logits / temperature
                        if top_k:
                            z = torch.where(z < z.topk(top_k, dim=-1).values[:, -1:], -math.inf, z)
                        nxt = torch.multinomial(torch.softmax(z, dim=-1), 1, generator=generator)[:, 0]
                    if eos_id is not None:
                        nxt = torch.where(done, eos_id, nxt)
                        done = done | (nxt == eos_id)
                    out.append(nxt)
                    if return_logits:
                        kept.append(logits)
                    if t + 1 < T:
                        logits = self.decode_step(nxt, cache, max_keys=P + t + 1).float()
        finally:
            TNLinear.impl = linear_impl
            self.train(was_training)
            if draft is not None:
                draft.train(draft_training)
        tokens = torch.stack(out, dim=1)
        return (tokens, torch.stack(kept, dim=1)) if return_logits else tokens
