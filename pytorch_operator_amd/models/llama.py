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

    def __init__(self, fin: int, fout: int):
        super().__init__(fin, fout, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.impl == "fp8":
            from ..ops import fp8
            return fp8.fp8_linear(x, self.weight, self.fp8_grad_format)
        if self.impl == "tn" and x.is_cuda:
            from ..ops.llm import linear_tn
            return linear_tn(x, self.weight)
        return super().forward(x)


class LayerCache(NamedTuple):
    """One layer's view of an ``ops.decode.KVCache`` for one forward: ``k``, ``v`` [B, max_len, Hkv, D];
    a decode step also needs ``pos`` (the row to append at), ``lens`` (valid rows after the append),
    both int32 [B] on the device, and the host-known bound ``max_keys``.  A prefill leaves them None."""
    k: torch.Tensor
    v: torch.Tensor
    pos: Optional[torch.Tensor]
    lens: Optional[torch.Tensor]
    max_keys: Optional[int]


class Attention(nn.Module):
    """GQA attention with RoPE.  Which kernels run is chosen per call, for the prefill / training path
    and for the decode step alike: the hand-written HIP ones where the shape and dtype are theirs (bf16,
    head dim 64 or 128, ...), the library's ``scaled_dot_product_attention`` otherwise -- an fp32 model
    called without autocast, for instance, runs the library path on a GPU without an error (the
    ``ops`` wrappers themselves never fall back).  ``decode_calls`` counts the decode steps per path
    ("hip", "sdpa", "cpu"), so that a benchmark or a test can assert which one it ran."""

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
        the one query attends to the ``cache.lens[b]`` rows of the cache (``ops.decode``)."""
        B, S, _ = x.shape
        from ..ops import attention as A
        from ..ops.llm import rope_qkv
        if cache is not None and S == 1:
            from ..ops import decode as Dc
            q = Dc.rope_append(self.wqkv(x).reshape(B, -1), cos, sin, cache.k, cache.v, cache.pos, self.nh, self.nkv)
            hip = (self.decode_impl or self.impl) != "sdpa" and (not q.is_cuda or Dc.hip_supported(q, cache.k, cache.v))
            Attention.decode_calls["cpu" if not q.is_cuda else ("hip" if hip else "sdpa")] += 1
            o = Dc.decode_attention(q, cache.k, cache.v, cache.lens, cache.max_keys, "auto" if hip else "sdpa")
            return self.wo(o.reshape(B, 1, self.nh * self.hd))
        q, k, v = rope_qkv(self.wqkv(x), cos, sin, self.nh, self.nkv)
        if cache is not None:
            n = min(S, cache.k.shape[1])  # a prompt padded to the attention kernels' multiple may end past the cache
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


class FeedForward(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        # fused W1|W3 (gate | up) projection: one GEMM each way, packed SwiGLU between
        self.w13 = TNLinear(cfg.dim, 2 * cfg.ffn_hidden)
        self.w2 = TNLinear(cfg.ffn_hidden, cfg.dim)

    def forward(self, x):
        from ..ops.llm import swiglu_packed
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
    def _low_precision(self, device) -> bool:
        """The projections run in bf16: under autocast, or with bf16 matmul weights."""
        return torch.is_autocast_enabled(device.type) or self.layers[0].attention.wqkv.weight.dtype == torch.bfloat16

    def new_cache(self, B: int, max_len: int, dtype=None):
        """An empty ``ops.decode.KVCache`` for ``B`` sequences of up to ``max_len`` tokens, in the dtype
        the projections write (bf16 under autocast or with bf16 weights, else the weights' own)."""
        from ..ops.decode import KVCache
        w = self.layers[0].attention.wqkv.weight
        if dtype is None:
            dtype = torch.bfloat16 if self._low_precision(w.device) else w.dtype
        return KVCache(self.cfg.n_layers, B, max_len, self.cfg.n_kv_heads, self.cfg.head_dim, dtype, w.device)

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
            h, d = blk(h, d, cos, sin, None, LayerCache(cache.k[i], cache.v[i], None, None, None))
        rows, last = torch.arange(B, device=tokens.device), prompt_lens.to(tokens.device).long() - 1
        logits = self.output(self.norm.add_forward(h[rows, last].unsqueeze(1), d[rows, last].unsqueeze(1))[1])
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
        for i, blk in enumerate(self.layers):
            h, d = blk(h, d, cos, sin, None, LayerCache(cache.k[i], cache.v[i], pos, lens, mk))
        logits = self.output(self.norm.add_forward(h, d)[1])
        cache.lens = lens
        return logits[:, 0]

    def generate(self, prompts: torch.Tensor, prompt_lens=None, max_new_tokens: int = 32, temperature: float = 0.0,
                 top_k: int = 0, eos_id: Optional[int] = None, generator: Optional[torch.Generator] = None,
                 return_logits: bool = False, max_len: Optional[int] = None):
        """Continue ``prompts`` [B, P] (right-padded; ``prompt_lens`` [B], default all P) by
        ``max_new_tokens`` tokens: LongTensor [B, max_new_tokens] (and the fp32 logits [B, T, V] each was
        chosen from, with ``return_logits``).  Greedy at temperature 0, else temperature / top-k sampling
        with ``torch.multinomial`` from ``generator``; a row that has emitted ``eos_id`` keeps emitting it.
        Runs without gradients in eval mode with bf16 projections on a GPU (never FP8).  The token loop
        reads nothing back from the device; the one synchronisation is the caller's use of the result."""
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
        max_len = P + T if max_len is None else max_len
        if not P + T <= max_len <= self.cfg.max_seq_len:
            raise ValueError(f"generate: need P + max_new_tokens = {P + T} <= max_len = {max_len} <= "
                             f"max_seq_len = {self.cfg.max_seq_len}")
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
        self.eval()
        if TNLinear.impl == "fp8":
            TNLinear.impl = "tn"
        try:
            with torch.no_grad(), torch.autocast(device_type=dev.type, dtype=torch.bfloat16, enabled=amp_on):
                cache = self.new_cache(B, max_len, torch.bfloat16 if amp_on else None)
                self._rope(cache, max(max_len, self._prefill_len(P, dev)))  # the tables, once: the padded prompt's too
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
        tokens = torch.stack(out, dim=1)
        return (tokens, torch.stack(kept, dim=1)) if return_logits else tokens
