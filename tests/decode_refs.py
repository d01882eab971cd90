"""fp64 reference, the derived element-wise error bound and input builders for the decode attention
(csrc/kernels/decode_attention.hip, ops/decode.py).  Plain PyTorch on the CPU:
tests/test_decode_cpu.py shows that the bound admits a correctly rounding implementation and
rejects wrong ones; tests/test_decode_gpu.py holds the kernels to it.

Layout as the kernels see it: q, o [B, Hq, D]; k_cache, v_cache [B, max_len, Hkv, D]; lens [B].
"""
import functools
import math

import torch

from llm_refs import BF16_O, FP32_E

CHUNK = 256   # keys per workgroup of decode_attn_kernel (the GPU test checks it against the library)
GAMMA = 2.0   # one-hot inputs: q = GAMMA * k_target (exact in bf16)


def key_mask(lens, max_len, max_keys=None):
    """bool [B, max_len]: key j of row b is one of the first min(lens[b], max_keys)."""
    n = lens.long().clamp(max=max_len if max_keys is None else max_keys)
    return torch.arange(max_len).view(1, -1) < n.view(-1, 1)


def attend_fp64(q, k_cache, v_cache, mask, scale=None):
    """o, p [B, Hq, max_len] and sum_j p_j |v_jd| in fp64 over the keys ``mask`` [B, max_len] admits.
    Masked by selection: whatever the other rows hold (NaN, Inf) never enters.  A row without a key is 0."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[2]
    sel = mask.view(B, -1, 1, 1)
    k = torch.where(sel, k_cache.double(), 0.0).repeat_interleave(Hq // Hkv, dim=2)
    v = torch.where(sel, v_cache.double(), 0.0).repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bhd,bjhd->bhj", q.double(), k) * (1.0 / math.sqrt(D) if scale is None else scale)
    s = torch.where(mask.view(B, 1, -1), s, -math.inf)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.where(mask.view(B, 1, -1), torch.exp(s - m), 0.0)
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / l, 0.0)
    return dict(o=torch.einsum("bhj,bjhd->bhd", p, v), p=p, pv=torch.einsum("bhj,bjhd->bhd", p, v.abs()))


def decode_fp64(q, k_cache, v_cache, lens, max_keys=None, p_bf16=False):
    """The reference o and its bound b_o:

        |o - o64| <= BF16_O |o64| + (FP32_E + r) sum_j p_j |v_jd|,    r = BF16_O if p_bf16 else 0.

    The chain, for the HIP kernel (p_bf16 = False: its P stays fp32, VALU dots, no MFMA):
      inputs    q, K, V are bf16 and exact in fp32; every product q_d k_d and p v_d is one fp32 FMA;
      scores    8 FMAs per lane, a 3- or 4-level cross-lane tree (D / 8 lanes) and the scale: depth <= 13
                roundings of 2^-24 on sum_d |q_d k_d| / sqrt(D), so the exponent is off by a few 1e-6 at
                the |scores| of these tests (<= 23), and p relatively by as much, plus the device exp
                (2 ulp) and its argument's rounding;
      l         a 6-level wave tree, 3 wave adds, <= 4 chunk FMAs in the combine;
      p . V     <= CHUNK / 16 = 16 FMAs per lane, a 2- or 3-level tree, 3 wave adds, <= 4 chunk FMAs
                with the exp(m_c - M) factors, one division: under 30 roundings = 1.8e-6;
      together below FP32_E = 1e-5 (tests/llm_refs.py) relative to sum_j p_j |v_jd| -- every term of
      the chain scales with the magnitudes before they cancel;
      o         one RNE rounding to bf16 on store: BF16_O |o64|.
    A kernel that rounds P to bf16 for an MFMA (the library's flash kernels do) perturbs each p_j by
    BF16_O relatively: r = BF16_O."""
    mask = key_mask(lens, k_cache.shape[1], max_keys)
    ref = attend_fp64(q, k_cache, v_cache, mask)
    ref["b_o"] = BF16_O * ref["o"].abs() + (FP32_E + (BF16_O if p_bf16 else 0.0)) * ref["pv"]
    ref["mask"] = mask
    return ref


def worst(got, ref):
    """max |got - o64| / bound over the elements; 0/0 counts as 0, err/0 and NaN as inf."""
    err = (got.double() - ref["o"]).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / ref["b_o"])
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


def bf16_round(x):
    return x.float().to(torch.bfloat16)


# ------------------------------------------------------------------------- the model in fp64
def llama_fp64(model, tokens):
    """Logits [B, S, V] of ``models.llama.Llama`` in fp64 on the CPU, written out in plain arithmetic on
    the model's weights and its own fp32 RoPE tables (read as they are): nothing of ops/ is called."""
    from pytorch_operator_amd.models.llama import rope_tables
    cfg = model.cfg
    w = {n: p.detach().double().cpu() for n, p in model.state_dict().items()}
    tokens = tokens.cpu()
    B, S = tokens.shape
    Hq, Hkv, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    cos, sin = (t.double().view(1, S, 1, D // 2) for t in rope_tables(D, S, cfg.rope_theta))

    def norm(x, wn):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.norm_eps) * wn

    def rope(x):
        x0, x1 = x[..., 0::2], x[..., 1::2]
        return torch.stack((x0 * cos - x1 * sin, x0 * sin + x1 * cos), dim=-1).flatten(-2)

    causal = torch.ones(S, S, dtype=torch.bool).tril()
    h = w["tok_embeddings.weight"][tokens]
    for i in range(cfg.n_layers):
        pre = f"layers.{i}."
        qkv = norm(h, w[pre + "attention_norm.weight"]) @ w[pre + "attention.wqkv.weight"].t()
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q, k = rope(q.view(B, S, Hq, D)), rope(k.view(B, S, Hkv, D))
        k = k.repeat_interleave(Hq // Hkv, dim=2)
        v = v.view(B, S, Hkv, D).repeat_interleave(Hq // Hkv, dim=2)
        s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(D)
        p = torch.softmax(s.masked_fill(~causal, -math.inf), dim=-1)
        o = torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, S, Hq * D)
        h = h + o @ w[pre + "attention.wo.weight"].t()
        a, b = (norm(h, w[pre + "ffn_norm.weight"]) @ w[pre + "feed_forward.w13.weight"].t()).chunk(2, dim=-1)
        h = h + (a * torch.sigmoid(a) * b) @ w[pre + "feed_forward.w2.weight"].t()
    return norm(h, w["norm.weight"]) @ w["output.weight"].t()


def teacher_forced(prompt_lens, steps, vocab, seed=0):
    """Ragged prompts and ``steps`` forced tokens per row: (prompts [B, Pmax] right-padded with 0,
    forced [B, steps], full [B, Pmax + steps] = each row's prompt then its forced tokens then 0s)."""
    g = torch.Generator(device="cpu").manual_seed(4000 + seed)
    B, P = len(prompt_lens), max(prompt_lens)
    prompts = torch.randint(1, vocab, (B, P), generator=g)
    forced = torch.randint(1, vocab, (B, steps), generator=g)
    full = torch.zeros(B, P + steps, dtype=torch.long)
    for b, n in enumerate(prompt_lens):
        prompts[b, n:] = 0
        full[b, :n] = prompts[b, :n]
        full[b, n:n + steps] = forced[b]
    return prompts, forced, full


def cached_logits(model, prompts, prompt_lens, forced, cache):
    """[B, steps + 1, V]: the logits after the prompt and after each forced token, through
    prefill + decode_step."""
    dev = cache.k.device
    lens = torch.tensor(prompt_lens, dtype=torch.int32, device=dev)
    out = [model.prefill(prompts.to(dev), lens, cache)]
    for i in range(forced.shape[1]):
        out.append(model.decode_step(forced[:, i].to(dev), cache))
    return torch.stack(out, dim=1)


def at_positions(logits, prompt_lens, steps):
    """Rows of full-sequence logits [B, S, V] at the positions cached_logits reports: [B, steps + 1, V]."""
    idx = torch.tensor([[n - 1 + i for i in range(steps + 1)] for n in prompt_lens], device=logits.device)
    return torch.gather(logits, 1, idx.unsqueeze(-1).expand(-1, -1, logits.shape[-1]))


# ----------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def gaussian_inputs(B, max_len, Hq, Hkv, D, seed=0):
    """Unit gaussian q, k_cache, v_cache rounded to bf16, from a seeded CPU generator (a CPU test and a
    GPU test of one case see the same values).  Callers must not modify them."""
    g = torch.Generator(device="cpu").manual_seed(2000 + seed)
    q = torch.randn(B, Hq, D, generator=g)
    k = torch.randn(B, max_len, Hkv, D, generator=g)
    v = torch.randn(B, max_len, Hkv, D, generator=g)
    return tuple(t.to(torch.bfloat16).contiguous() for t in (q, k, v))


@functools.lru_cache(maxsize=None)
def onehot_inputs(B, max_len, Hq, Hkv, D, targets, seed=0):
    """k entries +-1 and q = GAMMA * k[target[b]]: the target key's score is 2 sqrt(D) (>= 16), every
    other one is 2 N(0, 1), so the target carries nearly all of the row and o ~ v[target].  An
    implementation that loses the target, or lets a target through that it must not see, is off by
    about |v|; one with the scale 1 / D sees a nearly uniform row."""
    g = torch.Generator(device="cpu").manual_seed(3000 + seed)
    k = torch.where(torch.randn(B, max_len, Hkv, D, generator=g) >= 0, 1.0, -1.0)
    v = torch.randn(B, max_len, Hkv, D, generator=g)
    t = torch.tensor(targets).view(B, 1, 1, 1).expand(B, 1, Hkv, D)
    q = GAMMA * torch.gather(k, 1, t)[:, 0].repeat_interleave(Hq // Hkv, dim=1)
    return tuple(x.to(torch.bfloat16).contiguous() for x in (q, k, v))


def poison(k_cache, v_cache, lens, max_keys=None):
    """Copies of the caches with NaN in every row at or past min(lens[b], max_keys)."""
    dead = ~key_mask(lens, k_cache.shape[1], max_keys).view(k_cache.shape[0], -1, 1, 1)
    nan = torch.full((), math.nan, dtype=k_cache.dtype)
    return torch.where(dead, nan, k_cache).contiguous(), torch.where(dead, nan, v_cache).contiguous()
