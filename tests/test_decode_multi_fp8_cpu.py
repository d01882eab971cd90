"""The multi-token decode step on an e4m3 KV cache on the CPU: ops.decode.append_rows / attend_rows against the
per-token rope_append and the per-row decode_attention on the same cache, and greedy speculative generate
against the single-token loop with the same cache dtype.
"""
import pytest
import torch

import decode_refs as R
from pytorch_operator_amd.models.llama import CONFIGS, Llama, rope_tables
from pytorch_operator_amd.ops import decode as Dc

FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("S,hq,hkv", [(1, 4, 1), (3, 4, 2), (4, 8, 2)])
def test_cpu_rows_on_an_e4m3_cache_equal_single_token_calls(S, hq, hkv):
    B, D, max_len = 3, 64, 40
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B, S, (hq + 2 * hkv) * D, generator=g)
    cos, sin = rope_tables(D, max_len, 500000.0)
    pos = torch.tensor([0, 17, max_len - 2], dtype=torch.int32)   # the last sequence runs off the cache
    c1, c2 = (Dc.KVCache(1, B, max_len, hkv, D, FP8) for _ in range(2))
    (k1, v1, ks1, vs1), (k2, v2, ks2, vs2) = ((c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]) for c in (c1, c2))
    q = Dc.append_rows(qkv, cos, sin, k1, v1, pos, hq, hkv, ks1, vs1)
    want = torch.stack([Dc.rope_append(qkv[:, s], cos, sin, k2, v2, pos + s, hq, hkv, ks2, vs2) for s in range(S)], 1)
    assert torch.equal(q, want) and torch.equal(ks1, ks2) and torch.equal(vs1, vs2)
    assert torch.equal(k1.view(torch.uint8), k2.view(torch.uint8)) and torch.equal(v1.view(torch.uint8), v2.view(torch.uint8))
    assert k1.view(torch.uint8)[0, :S].any() and not k1.view(torch.uint8)[2, :max_len - 2].any()
    lens = (pos + S).clamp(max=max_len)
    for mk in (max_len, 19):
        o = Dc.attend_rows(q, k1, v1, lens, mk, k_scale=ks1, v_scale=vs1)
        for s in range(S):
            one = Dc.decode_attention(q[:, s], k1, v1, lens.clamp(max=mk) - (S - 1 - s), mk, k_scale=ks1, v_scale=vs1)
            assert torch.equal(o[:, s], one)
    with pytest.raises(ValueError):
        Dc.attend_rows(q, k1, v1, lens, impl="sdpa", k_scale=ks1, v_scale=vs1)


def test_speculative_generate_on_an_e4m3_cache_emits_the_single_token_loops_tokens():
    torch.manual_seed(3)
    model = Llama(CONFIGS["llama-mini"]).eval()
    torch.manual_seed(4)
    draft = Llama(CONFIGS["llama-mini"]).eval()
    plens, T = (9, 5, 12), 10
    prompts, _, _ = R.teacher_forced(plens, 1, model.cfg.vocab_size)
    toks, logits = model.generate(prompts, list(plens), max_new_tokens=T, return_logits=True, draft=draft,
                                  draft_tokens=3, kv_dtype=FP8)
    assert toks.shape == (3, T) and torch.equal(toks, logits.argmax(-1))
    plain = model.generate(prompts, list(plens), max_new_tokens=T, kv_dtype=FP8)
    assert torch.equal(plain, toks)     # fp32 on one device: the same quantiser and the same choices on both sides
