"""The FP8 KV cache of ops/decode.py on the CPU: the PyTorch path of rope_append, quantize_kv and
decode_attention against a hand-written dequantise-then-attend in fp64, the prefill's and the append's
bytes, and generate on llama-tiny.
"""
import pytest
import torch

import decode_refs as R
from pytorch_operator_amd.models.llama import CONFIGS, Llama, rope_tables
from pytorch_operator_amd.ops import decode as Dc
from pytorch_operator_amd.ops.llm import rope_qkv_reference

FP8 = torch.float8_e4m3fn
B, S, HQ, HKV, D, MAX_LEN = 2, 5, 4, 2, 64, 9


def _filled():
    """A cache layer filled from a seeded sequence: the first S - 1 tokens by quantize_kv, the last by rope_append."""
    g = torch.Generator().manual_seed(5)
    seq = (torch.randn(B, S, (HQ + 2 * HKV) * D, generator=g) * 3).to(torch.bfloat16)
    cos, sin = rope_tables(D, MAX_LEN, 500000.0)
    q, k, v = rope_qkv_reference(seq, cos[:S], sin[:S], HQ, HKV)
    c = Dc.KVCache(1, B, MAX_LEN, HKV, D, FP8)
    Dc.quantize_kv(k[:, :S - 1], v[:, :S - 1], c.k[0], c.v[0], c.k_scale[0], c.v_scale[0])
    pos = torch.full((B,), S - 1, dtype=torch.int32)
    ql = Dc.rope_append(seq[:, S - 1], cos, sin, c.k[0], c.v[0], pos, HQ, HKV, c.k_scale[0], c.v_scale[0])
    return c, ql, q, k, v


def test_fp8_cache_path_is_the_fp64_attention_on_the_dequantised_rows():
    c, ql, q, k, v = _filled()
    assert c.k.dtype == FP8 and c.k_scale.shape == (1, B, HKV, 12) and torch.equal(ql, q[:, S - 1])
    kd, vd = (c.k[0].double() * c.k_scale[0][:, :, :MAX_LEN].transpose(1, 2).unsqueeze(-1).double(),
              c.v[0].double() * c.v_scale[0][:, :, :MAX_LEN].transpose(1, 2).unsqueeze(-1).double())
    # the quantiser: within half an e4m3 step (2^-4 relative to the row's scaled maximum of 448) of the bf16 rows
    for got, want, sc in ((kd, k, c.k_scale), (vd, v, c.v_scale)):
        step = 16.0 * sc[0][:, :, :S].transpose(1, 2).unsqueeze(-1).double()
        assert ((got[:, :S] - want.double()).abs() <= step).all() and (got[:, :S].abs().amax(-1) > 0).all()
    lens = torch.tensor([S, 3], dtype=torch.int32)
    c.k[0].view(torch.uint8)[1, 3:] = 0x7f   # NaN codes and scales past the lengths must not reach the result
    c.k_scale[0][1, :, 3:] = float("nan")
    o = Dc.decode_attention(ql, c.k[0], c.v[0], lens, k_scale=c.k_scale[0], v_scale=c.v_scale[0])
    ref = R.decode_fp64(ql, kd, vd, lens)
    assert R.worst(o, ref) <= 1.0


def test_prefill_and_append_store_the_same_bytes():
    c, _, _, k, v = _filled()
    whole = Dc.KVCache(1, B, MAX_LEN, HKV, D, FP8)
    Dc.quantize_kv(k, v, whole.k[0], whole.v[0], whole.k_scale[0], whole.v_scale[0])
    for a, b in ((c.k, whole.k), (c.v, whole.v)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(c.k_scale, whole.k_scale) and torch.equal(c.v_scale, whole.v_scale)


def test_generate_with_an_fp8_cache_on_llama_tiny():
    torch.manual_seed(3)
    model = Llama(CONFIGS["llama-tiny"]).eval()
    prompts = torch.randint(1, 256, (2, 6))
    toks, logits = model.generate(prompts, [6, 3], max_new_tokens=4, return_logits=True, kv_dtype=FP8)
    ref, ref_logits = model.generate(prompts, [6, 3], max_new_tokens=4, return_logits=True)
    assert toks.shape == (2, 4) and torch.equal(toks, logits.argmax(-1))
    d = float((logits - ref_logits).abs().max())
    assert 0 < d < 0.1 * float(ref_logits.abs().max())     # the quantiser is in the numbers, and small


@pytest.mark.parametrize("bad", ["no_scales", "shape", "dtype", "sdpa", "scales_on_bf16"])
def test_fp8_refusals(bad):
    c, ql, *_ = _filled()
    kw = dict(q=ql, k_layer=c.k[0], v_layer=c.v[0], lens=torch.ones(B, dtype=torch.int32),
              k_scale=c.k_scale[0], v_scale=c.v_scale[0])
    kw.update({"no_scales": dict(v_scale=None), "shape": dict(k_scale=c.k_scale[0][:, :, :8].contiguous()),
               "dtype": dict(k_scale=c.k_scale[0].double()), "sdpa": dict(impl="sdpa"),
               "scales_on_bf16": dict(k_layer=c.k[0].to(torch.bfloat16), v_layer=c.v[0].to(torch.bfloat16))}[bad])
    with pytest.raises(ValueError):
        Dc.decode_attention(**kw)
