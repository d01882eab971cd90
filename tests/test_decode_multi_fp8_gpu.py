"""The multi-token decode kernels on the e4m3 KV cache (csrc/kernels/decode_attention_multi_fp8.hip) on the GPU:
append_rows byte for byte against S rope_append calls, attend_rows inside the bf16 multi-token bound of the fp64
reference on the dequantised cache with NaN codes, NaN scales and a NaN workspace wherever it must not read, and
decode_steps / speculative generate of the models on an e4m3 cache against the fp64 forward.
"""
import functools
import math

import pytest
import torch

import decode_refs as R
from llm_refs import BF16_O, FP32_E
from pytorch_operator_amd.ops import decode as Dc
from pytorch_operator_amd.ops.skinny import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu

DEV, FP8, C = "cuda", torch.float8_e4m3fn, R.CHUNK
MAX_LEN, HKV = 3 * C + 1, 2
SENT_BYTE, SENT = 0x55, -7.0
P_SPLIT = 2.0 ** -16  # P enters the MFMA as bf16(p') + bf16(p' - bf16(p')): what the second rounding leaves


def _quantized(k, v, lens, max_keys=None, k_exp=(0, 0), v_exp=(0, 0)):
    """k, v [B, MAX_LEN, HKV, D] scaled per (token, head) by 2^[lo, hi] and quantised: (codes and padded scales
    with NaN in every row at or past min(lens, max_keys), on the GPU), and the dequantised caches."""
    B, D = k.shape[0], k.shape[-1]
    g = torch.Generator().manual_seed(77)
    dead = ~R.key_mask(lens, MAX_LEN, max_keys)
    out = []
    for x, (lo, hi) in ((k, k_exp), (v, v_exp)):
        x = x.float() * torch.exp2(torch.randint(lo, hi + 1, (B, MAX_LEN, HKV, 1), generator=g).float())
        code, s = quantize_rows(x.to(torch.bfloat16).view(-1, D))
        out.append(dequantize_rows(code, s).view(x.shape))
        code = code.view(x.shape).view(torch.uint8).masked_fill(dead.view(B, MAX_LEN, 1, 1), 0x7f).view(FP8)
        s = s.view(B, MAX_LEN, HKV).masked_fill(dead.view(B, MAX_LEN, 1), math.nan).transpose(1, 2)
        out += [code.contiguous().to(DEV), torch.nn.functional.pad(s, (0, -MAX_LEN % 4), value=math.nan).contiguous().to(DEV)]
    kd, kc, ks, vd, vc, vs = out
    return (kc, vc, ks, vs), kd, vd


def _ref(q, kd, vd, lens, max_keys=None):
    """fp64 o and the bound per query row of q [B, S, Hq, D], each with its own n_s."""
    S = q.shape[1]
    n = lens.clamp(max=MAX_LEN if max_keys is None else max_keys)
    rows = [R.decode_fp64(q[:, s], kd, vd, n - (S - 1 - s)) for s in range(S)]
    o, pv = (torch.stack([r[key] for r in rows], dim=1) for key in ("o", "pv"))
    return dict(o=o, b_o=BF16_O * o.abs() + (FP32_E + P_SPLIT) * pv)


def _run(q, cache, lens, max_keys=None):
    kc, vc, ks, vs = cache
    q = q.contiguous().to(DEV)
    Dc._partials(q.device, q.numel() // q.shape[-1] * 4 * (q.shape[-1] + 2)).fill_(math.nan)
    return Dc.attend_rows(q, kc, vc, lens.to(DEV), max_keys, k_scale=ks, v_scale=vs)


# ------------------------------------------------------------------------------ append_rows
@pytest.mark.parametrize("D", [64, 128])
def test_append_rows_is_s_rope_appends_byte_for_byte(D):
    from pytorch_operator_amd.models.llama import rope_tables
    B, S, hq, hkv, max_len = 3, 4, 4, 2, 64
    H = hq + 2 * hkv
    g = torch.Generator().manual_seed(D)
    mag = torch.exp2(torch.randint(-20, 21, (B, S, H, 1), generator=g).float())
    mag[:, :, [1, hq + 1, H - 1]] = torch.tensor([0.0, 2.0 ** 20, 2.0 ** -20]).view(1, 1, 3, 1)
    qkv = (torch.randn(B, S, H, D, generator=g) * mag).to(torch.bfloat16)
    qkv[0, 1, hq] = 0                                                           # an all-zero k head: scale 1
    qkv = qkv.view(B, S, H * D).to(DEV)
    cos, sin = rope_tables(D, max_len, 500000.0, DEV)
    pos = torch.tensor((5, max_len - 3, -2), dtype=torch.int32, device=DEV)  # last token at max_len; a negative start

    def fresh():  # sentinels in every byte and every scale that must stay
        pad = -(-max_len // 4) * 4
        return (*(torch.full((B, max_len, hkv, D), SENT_BYTE, dtype=torch.uint8, device=DEV).view(FP8) for _ in range(2)),
                *(torch.full((B, hkv, pad), SENT, device=DEV) for _ in range(2)))

    (k1, v1, ks1, vs1), (k2, v2, ks2, vs2) = fresh(), fresh()
    q = Dc.append_rows(qkv, cos, sin, k1, v1, pos, hq, hkv, ks1, vs1)
    want = torch.stack([Dc.rope_append(qkv[:, s].contiguous(), cos, sin, k2, v2, pos + s, hq, hkv, ks2, vs2)
                        for s in range(S)], 1)
    assert torch.equal(q.view(torch.int16), want.view(torch.int16))
    for a, b in ((k1, k2), (v1, v2)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for a, b in ((ks1, ks2), (vs1, vs2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (k1.view(torch.uint8) != SENT_BYTE).any(-1).any(-1).sum(1).tolist() == [4, 3, 2]
    assert (ks1 != SENT).any(1).sum(1).tolist() == [4, 3, 2] and float(ks1[0, 0, 6]) == 1.0


# ------------------------------------------------------------------------------ attend_rows
@functools.lru_cache(maxsize=None)
def _case(D, G, S, max_keys):
    lens = torch.tensor((S, C - 1, C, C + 1, 2 * C + 1, MAX_LEN, 1), dtype=torch.int32)
    q, k, v = R.gaussian_inputs(len(lens), MAX_LEN, S * HKV * G, HKV, D)   # S * Hq "heads" of q: [B, S, Hq, D]
    q = q.view(len(lens), S, HKV * G, D)
    cache, kd, vd = _quantized(k, v, lens, max_keys, (-2, 1), (-6, 6))
    return q, cache, lens, _ref(q, kd, vd, lens, max_keys)


@pytest.mark.parametrize("max_keys", [None, C + 1])
@pytest.mark.parametrize("G,S", [(1, 16), (2, 3), (4, 4), (4, 3), (8, 2), (4, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_attend_rows_inside_the_bound_with_nan_past_the_lengths_and_in_the_workspace(D, G, S, max_keys):
    q, cache, lens, ref = _case(D, G, S, max_keys)
    o = _run(q, cache, lens, max_keys)
    got = o.cpu()
    w = R.worst(got, ref)
    print(f"D {D} G {G} S {S} max_keys {max_keys}: worst error / bound {w:.3f}")
    assert got.shape == q.shape and got.dtype == torch.bfloat16 and not torch.isnan(got.float()).any()
    assert w <= 1.0
    assert not got[-1, :S - 1].any()                        # lens 1: only the last query has a key
    assert torch.equal(o.view(torch.int16), _run(q, cache, lens, max_keys).view(torch.int16))


@pytest.mark.parametrize("s0", [0, 2, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_a_query_sees_the_key_at_its_own_position_and_none_after(D, s0):
    G, S, lens = 4, 4, (7, C + 1, 2 * C + 1, MAX_LEN)
    targets = tuple(n - S + s0 for n in lens)                # the key that query s0 appends
    q, k, v = R.onehot_inputs(len(lens), MAX_LEN, HKV * G, HKV, D, targets)
    q, lens_t = q.unsqueeze(1).expand(-1, S, -1, -1), torch.tensor(lens, dtype=torch.int32)
    cache, kd, vd = _quantized(k, v, lens_t)
    got = _run(q, cache, lens_t).cpu()
    assert R.worst(got, _ref(q, kd, vd, lens_t)) <= 1.0
    vt = torch.stack([vd[b, t] for b, t in enumerate(targets)]).repeat_interleave(G, dim=1).float()  # [B, Hq, D]
    off = (got.float() - vt.unsqueeze(1)).abs().amax(dim=(2, 3))                                     # [B, S]
    print(f"D {D} s0 {s0}: max |o - v[target]| per sequence and query {off.tolist()}")
    assert (off[:, s0:] < 0.05).all() and (off[:, :s0] > 0.5).all()


@pytest.mark.parametrize("bad", ["bf16_scales", "shape", "dtype", "device", "rows", "sdpa", "d32"])
def test_refusals(bad):
    def mk(S, Hq, D=64, dtype=FP8):
        z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        return dict(q=z(2, S, Hq, D), k_layer=z(2, 8, 1, D).to(dtype), v_layer=z(2, 8, 1, D).to(dtype),
                    lens=torch.ones(2, dtype=torch.int32, device=DEV), k_scale=z(2, 1, 8, dt=torch.float32) + 1,
                    v_scale=z(2, 1, 8, dt=torch.float32) + 1)
    ok = mk(4, 4)
    assert Dc.attend_rows(**ok).shape == (2, 4, 4, 64)
    kw = {"bf16_scales": mk(4, 4, dtype=torch.bfloat16), "shape": dict(ok, k_scale=ok["k_scale"][:, :, :7].contiguous()),
          "dtype": dict(ok, v_scale=ok["v_scale"].double()), "device": dict(ok, k_scale=ok["k_scale"].cpu()),
          "rows": mk(4, 8), "sdpa": dict(ok, impl="sdpa"), "d32": mk(4, 4, 32)}[bad]
    with pytest.raises(ValueError):
        Dc.attend_rows(**kw)
    if bad in ("bf16_scales", "shape", "dtype", "device", "d32"):
        D = kw["q"].shape[-1]
        with pytest.raises(ValueError):
            Dc.append_rows(torch.zeros(2, 2, 6 * D, dtype=torch.bfloat16, device=DEV), *(torch.zeros(8, D // 2, device=DEV),) * 2,
                           kw["k_layer"], kw["v_layer"], kw["lens"], 4, 1, kw["k_scale"], kw["v_scale"])


# ------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_fp8_cache_decode_steps_and_speculative_generate_against_the_fp64_forward(name):
    """Tolerance: base8 + 2 base, the FP8 model test's rule.  base8 is the quantiser alone: the fp32 CPU model
    through prefill + decode_step with an e4m3 cache against the fp64 forward; base, and its factor 2, are the bf16
    model test's: the uncached bf16 GPU forward against the same fp64 forward.  Both are measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Attention, Llama
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    torch.manual_seed(12)
    draft = Llama(CONFIGS[name]).eval().to(DEV)
    plens, steps, S, L = (130, 128, 7), 8, 4, model.cfg.n_layers
    prompts, forced, full = R.teacher_forced(plens, steps, model.cfg.vocab_size)
    with torch.no_grad():
        want = R.at_positions(R.llama_fp64(model, full), plens, steps)
        got8 = R.cached_logits(model, prompts, plens, forced, model.new_cache(len(plens), max(plens) + steps, FP8))
        base8 = float((got8.double() - want).abs().max())
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        before = dict(Attention.decode_calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((R.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            cache = model.new_cache(len(plens), max(plens) + steps, FP8)
            got = [model.prefill(prompts.to(DEV), torch.tensor(plens, dtype=torch.int32, device=DEV), cache).unsqueeze(1)]
            got += [model.decode_steps(forced[:, i:i + S].to(DEV), cache) for i in range(0, steps, S)]
    assert cache.k.dtype == FP8 and cache.lens.tolist() == [n + steps for n in plens]
    dev = float((torch.cat(got, dim=1).double().cpu() - want).abs().max())
    print(f"{name}: fp32 CPU with an e4m3 cache vs fp64 (base8) {base8:.4e}; uncached bf16 forward vs fp64 (base) "
          f"{base:.4e}; bf16 GPU prefill + decode_steps with an e4m3 cache vs fp64 {dev:.4e}")
    assert base > 0 and base8 > 0 and dev <= base8 + 2 * base
    calls = Attention.decode_calls
    assert calls["hip-rows-fp8"] - before.get("hip-rows-fp8", 0) == (steps // S) * L
    mid = dict(calls)
    run = lambda: model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True, draft=draft,  # noqa: E731
                                 draft_tokens=3, kv_dtype=FP8)
    toks, logits = run()
    assert toks.shape == (3, 8) and torch.equal(toks, logits.argmax(-1))
    # a round: one multi-token target step and k + 1 single draft steps, each once per layer (the draft has L too)
    rounds, rem = divmod(calls["hip-rows-fp8"] - mid["hip-rows-fp8"], L)
    assert rounds >= 1 and rem == 0 and calls["hip-fp8"] - mid.get("hip-fp8", 0) == rounds * 4 * L
    assert calls["sdpa"] == before.get("sdpa", 0) and calls["hip-rows"] == before.get("hip-rows", 0)
    again, logits2 = run()
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
