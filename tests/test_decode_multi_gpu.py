"""The multi-token decode kernels (csrc/kernels/decode_attention_multi.hip) on the GPU: append_rows bit for bit
against S rope_append calls, attend_rows inside a derived bound of the fp64 reference per query row with NaN
in every cache row it must not read and in the partials workspace, and decode_steps / speculative generate of
the bf16 models against an fp64 forward.
"""
import functools
import math

import pytest
import torch

import decode_refs as R
from llm_refs import BF16_O, FP32_E

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = R.CHUNK
MAX_LEN = 3 * C + 1
HKV = 2
P_SPLIT = 2.0 ** -16  # P enters the MFMA as bf16(p) + bf16(p - bf16(p)): what the second rounding leaves


@pytest.fixture(scope="module")
def Dc():
    from pytorch_operator_amd.ops import _native, decode
    assert int(_native.load().pto_decode_chunk()) == C and int(_native.load().pto_decode_multi_rows()) == 16
    return decode


def _lengths(S):  # one key per row at the least, around one chunk boundary, past two, the whole cache; and too few
    return (S, C - 1, C, C + 1, 2 * C + 1, MAX_LEN, 1)


def _ref(q, k, v, lens, max_keys=None):
    """Poisoned caches, and fp64 o and the bound per query row of q [B, S, Hq, D], each with its own n_s."""
    S, lens = q.shape[1], torch.tensor(lens, dtype=torch.int32)
    n = lens.clamp(max=MAX_LEN if max_keys is None else max_keys)
    rows = [R.decode_fp64(q[:, s], k, v, n - (S - 1 - s)) for s in range(S)]
    o, pv = (torch.stack([r[key] for r in rows], dim=1) for key in ("o", "pv"))
    kp, vp = R.poison(k, v, lens, max_keys)
    return q.contiguous(), kp, vp, lens, dict(o=o, b_o=BF16_O * o.abs() + (FP32_E + P_SPLIT) * pv)


@functools.lru_cache(maxsize=None)
def _case(D, G, S, max_keys):
    lens = _lengths(S)
    q, k, v = R.gaussian_inputs(len(lens), MAX_LEN, S * HKV * G, HKV, D)   # S * Hq "heads" of q: [B, S, Hq, D]
    return _ref(q.view(len(lens), S, HKV * G, D), k, v, lens, max_keys)


def _run(Dc, q, kp, vp, lens, max_keys=None):
    q, kp, vp, lens = (t.to(DEV) for t in (q, kp, vp, lens))
    Dc._partials(q.device, q.numel() // q.shape[-1] * 4 * (q.shape[-1] + 2)).fill_(math.nan)
    return Dc.attend_rows(q, kp, vp, lens, max_keys)


# ------------------------------------------------------------------------------ append_rows
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_rows_is_s_rope_appends_bit_for_bit(Dc, D, dtype):
    from pytorch_operator_amd.models.llama import rope_tables
    B, S, hq, hkv, max_len = 3, 4, 4, 2, 64
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    qkv = torch.randn(B, S, (hq + 2 * hkv) * D, generator=torch.Generator().manual_seed(D)).to(dtype).to(DEV)
    cos, sin = rope_tables(D, max_len, 500000.0, DEV)
    pos = torch.tensor((5, max_len - 3, -2), dtype=torch.int32, device=DEV)  # last token at max_len; a negative start

    def fresh():  # sentinels in every byte that must stay
        return (torch.full((B, max_len, hkv, D), 7.0, dtype=dtype, device=DEV),
                torch.full((B, max_len, hkv, D), -3.0, dtype=dtype, device=DEV))

    (k1, v1), (k2, v2) = fresh(), fresh()
    q = Dc.append_rows(qkv, cos, sin, k1, v1, pos, hq, hkv)
    want = torch.stack([Dc.rope_append(qkv[:, s].contiguous(), cos, sin, k2, v2, pos + s, hq, hkv) for s in range(S)], 1)
    assert torch.equal(q.view(bits), want.view(bits))
    assert torch.equal(k1.view(bits), k2.view(bits)) and torch.equal(v1.view(bits), v2.view(bits))
    written = (k1 != 7.0).any(-1).any(-1).sum(1).tolist()   # rows per sequence: the tokens that fall off store nothing
    assert written == [4, 3, 2]


# ------------------------------------------------------------------------------ attend_rows
@pytest.mark.parametrize("max_keys", [None, C + 1])
@pytest.mark.parametrize("G,S", [(1, 16), (2, 3), (4, 4), (4, 3), (8, 2), (4, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_attend_rows_inside_the_bound_with_nan_past_the_lengths_and_in_the_workspace(Dc, D, G, S, max_keys):
    q, kp, vp, lens_t, ref = _case(D, G, S, max_keys)
    o = _run(Dc, q, kp, vp, lens_t, max_keys)
    got = o.cpu()
    w = R.worst(got, ref)
    print(f"D {D} G {G} S {S} max_keys {max_keys}: worst error / bound {w:.3f}")
    assert got.shape == q.shape and got.dtype == torch.bfloat16 and not torch.isnan(got.float()).any()
    assert w <= 1.0
    assert not got[-1, :S - 1].any()                        # lens 1: only the last query has a key
    assert torch.equal(o.view(torch.int16), _run(Dc, q, kp, vp, lens_t, max_keys).view(torch.int16))


@pytest.mark.parametrize("s0", [0, 2, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_a_query_sees_the_key_at_its_own_position_and_none_after(Dc, D, s0):
    G, S, lens = 4, 4, (7, C + 1, 2 * C + 1, MAX_LEN)
    targets = tuple(n - S + s0 for n in lens)                # the key that query s0 appends
    q, k, v = R.onehot_inputs(len(lens), MAX_LEN, HKV * G, HKV, D, targets)
    q, kp, vp, lens_t, ref = _ref(q.unsqueeze(1).expand(-1, S, -1, -1), k, v, lens)
    got = _run(Dc, q, kp, vp, lens_t).cpu()
    assert R.worst(got, ref) <= 1.0
    vt = torch.stack([v[b, t] for b, t in enumerate(targets)]).repeat_interleave(G, dim=1).float()  # [B, Hq, D]
    off = (got.float() - vt.unsqueeze(1)).abs().amax(dim=(2, 3))                                     # [B, S]
    print(f"D {D} s0 {s0}: max |o - v[target]| per sequence and query {off.tolist()}")
    assert (off[:, s0:] < 0.05).all() and (off[:, :s0] > 0.5).all()


def test_refusals(Dc):
    def mk(S, Hq, Hkv, D=64, dtype=torch.bfloat16):
        return (torch.zeros(2, S, Hq, D, dtype=dtype, device=DEV), torch.zeros(2, 8, Hkv, D, dtype=dtype, device=DEV),
                torch.zeros(2, 8, Hkv, D, dtype=dtype, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV))
    Dc.attend_rows(*mk(4, 4, 1))
    q, k, v, lens = mk(2, 4, 1)
    k8 = torch.zeros(2, 9, 1, 64, dtype=torch.bfloat16, device=DEV).view(-1)[4:4 + k.numel()].view(k.shape)  # 8 bytes off
    for bad in (dict(zip(("q", "k_layer", "v_layer", "lens"), mk(4, 8, 1))),   # S * G = 32
                dict(k_layer=k.to(Dc.FP8), v_layer=v.to(Dc.FP8)), dict(k_layer=k8), dict(lens=lens.cpu()),
                dict(zip(("q", "k_layer", "v_layer", "lens"), mk(2, 4, 1, 32))),
                dict(zip(("q", "k_layer", "v_layer", "lens"), mk(2, 4, 1, 64, torch.float32)))):
        with pytest.raises(ValueError):
            Dc.attend_rows(**dict(dict(q=q, k_layer=k, v_layer=v, lens=lens), **bad))
    # the library path serves what the kernel does not
    assert Dc.attend_rows(*mk(4, 8, 1, 32, torch.float32), impl="sdpa").shape == (2, 4, 8, 32)
    cos = sin = torch.zeros(8, 32, device=DEV)
    with pytest.raises(ValueError):
        Dc.append_rows(torch.zeros(2, 2, 6 * 64, dtype=torch.bfloat16, device=DEV), cos, sin, k.to(Dc.FP8), v.to(Dc.FP8),
                       lens, 4, 1)


# ------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_bf16_decode_steps_and_speculative_generate_against_the_fp64_forward(Dc, name):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU Llama.forward from the fp64 CPU forward on the
    same sequences and positions, measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Attention, Llama
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    torch.manual_seed(12)
    draft = Llama(CONFIGS[name]).eval().to(DEV)
    plens, steps, S = (130, 128, 7), 8, 4
    prompts, forced, full = R.teacher_forced(plens, steps, model.cfg.vocab_size)
    with torch.no_grad():
        want = R.at_positions(R.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        before = dict(Attention.decode_calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((R.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            cache = model.new_cache(len(plens), max(plens) + steps)
            got = [model.prefill(prompts.to(DEV), torch.tensor(plens, dtype=torch.int32, device=DEV), cache).unsqueeze(1)]
            got += [model.decode_steps(forced[:, i:i + S].to(DEV), cache) for i in range(0, steps, S)]
    assert cache.lens.tolist() == [n + steps for n in plens]
    dev = float((torch.cat(got, dim=1).double().cpu() - want).abs().max())
    print(f"{name}: uncached bf16 forward vs fp64 {base:.4e}; prefill + decode_steps vs fp64 {dev:.4e}")
    assert base > 0 and dev <= 2 * base
    assert Attention.decode_calls["hip-rows"] - before.get("hip-rows", 0) == (steps // S) * model.cfg.n_layers
    assert Attention.decode_calls["sdpa"] == before.get("sdpa", 0)
    T = 8
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=T, return_logits=True, draft=draft,
                                  draft_tokens=3)
    assert toks.shape == (3, T) and torch.equal(toks, logits.argmax(-1))
    assert Attention.decode_calls["hip-rows"] > before.get("hip-rows", 0) + (steps // S) * model.cfg.n_layers
    for b, n in enumerate(plens):
        with torch.no_grad():
            ref = R.llama_fp64(model, torch.cat([prompts[b, :n], toks[b].cpu()]).unsqueeze(0))[0, n - 1:n - 1 + T]
        assert float((logits[b].double().cpu() - ref).abs().max()) <= 2 * base
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=T, return_logits=True, draft=draft,
                                    draft_tokens=3)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
