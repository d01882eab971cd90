"""The FP8 KV cache kernels (csrc/kernels/decode_attention_fp8.hip) on the GPU: the append and the
prefill's copy against ops.skinny.quantize_rows with sentinels around every written row, the attention
inside the bound of tests/decode_refs.py on the dequantised cache with NaN codes and NaN scales wherever
it must not read, and the models through prefill + decode_step + generate.
"""
import functools

import pytest
import torch

import decode_refs as R
from pytorch_operator_amd.ops import decode as Dc
from pytorch_operator_amd.ops.skinny import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu

DEV, FP8, C = "cuda", torch.float8_e4m3fn, R.CHUNK
MAX_LEN, B, HKV = 3 * C + 1, 4, 2
LENS = {"a": (0, 1, C - 1, C), "b": (C + 1, 2 * C + 1, MAX_LEN, 1), "tile": (15, 16, 17, C + 17)}
SENT_BYTE, SENT = 0x55, -7.0


def _i32(n):
    return torch.tensor(n, dtype=torch.int32)


def _fresh(Bq, max_len, hkv, D):
    pad = -(-max_len // 4) * 4
    return (*(torch.full((Bq, max_len, hkv, D), SENT_BYTE, dtype=torch.uint8, device=DEV).view(FP8) for _ in range(2)),
            *(torch.full((Bq, hkv, pad), SENT, device=DEV) for _ in range(2)))


def _check_rows(layer, scale, want, rows):
    """``layer`` / ``scale`` hold quantize_rows of ``want[b, p]`` [Hkv, D] (bf16) at every (b, p) of ``rows``
    and the sentinels everywhere else."""
    layer, scale = layer.cpu(), scale.cpu()
    touched = torch.zeros(layer.shape[:2], dtype=torch.bool)
    for b, p in rows:
        q, s = quantize_rows(want[b, p].cpu())
        assert torch.equal(scale[b, :, p], s)
        assert torch.equal(dequantize_rows(layer[b, p], scale[b, :, p]), dequantize_rows(q, s))
        touched[b, p] = True
    assert (layer.view(torch.uint8)[~touched] == SENT_BYTE).all()
    pad = torch.zeros(scale.shape[0], scale.shape[2], dtype=torch.bool)
    pad[:, :touched.shape[1]] = touched
    assert (scale.transpose(1, 2)[~pad] == SENT).all()


# ------------------------------------------------------------------------------ the writers
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 1), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_append_is_quantize_rows_of_the_bf16_row_and_writes_one_row(D, hq, hkv):
    from pytorch_operator_amd.models.llama import rope_tables
    Bq, max_len, H, pos = 3, 256, hq + 2 * hkv, (0, 129, 255)
    g = torch.Generator().manual_seed(D + hq)
    mag = torch.exp2(torch.randint(-20, 21, (Bq, H, 1), generator=g).float())
    mag[:, [1, hq, H - 1]] = torch.tensor([0.0, 2.0 ** 20, 2.0 ** -20]).view(1, 3, 1)   # one all-zero head, both ends
    qkv = (torch.randn(Bq, H, D, generator=g) * mag).to(torch.bfloat16).view(Bq, H * D).to(DEV)
    qkv[0, hq * D:(hq + 1) * D] = 0                                                      # a zero k row: scale 1
    cos, sin = rope_tables(D, max_len, 500000.0, DEV)
    for p0 in (pos[0], max_len, -1):                       # row 0 inside, past and before the cache
        p = _i32((p0,) + pos[1:]).to(DEV)
        kb, vb = (torch.zeros(Bq, max_len, hkv, D, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        q_ref = Dc.rope_append(qkv, cos, sin, kb, vb, p, hq, hkv)
        kc, vc, ks, vs = _fresh(Bq, max_len, hkv, D)
        q = Dc.rope_append(qkv, cos, sin, kc, vc, p, hq, hkv, ks, vs)
        assert torch.equal(q.view(torch.int16), q_ref.view(torch.int16))
        rows = [(b, pp) for b, pp in enumerate(p.tolist()) if 0 <= pp < max_len]
        _check_rows(kc, ks, kb, rows)
        _check_rows(vc, vs, vb, rows)


@pytest.mark.parametrize("max_len", [128, 256])
@pytest.mark.parametrize("D", [64, 128])
def test_quantize_kv_fills_rows_below_n_and_no_other(D, max_len):
    Bq, S, hkv = 2, 130, 2
    g = torch.Generator().manual_seed(D + max_len)
    k, v = ((torch.randn(Bq, S, hkv, D, generator=g) * torch.exp2(torch.randint(-20, 21, (Bq, S, hkv, 1), generator=g)
                                                                  .float())).to(torch.bfloat16) for _ in range(2))
    kc, vc, ks, vs = _fresh(Bq, max_len, hkv, D)
    Dc.quantize_kv(k.to(DEV), v.to(DEV), kc, vc, ks, vs)
    rows = [(b, p) for b in range(Bq) for p in range(min(S, max_len))]
    _check_rows(kc, ks, k, rows)
    _check_rows(vc, vs, v, rows)


# -------------------------------------------------------------------------- decode_attention
@functools.lru_cache(maxsize=None)
def _case(D, G, which, max_keys=None):
    """An e4m3 cache whose rows differ in scale by far more than the bound, NaN codes and NaN scales in every
    row that must not be read, and the fp64 reference on the dequantised cache: computed once."""
    lens = _i32(LENS[which])
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HKV * G, HKV, D)
    g = torch.Generator().manual_seed(77)
    out = []
    for x, lo, hi in ((k, -2, 1), (v, -6, 6)):
        x = x.float() * torch.exp2(torch.randint(lo, hi + 1, (B, MAX_LEN, HKV, 1), generator=g).float())
        code, s = quantize_rows(x.to(torch.bfloat16).view(-1, D))
        deq = dequantize_rows(code, s).view(x.shape)
        dead = ~R.key_mask(lens, MAX_LEN, max_keys)
        code = code.view(x.shape).view(torch.uint8).masked_fill(dead.view(B, MAX_LEN, 1, 1), 0x7f).view(FP8)
        s = s.view(B, MAX_LEN, HKV).masked_fill(dead.view(B, MAX_LEN, 1), float("nan")).transpose(1, 2)
        out += [code.contiguous(), torch.nn.functional.pad(s, (0, -MAX_LEN % 4), value=float("nan")).contiguous(), deq]
    kc, ks, kd, vc, vs, vd = out
    return (q, kc, vc, lens), dict(k_scale=ks, v_scale=vs), R.decode_fp64(q, kd, vd, lens, max_keys, p_bf16=False)


def _run(args, kw, **more):
    return Dc.decode_attention(*(t.to(DEV) for t in args), **{n: t.to(DEV) for n, t in kw.items()}, **more)


@pytest.mark.parametrize("which", sorted(LENS))
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_fp8_attention_inside_the_bound_with_nan_past_the_lengths(D, G, which):
    args, kw, ref = _case(D, G, which)
    o, o2 = _run(args, kw), _run(args, kw)
    got = o.cpu()
    w = R.worst(got, ref)
    print(f"D {D} G {G} lens {LENS[which]}: worst error / bound {w:.3f}")
    assert got.shape == (B, HKV * G, D) and got.dtype == torch.bfloat16 and not torch.isnan(got.float()).any()
    assert w <= 1.0
    assert all(not got[b].any() for b, n in enumerate(LENS[which]) if n == 0)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16))  # the same bits every call


@pytest.mark.parametrize("max_keys", [1, C, C + 1])
def test_fp8_max_keys_clamps(max_keys):
    args, kw, ref = _case(128, 4, "b", max_keys)
    w = R.worst(_run(args, kw, max_keys=max_keys).cpu(), ref)
    print(f"max_keys {max_keys}: worst error / bound {w:.3f}")
    assert w <= 1.0


@pytest.mark.parametrize("bad", ["no_scales", "shape", "dtype", "device", "sdpa"])
def test_fp8_refusals(bad):
    args, kw, _ = _case(64, 1, "a")
    q, kc, vc, lens = (t.to(DEV) for t in args)
    ks, vs = kw["k_scale"].to(DEV), kw["v_scale"].to(DEV)
    kw = dict(k_scale=ks, v_scale=vs)
    kw.update({"no_scales": dict(v_scale=None), "shape": dict(k_scale=ks[:, :, :MAX_LEN - 1].contiguous()),
               "dtype": dict(v_scale=vs.double()), "device": dict(k_scale=ks.cpu()), "sdpa": dict(impl="sdpa")}[bad])
    with pytest.raises(ValueError):
        Dc.decode_attention(q, kc, vc, lens, **kw)


# ------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_fp8_cache_prefill_decode_and_generate_against_the_fp64_forward(name):
    """Tolerance: base8 + 2 base.  base8 is the quantiser alone: the fp32 CPU model through prefill +
    decode_step with an e4m3 cache against the fp64 forward; base, and its factor 2, are the bf16 model
    test's: the uncached bf16 GPU forward against the same fp64 forward."""
    from pytorch_operator_amd.models import llama
    torch.manual_seed(11)
    model = llama.Llama(llama.CONFIGS[name]).eval()
    plens, steps = (130, 128, 7), 8
    prompts, forced, full = R.teacher_forced(plens, steps, model.cfg.vocab_size)
    with torch.no_grad():
        want = R.at_positions(R.llama_fp64(model, full), plens, steps)
        got8 = R.cached_logits(model, prompts, plens, forced, model.new_cache(len(plens), max(plens) + steps, FP8))
        base8 = float((got8.double() - want).abs().max())
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)   # whole tiles: the HIP flash path
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((R.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            cache = model.new_cache(len(plens), max(plens) + steps, FP8)
            got = R.cached_logits(model, prompts, plens, forced, cache)
    assert cache.k.dtype == FP8 and cache.lens.tolist() == [n + steps for n in plens]
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name}: fp32 CPU with an e4m3 cache vs fp64 (base8) {base8:.4e}; uncached bf16 forward vs fp64 (base) "
          f"{base:.4e}; bf16 GPU prefill + decode_step with an e4m3 cache vs fp64 {dev:.4e}")
    assert base > 0 and base8 > 0 and dev <= base8 + 2 * base
    before = dict(llama.Attention.decode_calls)
    run = lambda: model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True, kv_dtype=FP8)  # noqa: E731
    toks, logits = run()
    calls = llama.Attention.decode_calls
    assert calls["hip-fp8"] - before.get("hip-fp8", 0) == 7 * model.cfg.n_layers
    assert calls["hip"] == before.get("hip", 0) and calls["sdpa"] == before.get("sdpa", 0)
    again, logits2 = run()
    assert toks.shape == (3, 8) and torch.equal(toks, again) and torch.equal(logits, logits2)
