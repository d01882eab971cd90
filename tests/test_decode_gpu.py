"""The decode kernels (csrc/kernels/decode_attention.hip) on the GPU: rope_append bit for bit against
rope_qkv with sentinels around every written row, decode_attention inside the derived bound of
tests/decode_refs.py with NaN in every cache row it must not read, and prefill + decode_step +
generate of the bf16 models against an fp64 forward.
"""
import functools

import pytest
import torch

import decode_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = R.CHUNK
MAX_LEN = 3 * C + 1
B, HKV = 4, 2
# every length class: none, one key, around one chunk boundary, past two, the whole cache
LENS = {"a": (0, 1, C - 1, C), "b": (C + 1, 2 * C + 1, MAX_LEN, 1)}


@pytest.fixture(scope="module")
def Dc():
    from pytorch_operator_amd.ops import _native, decode
    assert int(_native.load().pto_decode_chunk()) == C
    return decode


def _lens(n):
    return torch.tensor(n, dtype=torch.int32)


# ------------------------------------------------------------------------------ rope_append
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 1), (8, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_is_rope_qkv_bit_for_bit_and_writes_one_row(Dc, D, hq, hkv, dtype):
    from pytorch_operator_amd.models.llama import rope_tables
    from pytorch_operator_amd.ops.llm import rope_qkv
    Bq, max_len, W = 3, 256, (hq + 2 * hkv) * D
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    g = torch.Generator().manual_seed(D + hq)
    qkv = torch.randn(Bq, W, generator=g).to(dtype).to(DEV)
    cos, sin = rope_tables(D, max_len, 500000.0, DEV)
    pos = (0, 129, 255)
    seq = torch.zeros(1, max_len, W, dtype=dtype, device=DEV)
    seq[0, list(pos)] = qkv
    rq, rk, rv = rope_qkv(seq, cos, sin, hq, hkv)          # token p of one sequence is rotated at p

    def fresh():
        return (torch.full((Bq, max_len, hkv, D), 7.0, dtype=dtype, device=DEV),
                torch.full((Bq, max_len, hkv, D), -3.0, dtype=dtype, device=DEV))

    def expect(rows):
        ek, ev = fresh()
        for b, p in rows:
            ek[b, p], ev[b, p] = rk[0, p], rv[0, p]
        return ek, ev

    kc, vc = fresh()
    q = Dc.rope_append(qkv, cos, sin, kc, vc, _lens(pos).to(DEV), hq, hkv)
    ek, ev = expect(list(enumerate(pos)))
    assert torch.equal(q.view(bits), rq[0, list(pos)].view(bits))
    assert torch.equal(kc.view(bits), ek.view(bits)) and torch.equal(vc.view(bits), ev.view(bits))
    # row 0 past the cache: nothing of it is stored (a missing guard would write batch row 1's row 0)
    kc, vc = fresh()
    q = Dc.rope_append(qkv, cos, sin, kc, vc, _lens((max_len,) + pos[1:]).to(DEV), hq, hkv)
    ek, ev = expect([(1, pos[1]), (2, pos[2])])
    assert torch.equal(kc.view(bits), ek.view(bits)) and torch.equal(vc.view(bits), ev.view(bits))
    assert torch.equal(q[1:].view(bits), rq[0, list(pos[1:])].view(bits)) and not torch.isnan(q[0].float()).any()
    # a negative position likewise
    kc, vc = fresh()
    Dc.rope_append(qkv, cos, sin, kc, vc, _lens((-1,) + pos[1:]).to(DEV), hq, hkv)
    assert torch.equal(kc.view(bits), ek.view(bits)) and torch.equal(vc.view(bits), ev.view(bits))


def test_rope_append_refusals(Dc):
    qkv = torch.zeros(2, 6 * 64, dtype=torch.bfloat16, device=DEV)
    cos = sin = torch.zeros(16, 32, device=DEV)
    kc, vc = (torch.zeros(2, 16, 1, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    pos = torch.zeros(2, dtype=torch.int32, device=DEV)
    ok = dict(qkv=qkv, cos=cos, sin=sin, k_layer=kc, v_layer=vc, pos=pos, hq=4, hkv=1)
    Dc.rope_append(**ok)
    for bad in (dict(pos=pos.long()), dict(pos=pos.cpu()), dict(k_layer=kc.float()), dict(hq=3),
                dict(cos=cos[:, :16]), dict(k_layer=kc[:, :, :, :32]), dict(qkv=qkv.half())):
        with pytest.raises(ValueError):
            Dc.rope_append(**dict(ok, **bad))


# -------------------------------------------------------------------------- decode_attention
@functools.lru_cache(maxsize=None)
def _case(D, G, which, max_keys=None, p_bf16=False):
    """Inputs with NaN in every row that must not be read, and the fp64 reference: computed once."""
    lens = _lens(LENS[which])
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HKV * G, HKV, D)
    kp, vp = R.poison(k, v, lens, max_keys)
    return q, kp, vp, lens, R.decode_fp64(q, kp, vp, lens, max_keys, p_bf16)


def _to(*ts):
    return tuple(t.to(DEV) for t in ts)


@pytest.mark.parametrize("which", sorted(LENS))
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_inside_the_bound_with_nan_past_the_lengths(Dc, D, G, which):
    q, kp, vp, lens, ref = _case(D, G, which)
    q, kp, vp, lens = _to(q, kp, vp, lens)
    o = Dc.decode_attention(q, kp, vp, lens)
    o2 = Dc.decode_attention(q, kp, vp, lens)
    got = o.cpu()
    w = R.worst(got, ref)
    print(f"D {D} G {G} lens {LENS[which]}: worst error / bound {w:.3f}")
    assert got.shape == (B, HKV * G, D) and got.dtype == torch.bfloat16
    assert not torch.isnan(got.float()).any()
    assert w <= 1.0
    for b, n in enumerate(LENS[which]):
        if n == 0:
            assert not got[b].any()
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16))  # the same bits every call


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_finds_a_one_hot_target_at_every_boundary(Dc, D):
    lens = _lens((1, C, C + 1, MAX_LEN))
    q, k, v = R.onehot_inputs(B, MAX_LEN, HKV * 4, HKV, D, tuple(int(n) - 1 for n in lens))
    kp, vp = R.poison(k, v, lens)
    ref = R.decode_fp64(q, kp, vp, lens)
    w = R.worst(Dc.decode_attention(*_to(q, kp, vp, lens)).cpu(), ref)
    print(f"one-hot, last valid key, D {D}: worst error / bound {w:.3f}")
    assert w <= 1.0


def test_long_then_short_lengths_share_the_workspace(Dc):
    """The partials of a call over the whole cache must not reach a later call over one key."""
    D, G = 128, 4
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HKV * G, HKV, D)
    for n in (MAX_LEN, 1, MAX_LEN):
        lens = _lens((n,) * B)
        kp, vp = R.poison(k, v, lens)
        w = R.worst(Dc.decode_attention(*_to(q, kp, vp, lens)).cpu(), R.decode_fp64(q, kp, vp, lens))
        print(f"lens {n}: worst error / bound {w:.3f}")
        assert w <= 1.0


@pytest.mark.parametrize("max_keys", [1, C, C + 1])
def test_max_keys_clamps(Dc, max_keys):
    q, kp, vp, lens, ref = _case(128, 4, "b", max_keys)
    w = R.worst(Dc.decode_attention(*_to(q, kp, vp, lens), max_keys=max_keys).cpu(), ref)
    print(f"max_keys {max_keys}: worst error / bound {w:.3f}")
    assert w <= 1.0


def test_decode_attention_refusals(Dc):
    def mk(Hq, Hkv, D, dtype=torch.bfloat16):
        return (torch.zeros(2, Hq, D, dtype=dtype, device=DEV), torch.zeros(2, 8, Hkv, D, dtype=dtype, device=DEV),
                torch.zeros(2, 8, Hkv, D, dtype=dtype, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV))
    Dc.decode_attention(*mk(4, 1, 64))
    for shape in ((4, 1, 32), (6, 2, 64), (16, 1, 128), (4, 1, 64, torch.float32), (4, 1, 64, torch.float16),
                  (4, 3, 64)):
        with pytest.raises(ValueError):
            Dc.decode_attention(*mk(*shape))
    q, k, v, lens = mk(4, 1, 64)
    for bad in (dict(lens=lens.long()), dict(lens=lens.cpu()), dict(max_keys=9), dict(max_keys=0),
                dict(impl="eager"), dict(v_layer=v[:, :4]), dict(k_layer=k.float())):
        with pytest.raises(ValueError):
            Dc.decode_attention(**dict(dict(q=q, k_layer=k, v_layer=v, lens=lens), **bad))
    # the library path serves what the kernel does not, a q that is a strided view included
    assert Dc.decode_attention(*mk(6, 2, 32, torch.float32), impl="sdpa").shape == (2, 6, 32)
    q, k, v, lens = mk(6, 2, 32, torch.float32)
    wide = torch.zeros(2, 6, 64, device=DEV)
    assert Dc.decode_attention(wide[:, :, :32], k, v, lens, impl="sdpa").shape == (2, 6, 32)


def test_each_stream_has_its_own_partials(Dc):
    q, kp, vp, lens, ref = _case(128, 4, "b")
    q, kp, vp, lens = _to(q, kp, vp, lens)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    n0 = len(Dc._workspace)
    with torch.cuda.stream(side):
        o = Dc.decode_attention(q, kp, vp, lens)
    side.synchronize()
    assert len(Dc._workspace) >= n0 and (torch.device(DEV, torch.cuda.current_device()), side.cuda_stream) in Dc._workspace
    assert R.worst(o.cpu(), ref) <= 1.0


def test_sdpa_path_inside_the_bound(Dc):
    """The library's kernels round P to bf16 for their MFMAs: r = BF16_O in the bound's second term."""
    q, kp, vp, lens, ref = _case(128, 4, "b", None, True)
    got = Dc.decode_attention(*_to(q, kp, vp, lens), impl="sdpa").cpu()
    w = R.worst(got, ref)
    print(f"sdpa: worst error / bound (r = BF16_O) {w:.3f}; against the HIP kernel's bound (r = 0) "
          f"{R.worst(got, _case(128, 4, 'b')[4]):.3f}")
    assert not torch.isnan(got.float()).any() and w <= 1.0
    q, kp, vp, lens, ref = _case(128, 4, "a", None, True)
    got = Dc.decode_attention(*_to(q, kp, vp, lens), impl="sdpa").cpu()
    assert not torch.isnan(got.float()).any() and not got[0].any() and R.worst(got, ref) <= 1.0


# ------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_bf16_prefill_decode_and_generate_against_the_fp64_forward(Dc, name, monkeypatch):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU Llama.forward from the fp64 CPU forward on
    the same sequences and positions, measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    plens, steps = (130, 128, 7), 8
    prompts, forced, full = R.teacher_forced(plens, steps, model.cfg.vocab_size)
    with torch.no_grad():
        want = R.at_positions(R.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)   # whole tiles: the HIP flash path
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((R.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            cache = model.new_cache(len(plens), max(plens) + steps)
            got = R.cached_logits(model, prompts, plens, forced, cache)
    assert cache.k.dtype == torch.bfloat16 and cache.lens.tolist() == [n + steps for n in plens]
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name}: uncached bf16 forward vs fp64 {base:.4e}; prefill + decode_step vs fp64 {dev:.4e}; "
          f"logit scale {float(want.abs().max()):.3f}")
    assert base > 0 and dev <= 2 * base
    from pytorch_operator_amd.models import llama
    calls, real, before = [], llama.rope_tables, dict(llama.Attention.decode_calls)
    monkeypatch.setattr(llama, "rope_tables", lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert toks.shape == (3, 8) and torch.equal(toks, logits.argmax(-1))
    assert calls == [256]                                   # the tables once, the padded prompt's rows included
    assert llama.Attention.decode_calls["hip"] - before.get("hip", 0) == 7 * model.cfg.n_layers
    assert llama.Attention.decode_calls["sdpa"] == before.get("sdpa", 0)   # every decode step ran the HIP kernels
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
