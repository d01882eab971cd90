"""Decode attention on the CPU: the fp64 reference's bound (tests/decode_refs.py) admits a correctly
rounding implementation and rejects wrong ones; the PyTorch paths of ops/decode.py; prefill +
decode_step of models/llama.py against an fp64 forward; generate's argument checks and
self-consistency.  The HIP kernels are held to the same bound in tests/test_decode_gpu.py.
"""
import math

import pytest
import torch

import decode_refs as R
from pytorch_operator_amd.models.llama import CONFIGS, Llama
from pytorch_operator_amd.ops import decode as Dc
from pytorch_operator_amd.ops.llm import rope_qkv_reference

B, HQ, HKV, D = 4, 4, 2, 128
MAX_LEN = 3 * R.CHUNK + 1


def _lens(*n):
    return torch.tensor(n, dtype=torch.int32)


# ------------------------------------------------------------------------------ the bound
def test_bound_admits_the_fp32_reference_path_from_bf16_inputs():
    lens = _lens(0, 1, R.CHUNK + 1, MAX_LEN)
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HQ, HKV, D)
    kp, vp = R.poison(k, v, lens)
    ref = R.decode_fp64(q, kp, vp, lens)
    got = Dc.decode_attention_reference(q, kp, vp, lens)
    assert got.dtype == torch.bfloat16 and not torch.isnan(got).any()
    w = R.worst(got, ref)
    print("reference path, worst error / bound:", w)
    assert w <= 1.0
    assert not got[0].any()  # lens 0: a zero row
    # and the fp64 result rounded once to bf16: the best any implementation can do
    assert R.worst(R.bf16_round(ref["o"]), ref) <= 1.0


def _onehot(targets, lens):
    q, k, v = R.onehot_inputs(B, MAX_LEN, HQ, HKV, D, tuple(targets))
    return q, k, v, R.decode_fp64(q, k, v, lens)


def test_bound_rejects_a_dropped_last_key():
    lens = _lens(1, R.CHUNK, R.CHUNK + 1, MAX_LEN)
    q, k, v, ref = _onehot([int(n) - 1 for n in lens], lens)       # every row looks at its last valid key
    assert R.worst(R.bf16_round(ref["o"]), ref) <= 1.0
    wrong = R.attend_fp64(q, k, v, R.key_mask(lens - 1, MAX_LEN))["o"]
    w = R.worst(R.bf16_round(wrong), ref)
    print("last key dropped, worst error / bound:", w)
    assert w > 10.0


def test_bound_rejects_a_stale_key():
    lens = _lens(1, R.CHUNK - 1, R.CHUNK, 2 * R.CHUNK + 1)
    q, k, v, ref = _onehot([int(n) for n in lens], lens)           # the first row past the valid ones
    wrong = R.attend_fp64(q, k, v, R.key_mask(lens + 1, MAX_LEN))["o"]
    w = R.worst(R.bf16_round(wrong), ref)
    print("one stale key included, worst error / bound:", w)
    assert w > 10.0


def test_bound_rejects_a_dropped_chunk():
    lens = _lens(MAX_LEN, MAX_LEN, MAX_LEN, MAX_LEN)
    q, k, v, ref = _onehot([0, R.CHUNK, 2 * R.CHUNK + 7, 3 * R.CHUNK], lens)   # a target in every chunk
    for c in range(4):
        mask = ref["mask"].clone()
        mask[:, c * R.CHUNK:(c + 1) * R.CHUNK] = False
        wrong = R.attend_fp64(q, k, v, mask)["o"]
        w = R.worst(R.bf16_round(wrong[c:c + 1]), {n: t[c:c + 1] for n, t in ref.items()})
        print(f"chunk {c} dropped, worst error / bound in the row that looks at it:", w)
        assert w > 10.0


def test_bound_rejects_the_scale_one_over_d():
    lens = _lens(2, R.CHUNK, R.CHUNK + 1, MAX_LEN)
    q, k, v, ref = _onehot([0, 5, R.CHUNK, MAX_LEN - 1], lens)
    wrong = R.attend_fp64(q, k, v, ref["mask"], scale=1.0 / D)["o"]
    w = R.worst(R.bf16_round(wrong), ref)
    print("scale 1/D, worst error / bound:", w)
    assert w > 10.0
    # on gaussian inputs as well
    lens = _lens(2, R.CHUNK, R.CHUNK + 1, MAX_LEN)
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HQ, HKV, D)
    ref = R.decode_fp64(q, k, v, lens)
    assert R.worst(R.bf16_round(R.attend_fp64(q, k, v, ref["mask"], scale=1.0 / D)["o"]), ref) > 10.0


def test_max_keys_clamps_the_reference_path():
    lens = _lens(0, 5, 300, MAX_LEN)
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HQ, HKV, D)
    kp, vp = R.poison(k, v, lens, max_keys=257)
    ref = R.decode_fp64(q, kp, vp, lens, max_keys=257)
    assert R.worst(Dc.decode_attention(q, kp, vp, lens, max_keys=257), ref) <= 1.0
    assert R.worst(Dc.decode_attention(q, k, v, lens), ref) > 10.0   # rows 257.. do matter


# ------------------------------------------------------------------------ the other wrappers
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_append_reference_equals_rope_qkv_reference(dtype):
    from pytorch_operator_amd.models.llama import rope_tables
    Bq, hq, hkv, Dh, max_len = 3, 4, 2, 64, 32
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(Bq, (hq + 2 * hkv) * Dh, generator=g).to(dtype)
    cos, sin = rope_tables(Dh, max_len, 500000.0)
    pos = torch.tensor([0, 17, 31], dtype=torch.int32)
    kc = torch.full((Bq, max_len, hkv, Dh), 7.0, dtype=dtype)
    vc = torch.full_like(kc, 7.0)
    q = Dc.rope_append(qkv, cos, sin, kc, vc, pos, hq, hkv)
    for b, p in enumerate(pos.tolist()):
        # the packed row as token p of a sequence of max_len: rope_qkv_reference rotates it at position p
        seq = torch.zeros(1, max_len, qkv.shape[1], dtype=dtype)
        seq[0, p] = qkv[b]
        rq, rk, rv = rope_qkv_reference(seq, cos, sin, hq, hkv)
        assert torch.equal(q[b], rq[0, p]) and torch.equal(kc[b, p], rk[0, p]) and torch.equal(vc[b, p], rv[0, p])
        others = torch.arange(max_len) != p
        assert (kc[b, others] == 7.0).all() and (vc[b, others] == 7.0).all()
    # a position outside the cache stores nothing
    kc2, vc2 = torch.full_like(kc, 7.0), torch.full_like(vc, 7.0)
    Dc.rope_append(qkv, cos, sin, kc2, vc2, torch.tensor([max_len, -1, 5], dtype=torch.int32), hq, hkv)
    assert (kc2[:2] == 7.0).all() and (vc2[:2] == 7.0).all() and not (kc2[2, 5] == 7.0).all()


def test_kvcache_shapes():
    c = Dc.KVCache(3, 2, 40, 4, 64, torch.bfloat16, "cpu")
    assert c.k.shape == c.v.shape == (3, 2, 40, 4, 64) and c.k.dtype == torch.bfloat16
    assert c.lens.shape == (2,) and c.lens.dtype == torch.int32 and not c.lens.any()
    k0, v0 = c.layer(1)
    assert k0.shape == (2, 40, 4, 64) and k0.is_contiguous() and k0.data_ptr() == c.k[1].data_ptr()
    with pytest.raises(ValueError):
        Dc.KVCache(0, 2, 40, 4, 64)


def test_wrapper_refusals():
    q, k, v = R.gaussian_inputs(B, MAX_LEN, HQ, HKV, D)
    lens = _lens(1, 1, 1, 1)
    for bad in (dict(lens=lens.long()), dict(lens=lens[:3]), dict(max_keys=0), dict(max_keys=MAX_LEN + 1),
                dict(impl="flash"), dict(q=q.float()), dict(q=q[:, :3]), dict(v_layer=v[:, :5])):
        kw = dict(q=q, k_layer=k, v_layer=v, lens=lens, max_keys=None, impl="auto")
        kw.update(bad)
        with pytest.raises(ValueError):
            Dc.decode_attention(**kw)


# ------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(3)
    return Llama(CONFIGS["llama-tiny"]).eval()


def test_prefill_and_decode_steps_match_the_fp64_forward(tiny):
    """Tolerance: 4 x the largest deviation of the uncached fp32 Llama.forward from the fp64 forward on
    the same sequences and positions -- a quantity of the reference alone; the factor covers the other
    summation order of the S = 1 matmuls."""
    plens, steps = (5, 16, 1), 12
    prompts, forced, full = R.teacher_forced(plens, steps, tiny.cfg.vocab_size)
    with torch.no_grad():
        want = R.at_positions(R.llama_fp64(tiny, full), plens, steps)
        base = float((R.at_positions(tiny(full), plens, steps).double() - want).abs().max())
        cache = tiny.new_cache(len(plens), max(plens) + steps)
        got = R.cached_logits(tiny, prompts, plens, forced, cache)
    dev = float((got.double() - want).abs().max())
    print(f"uncached fp32 forward vs fp64: {base:.3e}; prefill + decode_step vs fp64: {dev:.3e}; "
          f"logit scale {float(want.abs().max()):.3f}")
    assert cache.lens.tolist() == [n + steps for n in plens]
    assert base > 0 and dev <= 4 * base


def test_generate_refusals(tiny):
    p = torch.ones(2, 4, dtype=torch.long)
    for kw in (dict(max_new_tokens=0), dict(temperature=-1.0), dict(top_k=-1), dict(top_k=10 ** 6),
               dict(eos_id=tiny.cfg.vocab_size), dict(max_new_tokens=tiny.cfg.max_seq_len),
               dict(max_len=5, max_new_tokens=4), dict(max_len=tiny.cfg.max_seq_len + 1),
               dict(prompt_lens=[0, 4]), dict(prompt_lens=[5, 4]), dict(prompt_lens=[4])):
        with pytest.raises(ValueError):
            tiny.generate(p, **kw)
    for bad in (p.int(), p[0], p.new_full((2, 4), tiny.cfg.vocab_size), -p):
        with pytest.raises(ValueError):
            tiny.generate(bad, max_new_tokens=2)


def test_generate_greedy_is_the_argmax_of_its_own_logits_and_stays_on_eos(tiny):
    prompts, _, _ = R.teacher_forced((5, 16, 1), 1, tiny.cfg.vocab_size, seed=1)
    tiny.train()
    toks, logits = tiny.generate(prompts, [5, 16, 1], max_new_tokens=10, return_logits=True)
    assert tiny.training  # the mode is restored
    tiny.eval()
    assert toks.shape == (3, 10) and toks.dtype == torch.long and logits.shape == (3, 10, tiny.cfg.vocab_size)
    assert torch.equal(toks, logits.argmax(-1))
    assert torch.equal(toks, tiny.generate(prompts, [5, 16, 1], max_new_tokens=10))
    # declare row 1's third token the end of text: it repeats from there, the other rows as far as
    # they do not emit it themselves
    eos = int(toks[1, 2])
    t2 = tiny.generate(prompts, [5, 16, 1], max_new_tokens=10, eos_id=eos)
    assert (t2[1, 2:] == eos).all() and torch.equal(t2[1, :2], toks[1, :2])
    for b in range(3):
        hit = (t2[b] == eos).nonzero()
        if len(hit):
            assert (t2[b, int(hit[0]):] == eos).all()


def test_generate_sampling_repeats_with_a_seeded_generator(tiny):
    prompts, _, _ = R.teacher_forced((5, 16, 1), 1, tiny.cfg.vocab_size, seed=2)
    run = lambda seed: tiny.generate(prompts, [5, 16, 1], max_new_tokens=12, temperature=0.9, top_k=20,  # noqa: E731
                                     generator=torch.Generator().manual_seed(seed))
    a, b, c = run(7), run(7), run(8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < tiny.cfg.vocab_size
    # top_k = 1 is greedy whatever the temperature
    assert torch.equal(tiny.generate(prompts, [5, 16, 1], max_new_tokens=6, temperature=2.0, top_k=1,
                                     generator=torch.Generator().manual_seed(1)),
                       tiny.generate(prompts, [5, 16, 1], max_new_tokens=6))


def test_generate_builds_the_rope_tables_once_and_counts_its_decode_steps(tiny, monkeypatch):
    from pytorch_operator_amd.models import llama
    calls = []
    real = llama.rope_tables
    monkeypatch.setattr(llama, "rope_tables", lambda *a, **k: calls.append(a[1]) or real(*a, **k))
    before = llama.Attention.decode_calls["cpu"]
    tiny.generate(torch.ones(2, 16, dtype=torch.long), max_new_tokens=8)
    assert calls == [24]
    assert llama.Attention.decode_calls["cpu"] - before == 7 * tiny.cfg.n_layers   # the first token is the prefill's
    # on a GPU with the HIP attention on, a prompt runs at whole 128-token tiles: the tables cover them
    mini = Llama(CONFIGS["llama-mini64"])
    assert mini._prefill_len(16, torch.device("cuda")) == 128 and mini._prefill_len(128, torch.device("cuda")) == 128
    assert mini._prefill_len(129, torch.device("cuda")) == 256 and mini._prefill_len(16, torch.device("cpu")) == 16
    assert tiny._prefill_len(16, torch.device("cuda")) == 16                        # head dim 16: the library path
