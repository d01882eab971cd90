"""The skinny GEMMs with the residual add and RMSNorm folded in (csrc/kernels/skinny_gemm_fused.hip) on the GPU,
against tests/skinny_fused_refs.py: the residual epilogue's h and a bit for bit and its ss inside the bound, with
NaN after the input rows and sentinels after the output rows; the row-scale epilogue inside its bound, with the
same bits for every tile count and call, and its SwiGLU form bit for bit the two launches; one into the other
against fp64 add + RMSNorm + linear; the refusals; and the models' decode steps with the switch on."""
import pytest
import torch

import decode_refs as D
import skinny_fused_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
TILES = {"bf16": [0], "e4m3": [0, 1, 2, 4]}


@pytest.fixture(scope="module")
def S():
    from pytorch_operator_amd.ops import _native, skinny
    assert int(_native.load().pto_skinny_fused_chains()) == R.CHAINS and skinny.SS_TILE == 16
    return skinny


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def padded(t, fill=float("nan"), rows=2):
    """t on the GPU as the first rows of a buffer whose other rows hold ``fill``."""
    buf = torch.full((t.shape[0] + rows, t.shape[1]), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf


def fn(S, name, fmt):
    return getattr(S, name + ("_fp8" if fmt == "e4m3" else ""))


def forced(fmt, tiles):
    return {"tiles": tiles} if fmt == "e4m3" else {}


@pytest.mark.parametrize("fmt,K,N", R.CASES)
@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("stream", [torch.float32, BF16])
def test_residual_epilogue_bits_of_h_and_a_and_ss_inside_the_bound(S, stream, M, fmt, K, N):
    from pytorch_operator_amd.ops import _native
    x, wargs, _, _ = R.gemm(fmt, M, K, N)
    resid, gamma = R.extras(M, N)
    wargs, gamma = [t.to(DEV) for t in wargs], gamma.to(DEV)
    xbuf, rbuf = padded(x), padded(resid.to(stream))
    d = fn(S, "linear_rows", fmt)(xbuf[:M], *wargs)
    want_h, want_a, ss_ref = R.add_norm_ref(d.cpu(), rbuf[:M].cpu(), gamma.cpu())
    out = [torch.full((18, n), 1234.0, dtype=t, device=DEV) for n, t in ((N, stream), (N, BF16), (N // 16, torch.float32))]
    lib, tail = _native.load(), (M, N, K, int(stream == BF16))
    ptrs = [t.data_ptr() for t in (xbuf, *wargs, rbuf, gamma, *out)]
    if fmt == "bf16":
        rc = lib.pto_skinny_add_norm(*ptrs, *tail, _native.current_stream_ptr())
    else:
        rc = lib.pto_skinny_fp8_add_norm(*ptrs, *tail, 0, _native.current_stream_ptr())
    h, a, ss = (t[:M] for t in out)
    worst = D.worst(ss.cpu(), ss_ref)
    print(f"{fmt} {stream} M {M} K {K} N {N}: ss worst error / bound {worst:.3f}")
    assert rc == 0 and torch.equal(bits(h), bits(want_h)) and torch.equal(bits(a), bits(want_a)) and worst <= 1.0
    assert all(bool((t[M:] == 1234.0).all()) for t in out)                   # nothing past row M - 1 was written
    for tiles in TILES[fmt]:                                                 # the wrapper, and every tile count
        got = fn(S, "linear_rows_add_norm", fmt)(xbuf[:M], *wargs, rbuf[:M], gamma, **forced(fmt, tiles))
        assert all(g.shape == o.shape and torch.equal(bits(g), bits(o)) for g, o in zip(got, (h, a, ss))), tiles


@pytest.mark.parametrize("fmt,K,N", R.CASES)
@pytest.mark.parametrize("M", [1, 7, 16])
def test_row_scale_epilogue_inside_the_bound_with_the_same_bits_for_every_tile_count_and_call(S, M, fmt, K, N):
    a, wargs, w64, e = R.gemm(fmt, M, K, N)
    ss = R.tile_sums(R.extras(M, K, seed=1)[0])
    wargs, abuf, sbuf = [t.to(DEV) for t in wargs], padded(a), padded(ss)
    run = fn(S, "linear_rows_scaled", fmt)
    y = run(abuf[:M], *wargs, sbuf[:M], R.EPS)
    worst = D.worst(y.cpu(), R.scaled_ref(a, w64, e, ss))
    print(f"{fmt} M {M} K {K} N {N}: {K // 16} partials, worst error / bound {worst:.3f}")
    assert y.shape == (M, N) and worst <= 1.0
    for tiles in TILES[fmt]:
        assert torch.equal(bits(run(abuf[:M], *wargs, sbuf[:M], R.EPS, **forced(fmt, tiles))), bits(y)), tiles


@pytest.mark.parametrize("fmt,K,F", [c for c in R.CASES if c[1] in (192, 224, 1088)])
@pytest.mark.parametrize("M", [1, 16])
def test_row_scale_swiglu_is_the_two_launches_bit_for_bit(S, M, fmt, K, F):
    from pytorch_operator_amd.ops.llm import swiglu_packed
    a, wargs, _, _ = R.gemm(fmt, M, K, 2 * F, seed=1)
    ss = R.tile_sums(R.extras(M, K, seed=1)[0]).to(DEV)
    a, wargs = a.to(DEV), [t.to(DEV) for t in wargs]
    run = fn(S, "linear_rows_scaled", fmt)
    two = swiglu_packed(run(a, *wargs, ss, R.EPS))
    assert two.shape == (M, F) and two.abs().max() > 0
    for tiles in TILES[fmt]:
        fused = run(a.view(1, M, K), *wargs, ss.view(1, M, -1), R.EPS, swiglu=True, **forced(fmt, tiles))
        assert torch.equal(bits(fused[0]), bits(two)), tiles


@pytest.mark.parametrize("fmt,stream,K", [("bf16", torch.float32, 224), ("e4m3", BF16, 192)])
def test_residual_into_row_scale_against_fp64_add_norm_linear(S, fmt, stream, K):
    M, N, Nc = 7, 1088, 48
    x, wp, wp64, ep = R.gemm(fmt, M, K, N)
    _, wc, wc64, ec = R.gemm(fmt, M, N, Nc, seed=2)
    resid, gamma = R.extras(M, N)
    resid = resid.to(stream)
    h, a, ss = fn(S, "linear_rows_add_norm", fmt)(x.to(DEV), *[t.to(DEV) for t in wp], resid.to(DEV), gamma.to(DEV))
    y = fn(S, "linear_rows_scaled", fmt)(a, *[t.to(DEV) for t in wc], ss, R.EPS)
    worst = D.worst(y.cpu(), R.chain_ref(x, wp64, ep, resid, gamma, wc64, ec))
    print(f"{fmt} {stream}: chain worst error / bound {worst:.3f}")
    assert h.dtype == stream and worst <= 1.0


def test_refusals(S):
    M, K, N = 16, 64, 32
    x, w = torch.zeros(M, K, dtype=BF16, device=DEV), torch.zeros(N, K, dtype=BF16, device=DEV)
    q, scale = S.quantize_rows(w)
    resid, gamma = torch.zeros(M, N, device=DEV), torch.ones(N, device=DEV)
    ss = torch.ones(M, K // 16, device=DEV)
    x17, r17 = torch.zeros(17, K, dtype=BF16, device=DEV), torch.zeros(17, N, device=DEV)
    wide = torch.zeros(M, 2 * N, device=DEV)
    for add, sc, wa in ((S.linear_rows_add_norm, S.linear_rows_scaled, (w,)),
                        (S.linear_rows_add_norm_fp8, S.linear_rows_scaled_fp8, (q, scale))):
        add(x, *wa, resid, gamma), sc(x, *wa, ss, 1e-5)
        bad_add = [(x.float(), resid, gamma), (x, resid.half(), gamma), (x, resid, gamma.to(BF16)),
                   (x, torch.zeros(M * N + 1, device=DEV)[1:].view(M, N), gamma), (x, wide[:, :N], gamma),
                   (x17, r17, gamma), (x.clone().requires_grad_(), resid, gamma)]
        for xb, rb, gb in bad_add:
            with pytest.raises(ValueError):
                add(xb, *wa, rb, gb)
        bad_sc = [(x.float(), ss), (x, ss.double()), (x, ss[:, :3]), (x, torch.ones(M, K // 16 + 1, device=DEV)),
                  (x17, torch.ones(17, K // 16, device=DEV)), (x.clone().requires_grad_(), ss)]
        for ab, sb in bad_sc:
            with pytest.raises(ValueError):
                sc(ab, *wa, sb, 1e-5)


@pytest.fixture
def fused():
    from pytorch_operator_amd.models.llama import TNLinear
    TNLinear.rows_fuse_norm = True
    yield TNLinear
    TNLinear.rows_impl, TNLinear.rows_fuse_norm = "lib", False


# llama-mini64 is the smallest configuration, and inside the e4m3 kernels' K % 64 == 0 (K = 256 and 512)
@pytest.mark.parametrize("name,impl", [("llama-mini", "hip"), ("llama-mini64", "hip"), ("llama-mini64", "hip-fp8")])
def test_models_decode_with_the_norms_folded_in_against_the_fp64_forward(S, fused, name, impl):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU forward from the fp64 forward, measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    to_bf16_matmul_weights(model)
    if impl == "hip-fp8":
        model.quantize_decode_weights(snap=True)
    fused.rows_impl = impl
    plens, steps, L = (130, 128, 7), 10, model.cfg.n_layers
    prompts, tokens, full = D.teacher_forced(plens, steps, model.cfg.vocab_size)
    before = dict(fused.rows_calls)
    with torch.no_grad():
        want = D.at_positions(D.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        pad = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        with torch.autocast("cuda", dtype=BF16):
            base = float((D.at_positions(model(pad), plens, steps).double().cpu() - want).abs().max())
            cache = model.new_cache(len(plens), max(plens) + steps)
            got = D.cached_logits(model, prompts, plens, tokens[:, :8], cache)          # prefill + 8 decode_steps
            got = torch.cat([got, model.decode_steps(tokens[:, 8:].to(DEV), cache)], dim=1)   # and 2 tokens at once
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name} {impl}: uncached bf16 forward vs fp64 {base:.4e}; decode with the norms folded in {dev:.4e}")
    assert base > 0 and dev <= 2 * base
    delta = {k: fused.rows_calls[k] - before.get(k, 0) for k in fused.rows_calls}
    # 9 steps.  The first block's wqkv is the plain GEMM behind the step's one rms_norm, so of the 2 L + 1
    # projections that consume a norm 2 L are row-scale calls; the prefill's lm-head is one more plain call.
    assert delta[impl + "-scaled"] == 9 * 2 * L and delta[impl + "-add-norm"] == 9 * 2 * L
    assert delta["rms-norm"] == 9 and delta[impl] == 9 + 1 and delta.get("lib", 0) == 0
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
    assert fused.rows_calls["lib"] == before.get("lib", 0) and fused.rows_calls[impl + "-scaled"] > before.get(
        impl + "-scaled", 0) + 9 * 2 * L
