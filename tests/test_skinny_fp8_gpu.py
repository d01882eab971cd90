"""The FP8-weight skinny GEMM (csrc/kernels/skinny_gemm_fp8.hip) on the GPU: inside the derived bound of
tests/skinny_fp8_refs.py at the smallest shapes at which its split can go wrong, for every forced tile count, with
NaN after x's rows and a sentinel around y, and the same bits for every tile count; every e4m3 code at every k
position, exactly; the fused SwiGLU bit for bit against the two launches; the refusals; and the snapped models
with every decode-step projection on the kernel against their fp64 forward."""
import pytest
import torch

import decode_refs as D
import skinny_fp8_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (K, N): the half step alone, every other wave idle; one step; step + half step, 5 tiles (T = 2 and 4 end ragged);
# 8 waves, 9 steps split unevenly, half step; 16 waves, 17 steps, 17 tiles
SHAPES = [(64, 16), (128, 16), (192, 80), (1216, 48), (2176, 272)]


@pytest.fixture(scope="module")
def S():
    from pytorch_operator_amd.ops import _native, skinny
    lib = _native.load()
    assert skinny.MAX_ROWS == 16 and {K: int(lib.pto_skinny_fp8_waves(K)) for K, _ in SHAPES} == \
        {64: 4, 128: 4, 192: 4, 1216: 8, 2176: 16} == {K: R.waves(K) for K, _ in SHAPES}   # one case per choice
    return skinny


def bits(t):
    return t.view(torch.int16).cpu()


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("tiles", [1, 2, 4])
def test_inside_the_bound_for_every_tile_count_with_the_same_bits(S, tiles, M, K, N):
    from pytorch_operator_amd.ops import _native
    x, _, q, scale = R.inputs(M, K, N)
    xbuf = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    xbuf[:M] = x.to(DEV)
    ybuf = torch.full((18, N), 1234.0, dtype=torch.bfloat16, device=DEV)
    q, scale = q.to(DEV), scale.to(DEV)
    rc = _native.load().pto_skinny_fp8_gemm(xbuf.data_ptr(), q.data_ptr(), scale.data_ptr(), ybuf.data_ptr(), M, N, K,
                                            0, tiles, _native.current_stream_ptr())
    got = ybuf[:M].cpu()
    worst = D.worst(got, R.linear_fp64(M, K, N))
    print(f"M {M} K {K} N {N} tiles {tiles}: {R.waves(K)} waves, worst error / bound {worst:.3f}")
    assert rc == 0 and worst <= 1.0
    assert bool((ybuf[M:] == 1234.0).all())                                  # nothing past row M - 1 was written
    one, auto = S.linear_rows_fp8(xbuf[:M], q, scale, tiles=1), S.linear_rows_fp8(xbuf[:M], q, scale)
    assert one.shape == (M, N) and torch.equal(bits(one), bits(got)) and torch.equal(bits(auto), bits(got))


@pytest.mark.parametrize("N,swiglu,want", [(16, 0, 1), (8192, 0, 2), (16384, 0, 4), (32, 1, 2), (16384, 1, 4)])
def test_each_automatic_tile_count_runs_and_gives_the_bits_of_the_smallest(S, N, swiglu, want):
    from pytorch_operator_amd.ops import _native
    M, K = 16, 64
    assert int(_native.load().pto_skinny_fp8_tiles(M, N, swiglu)) == want
    x, _, q, scale = (t.to(DEV) for t in R.inputs(M, K, N))
    auto = S.linear_rows_fp8(x, q, scale, bool(swiglu))
    assert torch.equal(bits(auto), bits(S.linear_rows_fp8(x, q, scale, bool(swiglu), tiles=1)))
    if not swiglu:
        assert D.worst(auto.cpu(), R.linear_fp64(M, K, N)) <= 1.0


def test_every_e4m3_code_at_every_k_position_is_widened_exactly(S):
    """One-hot x rows read single weights back: y[m, n] = scale[n] * q[n, offset + m].  Equality of values: of
    bits for every nonzero, and a -0 code reads back as +0, the sum of -0 and the accumulator's +0."""
    K, N, M = 192, 32, 16
    codes = (torch.arange(N * K, dtype=torch.int32) * 7 % 256).view(N, K)   # 7 is odd: every code, 24 times each
    codes = torch.where(codes % 128 == 127, codes - 126, codes).to(torch.uint8)          # the two NaN codes
    assert len(codes.unique()) == 254
    q = codes.view(torch.float8_e4m3fn)
    scale = 2.0 ** (torch.arange(N) % 7 - 3).float()
    want = (q.float() * scale[:, None]).to(torch.bfloat16)                  # exact
    assert torch.equal(want.float(), q.float() * scale[:, None]) and bool(want.isfinite().all())
    qd, sd = q.to(DEV), scale.to(DEV)
    for offset in range(0, K, 16):
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), offset + torch.arange(M)] = 1
        for tiles in (1, 2):
            y = S.linear_rows_fp8(x.to(DEV), qd, sd, tiles=tiles).cpu()
            assert torch.equal(y.float(), want[:, offset:offset + M].t().float()), (offset, tiles)


@pytest.mark.parametrize("K,F", SHAPES[1:4])
@pytest.mark.parametrize("M", [1, 16])
def test_fused_swiglu_is_the_two_launches_bit_for_bit(S, M, K, F):
    from pytorch_operator_amd.ops.llm import swiglu_packed
    x, _, q, scale = (t.to(DEV) for t in R.inputs(M, K, 2 * F, seed=1))
    fused = S.linear_rows_fp8(x.view(1, M, K), q, scale, swiglu=True)
    two = swiglu_packed(S.linear_rows_fp8(x, q, scale))
    assert fused.shape == (1, M, F) and two.abs().max() > 0
    assert torch.equal(bits(fused[0]), bits(two))
    assert torch.equal(bits(S.linear_rows_fp8(x, q, scale, swiglu=True, tiles=4)), bits(two))


def test_refusals(S):
    x = torch.zeros(16, 64, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(32, 64, device=DEV).to(torch.float8_e4m3fn)
    s = torch.ones(32, device=DEV)
    S.linear_rows_fp8(x, q, s)
    x17, q48 = torch.zeros(17, 64, dtype=torch.bfloat16, device=DEV), q[:, :48].contiguous()
    bad = [(x17, q, s, False, 0), (x[:, :48], q48, s, False, 0), (x, q[:24], s[:24], False, 0),
           (x, q[:16], s[:16], True, 0), (x, q.to(torch.bfloat16), s, False, 0), (x, q, s.half(), False, 0),
           (x, q.t().contiguous().t(), s, False, 0), (x, q, s[:31], False, 0),
           (x.clone().requires_grad_(), q, s, False, 0), (x, q, s, False, 3)]
    for case in bad:
        assert not S.hip_supported_fp8(*case)
        with pytest.raises(ValueError):
            S.linear_rows_fp8(*case)


@pytest.fixture
def rows_fp8():
    from pytorch_operator_amd.models.llama import TNLinear
    TNLinear.rows_impl = "hip-fp8"
    yield TNLinear
    TNLinear.rows_impl = "lib"


@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_snapped_models_decode_on_the_kernel_against_their_fp64_forward(S, rows_fp8, name):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU forward of the same snapped model from its fp64
    forward, measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    to_bf16_matmul_weights(model)
    keys = list(model.state_dict())
    assert model.quantize_decode_weights(snap=True) == 4 * model.cfg.n_layers + 1 and list(model.state_dict()) == keys
    w = model.layers[0].attention.wo
    assert torch.equal(w.weight, S.dequantize_rows(w.rows_q, w.rows_scale))
    plens, steps, L = (130, 128, 7), 8, model.cfg.n_layers
    prompts, forced, full = D.teacher_forced(plens, steps, model.cfg.vocab_size)
    before = dict(rows_fp8.rows_calls)
    with torch.no_grad():
        want = D.at_positions(D.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((D.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            got = D.cached_logits(model, prompts, plens, forced, model.new_cache(len(plens), max(plens) + steps))
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name}: uncached bf16 forward vs fp64 {base:.4e}; prefill + decode_step on the FP8 skinny GEMM {dev:.4e}")
    assert base > 0 and dev <= 2 * base
    # wqkv, wo, the fused w13 and w2 per layer and the lm-head per step, and the prefill's lm-head
    assert rows_fp8.rows_calls["hip-fp8"] - before.get("hip-fp8", 0) == steps * (4 * L + 1) + 1
    assert rows_fp8.rows_calls["lib"] == before.get("lib", 0)
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
    assert rows_fp8.rows_calls["lib"] == before.get("lib", 0)
