"""The MXFP4-weight skinny GEMM (csrc/kernels/skinny_gemm_fp4.hip) on the GPU: every byte of codes at every scale,
exactly; inside the derived bound of tests/skinny_fp4_refs.py at the smallest shapes at which its split can go wrong,
for every forced tile count, with NaN after x's rows and a sentinel around y, and the same bits for every tile count
and every call; the fused SwiGLU bit for bit against the two launches; the refusals; and the snapped models with every
decode-step projection on the kernel against their fp64 forward."""
import pytest
import torch

import decode_refs as D
import skinny_fp4_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# K: a lone half step; one step; a step and a half step (three waves idle); 16 waves, 8 steps and a half step
KS = [128, 256, 384, 2048 + 128]
# N: one tile; 3 and 5 tiles, a partial last workgroup at 2 and at 4 tiles per workgroup
NS = [16, 48, 80]


@pytest.fixture(scope="module")
def S():
    from pytorch_operator_amd.ops import _native, skinny
    lib = _native.load()
    assert skinny.MAX_ROWS == 16 and all(int(lib.pto_skinny_fp4_waves(K)) == R.waves(K) for K in KS)
    assert [int(lib.pto_skinny_fp4_tiles(1, N, e)) for N, e in [(16, 0), (8192, 0), (16384, 0), (32, 1)]] == [1, 2, 4, 2]
    return skinny


def bits(t):
    return t.view(torch.int16).cpu()


def test_every_code_byte_at_every_scale_is_widened_exactly(S):
    """One-hot x rows read single weights back: with x[m, offset + m] = 1, y[m, n] = w[n, offset + m].  Row n =
    16 i + rot holds the 256 byte values rotated by 16 rot bytes, so that over rot every byte value visits every one
    of the row's 16 scale blocks, and block k of the row has the scale byte 2 + (i + k) % 251: the 251 i put every
    byte, in every block, under every scale byte in [2, 252], and neighbouring blocks differ.  Equality of values: of
    bits for every nonzero, and a zero code of either sign reads back as zero."""
    N, K, M = 251 * 16, 512, 16
    n = torch.arange(N)[:, None]
    q = ((torch.arange(256)[None, :] + 16 * (n % 16)) % 256).to(torch.uint8)
    scale = (2 + (n // 16 + torch.arange(16)[None, :]) % 251).to(torch.uint8)
    seen = torch.zeros(256, 256, dtype=torch.bool)
    seen[q.flatten().long(), scale.repeat_interleave(16, 1).flatten().long()] = True
    assert bool(seen[:, 2:253].all())
    want = S.dequantize_rows_fp4(q, scale, torch.float64)
    assert bool(want.isfinite().all()) and torch.equal(want.to(torch.bfloat16).double(), want)
    qd, sd = q.to(DEV), scale.to(DEV)
    for offset in range(0, K, M):
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), offset + torch.arange(M)] = 1
        y = S.linear_rows_fp4(x.to(DEV), qd, sd).cpu()
        assert torch.equal(y.double(), want[:, offset:offset + M].t()), offset


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", [1, 5, 16])
def test_inside_the_bound_with_the_same_bits_for_every_tile_count_and_call(S, M, N, K):
    from pytorch_operator_amd.ops import _native
    x, _, q, scale = R.inputs(M, K, N)
    xbuf = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    xbuf[:M] = x.to(DEV)
    q, scale = q.to(DEV), scale.to(DEV)
    auto = S.linear_rows_fp4(xbuf[:M], q, scale)
    worst = D.worst(auto.cpu(), R.linear_fp64(M, K, N))
    print(f"M {M} K {K} N {N}: {R.waves(K)} waves, {R.roundings(K)} roundings, worst error / bound {worst:.3f}")
    assert auto.shape == (M, N) and worst <= 1.0
    assert torch.equal(bits(S.linear_rows_fp4(xbuf[:M], q, scale)), bits(auto))        # two calls
    for tiles in (1, 2, 4):
        ybuf = torch.full((18, N), 1234.0, dtype=torch.bfloat16, device=DEV)
        rc = _native.load().pto_skinny_fp4_gemm(xbuf.data_ptr(), q.data_ptr(), scale.data_ptr(), ybuf.data_ptr(), M, N,
                                                K, 0, tiles, _native.current_stream_ptr())
        assert rc == 0 and torch.equal(bits(ybuf[:M]), bits(auto)), tiles
        assert bool((ybuf[M:] == 1234.0).all())                              # nothing past row M - 1 was written


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("M", [1, 16])
def test_fused_swiglu_is_the_two_launches_bit_for_bit(S, M, N, K):
    from pytorch_operator_amd.ops.llm import swiglu_packed
    x, _, q, scale = (t.to(DEV) for t in R.inputs(M, K, N, seed=1))
    two = swiglu_packed(S.linear_rows_fp4(x, q, scale))
    fused = S.linear_rows_fp4(x.view(1, M, K), q, scale, swiglu=True)
    assert fused.shape == (1, M, N // 2) and two.abs().max() > 0
    for tiles in (1, 2, 4):
        assert torch.equal(bits(S.linear_rows_fp4(x, q, scale, swiglu=True, tiles=tiles)), bits(two)), tiles
    assert torch.equal(bits(fused[0]), bits(two))


def test_refusals(S):
    x = torch.zeros(16, 128, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(32, 64, dtype=torch.uint8, device=DEV)
    s = torch.full((32, 4), 127, dtype=torch.uint8, device=DEV)
    assert not S.linear_rows_fp4(x, q, s).any()
    x17 = torch.zeros(17, 128, dtype=torch.bfloat16, device=DEV)
    odd = torch.zeros(32 * 64 + 16, dtype=torch.uint8, device=DEV)
    bad = [(x17, q, s, False, 0), (x[:, :64], q[:, :32].contiguous(), s[:, :2].contiguous(), False, 0),
           (x, q[:24], s[:24], False, 0), (x, q[:16], s[:16], True, 0), (x.float(), q, s, False, 0),
           (x, q.to(torch.int8), s, False, 0), (x, q, s.float(), False, 0), (x, q.t().contiguous().t(), s, False, 0),
           (x, q, s[:, :3], False, 0), (x, odd[8:8 + 32 * 64].view(32, 64), s, False, 0),
           (x, q, odd[1:1 + 32 * 4].view(32, 4), False, 0), (x.clone().requires_grad_(), q, s, False, 0),
           (x, q, s, False, 3), (x, q.cpu(), s, False, 0)]
    for case in bad:
        assert not S.hip_supported_fp4(*case)
        with pytest.raises(ValueError):
            S.linear_rows_fp4(*case)


@pytest.fixture
def rows_fp4():
    from pytorch_operator_amd.models.llama import TNLinear
    TNLinear.rows_impl = "hip-fp4"
    yield TNLinear
    TNLinear.rows_impl = "lib"


@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_snapped_models_decode_on_the_kernel_against_their_fp64_forward(S, rows_fp4, name):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU forward of the same snapped model from its fp64
    forward, measured here (the bf16 model test's rule)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    to_bf16_matmul_weights(model)
    assert model.quantize_decode_weights(fmt="fp4", snap=True) == 4 * model.cfg.n_layers + 1
    w = model.layers[0].attention.wo
    assert torch.equal(w.weight, S.dequantize_rows_fp4(w.rows_q4, w.rows_scale4))
    plens, steps, L = (130, 128, 7), 8, model.cfg.n_layers
    prompts, forced, full = D.teacher_forced(plens, steps, model.cfg.vocab_size)
    before = dict(rows_fp4.rows_calls)
    with torch.no_grad():
        want = D.at_positions(D.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((D.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            got = D.cached_logits(model, prompts, plens, forced, model.new_cache(len(plens), max(plens) + steps))
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name}: uncached bf16 forward vs fp64 {base:.4e}; prefill + decode_step on the MXFP4 skinny GEMM {dev:.4e}")
    assert base > 0 and dev <= 2 * base
    # wqkv, wo, the fused w13 and w2 per layer and the lm-head per step, and the prefill's lm-head
    assert rows_fp4.rows_calls["hip-fp4"] - before.get("hip-fp4", 0) == steps * (4 * L + 1) + 1
    assert rows_fp4.rows_calls["lib"] == before.get("lib", 0)
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
    assert rows_fp4.rows_calls["hip-fp4"] > before.get("hip-fp4", 0) + steps * (4 * L + 1) + 1
    assert rows_fp4.rows_calls["lib"] == before.get("lib", 0)
