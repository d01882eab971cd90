"""The skinny GEMM (csrc/kernels/skinny_gemm.hip) on the GPU: inside the derived bound of tests/skinny_refs.py
at the smallest shapes at which its work split can go wrong, with NaN after x's rows and a sentinel around y;
the fused SwiGLU bit for bit against the two launches; the refusals; and the bf16 models with every decode-step
projection on the kernel against the fp64 forward."""
import pytest
import torch

import decode_refs as D
import skinny_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (K, N): one MFMA and every wave but one idle; fewer steps than waves; 7 slices, uneven, 5 tiles; 33 slices
# (8 waves, a remainder after the batches, the half step); several workgroups per CU at 16 waves
SHAPES = [(32, 16), (64, 16), (224, 80), (1056, 48), (2048, 272)]


@pytest.fixture(scope="module")
def S():
    from pytorch_operator_amd.ops import _native, skinny
    lib = _native.load()
    assert skinny.MAX_ROWS == 16 and {K: int(lib.pto_skinny_waves(K)) for K, _ in SHAPES} == \
        {32: 4, 64: 4, 224: 4, 1056: 8, 2048: 16} == {K: R.waves(K) for K, _ in SHAPES}   # one case per choice
    return skinny


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("M", [1, 7, 8, 16])
def test_inside_the_bound_with_nan_after_x_and_a_sentinel_around_y(S, M, K, N):
    from pytorch_operator_amd.ops import _native
    x, w = R.inputs(M, K, N)
    xbuf = torch.full((M + 2, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    xbuf[:M] = x.to(DEV)
    ybuf = torch.full((18, N), 1234.0, dtype=torch.bfloat16, device=DEV)
    w = w.to(DEV)
    rc = _native.load().pto_skinny_gemm(xbuf.data_ptr(), w.data_ptr(), ybuf.data_ptr(), M, N, K, 0,
                                        _native.current_stream_ptr())
    got = ybuf[:M].cpu()
    worst = D.worst(got, R.linear_fp64(M, K, N))
    print(f"M {M} K {K} N {N}: {R.waves(K)} waves, worst error / bound {worst:.3f}")
    assert rc == 0 and worst <= 1.0
    assert bool((ybuf[M:] == 1234.0).all())                                  # nothing past row M - 1 was written
    again = S.linear_rows(xbuf[:M], w)                                       # the wrapper, and the same bits again
    assert again.shape == (M, N) and torch.equal(again.view(torch.int16).cpu(), got.view(torch.int16))


@pytest.mark.parametrize("K,F", SHAPES[1:4])
@pytest.mark.parametrize("M", [1, 8, 16])
def test_fused_swiglu_is_the_two_launches_bit_for_bit(S, M, K, F):
    from pytorch_operator_amd.ops.llm import swiglu_packed
    x, w = (t.to(DEV) for t in R.inputs(M, K, 2 * F, seed=1))
    fused = S.linear_rows(x.view(1, M, K), w, swiglu=True)
    two = swiglu_packed(S.linear_rows(x, w))
    assert fused.shape == (1, M, F) and two.abs().max() > 0
    assert torch.equal(fused[0].view(torch.int16), two.view(torch.int16))


def test_refusals(S):
    x, w = (torch.zeros(s, dtype=torch.bfloat16, device=DEV) for s in ((16, 64), (32, 64)))
    S.linear_rows(x, w)
    bad = [(torch.zeros(17, 64, dtype=torch.bfloat16, device=DEV), w), (x, w[:24]), (x[:, :48], w[:, :48].contiguous()),
           (x.float(), w.float()), (x.half(), w.half()), (x, w.float()), (x, w.t().contiguous().t()),
           (x, w.clone().requires_grad_())]
    for xb, wb in bad:
        assert not S.hip_supported(xb, wb) or wb.requires_grad
        with pytest.raises(ValueError):
            S.linear_rows(xb, wb)
    with pytest.raises(ValueError):
        S.linear_rows(x, w[:16], swiglu=True)                                # F = 8: no whole tile per half


@pytest.fixture
def rows_hip():
    from pytorch_operator_amd.models.llama import TNLinear
    TNLinear.rows_impl = "hip"
    yield TNLinear
    TNLinear.rows_impl = "lib"


@pytest.mark.parametrize("name", ["llama-mini", "llama-mini64"])
def test_bf16_models_decode_on_the_kernel_against_the_fp64_forward(S, rows_hip, name):
    """Tolerance: 2 x the deviation of the uncached bf16 GPU forward from the fp64 forward, measured here."""
    from pytorch_operator_amd.models.llama import CONFIGS, Attention, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(11)
    model = Llama(CONFIGS[name]).eval()
    to_bf16_matmul_weights(model)
    plens, steps, L = (130, 128, 7), 8, model.cfg.n_layers
    prompts, forced, full = D.teacher_forced(plens, steps, model.cfg.vocab_size)
    before, attn = dict(rows_hip.rows_calls), dict(Attention.decode_calls)
    with torch.no_grad():
        want = D.at_positions(D.llama_fp64(model, full), plens, steps)
        model.to(DEV)
        padded = torch.nn.functional.pad(full, (0, 256 - full.shape[1])).to(DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            base = float((D.at_positions(model(padded), plens, steps).double().cpu() - want).abs().max())
            got = D.cached_logits(model, prompts, plens, forced, model.new_cache(len(plens), max(plens) + steps))
    dev = float((got.double().cpu() - want).abs().max())
    print(f"{name}: uncached bf16 forward vs fp64 {base:.4e}; prefill + decode_step on the skinny GEMM {dev:.4e}")
    assert base > 0 and dev <= 2 * base
    # wqkv, wo, the fused w13 and w2 per layer and the lm-head per step, and the prefill's lm-head
    assert rows_hip.rows_calls["hip"] - before.get("hip", 0) == steps * (4 * L + 1) + 1
    assert rows_hip.rows_calls["lib"] == before.get("lib", 0)
    assert Attention.decode_calls["hip"] - attn.get("hip", 0) == steps * L
    toks, logits = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    again, logits2 = model.generate(prompts.to(DEV), list(plens), max_new_tokens=8, return_logits=True)
    assert torch.equal(toks, again) and torch.equal(logits, logits2)
    assert rows_hip.rows_calls["lib"] == before.get("lib", 0) and Attention.decode_calls["sdpa"] == attn.get("sdpa", 0)
