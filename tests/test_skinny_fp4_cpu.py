"""ops.skinny.quantize_rows_fp4 / dequantize_rows_fp4 against a brute-force nearest-of-16 in fp64; linear_rows_fp4 on
the CPU is its reference and refuses what is outside the contract; generate's hip-fp4 switch; the snapped model."""
import pytest
import torch
import torch.nn.functional as F

import skinny_fp4_refs as R

MAGS = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


def brute_force(w):
    """(codes [N, K], e [N, K / 32]) in fp64: e the least integer with amax <= 6 * 2^e, found by search; the code
    the nearest of the 16 values to w / 2^e, a tie to the even index, the sign kept, never 0x8."""
    N, K = w.shape
    blk = w.double().reshape(N, K // 32, 32)
    amax = blk.abs().amax(-1)
    es = torch.arange(-125, 126)
    e = es[torch.searchsorted(6 * 2.0 ** es.double(), amax.clamp(max=6 * 2.0 ** 125))]
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    v = blk / 2.0 ** e.double()[..., None]
    d = (v.abs()[..., None] - MAGS).abs()
    near = d == d.amin(-1, keepdim=True)
    idx = (near * (2 - torch.arange(8) % 2)).argmax(-1)          # among the nearest, the even index first
    return (idx + 8 * ((v < 0) & (idx > 0))).reshape(N, K), e


def test_quantize_rows_fp4_is_the_brute_force_and_the_round_trip_is_exact():
    from pytorch_operator_amd.ops.skinny import dequantize_rows_fp4, quantize_rows_fp4
    w = R.inputs(5, 384, 48)[1].clone()
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    grid = torch.cat([torch.tensor([6.0]), mids, -mids, MAGS.float(), -MAGS.float(), torch.tensor([-5.9])])
    w[0, :32] = grid * 2.0 ** 3                       # every tie and every code, amax = 6 * 2^3: the ceil's edge
    w[1, 32:64] = grid * 2.0 ** -9 * (4 / 6)          # amax an exact power of two
    w[2, :32] = torch.nextafter(torch.tensor(6.0), torch.tensor(7.0)) * grid / 6   # just past the edge
    w[3, 64:96] = 0                                   # a zero block
    w[4, :32] = grid * 2.0 ** -130                    # under the clamp: e = -125
    q, scale = quantize_rows_fp4(w)
    assert q.dtype == scale.dtype == torch.uint8 and q.shape == (48, 192) and scale.shape == (48, 12)
    assert q.is_contiguous() and scale.is_contiguous()
    codes, e = brute_force(w)
    assert torch.equal(scale.long() - 127, e) and scale[3, 2] == 127 and scale[0, 0] == 130 and scale[4, 0] == 2
    assert torch.equal((q & 15).long(), codes[:, 0::2]) and torch.equal((q >> 4).long(), codes[:, 1::2])
    assert not bool((codes == 8).any()) and not q[3, 32:48].any()
    want = torch.where(codes >= 8, -MAGS[codes % 8], MAGS[codes % 8]) * (2.0 ** e.double()).repeat_interleave(32, 1)
    deq = dequantize_rows_fp4(q, scale)
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.double(), want)
    assert torch.equal(dequantize_rows_fp4(q, scale, torch.float64), want)
    q2, scale2 = quantize_rows_fp4(deq)               # the snapped weight quantises to itself
    assert torch.equal(dequantize_rows_fp4(q2, scale2), deq)
    minus_zero = torch.full_like(q, 0x88)
    assert not dequantize_rows_fp4(minus_zero, scale, torch.float32).any()
    with pytest.raises(ValueError):
        quantize_rows_fp4(w[:, :48])


@pytest.mark.parametrize("swiglu", [False, True])
def test_linear_rows_fp4_on_the_cpu_is_its_reference_and_refuses(swiglu):
    from pytorch_operator_amd.ops import skinny
    x, _, q, scale = R.inputs(5, 384, 96)
    x3 = x.float().view(1, 5, 384)
    y = skinny.linear_rows_fp4(x3, q, scale, swiglu)
    full = F.linear(x3, skinny.dequantize_rows_fp4(q, scale, torch.float32))
    a, b = full.chunk(2, dim=-1)
    assert y.shape == (1, 5, 48 if swiglu else 96) and torch.equal(y, F.silu(a) * b if swiglu else full)
    assert not skinny.hip_supported_fp4(x, q, scale)
    for xb, qb, sb, t in [(torch.zeros(17, 384), q, scale, 0), (x3, q.float(), scale, 0), (x3, q, scale.float(), 0),
                          (x3, q, scale[:, :11], 0), (x3, q, scale, 3), (x3.clone().requires_grad_(), q, scale, 0),
                          (x3[..., :320], q[:, :160].contiguous(), scale[:, :10].contiguous(), 0),
                          (x3, q[:24], scale[:24], 0), (x3, q.t().contiguous().t(), scale, 0)]:
        with pytest.raises(ValueError):
            skinny.linear_rows_fp4(xb, qb, sb, swiglu, t)


def test_generate_parses_hip_fp4_and_refuses_it_with_fuse_norm():
    from pytorch_operator_amd.harness.generate import parse_args
    argv = ["--model", "llama-mini", "--ckpt-dir", "c", "--prompt", "1,2", "--decode-linear", "hip-fp4"]
    assert parse_args(argv).decode_linear == "hip-fp4"
    with pytest.raises(SystemExit):
        parse_args(argv + ["--decode-fuse-norm"])


def test_fp32_llama_mini_generates_the_tokens_of_the_snapped_weights():
    from pytorch_operator_amd.models.llama import CONFIGS, Llama, TNLinear
    from pytorch_operator_amd.ops.skinny import dequantize_rows_fp4, quantize_rows_fp4
    torch.manual_seed(12)
    model = Llama(CONFIGS["llama-mini"]).eval()
    plain = Llama(CONFIGS["llama-mini"]).eval()
    plain.load_state_dict(model.state_dict())
    keys = list(model.state_dict())
    assert model.quantize_decode_weights(fmt="fp4") == 4 * model.cfg.n_layers + 1 and list(model.state_dict()) == keys
    with pytest.raises(ValueError):
        model.quantize_decode_weights(fmt="fp6")
    with torch.no_grad():
        for m in [m for m in plain.modules() if isinstance(m, TNLinear)] + [plain.output]:
            m.weight.copy_(dequantize_rows_fp4(*quantize_rows_fp4(m.weight), torch.float32))
    wo = model.layers[0].attention.wo
    assert wo.rows_q4.shape == (512, 256) and wo.rows_scale4.shape == (512, 16) and not hasattr(wo, "rows_q")
    assert torch.equal(wo.weight, dequantize_rows_fp4(wo.rows_q4, wo.rows_scale4, torch.float32))
    assert torch.equal(wo.weight, plain.layers[0].attention.wo.weight)
    prompts = torch.randint(1, 512, (2, 9), generator=torch.Generator().manual_seed(3))
    TNLinear.rows_impl = "hip-fp4"
    try:
        got = model.generate(prompts, [9, 5], max_new_tokens=6)
    finally:
        TNLinear.rows_impl = "lib"
    assert torch.equal(got, plain.generate(prompts, [9, 5], max_new_tokens=6))
