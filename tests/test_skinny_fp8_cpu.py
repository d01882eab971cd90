"""ops.skinny.quantize_rows / dequantize_rows; the FP8 skinny GEMM's bound (tests/skinny_fp8_refs.py) admits a
correctly rounding implementation and rejects wrong ones; linear_rows_fp8 on the CPU is its reference."""
import pytest
import torch
import torch.nn.functional as F

import skinny_fp8_refs as R
from decode_refs import worst

CASES = [(1, 64, 16), (7, 192, 80), (16, 1216, 48), (7, 2176, 272)]


def test_quantize_rows_scales_are_powers_of_two_and_the_round_trip_is_exact():
    from pytorch_operator_amd.ops.skinny import dequantize_rows, quantize_rows
    w = R.inputs(7, 192, 80)[1].clone()
    w[5] = 0
    w[6] *= 448 * 2.0 ** -3 / w[6].abs().max()              # amax / 448 an exact power of two: the ceil's edge
    q, scale = quantize_rows(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape and q.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (80,)
    assert torch.equal(torch.frexp(scale)[0], torch.full((80,), 0.5))            # powers of two
    assert scale[5] == 1 and not q[5].float().any() and scale[6] == 2.0 ** -3
    qf = q.float()
    live = torch.arange(80) != 5
    amax = (w.abs().amax(dim=1) / scale)[live]              # the quotient's, in (224, 448]; rounding may give 224
    assert bool((amax > 224).all()) and bool((amax <= 448).all())
    assert bool((qf.abs().amax(dim=1)[live] >= 224).all()) and bool((qf.abs() <= 448).all())
    deq = dequantize_rows(q, scale)
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.float(), qf * scale[:, None])
    err, ratio = (w - qf * scale[:, None]).abs(), w.abs() / scale[:, None]
    normal = ratio >= 2.0 ** -6
    assert bool((err[normal] <= 2.0 ** -4 * w.abs()[normal]).all())
    assert bool((err <= (scale * 2.0 ** -10)[:, None])[~normal].all())


@pytest.mark.parametrize("M,K,N", CASES)
def test_bound_admits_fp32_linear_and_rejects_a_dropped_slice_a_dropped_row_and_rotated_scales(M, K, N):
    x, _, q, scale = R.inputs(M, K, N)
    ref = R.linear_fp64(M, K, N)
    acc = F.linear(x.float(), q.float())
    good = (acc * scale).to(torch.bfloat16)
    no_slice = (F.linear(x.float()[:, :K - 64], q.float()[:, :K - 64]) * scale).to(torch.bfloat16)
    no_row = good.clone()
    no_row[M - 1] = 0
    rotated = (acc * scale.roll(1)).to(torch.bfloat16)
    bad = [worst(t, ref) for t in (no_slice, no_row, rotated)]
    print(f"M {M} K {K} N {N}: fp32 linear {worst(good, ref):.3f}; last slice dropped, last row dropped, scales "
          f"rotated {bad} (error / bound)")
    assert worst(good, ref) <= 1.0 and min(bad) > 1.0


@pytest.mark.parametrize("swiglu", [False, True])
def test_linear_rows_fp8_on_the_cpu_is_its_reference(swiglu):
    from pytorch_operator_amd.ops import skinny
    x, _, q, scale = R.inputs(7, 192, 96)
    x3 = x.float().view(1, 7, 192)
    y = skinny.linear_rows_fp8(x3, q, scale, swiglu)
    full = F.linear(x3, q.float() * scale[:, None])
    a, b = full.chunk(2, dim=-1)
    assert y.shape == (1, 7, 48 if swiglu else 96) and torch.equal(y, F.silu(a) * b if swiglu else full)
    assert not skinny.hip_supported_fp8(x, q, scale)
    for xb, qb, sb, t in [(torch.zeros(17, 192), q, scale, 0), (x3, q.float(), scale, 0), (x3, q, scale.half(), 0),
                          (x3, q, scale[:95], 0), (x3, q, scale, 3), (x3.clone().requires_grad_(), q, scale, 0)]:
        with pytest.raises(ValueError):
            skinny.linear_rows_fp8(xb, qb, sb, swiglu, t)


def test_generate_parses_decode_linear_hip_fp8():
    from pytorch_operator_amd.harness.generate import parse_args
    a = parse_args(["--model", "llama-mini", "--ckpt-dir", "c", "--prompt", "1,2", "--decode-linear", "hip-fp8"])
    assert a.decode_linear == "hip-fp8"
