"""The skinny GEMM's bound (tests/skinny_refs.py) admits a correctly rounding implementation and rejects
wrong ones; ops.skinny.linear_rows on the CPU is its reference."""
import pytest
import torch
import torch.nn.functional as F

import skinny_refs as R
from decode_refs import worst

CASES = [(1, 32, 16), (7, 224, 80), (16, 1056, 48), (8, 2048, 272)]


@pytest.mark.parametrize("M,K,N", CASES)
def test_bound_admits_fp32_linear_and_rejects_a_dropped_slice_or_row(M, K, N):
    x, w = R.inputs(M, K, N)
    ref = R.linear_fp64(M, K, N)
    good = F.linear(x.float(), w.float()).to(torch.bfloat16)
    no_slice = F.linear(x.float()[:, :K - 32], w.float()[:, :K - 32]).to(torch.bfloat16)
    no_row = good.clone()
    no_row[M - 1] = 0
    print(f"M {M} K {K} N {N}: fp32 linear {worst(good, ref):.3f}, last slice dropped {worst(no_slice, ref):.1f}, "
          f"last row dropped {worst(no_row, ref):.1f} (error / bound)")
    assert worst(good, ref) <= 1.0
    assert worst(no_slice, ref) > 1.0 and worst(no_row, ref) > 1.0


@pytest.mark.parametrize("swiglu", [False, True])
def test_linear_rows_on_the_cpu_is_its_reference(swiglu):
    from pytorch_operator_amd.ops import skinny
    x, w = R.inputs(7, 224, 80)
    x3 = x.float().view(1, 7, 224)
    y = skinny.linear_rows(x3, w.float(), swiglu)
    assert y.shape == (1, 7, 40 if swiglu else 80)
    assert torch.equal(y, skinny.linear_rows_reference(x3, w.float(), swiglu))
    a, b = F.linear(x3, w.float()).chunk(2, dim=-1)
    assert torch.equal(y, F.silu(a) * b if swiglu else F.linear(x3, w.float()))
    assert skinny.MAX_ROWS == 16 and not skinny.hip_supported(x, w)
    with pytest.raises(ValueError):
        skinny.linear_rows(torch.zeros(17, 224), w.float())
    with pytest.raises(ValueError):
        skinny.linear_rows(x3.requires_grad_(), w.float())
