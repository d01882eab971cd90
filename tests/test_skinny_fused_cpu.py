"""ops.skinny's fused residual / row-scale wrappers on the CPU (plain PyTorch) against the unfused composition and
the references of tests/skinny_fused_refs.py; their refusals; and the model switch, which a CPU model ignores."""
import pytest
import torch

import decode_refs as D
import skinny_fused_refs as R
from pytorch_operator_amd.ops import skinny as S

FMTS = [("bf16", S.linear_rows, S.linear_rows_add_norm, S.linear_rows_scaled),
        ("e4m3", S.linear_rows_fp8, S.linear_rows_add_norm_fp8, S.linear_rows_scaled_fp8)]


@pytest.mark.parametrize("fmt,plain,add,scaled", FMTS)
@pytest.mark.parametrize("stream", [torch.float32, torch.bfloat16])
def test_cpu_paths_are_the_unfused_composition(fmt, plain, add, scaled, stream):
    M, K, N = 7, 192, 1088
    x, wp, wp64, ep = R.gemm(fmt, M, K, N)
    _, wc, wc64, ec = R.gemm(fmt, M, N, 96, seed=2)
    resid, gamma = R.extras(M, N)
    resid = resid.to(stream)
    h, a, ss = add(x.view(1, M, K), *wp, resid.view(1, M, N), gamma)
    want_h, want_a, ss_ref = R.add_norm_ref(plain(x, *wp), resid, gamma)
    assert h.dtype == stream and ss.shape == (1, M, N // 16)
    assert torch.equal(h[0], want_h) and torch.equal(a[0], want_a) and D.worst(ss[0], ss_ref) <= 1.0
    y = scaled(a[0], *wc, ss[0], R.EPS)
    assert D.worst(y, R.scaled_ref(a[0], wc64, ec, ss[0])) <= 1.0
    assert D.worst(y, R.chain_ref(x, wp64, ep, resid, gamma, wc64, ec)) <= 1.0
    packed = scaled(a, *wc, ss, R.EPS, swiglu=True)
    assert torch.equal(packed[0], S.swiglu_packed_reference(y))


@pytest.mark.parametrize("fmt,plain,add,scaled", FMTS)
def test_cpu_refusals(fmt, plain, add, scaled):
    M, K, N = 16, 64, 32
    x, w = torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(N, K, dtype=torch.bfloat16)
    wa = (w,) if fmt == "bf16" else S.quantize_rows(w)
    resid, gamma, ss = torch.zeros(M, N), torch.ones(N), torch.ones(M, K // 16)
    add(x, *wa, resid, gamma), scaled(x, *wa, ss, 1e-5)
    for xb, rb, gb in [(x, resid.half(), gamma), (x, resid, gamma.double()), (x, resid[:, :16], gamma),
                       (torch.zeros(17, K, dtype=torch.bfloat16), torch.zeros(17, N), gamma),
                       (x.clone().requires_grad_(), resid, gamma)]:
        with pytest.raises(ValueError):
            add(xb, *wa, rb, gb)
    for ab, sb in [(x, ss.double()), (x, ss[:, :3]), (x, torch.ones(M, K // 16 + 1)),
                   (torch.zeros(17, K, dtype=torch.bfloat16), torch.ones(17, K // 16)), (x, ss.clone().requires_grad_())]:
        with pytest.raises(ValueError):
            scaled(ab, *wa, sb, 1e-5)


def test_a_cpu_model_takes_the_existing_path_with_the_switch_on():
    from pytorch_operator_amd.models.llama import CONFIGS, Llama, TNLinear
    torch.manual_seed(3)
    model = Llama(CONFIGS["llama-tiny"]).eval()
    prompts = torch.randint(1, 256, (2, 9))
    want = model.generate(prompts, max_new_tokens=4, return_logits=True)
    before = dict(TNLinear.rows_calls)
    TNLinear.rows_impl, TNLinear.rows_fuse_norm = "hip", True
    try:
        got = model.generate(prompts, max_new_tokens=4, return_logits=True)
    finally:
        TNLinear.rows_impl, TNLinear.rows_fuse_norm = "lib", False
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and dict(TNLinear.rows_calls) == before


def test_generate_parses_decode_fuse_norm():
    from pytorch_operator_amd.harness.generate import parse_args
    base = ["--model", "llama-mini", "--ckpt-dir", "c", "--prompt", "1,2", "--decode-linear", "hip"]
    assert parse_args(base + ["--decode-fuse-norm"]).decode_fuse_norm and not parse_args(base).decode_fuse_norm
