"""CPU: the head-dim-64 attention path.  The rounding model of tests/attention_refs.py stays within
every derived bound on every case tests/test_attention_d64_gpu.py runs (so the bounds admit a
correctly rounding D = 64 kernel), the one-hot inputs do concentrate each row on its target key, and
the Python layer knows the second head dim."""
import pytest
import torch

from attention_refs import OUTPUTS, case_id, case_mask, ratios, rounding_model
from attention_d64_cases import ALL_CASES, D64, case_inputs64, case_reference64, onehot_rest


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_rounding_model_within_every_bound_d64(case):
    ref = case_reference64(case)
    assert ref["o"].shape[-1] == D64
    if case.kind == "onehot":
        rest = float(onehot_rest(case).max())
        print(case_id(case), f"one-hot rest {rest:.3g}")
        assert rest <= 1e-3, rest
    rs = ratios(rounding_model(*case_inputs64(case), case.scale, case_mask(case)), ref)
    print(case_id(case), " ".join(f"{n} {rs[n][0]:.3f}" for n in OUTPUTS))
    assert all(rs[n][0] <= 1 for n in OUTPUTS), rs


def test_head_dims():
    from pytorch_operator_amd.ops import attention as A
    assert A.HEAD_DIMS == (64, 128)
    assert A.HEAD_DIM == 128


@pytest.mark.parametrize("causal", [True, False])
def test_cpu_call_at_d64_is_the_reference(causal):
    from pytorch_operator_amd.ops import attention as A
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 128, 4, D64, generator=g).to(torch.bfloat16)
    k = torch.randn(2, 128, 2, D64, generator=g).to(torch.bfloat16)
    v = torch.randn(2, 128, 2, D64, generator=g).to(torch.bfloat16)
    assert not A.hip_supported(q, k, v)  # CPU tensors never take the HIP path
    assert torch.equal(A.flash_attention(q, k, v, causal), A.attention_reference(q, k, v, causal))
    if causal:
        ds = torch.zeros(2, 128, dtype=torch.int32)
        ds[:, 50:] = 50
        assert torch.equal(A.flash_attention(q, k, v, True, doc_start=ds),
                           A.attention_reference(q, k, v, True, doc_start=ds))


def test_llama_mini64_config_and_cpu_step():
    from pytorch_operator_amd.harness.ddp_train import MODELS
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    cfg = CONFIGS["llama-mini64"]
    assert "llama-mini64" in MODELS
    assert (cfg.dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.ffn_hidden, cfg.max_seq_len) == (
        256, 2, 4, 2, 512, 512, 1024)
    assert cfg.head_dim == D64 and CONFIGS["llama3-1b"].head_dim == D64
    torch.manual_seed(0)
    m = Llama(cfg)
    tok = torch.randint(0, cfg.vocab_size, (2, 128))
    loss = m(tok, tok)
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert float(m.layers[0].attention.wqkv.weight.grad.abs().max()) > 0
