"""Document-masked attention for packed sequences, the parts that need no GPU: the doc_start
helpers, the fp32 masked reference and the Llama model against running each document on its own,
the worker's --doc-len-mean option, and the register budget of the three HIP kernels
(the attn_doc_* kernels of csrc/kernels/attention.hip) in the built library."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "pytorch_operator_amd" / "_lib" / "libpto_hip.so"
EOS = 9


def _starts_by_hand(row):
    out, cur = [], 0
    for i in range(len(row)):
        if i > 0 and row[i - 1] == EOS:
            cur = i
        out.append(cur)
    return out


def _ends_by_hand(starts):
    S = len(starts)
    return [next((j for j in range(i + 1, S) if starts[j] == j), S) for i in range(S)]


@pytest.mark.parametrize("row,want", [
    ([EOS, 1, 2, 3, 4, 5], [0, 1, 1, 1, 1, 1]),        # EOS at position 0: a one-token document
    ([1, 2, 3, 4, 5, EOS], [0, 0, 0, 0, 0, 0]),        # EOS at the last position closes the only document
    ([1, 2, EOS, EOS, 3, 4], [0, 0, 0, 3, 4, 4]),      # adjacent EOS: a one-token document
    ([1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0]),          # no EOS
])
def test_doc_start_helpers_on_hand_written_rows(row, want):
    from pytorch_operator_amd.ops.attention import doc_ends, doc_starts_from_tokens, validate_doc_start
    assert _starts_by_hand(row) == want
    ds = doc_starts_from_tokens(torch.tensor([row, row]), EOS)
    assert ds.dtype == torch.int32 and ds.shape == (2, len(row))
    assert ds[0].tolist() == want and ds[1].tolist() == want
    de = doc_ends(ds)
    assert de.dtype == torch.int32 and de[0].tolist() == _ends_by_hand(want)
    assert doc_ends(ds.long())[1].tolist() == _ends_by_hand(want)
    validate_doc_start(ds)
    validate_doc_start(ds.long())


def test_doc_helpers_differ_per_batch_row():
    from pytorch_operator_amd.ops.attention import doc_ends, doc_starts_from_tokens
    rows = [[1, EOS, 2, 3, EOS, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7, 8]]
    ds = doc_starts_from_tokens(torch.tensor(rows), EOS)
    assert ds.tolist() == [[0, 0, 2, 2, 2, 5, 5, 5], [0] * 8]
    assert doc_ends(ds).tolist() == [[2, 2, 5, 5, 5, 8, 8, 8], [8] * 8]


@pytest.mark.parametrize("bad", [
    [0, 0, 2, 1, 1],   # decreasing
    [0, 2, 2, 2, 2],   # a start greater than its index
    [0, 0, 1, 1, 1],   # neither the previous value nor its own index
    [1, 1, 1, 1, 1],   # the first token starts no document
])
def test_validate_doc_start_rejects(bad):
    from pytorch_operator_amd.ops.attention import validate_doc_start
    with pytest.raises(ValueError):
        validate_doc_start(torch.tensor([[0, 0, 0, 0, 0], bad], dtype=torch.int32))
    with pytest.raises(ValueError):
        validate_doc_start(torch.tensor([bad]).float())


DOC_LENS = (1, 17, 30, 16)  # one sequence of 64 tokens


def _doc_start_of(lens, device="cpu"):
    starts = []
    for n in lens:
        starts += [len(starts)] * n
    return torch.tensor([starts], dtype=torch.int32, device=device)


def test_llama_packed_forward_equals_documents_run_separately():
    """llama-tiny in fp32: the packed sequence with doc_start gives the logits of the four
    documents run on their own (RoPE is relative, so their positions need not restart).  Measured
    with a dense-mask prototype: 1.8e-7 with the mask, 0.30 without it."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-tiny"]).eval()
    tok = torch.randint(0, CONFIGS["llama-tiny"].vocab_size, (1, sum(DOC_LENS)))
    with torch.no_grad():
        packed = m(tok, doc_start=_doc_start_of(DOC_LENS))
        parts, at = [], 0
        for n in DOC_LENS:
            parts.append(m(tok[:, at:at + n]))
            at += n
        unmasked = m(tok)
    alone = torch.cat(parts, dim=1)
    err = float((packed - alone).abs().max())
    print("packed vs separate:", err, "unmasked vs separate:", float((unmasked - alone).abs().max()))
    assert torch.allclose(packed, alone, atol=1e-5, rtol=0), err
    assert float((unmasked - alone).abs().max()) > 1e-2  # the mask is what makes them equal


def test_llama_doc_start_through_grad_checkpoint():
    """--grad-checkpoint threads doc_start through torch.utils.checkpoint: same loss and gradients."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    tok = torch.randint(0, 256, (2, 64), generator=torch.Generator().manual_seed(1))
    ds = _doc_start_of(DOC_LENS).expand(2, -1).contiguous()
    out = []
    for ck in (False, True):
        torch.manual_seed(0)
        m = Llama(CONFIGS["llama-tiny"], checkpoint_layers=ck).train()
        loss = m(tok, tok, doc_start=ds)
        loss.backward()
        out.append((float(loss.detach()), m.layers[0].attention.wqkv.weight.grad.clone()))
    assert out[0][0] == pytest.approx(out[1][0], rel=1e-6)
    assert torch.allclose(out[0][1], out[1][1], atol=1e-6)


def test_reference_with_doc_start_equals_per_document_reference():
    """Output and the three gradients.  Both sides are fp32 sums of at most 64 O(1) terms (masked
    keys add exact zeros), so they differ by a few fp32 roundings (1.2e-7 each): 1e-5 absolute."""
    from pytorch_operator_amd.ops.attention import attention_reference
    g = torch.Generator().manual_seed(2)
    B, S, Hq, Hkv, D = 1, sum(DOC_LENS), 4, 2, 16
    q, k, v = (torch.randn(B, S, H, D, generator=g) for H in (Hq, Hkv, Hkv))
    do = torch.randn(B, S, Hq, D, generator=g)

    def run(fn):
        xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = fn(*xs)
        o.backward(do)
        return [o.detach()] + [x.grad for x in xs]

    def per_doc(a, b, c):
        outs, at = [], 0
        for n in DOC_LENS:
            outs.append(attention_reference(a[:, at:at + n], b[:, at:at + n], c[:, at:at + n], True))
            at += n
        return torch.cat(outs, dim=1)

    ds = _doc_start_of(DOC_LENS)
    masked = run(lambda a, b, c: attention_reference(a, b, c, True, doc_start=ds))
    alone = run(per_doc)
    for name, x, y in zip(("o", "dq", "dk", "dv"), masked, alone):
        assert torch.allclose(x, y, atol=1e-5, rtol=0), (name, float((x - y).abs().max()))
    # the library path with the dense mask, and the log-sum-exp of the masked rows
    from pytorch_operator_amd.ops.attention import sdpa_bshd
    assert torch.allclose(sdpa_bshd(q, k, v, True, doc_start=ds), alone[0], atol=1e-5, rtol=0)
    _, lse = attention_reference(q, k, v, True, return_lse=True, doc_start=ds)
    assert torch.isfinite(lse).all()
    assert float(lse[0, 0, 0]) == pytest.approx(float((q[0, 0, 0] @ k[0, 0, 0]) / math.sqrt(D)), abs=1e-5)


def test_doc_start_argument_errors_on_cpu():
    from pytorch_operator_amd.ops.attention import attention_reference, flash_attention, sdpa_bshd
    q = torch.zeros(1, 8, 2, 16)
    ds = torch.zeros(1, 8, dtype=torch.int32)
    for fn in (flash_attention, attention_reference, sdpa_bshd):
        with pytest.raises(ValueError):
            fn(q, q, q, causal=False, doc_start=ds)
        with pytest.raises(ValueError):
            fn(q, q, q, causal=True, doc_start=ds[:, :4])
        with pytest.raises(ValueError):
            fn(q, q, q, causal=True, doc_start=ds.float())


def _worker(extra):
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="1", WORLD_SIZE="1", RANK="0")
    cmd = [sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", "--model", "llama-tiny", "--no-cuda",
           "--seq-len", "64", "--batch-size", "2", "--steps", "2", "--warmup", "1", *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads([x for x in p.stdout.splitlines() if x.startswith('{"metric"')][-1])


def test_worker_doc_len_mean_option():
    plain = _worker([])
    docs = _worker(["--doc-len-mean", "8"])
    assert docs["attn_mask"] == "document" and docs["doc_len_mean"] == 8
    assert docs["docs_per_seq"] > 1.0 and math.isfinite(docs["loss"])
    assert set(docs) - set(plain) == {"doc_len_mean", "docs_per_seq", "attn_mask"}
    assert not {"doc_len_mean", "docs_per_seq", "attn_mask"} & set(plain)
    # the keys of the result line before the option existed
    assert list(plain) == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "data",
                           "params", "per_rank_batch", "seq_len", "loss", "tflops_per_gpu", "max_mem_gb",
                           "parallelism", "bucket_mb", "allreduce_dtype", "master_weights", "zero", "gemm_tuning",
                           "attn", "residual_norm", "linear_bwd", "opt_overlap"]


def test_doc_kernels_have_no_spills():
    if not LIB.exists():
        pytest.skip("libpto_hip.so not built")
    sys.path.insert(0, str(ROOT / "tools"))
    import isa_dump
    res = isa_dump.kernel_resources(LIB)
    for name, max_wg in (("attn_doc_fwd_kernel", 256), ("attn_doc_dq_kernel", 256), ("attn_doc_dkdv_kernel", 256)):
        hits = [k for k in res if name in k]
        assert len(hits) == 1, (name, hits)
        assert res[hits[0]]["spills"] == 0 and res[hits[0]]["max_wg"] == max_wg, (name, res[hits[0]])
