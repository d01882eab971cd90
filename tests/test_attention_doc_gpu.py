"""The document-masked HIP flash attention (the attn_doc_* kernels of csrc/kernels/attention.hip)
on the GPU: numerics
against the fp32 masked reference with the dense-mask SDPA's own bf16 error as the yardstick
(test_attention_gpu.py's), bit-identity with the plain 4-wave passes when there is one document,
bit-for-bit independence of the documents, and the Llama model's dispatch."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # B, S, Hq, Hkv: one block and several, GQA groups 1 / 4 / 4, more than one dK/dV key block
    (1, 128, 2, 2),
    (2, 256, 8, 2),
    (1, 384, 4, 1),
]
# boundaries inside a 32-row wave, on and beside 32- / 64- / 128-multiples, a one-token first
# document.  Rows 64.. of block 0 and rows 200.. of block 1 start after their block's first
# processed key tile: the rows whose first tiles are wholly masked (the NaN hazard).
DENSE = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
CASES = [(s, lay) for s in SHAPES for lay in ("dense", "last")] + [((2, 256, 8, 2), "mixed")]


def _row(bounds, S):
    out, cur, bs = [], 0, {b for b in bounds if 0 < b < S}
    for i in range(S):
        if i in bs:
            cur = i
        out.append(cur)
    return out


def _doc_start(shape, layout):
    B, S = shape[0], shape[1]
    rows = {"dense": [_row(DENSE, S)] * B, "last": [_row((S - 1,), S)] * B,
            "mixed": [_row(DENSE, S)] + [_row((), S)] * (B - 1)}[layout]
    return torch.tensor(rows, dtype=torch.int32, device="cuda")


def _inputs(B, S, Hq, Hkv, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda H: torch.randn(B, S, H, 128, device="cuda", generator=g).to(torch.bfloat16)  # noqa: E731
    return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


def _grads(fn, do, *xs):
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    out = fn(*xs)
    out.backward(do.to(out.dtype))
    return [out.detach()] + [x.grad for x in xs]


def _doc_fwd(q, k, v, ds):
    from pytorch_operator_amd.ops import _native
    B, S, Hq, _ = q.shape
    o = torch.empty_like(q)
    lse2 = torch.empty(B, Hq, S, device="cuda")
    _native.check(_native.load().pto_attn_doc_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                                  lse2.data_ptr(), ds.data_ptr(), B, S, Hq, k.shape[2], 128,
                                                  1 / math.sqrt(128), torch.cuda.current_stream().cuda_stream),
                  "attn_doc_fwd")
    torch.cuda.synchronize()
    return o, lse2


_REF = {}


def _reference(shape, layout):
    """fp32 masked reference (o, lse, dq, dk, dv) and the dense-mask SDPA's (o, dq, dk, dv), computed
    once per case and shared, unchanged, by the tests below."""
    if (shape, layout) not in _REF:
        from pytorch_operator_amd.ops.attention import attention_reference, sdpa_bshd
        q, k, v, do = _inputs(*shape)
        ds = _doc_start(shape, layout)
        ref = _grads(lambda a, b, c: attention_reference(a, b, c, True, doc_start=ds).float(), do, q.float(),
                     k.float(), v.float())
        _, lse = attention_reference(q.float(), k.float(), v.float(), True, return_lse=True, doc_start=ds)
        lib = _grads(lambda a, b, c: sdpa_bshd(a, b, c, True, doc_start=ds), do, q, k, v)
        _REF[(shape, layout)] = (ref, lse, lib)
    return _REF[(shape, layout)]


@pytest.mark.parametrize("shape,layout", CASES)
def test_doc_forward_matches_fp32_masked_reference(shape, layout):
    q, k, v, _ = _inputs(*shape)
    ds = _doc_start(shape, layout)
    ref, lse, lib = _reference(shape, layout)
    o, lse2 = _doc_fwd(q, k, v, ds)
    err, el = _rel(o, ref[0]), _rel(lib[0], ref[0])
    print(shape, layout, "o", err, "sdpa", el, "lse2 max abs",
          float((lse2 - lse * math.log2(math.e)).abs().max()))
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse2).all()
    assert err < max(2.0 * el, 4e-3), (err, el)
    assert torch.allclose(lse2, lse * math.log2(math.e), atol=2e-3, rtol=1e-4)  # log2 units


@pytest.mark.parametrize("shape,layout", CASES)
def test_doc_backward_matches_fp32_masked_reference(shape, layout):
    from pytorch_operator_amd.ops.attention import flash_attention
    q, k, v, do = _inputs(*shape)
    ds = _doc_start(shape, layout)
    ref, _, lib = _reference(shape, layout)
    ours = _grads(lambda a, b, c: flash_attention(a, b, c, True, doc_start=ds), do, q, k, v)
    for name, a, r, lb in zip(("o", "dq", "dk", "dv"), ours, ref, lib):
        e, el = _rel(a, r), _rel(lb, r)
        print(shape, layout, name, e, "sdpa", el)
        assert torch.isfinite(a.float()).all(), name
        assert e < max(2.0 * el, 4e-3 if name == "o" else 6e-3), (name, e, el)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_document_is_bit_identical_to_the_plain_passes(shape, dtype):
    """doc_start all zeros: the same operations in the same order as forward 4, dQ 4 and dK/dV 1
    (dQ and dK/dV: the same templated bodies; the forward: a sibling kernel whose text must follow
    the plain forward's), only the bounds and the forward's operand schedule differ."""
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.attention import flash_attention
    lib = _native.load()
    q, k, v, do = _inputs(*shape, seed=3)
    B, S, Hq, Hkv = shape
    ds = torch.zeros(B, S, dtype=dtype, device="cuda")
    old = lib.pto_attn_set_variant(4), lib.pto_attn_set_dq_variant(4), lib.pto_attn_set_dkdv_variant(1)
    try:
        o = torch.empty_like(q)
        lse2 = torch.empty(B, Hq, S, device="cuda")
        _native.check(lib.pto_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse2.data_ptr(), B, S,
                                       Hq, Hkv, 128, 1 / math.sqrt(128), 1,
                                       torch.cuda.current_stream().cuda_stream), "attn_fwd")
        plain = _grads(lambda a, b, c: flash_attention(a, b, c, True), do, q, k, v)
        torch.cuda.synchronize()
    finally:
        lib.pto_attn_set_variant(old[0])
        lib.pto_attn_set_dq_variant(old[1])
        lib.pto_attn_set_dkdv_variant(old[2])
    o_d, lse2_d = _doc_fwd(q, k, v, ds.to(torch.int32))
    docs = _grads(lambda a, b, c: flash_attention(a, b, c, True, doc_start=ds), do, q, k, v)
    assert torch.equal(o_d, o) and torch.equal(lse2_d, lse2)
    for name, a, b in zip(("o", "dq", "dk", "dv"), docs, plain):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape,layout", [(s, lay) for s in SHAPES for lay in ("dense", "last")])
def test_documents_are_independent_bit_for_bit(shape, layout):
    from pytorch_operator_amd.ops.attention import flash_attention
    q, k, v, do = _inputs(*shape, seed=5)
    ds = _doc_start(shape, layout)
    S = shape[1]
    first_end = int((ds[0] == 0).sum())       # the first document is [0, first_end)
    last_start = int(ds[0, S - 1])            # the last one is [last_start, S)
    assert 0 < first_end < S and 0 < last_start < S
    base = _grads(lambda a, b, c: flash_attention(a, b, c, True, doc_start=ds), do, q, k, v)
    # K and V inside the first document: later documents' output rows must not change
    k2, v2 = k.clone(), v.clone()
    k2[:, :first_end] += 1.0
    v2[:, :first_end] -= 2.0
    with torch.no_grad():
        o2 = flash_attention(q, k2, v2, True, doc_start=ds)
    assert not torch.equal(o2[:, :first_end], base[0][:, :first_end])
    assert torch.equal(o2[:, first_end:], base[0][:, first_end:])
    # dO inside the last document: earlier documents' dk / dv rows must not change
    do2 = do.clone()
    do2[:, last_start:] *= -3.0
    other = _grads(lambda a, b, c: flash_attention(a, b, c, True, doc_start=ds), do2, q, k, v)
    for name, a, b in zip(("dk", "dv"), other[2:], base[2:]):
        assert torch.equal(a[:, :last_start], b[:, :last_start]), name
    # (the last document's own dv rows do change; its dk is exactly zero when it is one token long)
    assert not torch.equal(other[3][:, last_start:], base[3][:, last_start:])


def test_doc_llama_block_matches_sdpa_dense_mask_path():
    """A D = 128 Llama config with packed documents through the model's attention dispatch: the HIP
    document path vs SDPA with the dense mask (test_flash_llama_block_matches_sdpa_path's bounds)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-mini"]).cuda()
    tok = torch.randint(0, CONFIGS["llama-mini"].vocab_size, (2, 256), device="cuda")
    ds = _doc_start((2, 256, 4, 2), "mixed")
    out = {}
    for impl in ("hip", "sdpa"):
        for blk in m.layers:
            blk.attention.impl = impl
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):  # the worker's setting
            loss = m(tok, tok, doc_start=ds)
        loss.backward()
        out[impl] = (float(loss.detach()), m.layers[0].attention.wqkv.weight.grad.float().clone())
    assert math.isfinite(out["hip"][0])
    assert abs(out["hip"][0] - out["sdpa"][0]) < 2e-2 * abs(out["sdpa"][0])
    assert _rel(out["hip"][1], out["sdpa"][1]) < 5e-2


def test_doc_start_argument_errors_on_gpu():
    from pytorch_operator_amd.ops.attention import flash_attention
    q = torch.zeros(1, 128, 2, 128, device="cuda", dtype=torch.bfloat16)
    ds = torch.zeros(1, 128, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=True, doc_start=ds[:, :64])
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=True, doc_start=ds.cpu())
    bad = torch.zeros(1, 100, 2, 128, device="cuda", dtype=torch.bfloat16)  # unsupported shape still raises
    with pytest.raises(ValueError):
        flash_attention(bad, bad, bad, doc_start=torch.zeros(1, 100, dtype=torch.int32, device="cuda"))
