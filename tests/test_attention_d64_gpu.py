"""GPU: the head-dim-64 flash-attention kernels (csrc/kernels/attention_d64.hip: the 4-wave forward,
dQ and dK/dV passes, plain and document-masked) row by row against fp64 arithmetic on the same
values, at the element-wise bounds of tests/attention_refs.py, the way
tests/test_attention_rows_gpu.py holds the D = 128 kernels; then the op, the dispatch and the
Llama-3.2-1B-shaped test model on top of them.  The launches of the row tests go through the C
entry points with the outputs inside NaN-filled guarded allocations.
tests/test_attention_d64_cpu.py runs a rounding model of the kernels through every case here.
"""
import math

import pytest
import torch

from attention_refs import LOG2_HW, OUTPUTS, case_doc_start, case_id, case_mask, ratios, target_keys, worst_at
from attention_d64_cases import (COUNTING, COUNTING_DOC, D64, DECOY, DECOY_DOC, GAUSSIAN, GAUSSIAN_DOC, ONEHOT, SCALES,
                                 SCALE64, case_inputs64, case_reference64, onehot_rest)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
_PAD = 64  # guard elements on each side of an output


def _guarded(shape, dtype):
    """(allocation, view): a NaN-filled allocation (bf16 0x7fc0 / fp32 0x7fc00000) with `shape` in
    its middle, at a 16-byte-aligned address."""
    n = math.prod(shape)
    base = torch.full((n + 2 * _PAD + 16,), math.nan, dtype=dtype, device="cuda")
    off = _PAD + (-(base.data_ptr() // base.element_size() + _PAD)) % (16 // base.element_size())
    view = base[off:off + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return base, view


def _check_guards(name, base, view):
    bits = base.view(torch.int16 if base.dtype == BF16 else torch.int32)
    nan_bits = 0x7fc0 if base.dtype == BF16 else 0x7fc00000
    off = (view.data_ptr() - base.data_ptr()) // base.element_size()
    assert bool((bits[:off] == nan_bits).all()) and bool((bits[off + view.numel():] == nan_bits).all()), \
        f"{name}: written outside the output"
    assert not bool(torch.isnan(view).any()), f"{name}: elements never written (or NaN)"


def _launch(inputs, shape, scale, causal, ds):
    """Forward and backward through the C entry points at Dh = 64 (the document entry points when ds,
    an int32 [B, S] device tensor, is given), the backward reading the o and lse2 the forward kernel
    wrote; the six outputs as CPU tensors, after the guard check."""
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.attention import doc_ends
    lib = _native.load()
    B, S, Hq, Hkv = shape
    q, k, v, do = (t.cuda() for t in inputs)
    bufs = {n: _guarded(s, dt) for n, s, dt in (
        ("o", q.shape, BF16), ("lse2", (B, Hq, S), F32), ("delta", (B, Hq, S), F32), ("dq", q.shape, BF16),
        ("dk", k.shape, BF16), ("dv", v.shape, BF16))}
    ptr = {n: view.data_ptr() for n, (_, view) in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    if ds is None:
        _native.check(lib.pto_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], ptr["lse2"], B, S, Hq, Hkv,
                                       D64, scale, int(causal), stream), "attn_fwd")
        _native.check(lib.pto_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], do.data_ptr(), ptr["lse2"],
                                       ptr["delta"], ptr["dq"], ptr["dk"], ptr["dv"], B, S, Hq, Hkv, D64, scale,
                                       int(causal), stream), "attn_bwd")
    else:
        de = doc_ends(ds)
        _native.check(lib.pto_attn_doc_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], ptr["lse2"],
                                           ds.data_ptr(), B, S, Hq, Hkv, D64, scale, stream), "attn_doc_fwd")
        _native.check(lib.pto_attn_doc_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], do.data_ptr(),
                                           ptr["lse2"], ptr["delta"], ptr["dq"], ptr["dk"], ptr["dv"], ds.data_ptr(),
                                           de.data_ptr(), B, S, Hq, Hkv, D64, scale, stream), "attn_doc_bwd")
    torch.cuda.synchronize()
    for n, (base, view) in bufs.items():
        _check_guards(n, base, view)
    return {n: view.cpu() for n, (_, view) in bufs.items()}


_RUNS = {}


def run(case):
    """The six outputs of one case (cached)."""
    if case not in _RUNS:
        ds = case_doc_start(case)
        _RUNS[case] = _launch(case_inputs64(case), case.shape, case.scale, case.mask == "causal",
                              None if ds is None else ds.cuda())
    return _RUNS[case]


def _where(name, at):
    """(b, h, row) of an index into an output: o / dq / dk / dv are [B, S, H, D], lse2 / delta [B, H, S]."""
    return (at[0], at[1], at[2]) if name in ("lse2", "delta") else (at[0], at[2], at[1])


def _hold(case, got, names=OUTPUTS):
    """Every element of the named outputs within its bound; prints the worst ratio and its (b, h, row)."""
    rs = ratios(got, case_reference64(case))
    print(case_id(case), " ".join(f"{n} {rs[n][0]:.3f}@{_where(n, rs[n][1])}" for n in names))
    bad = {n: (round(rs[n][0], 3), _where(n, rs[n][1])) for n in names if not rs[n][0] <= 1}
    assert not bad, (case_id(case), bad)


def _cases(cases):
    return pytest.mark.parametrize("case", cases, ids=case_id)


@_cases(GAUSSIAN + GAUSSIAN_DOC)
def test_gaussian_rows_within_bounds(case):
    _hold(case, run(case))


@_cases(COUNTING + COUNTING_DOC)
def test_counting_inputs_pin_the_key_count(case):
    """q = 0: l is the exact number of visible keys, so lse2 = log2(count) up to the hardware log2
    alone, on every row; o is the mean of the visible v rows; dk = scale * dS^T.q is exactly 0."""
    S = case.shape[1]
    got, ref = run(case), case_reference64(case)
    count = case_mask(case).sum(-1).double().expand_as(ref["lse2"])
    # a miscounted key moves lse2 by at least log2((S + 1) / S): the bound must stay below half of it
    assert LOG2_HW < 0.5 * math.log2((S + 1) / S)
    err, at = worst_at(got["lse2"], count.log2(), torch.ones_like(count))
    print(case_id(case), f"max |lse2 - log2(count)| {err:.3e} at (b, h, row) {at}")
    assert err <= LOG2_HW, (err, at)
    _hold(case, got, ("o", "delta", "dq", "dv"))
    assert bool((got["dk"] == 0).all())


@_cases(ONEHOT)
def test_onehot_rows_route_to_their_key(case):
    """One key carries all but 1e-3 of every row: o_i ~ v[pi(i)], dv_j sums the dO rows that chose j.
    A misrouted or skipped key, or a skipped tile, is a gross error."""
    B, S, Hq, Hkv = case.shape
    got, ref = run(case), case_reference64(case)
    for n in OUTPUTS:
        assert bool(torch.isfinite(got[n].float()).all()), n
    _hold(case, got)
    # o around v[pi(i)]: |o64 - v_pi| <= (1 - p_pi) (|v_pi| + max |v|)
    pi = target_keys(case)
    v = case_inputs64(case)[2].double()
    vt = torch.gather(v, 1, pi.view(B, S, 1, 1).expand(B, S, Hkv, D64)).repeat_interleave(Hq // Hkv, dim=2)
    rest = onehot_rest(case)
    assert float(rest.max()) <= 1e-3
    r, at = worst_at(got["o"], vt, ref["b_o"] + rest.unsqueeze(-1) * (vt.abs() + v.abs().max()))
    assert r <= 1, (r, at)


@_cases(DECOY + DECOY_DOC)
def test_decoy_key_stays_masked(case):
    """q_i = GAIN * k[i + 1] (causal) or GAIN * k[doc_start[i] - 1] (document): the nearest masked key
    would take nearly the whole row in any pass that let it through, at every row index."""
    _hold(case, run(case))


def _first_rows(case, rows):
    """A row that sees only its own key: p = 1, l = 1, so o[i] is v[i] (GQA-mapped) bit for bit and
    lse2[i] = s_ii * scale * log2(e) (the reference's value) within the lse2 bound."""
    got, ref = run(case), case_reference64(case)
    G = case.shape[2] // case.shape[3]
    v = case_inputs64(case)[2].repeat_interleave(G, dim=2)
    for b, i in rows:
        assert torch.equal(got["o"][b, i], v[b, i]), (b, i)
        assert bool(((got["lse2"][b, :, i].double() - ref["lse2"][b, :, i]).abs() <= ref["b_lse2"][b, :, i]).all())


@_cases([c for c in GAUSSIAN if c.mask == "causal"])
def test_first_row_is_exact(case):
    _first_rows(case, [(b, 0) for b in range(case.shape[0])])


@_cases(GAUSSIAN_DOC)
def test_first_row_of_every_document_is_exact(case):
    ds = case_doc_start(case)
    rows = [(b, i) for b in range(ds.shape[0]) for i in range(ds.shape[1]) if int(ds[b, i]) == i]
    assert len(rows) >= 2 * ds.shape[0] or case.mask == "mixed"
    _first_rows(case, rows)


@_cases(SCALES)
def test_scale_argument_reaches_every_output(case):
    """The kernels receive both c = scale * log2(e) (the exponent) and scale (dq, dk): away from
    1 / sqrt(64) a mix-up of the two, or a constant in place of either, breaks a bound."""
    _hold(case, run(case))


@_cases([c for c in GAUSSIAN if c.mask == "causal"])
def test_one_document_is_bit_identical_to_the_plain_kernels(case):
    """doc_start == 0: the document kernels run the plain D = 64 kernels' operations in their order."""
    B, S = case.shape[:2]
    doc = _launch(case_inputs64(case), case.shape, case.scale, True, torch.zeros(B, S, dtype=torch.int32, device="cuda"))
    plain = run(case)
    for n in ("o", "lse2", "dq", "dk", "dv"):
        assert torch.equal(doc[n], plain[n]), n


# ------------------------------------------------------------------------------------- the op
def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


def _doc_start(B, S):
    ds = torch.zeros(B, S, dtype=torch.int32)
    for lo in (1, 33, 64, 129, 200):
        if lo < S:
            ds[0, lo:] = lo
    ds[-1, S - 1] = S - 1
    return ds.cuda()


@pytest.mark.parametrize("mask", ["causal", "full", "doc"])
@pytest.mark.parametrize("shape", [(2, 256, 8, 2), (1, 384, 4, 4), (1, 512, 8, 1)])
def test_flash_attention_autograd_matches_fp32_reference(shape, mask):
    """flash_attention at D = 64 against attention_reference on float inputs, with the library
    SDPA's own bf16 error as the yardstick (tests/test_attention_gpu.py's criterion and values)."""
    from pytorch_operator_amd.ops.attention import attention_reference, flash_attention, sdpa_bshd
    B, S, Hq, Hkv = shape
    g = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda H: torch.randn(B, S, H, D64, device="cuda", generator=g).to(BF16)  # noqa: E731
    q, k, v, do = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    causal = mask != "full"
    ds = _doc_start(B, S) if mask == "doc" else None

    def grads(fn, *xs):
        xs = [x.detach().clone().requires_grad_(True) for x in xs]
        out = fn(*xs)
        out.backward(do.to(out.dtype))
        return [out.detach()] + [x.grad for x in xs]

    ref = grads(lambda a, b, c: attention_reference(a, b, c, causal, doc_start=ds).float(), q.float(), k.float(),
                v.float())
    ours = grads(lambda a, b, c: flash_attention(a, b, c, causal, doc_start=ds), q, k, v)
    lib = grads(lambda a, b, c: sdpa_bshd(a, b, c, causal, doc_start=ds), q, k, v)
    for name, a, r, lb in zip(("o", "dq", "dk", "dv"), ours, ref, lib):
        e, el = _rel(a, r), _rel(lb, r)
        print(shape, mask, name, f"hip {e:.2e} sdpa {el:.2e}")
        assert e < max(2.0 * el, 4e-3 if name == "o" else 6e-3), (name, e, el)
        assert torch.isfinite(a.float()).all(), name
    assert float((ours[0].float() - ref[0]).abs().max()) < 3e-2


@pytest.mark.parametrize("causal", [True, False])
def test_op_copies_strided_and_offset_arguments(causal):
    """flash_attention with q, k, v as non-contiguous slices of one packed [B, S, Hq + 2 Hkv, 64]
    projection output and a non-contiguous dO two bytes off a 16-byte boundary (the op's `_c()`
    copies) is bit-equal to the call on contiguous tensors."""
    from pytorch_operator_amd.ops.attention import flash_attention
    B, S, Hq, Hkv = 2, 256, 6, 3
    g = torch.Generator(device="cpu").manual_seed(77)
    packed = torch.randn(B, S, Hq + 2 * Hkv, D64, generator=g).to(BF16).cuda()
    dobuf = torch.randn(B * S * Hq * 2 * D64 + 1, generator=g).to(BF16).cuda()
    do = dobuf[1:].view(B, S, Hq, 2 * D64)[..., :D64]
    assert not do.is_contiguous() and do.data_ptr() % 16 == 2
    views = packed[:, :, :Hq], packed[:, :, Hq:Hq + Hkv], packed[:, :, Hq + Hkv:]
    assert not any(t.is_contiguous() for t in views)

    def grads(xs, dout):
        xs = [x.detach().requires_grad_(True) for x in xs]
        out = flash_attention(*xs, causal)
        out.backward(dout)
        return [out.detach()] + [x.grad for x in xs]

    strided = grads(views, do)
    dense = grads([t.contiguous() for t in views], do.contiguous())
    for name, a, b in zip(("o", "dq", "dk", "dv"), strided, dense):
        assert a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("dh", [32, 96])
def test_other_head_dims_are_still_refused(dh):
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.attention import flash_attention
    q = torch.zeros(1, 128, 2, dh, device="cuda", dtype=BF16)
    with pytest.raises(ValueError):
        flash_attention(q, q, q)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, doc_start=torch.zeros(1, 128, dtype=torch.int32, device="cuda"))
    lib = _native.load()
    o, lse2 = torch.zeros_like(q), torch.zeros(1, 2, 128, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ds = torch.zeros(1, 128, dtype=torch.int32, device="cuda")
    p = q.data_ptr()
    assert lib.pto_attn_fwd(p, p, p, o.data_ptr(), lse2.data_ptr(), 1, 128, 2, 2, dh, 0.125, 1, stream) == -1
    assert lib.pto_attn_doc_fwd(p, p, p, o.data_ptr(), lse2.data_ptr(), ds.data_ptr(), 1, 128, 2, 2, dh, 0.125,
                                stream) == -1
    assert lib.pto_attn_bwd(p, p, p, p, p, lse2.data_ptr(), lse2.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(),
                            1, 128, 2, 2, dh, 0.125, 1, stream) == -1
    assert lib.pto_attn_doc_bwd(p, p, p, p, p, lse2.data_ptr(), lse2.data_ptr(), o.data_ptr(), o.data_ptr(),
                                o.data_ptr(), ds.data_ptr(), ds.data_ptr(), 1, 128, 2, 2, dh, 0.125, stream) == -1
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(lse2.any())  # nothing was launched


@pytest.mark.parametrize("docs", [False, True])
def test_llama_mini64_takes_the_hip_path_and_matches_sdpa(docs, monkeypatch):
    """The head-dim-64 test model through the model's attention dispatch under impl "auto": the HIP
    entry points are taken (counted here), and loss and gradients match the library path on the same
    weights and tokens (the bounds of the llama-mini tests at D = 128)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops import _native
    cfg = CONFIGS["llama-mini64"]
    assert cfg.head_dim == D64
    torch.manual_seed(0)
    m = Llama(cfg).cuda()
    tok = torch.randint(0, cfg.vocab_size, (2, 256), device="cuda")
    ds = _doc_start(2, 256) if docs else None
    lib = _native.load()
    calls = []
    fwd_name = "pto_attn_doc_fwd" if docs else "pto_attn_fwd"
    real = getattr(lib, fwd_name)

    def counted(*args):
        calls.append(args[-3 if docs else -4])  # Dh
        return real(*args)

    monkeypatch.setattr(lib, fwd_name, counted)
    out = {}
    for impl in ("auto", "sdpa"):
        for blk in m.layers:
            blk.attention.impl = impl
        m.zero_grad(set_to_none=True)
        del calls[:]
        with torch.autocast("cuda", dtype=torch.bfloat16):  # the worker's setting
            loss = m(tok, tok, doc_start=ds)
        loss.backward()
        out[impl] = (float(loss.detach()), m.layers[0].attention.wqkv.weight.grad.float().clone(), list(calls))
    assert out["auto"][2] == [D64] * cfg.n_layers, out["auto"][2]
    assert out["sdpa"][2] == []
    assert math.isfinite(out["auto"][0])
    assert abs(out["auto"][0] - out["sdpa"][0]) < 2e-2 * abs(out["sdpa"][0])
    assert _rel(out["auto"][1], out["sdpa"][1]) < 5e-2


def test_default_scale_is_the_head_dims():
    """The op passes 1 / sqrt(64), not the D = 128 scale: o against the reference at both."""
    from pytorch_operator_amd.ops.attention import attention_reference, flash_attention
    g = torch.Generator(device="cuda").manual_seed(3)
    q = (3 * torch.randn(1, 128, 2, D64, device="cuda", generator=g)).to(BF16)
    k = torch.randn(1, 128, 2, D64, device="cuda", generator=g).to(BF16)
    v = torch.randn(1, 128, 2, D64, device="cuda", generator=g).to(BF16)
    o = flash_attention(q, k, v)
    assert SCALE64 == 0.125
    assert _rel(o, attention_reference(q.float(), k.float(), v.float())) < 4e-3
    wrong = attention_reference((q.float() * math.sqrt(64 / 128)), k.float(), v.float())
    assert _rel(o, wrong) > 5e-2
