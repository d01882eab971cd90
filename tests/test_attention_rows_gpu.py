"""GPU: the flash-attention kernels (csrc/kernels/attention.hip, attention_bwd_pipe.hip) row by
row against fp64 arithmetic on the same values, at the element-wise bounds derived in
tests/attention_refs.py.

tests/test_attention_gpu.py and test_attention_doc_gpu.py judge each tensor by one relative norm;
a key leaked to one row, a skipped tile, a wrong delta or a swapped scale argument stay far below
that criterion.  Here every element of o, lse2, delta, dq, dk and dv has its own bound, on inputs
built so that the mask decides the answer on every row (see attention_refs.case_inputs): Gaussian,
counting (q = 0), one-hot (one key carries the row) and decoy (the one-hot key is one the row must
not see).  All launches go through the C entry points with the outputs inside NaN-filled guarded
allocations, so a row a kernel never wrote cannot pass on stale memory.
tests/test_attention_refs_cpu.py runs a rounding model of the kernels through every case below.
"""
import math

import pytest
import torch

from attention_refs import (LOG2_HW, OUTPUTS, Case, case_doc_start, case_id, case_inputs, case_mask, case_reference,
                            ratios, target_keys, worst_at)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEFAULTS, PLAIN = (10, 9, 8), (4, 4, 1)  # forward, dQ, dK/dV variants: the default passes, the plain 4-wave ones
VSETS = [DEFAULTS, PLAIN]
VSET_IDS = ["default", "plain"]

SHAPES = [  # B, S, Hq, Hkv
    (1, 128, 2, 2),   # one block everywhere, 4-wave forward and dQ
    (3, 256, 6, 3),   # 8-wave forward and dQ with one block; B and Hkv no powers of two; G = 2
    (2, 384, 3, 1),   # 4-wave fallback with three query and key blocks; G = 3
    (1, 512, 8, 2),   # 8-wave with two blocks, heaviest-first order under the causal mask; G = 4
]
DOC_SHAPES = [(1, 128, 2, 2), (2, 256, 8, 2), (1, 384, 4, 1)]  # test_attention_doc_gpu.py's
DOC_LAYOUTS = [(s, lay) for s in DOC_SHAPES for lay in ("dense", "last")] + [((2, 256, 8, 2), "mixed")]
ONEHOT_SHAPES = [(3, 256, 6, 3), (1, 512, 8, 2)]

GAUSSIAN = [Case("gaussian", s, m) for s in SHAPES for m in ("causal", "full")]
GAUSSIAN_DOC = [Case("gaussian", s, lay) for s, lay in DOC_LAYOUTS]
COUNTING = [Case("counting", s, m, seed=1) for s in SHAPES for m in ("causal", "full")]
COUNTING_DOC = [Case("counting", s, lay, seed=1) for s, lay in DOC_LAYOUTS]
MAPS = ("diag", "first", "tile", "tile-1")  # the target key of row i: see attention_refs.target_keys
ONEHOT = ([Case("onehot", s, "causal", pmap=p, seed=2) for s in ONEHOT_SHAPES for p in MAPS]
          + [Case("onehot", s, "full", pmap="reverse", seed=2) for s in ONEHOT_SHAPES])
ONEHOT_DOC = [Case("onehot", (2, 256, 8, 2), lay, pmap=p, seed=2) for lay in ("dense", "last", "mixed") for p in MAPS]
DECOY = [Case("decoy", s, "causal", seed=3) for s in ONEHOT_SHAPES]
DECOY_DOC = [Case("decoy", (2, 256, 8, 2), lay, seed=3) for lay in ("dense", "mixed")]
SCALES = [Case("gaussian", (3, 256, 6, 3), "causal", scale=sc, seed=4) for sc in (0.05, 0.2)]
PLAIN_CASES = GAUSSIAN + COUNTING + ONEHOT + DECOY + SCALES   # pto_attn_fwd / pto_attn_bwd, both variant sets
DOC_CASES = GAUSSIAN_DOC + COUNTING_DOC + ONEHOT_DOC + DECOY_DOC  # pto_attn_doc_fwd / pto_attn_doc_bwd
ALL_CASES = PLAIN_CASES + DOC_CASES

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


_RUNS = {}


def run(case, vset=None):
    """Forward and backward of one case through the C entry points (the document entry points when
    the case has a document mask; `vset` selects the plain passes' variants), the backward reading
    the o and lse2 the forward kernel wrote.  Returns the six outputs as CPU tensors; cached."""
    if (case, vset) in _RUNS:
        return _RUNS[(case, vset)]
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.attention import doc_ends
    lib = _native.load()
    B, S, Hq, Hkv = case.shape
    q, k, v, do = (t.cuda() for t in case_inputs(case))
    ds = case_doc_start(case)
    assert (ds is None) != (vset is None)
    bufs = {n: _guarded(shape, dt) for n, shape, dt in (
        ("o", q.shape, BF16), ("lse2", (B, Hq, S), F32), ("delta", (B, Hq, S), F32), ("dq", q.shape, BF16),
        ("dk", k.shape, BF16), ("dv", v.shape, BF16))}
    ptr = {n: view.data_ptr() for n, (_, view) in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    if ds is None:
        old = (lib.pto_attn_set_variant(vset[0]), lib.pto_attn_set_dq_variant(vset[1]),
               lib.pto_attn_set_dkdv_variant(vset[2]))
        try:
            causal = int(case.mask == "causal")
            _native.check(lib.pto_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], ptr["lse2"], B, S, Hq,
                                           Hkv, 128, case.scale, causal, stream), "attn_fwd")
            _native.check(lib.pto_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], do.data_ptr(),
                                           ptr["lse2"], ptr["delta"], ptr["dq"], ptr["dk"], ptr["dv"], B, S, Hq, Hkv,
                                           128, case.scale, causal, stream), "attn_bwd")
            torch.cuda.synchronize()
        finally:
            lib.pto_attn_set_variant(old[0])
            lib.pto_attn_set_dq_variant(old[1])
            lib.pto_attn_set_dkdv_variant(old[2])
    else:
        dsg = ds.cuda()
        de = doc_ends(dsg)
        _native.check(lib.pto_attn_doc_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], ptr["lse2"],
                                           dsg.data_ptr(), B, S, Hq, Hkv, 128, case.scale, stream), "attn_doc_fwd")
        _native.check(lib.pto_attn_doc_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr["o"], do.data_ptr(),
                                           ptr["lse2"], ptr["delta"], ptr["dq"], ptr["dk"], ptr["dv"], dsg.data_ptr(),
                                           de.data_ptr(), B, S, Hq, Hkv, 128, case.scale, stream), "attn_doc_bwd")
        torch.cuda.synchronize()
    for n, (base, view) in bufs.items():
        _check_guards(n, base, view)
    _RUNS[(case, vset)] = {n: view.cpu() for n, (_, view) in bufs.items()}
    return _RUNS[(case, vset)]


def _where(name, at):
    """(b, h, row) of an index into an output: o / dq / dk / dv are [B, S, H, D], lse2 / delta [B, H, S]."""
    return (at[0], at[1], at[2]) if name in ("lse2", "delta") else (at[0], at[2], at[1])


def _hold(case, vset, got, names=OUTPUTS):
    """Every element of the named outputs within its bound; prints the worst ratio and its (b, h, row)."""
    rs = ratios(got, case_reference(case))
    print(case_id(case), vset or "doc", " ".join(f"{n} {rs[n][0]:.3f}@{_where(n, rs[n][1])}" for n in names))
    bad = {n: (round(rs[n][0], 3), _where(n, rs[n][1])) for n in names if not rs[n][0] <= 1}
    assert not bad, (case_id(case), vset, bad)


def _plain(cases):
    return pytest.mark.parametrize("case", cases, ids=case_id)


_vsets = pytest.mark.parametrize("vset", VSETS, ids=VSET_IDS)


@_vsets
@_plain(GAUSSIAN)
def test_gaussian_rows_within_bounds(case, vset):
    _hold(case, vset, run(case, vset))


@_plain(GAUSSIAN_DOC)
def test_gaussian_rows_within_bounds_doc(case):
    _hold(case, None, run(case))


def _counting(case, vset):
    """q = 0: l is the exact number of visible keys, so lse2 = log2(count) up to the hardware log2
    alone, on every row; o is the mean of the visible v rows; dk = scale * dS^T.q is exactly 0."""
    S = case.shape[1]
    got, ref = run(case, vset), case_reference(case)
    count = case_mask(case).sum(-1).double().expand_as(ref["lse2"])
    # a miscounted key moves lse2 by at least log2((S + 1) / S): the bound must stay below half of it
    assert LOG2_HW < 0.5 * math.log2((S + 1) / S)
    err, at = worst_at(got["lse2"], count.log2(), torch.ones_like(count))
    print(case_id(case), vset or "doc", f"max |lse2 - log2(count)| {err:.3e} at (b, h, row) {at}")
    assert err <= LOG2_HW, (err, at)
    _hold(case, vset, got, ("o", "delta", "dq", "dv"))
    assert bool((got["dk"] == 0).all())


@_vsets
@_plain(COUNTING)
def test_counting_inputs_pin_the_key_count(case, vset):
    """LOG2_HW: the device log2f against fp64 log2 over the counts 1..512 these cases produce.  The
    worst |lse2 - log2(count)| is printed: 9.466e-7 on an MI355X, at count 265 (just under one ulp of
    a result above 8, 2^-20 = 9.537e-7), 0 at every power of two; LOG2_HW = 2^-20 is the next power
    of two above it, 1500 times below the 1.4e-3 a miscounted key moves lse2 by at S = 512."""
    _counting(case, vset)


@_plain(COUNTING_DOC)
def test_counting_inputs_pin_the_key_count_doc(case):
    _counting(case, None)


def _onehot(case, vset):
    """One key carries >= 0.999 of every row: o_i ~ v[pi(i)], dv_j sums the dO rows that chose j.  A
    misrouted or skipped key, or a skipped tile, is a gross error; the large scores make the 8-wave
    forward's deferred rescale fire."""
    B, S, Hq, Hkv = case.shape
    got, ref = run(case, vset), case_reference(case)
    for n in OUTPUTS:
        assert bool(torch.isfinite(got[n].float()).all()), n
    _hold(case, vset, got)
    # o around v[pi(i)]: |o64 - v_pi| <= (1 - p_pi) (|v_pi| + max |v|)
    pi = target_keys(case)
    v = case_inputs(case)[2].double()
    vt = torch.gather(v, 1, pi.view(B, S, 1, 1).expand(B, S, Hkv, 128)).repeat_interleave(Hq // Hkv, dim=2)
    rest = 1 - torch.gather(ref["p"], 3, pi.view(B, 1, S, 1).expand(B, Hq, S, 1)).squeeze(-1).transpose(1, 2)
    assert float(rest.max()) <= 1e-3
    r, at = worst_at(got["o"], vt, ref["b_o"] + rest.unsqueeze(-1) * (vt.abs() + v.abs().max()))
    assert r <= 1, (r, at)


@_vsets
@_plain(ONEHOT)
def test_onehot_rows_route_to_their_key(case, vset):
    _onehot(case, vset)


@_plain(ONEHOT_DOC)
def test_onehot_rows_route_to_their_key_doc(case):
    _onehot(case, None)


@_vsets
@_plain(DECOY)
def test_decoy_key_past_the_diagonal_stays_masked(case, vset):
    """q_i = GAMMA * k[i + 1]: the first masked key would take nearly the whole row in any pass
    that let it through, at every row index."""
    _hold(case, vset, run(case, vset))


@_plain(DECOY_DOC)
def test_decoy_key_before_the_document_stays_masked(case):
    """q_i = GAMMA * k[doc_start[i] - 1]: the last key of the previous document."""
    _hold(case, None, run(case))


def _first_rows(case, vset, rows):
    """A row that sees only its own key: p = 1, l = 1, so o[i] is v[i] (GQA-mapped) bit for bit and
    lse2[i] = s_ii * scale * log2(e) (the reference's value) within the lse2 bound."""
    got, ref = run(case, vset), case_reference(case)
    G = case.shape[2] // case.shape[3]
    v = case_inputs(case)[2].repeat_interleave(G, dim=2)
    for b, i in rows:
        assert torch.equal(got["o"][b, i], v[b, i]), (b, i)
        assert bool(((got["lse2"][b, :, i].double() - ref["lse2"][b, :, i]).abs() <= ref["b_lse2"][b, :, i]).all())


@_vsets
@_plain([c for c in GAUSSIAN if c.mask == "causal"])
def test_first_row_is_exact(case, vset):
    _first_rows(case, vset, [(b, 0) for b in range(case.shape[0])])


@_plain(GAUSSIAN_DOC)
def test_first_row_of_every_document_is_exact(case):
    ds = case_doc_start(case)
    rows = [(b, i) for b in range(ds.shape[0]) for i in range(ds.shape[1]) if int(ds[b, i]) == i]
    assert len(rows) >= 2 * ds.shape[0] or case.mask == "mixed"
    _first_rows(case, None, rows)


@_vsets
@_plain(SCALES)
def test_scale_argument_reaches_every_output(case, vset):
    """The kernels receive both c = scale * log2(e) (the exponent) and scale (dq, dk): away from
    1 / sqrt(128) a mix-up of the two, or a constant in place of either, breaks a bound."""
    _hold(case, vset, run(case, vset))


@pytest.mark.parametrize("causal", [True, False])
def test_op_copies_strided_and_offset_arguments(causal):
    """flash_attention with q, k, v as non-contiguous slices of one packed [B, S, Hq + 2 Hkv, 128]
    projection output and a non-contiguous dO two bytes off a 16-byte boundary (the op's `_c()`
    copies) is bit-equal to the call on contiguous tensors."""
    from pytorch_operator_amd.ops.attention import flash_attention
    B, S, Hq, Hkv = 2, 256, 6, 3
    g = torch.Generator(device="cpu").manual_seed(77)
    packed = torch.randn(B, S, Hq + 2 * Hkv, 128, generator=g).to(BF16).cuda()
    dobuf = torch.randn(B * S * Hq * 256 + 1, generator=g).to(BF16).cuda()
    do = dobuf[1:].view(B, S, Hq, 256)[..., :128]
    assert not do.is_contiguous() and do.data_ptr() % 16 == 2
    views = packed[:, :, :Hq], packed[:, :, Hq:Hq + Hkv], packed[:, :, Hq + Hkv:]
    assert not any(t.is_contiguous() for t in views)

    def grads(xs, dout):
        xs = [x.detach().requires_grad_(True) for x in xs]
        out = flash_attention(*xs, causal)
        out.backward(dout)
        return [out.detach()] + [x.grad for x in xs]

    # leaves that are themselves the strided views: gradients come back in the views' shapes
    strided = grads(views, do)
    dense = grads([t.contiguous() for t in views], do.contiguous())
    for name, a, b in zip(("o", "dq", "dk", "dv"), strided, dense):
        assert a.shape == b.shape and torch.equal(a, b), name
