"""CPU: the checker of tests/test_attention_rows_gpu.py has teeth.  attention_refs.attention_fp64
equals fp64 autograd; a model of a correctly rounding kernel (attention_refs.rounding_model) stays
within every derived bound on every case the GPU module runs; and each wrong kernel below -- the
model with one fault injected -- breaks a bound on the input kind named beside it, for the mask
faults on the very row (or key) the fault touches."""
import math

import pytest
import torch

from attention_refs import (LOG2E, OUTPUTS, Case, attention_fp64, case_id, case_inputs, case_mask, case_reference,
                            ratios, rounding_model, target_keys, visibility, worst_at, doc_start_rows)
from test_attention_rows_gpu import ALL_CASES


@pytest.mark.parametrize("mask", ["causal", "full", "dense"])
def test_reference_equals_fp64_autograd(mask):
    """Against autograd through a plain fp64 softmax at a non-default scale (to 1e-10), and through
    ops.attention.attention_reference (which computes in fp32: to fp32 accuracy)."""
    from pytorch_operator_amd.ops.attention import attention_reference
    c = Case("gaussian", (2, 256, 4, 2), mask, seed=9)
    q, k, v, do = (t.double() for t in case_inputs(c))
    vis = case_mask(c)
    ds = None if mask in ("causal", "full") else doc_start_rows(256, 2, mask)

    def autograd(fn):
        xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = fn(*xs)
        o.backward(do)
        return [o.detach()] + [x.grad for x in xs]

    def plain(scale):
        def fn(a, b, c_):
            s = torch.einsum("bihd,bjhd->bhij", a, b.repeat_interleave(2, dim=2)) * scale
            p = torch.softmax(s.masked_fill(~vis, -math.inf), -1)
            return torch.einsum("bhij,bjhd->bihd", p, c_.repeat_interleave(2, dim=2))
        return fn

    lib = lambda a, b, c_: attention_reference(a, b, c_, mask != "full", doc_start=ds)  # noqa: E731
    for scale, fn, tol in ((0.2, plain(0.2), 1e-10), (1 / math.sqrt(128), lib, 2e-5)):
        ref = attention_fp64(q, k, v, do, scale, vis)
        for name, want in zip(("o", "dq", "dk", "dv"), autograd(fn)):
            assert float((ref[name] - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (scale, name)
        assert torch.allclose(ref["delta"], (do * ref["o"]).sum(-1).transpose(1, 2), atol=1e-12)
    s = torch.einsum("bihd,bjhd->bhij", q, k.repeat_interleave(2, dim=2)) / math.sqrt(128)
    lse = torch.logsumexp(s.masked_fill(~vis, -math.inf), -1)
    assert torch.allclose(ref["lse2"], lse * LOG2E, atol=1e-12)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_rounding_model_within_every_bound(case):
    """What makes the bounds usable: a kernel that rounds where the kernels round, and is otherwise
    exact, stays at ratio <= 1 on every element of every output of every GPU case."""
    ref = case_reference(case)
    if case.kind == "onehot":
        B, S, Hq, _ = case.shape
        p_target = torch.gather(ref["p"], 3, target_keys(case).view(B, 1, S, 1).expand(B, Hq, S, 1))
        assert float(p_target.min()) >= 0.999, float(p_target.min())
    rs = ratios(rounding_model(*case_inputs(case), case.scale, case_mask(case)), ref)
    print(case_id(case), " ".join(f"{n} {rs[n][0]:.3f}" for n in OUTPUTS))
    assert all(rs[n][0] <= 1 for n in OUTPUTS), rs


# ---------------------------------------------------------------------------------- mutants
BIG = (1, 512, 8, 2)       # G = 4: query head h reads kv head h // 4
DOC = (2, 256, 8, 2)
GAUSS, COUNT = Case("gaussian", BIG, "causal"), Case("counting", BIG, "causal", seed=1)
DECOY, DIAG = Case("decoy", BIG, "causal", seed=3), Case("onehot", BIG, "causal", pmap="diag", seed=2)
FIRST = Case("onehot", BIG, "causal", pmap="first", seed=2)
SCALED = Case("gaussian", (3, 256, 6, 3), "causal", scale=0.2, seed=4)
COUNT_DOC, DECOY_DOC = Case("counting", DOC, "dense", seed=1), Case("decoy", DOC, "dense", seed=3)


def _edit(case, b, h, rows, keys, value):
    B, _, Hq, _ = case.shape
    m = case_mask(case).expand(B, Hq, -1, -1).clone()
    m[b, h, rows, keys] = value
    return m


def _scaled_head(h, f):
    def fn(delta):
        delta = delta.clone()
        delta[:, h] *= f
        return delta
    return fn


def _zero_rows(rows):
    def fn(delta):
        delta = delta.clone()
        delta[:, :, rows] = 0
        return delta
    return fn


R, LAST = slice(416, 448), slice(480, 512)  # one 32-row wave; the last 32-query tile
ALL = slice(None)


def _mask(which, *edit):
    return lambda c: {which: _edit(c, *edit)}


LEAK = "row 400 of head 5 sees key 401"
DROP = "row 450 of head 2 drops key 0"
SKIP = "rows 416..447 of head 3 skip key tile 128..191"
DOCLEAK = "doc row 130 of head 3 sees key 128 = doc_start - 1"
WRONG_KV = dict(kv_of=torch.tensor([0, 0, 0, 0, 1, 0, 1, 1]))
# (fault, the input kind that catches it, the model's fault arguments, output, index of the touched
# row / key in that output: [b, h, row] for lse2 / delta, [b, row, h] for the others)
MUTANTS = [
    (LEAK + " (forward)", COUNT, _mask("fwd_mask", 0, 5, 400, 401, True), "lse2", (0, 5, 400)),
    (LEAK + " (forward)", DECOY, _mask("fwd_mask", 0, 5, 400, 401, True), "o", (0, 400, 5)),
    (LEAK + " (dQ pass)", DECOY, _mask("dq_mask", 0, 5, 400, 401, True), "dq", (0, 400, 5)),
    (LEAK + " (dK/dV pass)", DECOY, _mask("dkdv_mask", 0, 5, 400, 401, True), "dv", (0, 401, 1)),
    (LEAK + " (dK/dV pass)", DECOY, _mask("dkdv_mask", 0, 5, 400, 401, True), "dk", (0, 401, 1)),
    (DROP, COUNT, _mask("fwd_mask", 0, 2, 450, 0, False), "lse2", (0, 2, 450)),
    (DROP, FIRST, _mask("fwd_mask", 0, 2, 450, 0, False), "o", (0, 450, 2)),
    (SKIP, COUNT, _mask("fwd_mask", 0, 3, R, slice(128, 192), False), "lse2", (0, 3, R)),
    (SKIP, COUNT, _mask("fwd_mask", 0, 3, R, slice(128, 192), False), "o", (0, R, 3)),
    ("key block 384..511 skips query tile 480..511 of head 6 (dK/dV pass)", DIAG,
     _mask("dkdv_mask", 0, 6, LAST, slice(384, 512), False), "dv", (0, LAST, 1)),
    ("delta * 1.02 for head 4", DIAG, lambda c: dict(delta_fn=_scaled_head(4, 1.02)), "delta", (0, 4)),
    ("delta = 0 for rows 32..63", GAUSS, lambda c: dict(delta_fn=_zero_rows(slice(32, 64))), "delta",
     (0, ALL, slice(32, 64))),
    ("delta = 0 for rows 32..63", GAUSS, lambda c: dict(delta_fn=_zero_rows(slice(32, 64))), "dq", (0, slice(32, 64))),
    ("dq * scale * log2(e) instead of scale, scale = 0.2", SCALED, lambda c: dict(dq_scale=0.2 * LOG2E), "dq", ()),
    ("head 5 reads kv head 0 (its own is 1)", GAUSS, lambda c: WRONG_KV, "o", (0, ALL, 5)),
    ("head 5 reads kv head 0 (its own is 1)", GAUSS, lambda c: WRONG_KV, "dq", (0, ALL, 5)),
    (DOCLEAK + " (forward)", COUNT_DOC, _mask("fwd_mask", 0, 3, 130, 128, True), "lse2", (0, 3, 130)),
    (DOCLEAK + " (forward)", DECOY_DOC, _mask("fwd_mask", 0, 3, 130, 128, True), "o", (0, 130, 3)),
    (DOCLEAK + " (dQ pass)", DECOY_DOC, _mask("dq_mask", 0, 3, 130, 128, True), "dq", (0, 130, 3)),
    (DOCLEAK + " (dK/dV pass)", DECOY_DOC, _mask("dkdv_mask", 0, 3, 130, 128, True), "dv", (0, 128, 0)),
]


@pytest.mark.parametrize("fault,case,kwargs,name,where", MUTANTS,
                         ids=[f"{m[0]}|{m[1].kind}{'-' + m[1].pmap if m[1].pmap else ''}|{m[3]}" for m in MUTANTS])
def test_mutant_breaks_a_bound_where_it_acts(fault, case, kwargs, name, where):
    assert case in ALL_CASES  # the GPU module runs this very case
    ref = case_reference(case)
    got = rounding_model(*case_inputs(case), case.scale, case_mask(case), **kwargs(case))
    r, _ = worst_at(got[name][where], ref[name][where], ref["b_" + name][where])
    print(f"{fault}: caught by {case_id(case)} on {name} at ratio {r:.3g}")
    assert r > 1, (fault, r)


def test_whole_tensor_criterion_misses_the_leak():
    """The faults above at the criterion of test_attention_gpu.py (relative norm < 4e-3 / 6e-3): a key
    leaked to one row of Gaussian inputs stays an order of magnitude below it."""
    c = GAUSS
    ref = case_reference(c)
    for kw, name, limit in ((dict(fwd_mask=_edit(c, 0, 5, 400, 401, True)), "o", 4e-3),
                            (dict(dq_mask=_edit(c, 0, 5, 400, 401, True)), "dq", 6e-3)):
        got = rounding_model(*case_inputs(c), c.scale, case_mask(c), **kw)
        rel = float((got[name] - ref[name]).norm() / ref[name].norm())
        assert rel < limit, (name, rel)


def test_visibility_masks():
    ds = doc_start_rows(256, 2, "mixed")
    m = visibility(256, True, ds)
    assert m.shape == (2, 1, 256, 256) and bool(m[0, 0, 130, 129]) and not bool(m[0, 0, 130, 128])
    assert bool(m[1, 0, 130, 0]) and not bool(m[1, 0, 130, 131])
    assert int(visibility(128, True).sum()) == 128 * 129 // 2 and bool(visibility(128, False).all())
