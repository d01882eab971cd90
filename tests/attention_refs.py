"""fp64 reference, derived element-wise error bounds, a rounding model and input builders for the
flash-attention kernels (csrc/kernels/attention.hip, attention_bwd_pipe.hip).  Plain PyTorch on
the CPU: tests/test_attention_refs_cpu.py proves the reference equal to fp64 autograd and shows
that the bounds admit a correctly rounding kernel and reject wrong ones;
tests/test_attention_rows_gpu.py holds the kernels to them, row by row.

Tensors are laid out as the kernels see them: q, o, dO, dq [B, S, Hq, D]; k, v, dk, dv
[B, S, Hkv, D]; lse2, delta [B, Hq, S].  A mask is a boolean [B or 1, 1 or Hq, S, S], True where
query i may see key j.
"""
import collections
import functools
import math

import torch

from llm_refs import BF16_O, FP32_E

LOG2E = 1.4426950408889634
# Absolute error of the device log2f: measured against fp64 log2 over the exact integer l of the
# counting inputs by tests/test_attention_rows_gpu.py (9.466e-7 at l = 265, see
# test_counting_inputs_pin_the_key_count) and rounded up to the next power of two.
LOG2_HW = 2.0 ** -20

GAMMA = 2.0  # one-hot inputs: q_i = GAMMA * k_target (exact in bf16)
DENSE = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)  # test_attention_doc_gpu.py's boundaries
OUTPUTS = ("o", "lse2", "delta", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------ masks
def doc_start_rows(S, B, layout):
    """int32 [B, S] doc_start of test_attention_doc_gpu.py's layouts: "dense" (DENSE boundaries in
    every batch row), "last" (the last token is its own document), "mixed" (dense, then single
    documents)."""
    def row(bounds):
        out, cur, bs = [], 0, {b for b in bounds if 0 < b < S}
        for i in range(S):
            cur = i if i in bs else cur
            out.append(cur)
        return out
    rows = {"dense": [row(DENSE)] * B, "last": [row((S - 1,))] * B,
            "mixed": [row(DENSE)] + [row(())] * (B - 1)}[layout]
    return torch.tensor(rows, dtype=torch.int32)


def visibility(S, causal=True, doc_start=None):
    """bool [B or 1, 1, S, S]: full, causal (j <= i) or document (doc_start[b, i] <= j <= i)."""
    j = torch.arange(S)
    if doc_start is not None:
        ds = doc_start.to(torch.int64)
        return ((j.view(1, 1, S) <= j.view(1, S, 1)) & (j.view(1, 1, S) >= ds.view(-1, S, 1))).unsqueeze(1)
    m = (j.view(1, S) <= j.view(S, 1)) if causal else torch.ones(S, S, dtype=torch.bool)
    return m.view(1, 1, S, S)


# ------------------------------------------------------------------- the math, written once
def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def _f32(x):
    return x.float().double()


def _same(x):
    return x


def _run(q, k, v, do, scale, fwd_mask, dq_mask, dkdv_mask, kv_of, rnd, delta_fn=None, dq_scale=None):
    """Forward, dQ pass and dK/dV pass in fp64, the way the kernels split the work: the forward
    keeps lse2, the backward recomputes P from it, the dQ pass computes delta from the stored o.
    rnd: insert the kernels' roundings (rounding_model) or none (attention_fp64)."""
    r16, r32 = (_bf16, _f32) if rnd else (_same, _same)
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    qh, doh = q.double().transpose(1, 2), do.double().transpose(1, 2)           # [B, Hq, S, D]
    kh, vh = k.double()[:, :, kv_of].transpose(1, 2), v.double()[:, :, kv_of].transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale                                      # natural-log units
    sf = s.masked_fill(~fwd_mask, -math.inf)
    m = sf.amax(-1, keepdim=True)
    p = torch.exp(sf - m)
    l = p.sum(-1, keepdim=True)                                                  # of the unrounded p
    o = r16((r16(p) @ vh) / l)
    lse2 = r32((m + l.log()) * LOG2E).squeeze(-1)
    delta = r32((doh * o).sum(-1))
    if delta_fn is not None:
        delta = delta_fn(delta)
    T = doh @ vh.transpose(-1, -2) - delta.unsqueeze(-1)                         # dP - delta
    pb = torch.exp(s - lse2.unsqueeze(-1) / LOG2E)
    pq = pb.masked_fill(~dq_mask, 0.0)
    dq = r16((scale if dq_scale is None else dq_scale) * (r16(pq * T) @ kh))
    pk = pb.masked_fill(~dkdv_mask, 0.0)
    fold = lambda x: torch.zeros(B, Hkv, S, x.shape[-1], dtype=torch.float64).index_add_(1, kv_of, x)  # noqa: E731
    dv = r16(fold(r16(pk).transpose(-1, -2) @ doh))
    dk = r16(scale * fold(r16(pk * T).transpose(-1, -2) @ qh))
    out = dict(o=o.transpose(1, 2), lse2=lse2, delta=delta, dq=dq.transpose(1, 2), dk=dk.transpose(1, 2),
               dv=dv.transpose(1, 2))
    return out, dict(qh=qh, kh=kh, vh=vh, doh=doh, p=pq, dS=pq * T, fold=fold)


def _kv_of(Hq, Hkv):
    return torch.arange(Hq) // (Hq // Hkv)


def attention_fp64(q, k, v, do, scale, mask):
    """o, lse2 (log2 units), delta = rowsum(dO * O), dq, dk, dv in fp64 for GQA attention under a
    boolean visibility mask, the magnitude sums the bounds are made of, and the bounds ("b_" + name).

    Where the kernels round, and what each rounding costs (o = BF16_O = 2^-8 per bf16 rounding;
    e = FP32_E = 1e-5 for a chain of fp32 operations; c = scale * log2(e)):
      scores    s_ij in an fp32 MFMA accumulator, x = fma(s, c, -m) and exp2: the exponent is off by
                at most e * (c * sum_d |q||k| + |m|), so p is off by the relative
                  rp_i = e * (1 + Amax_i + |lse2_i|),   Amax_i = max_j c * sum_d |q_id||k_jd|  (visible j);
      o         P is rounded to bf16 before P.V, l sums the unrounded p, o is rounded on store:
                  |o - o64| <= o |o64| + (1 + o) (o + 3 rp_i) PV,        PV = sum_j p |v_j|
                (3 rp: p, l and the accumulation);
      lse2      = m + log2(l), l relative (rp + e), the hardware log2 and the last add:
                  |lse2 - lse2_64| <= 3 rp_i + LOG2_HW;
      delta     the dQ pass sums dO * o over the STORED o, whose error is the bound above:
                  |delta - delta64| <= sum_d |dO_d| b_o_d + e DOO,       DOO = sum_d |dO||o|;
      backward  P is recomputed as exp2(s c - lse2) from the forward's fp32 lse2:
                  rpb_i = rp_i + b_lse2_i;
      dS        = P (dP - delta) in fp32 (dP = dO.V^T off by e * sum_d |dO_i||v_j| = e DV_ij), then bf16:
                  E_ij = (o + rpb_i) |dS_ij| + p_ij (b_delta_i + e DV_ij);
      dq        = scale * sum_j dS k_j, bf16 on store:
                  |dq - dq64| <= o |dq64| + (1 + o) scale (sum_j E_ij |k_j| + e DSK),   DSK = sum_j |dS||k_j|;
      dk        the same over queries i and the G query heads of the kv head, with |q_i|  (DSQ);
      dv        = sum_i bf16(P) dO_i:
                  |dv - dv64| <= o |dv64| + (1 + o) sum_i (o + rpb_i + e) p_ij |dO_i|     (PDO = sum_i p |dO_i|).
    fp32 chain behind e: the longest accumulator is dK/dV's at (1, 512, 8, 2), 4 heads x 512 queries
    at 16 per MFMA = 128 updates, plus the 8 of a d-contraction and the fma / exp2 / scale: under
    160 roundings of 2^-24 = 9.5e-6.  Masked probabilities are exact zeros and add nothing."""
    B, S, Hq, _ = q.shape
    kv_of = _kv_of(Hq, k.shape[2])
    out, x = _run(q, k, v, do, scale, mask, mask, mask, kv_of, rnd=False)
    qa, ka, va, da = x["qh"].abs(), x["kh"].abs(), x["vh"].abs(), x["doh"].abs()
    p, dS, fold = x["p"], x["dS"].abs(), x["fold"]
    o, lse2 = out["o"].transpose(1, 2), out["lse2"]
    c = scale * LOG2E
    amax = ((qa @ ka.transpose(-1, -2)) * c).masked_fill(~mask, 0.0).amax(-1)
    rp = FP32_E * (1 + amax + lse2.abs())
    pv = p @ va
    b_o = BF16_O * o.abs() + (1 + BF16_O) * (BF16_O + 3 * rp).unsqueeze(-1) * pv
    b_lse2 = 3 * rp + LOG2_HW
    doo = (da * o.abs()).sum(-1)
    b_delta = (da * b_o).sum(-1) + FP32_E * doo
    rpb = rp + b_lse2
    E = (BF16_O + rpb).unsqueeze(-1) * dS + p * (b_delta.unsqueeze(-1) + FP32_E * (da @ va.transpose(-1, -2)))
    dsk, dsq, pdo = dS @ ka, fold(dS.transpose(-1, -2) @ qa), fold(p.transpose(-1, -2) @ da)
    t = lambda x: x.transpose(1, 2)  # noqa: E731
    out.update(
        pv=t(pv), doo=doo, dsk=t(dsk), dsq=t(dsq), pdo=t(pdo), amax=amax, p=p,
        b_o=t(b_o), b_lse2=b_lse2, b_delta=b_delta,
        b_dq=BF16_O * out["dq"].abs() + (1 + BF16_O) * scale * t(E @ ka + FP32_E * dsk),
        b_dk=BF16_O * out["dk"].abs() + (1 + BF16_O) * scale * t(fold(E.transpose(-1, -2) @ qa) + FP32_E * dsq),
        b_dv=BF16_O * out["dv"].abs() + (1 + BF16_O) * t(
            fold(((BF16_O + rpb + FP32_E).unsqueeze(-1) * p).transpose(-1, -2) @ da)))
    return out


def rounding_model(q, k, v, do, scale, mask, fwd_mask=None, dq_mask=None, dkdv_mask=None, kv_of=None,
                   delta_fn=None, dq_scale=None):
    """attention_fp64's math with bf16 roundings at the kernels' rounding points (P before P.V and
    dO^T.P, dS before the dQ / dK products, o / dq / dk / dv on store, delta from the rounded o, P
    recomputed from the fp32 lse2): what a correct kernel produces, up to fp32 effects.  The
    keyword arguments turn it into a wrong kernel: another mask in one pass, another kv head per
    query head, a transformed delta, another dq factor."""
    Hq = q.shape[2]
    full = lambda m: mask if m is None else m  # noqa: E731
    kv_of = _kv_of(Hq, k.shape[2]) if kv_of is None else kv_of
    out, _ = _run(q, k, v, do, scale, full(fwd_mask), full(dq_mask), full(dkdv_mask), kv_of, rnd=True,
                  delta_fn=delta_fn, dq_scale=dq_scale)
    return out


def worst_at(got, want, bound):
    """(max |got - want| / bound, its index); 0/0 counts as 0, err/0 and NaN as inf."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    at = int(ratio.argmax())
    return float(ratio.flatten()[at]), tuple(int(i) for i in torch.unravel_index(torch.tensor(at), ratio.shape))


def ratios(got, ref):
    """{output: (worst error / bound, index)} of a dict of outputs against attention_fp64's."""
    return {n: worst_at(got[n], ref[n], ref["b_" + n]) for n in OUTPUTS}


# ----------------------------------------------------------------------------------- inputs
# kind: "gaussian", "counting", "onehot" (pmap: "diag", "first", "tile", "tile-1", "reverse") or
# "decoy" (q_i = GAMMA * k of the first key row i may NOT see: i + 1, or doc_start[i] - 1 under a
# document mask; rows without one point at their first key).  mask: "causal", "full" or a doc layout.
Case = collections.namedtuple("Case", "kind shape mask scale pmap seed", defaults=(1 / math.sqrt(128), None, 0))


def case_id(c):
    return "-".join(str(x) for x in (c.kind, c.pmap, "x".join(map(str, c.shape)), c.mask, f"{c.scale:.3g}") if x)


def case_doc_start(c):
    return None if c.mask in ("causal", "full") else doc_start_rows(c.shape[1], c.shape[0], c.mask)


def case_mask(c):
    return visibility(c.shape[1], c.mask != "full", case_doc_start(c))


def target_keys(c):
    """int64 [B, S]: the key pi(i) a one-hot / decoy query row i is built from."""
    B, S = c.shape[:2]
    ds = case_doc_start(c)
    i = torch.arange(S).expand(B, S)
    lo = torch.zeros(B, S, dtype=torch.int64) if ds is None else ds.to(torch.int64)
    if c.kind == "decoy":
        past = (i + 1) if ds is None else (lo - 1)
        return torch.where((past >= 0) & (past < S), past, lo)
    t64 = i // 64 * 64
    pi = {"diag": i, "first": lo, "tile": torch.maximum(t64, lo), "reverse": S - 1 - i,
          "tile-1": torch.where(t64 - 1 >= lo, t64 - 1, torch.maximum(t64, lo))}[c.pmap]
    assert c.pmap == "reverse" or bool(((pi >= lo) & (pi <= i)).all())
    return pi


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """q, k, v, dO as bf16 CPU tensors, drawn from a seeded CPU generator and rounded to bf16, so a
    CPU test and a GPU test of one case see the same values.
      gaussian  unit q, k, v, dO;
      counting  q = 0: every score is exactly 0 and every visible p exactly 1, so l is the exact
                number of visible keys, lse2 = log2(count) and o the plain mean of the visible v rows;
      onehot    k entries +-1, q_i = GAMMA * k_pi(i): the target key carries >= 0.999 of row i, so
                o_i ~ v_pi(i) and dv_j sums the dO rows that chose j; dO_i = |gaussian| * sign(v_pi(i)), so
                that delta_i = sum_d |dO||o| up to 0.1 %: no cancellation hides a wrong delta;
      decoy     the one-hot construction aimed at a key the row must not see: a pass that lets it
                through gives it nearly all of the row."""
    B, S, Hq, Hkv = c.shape
    G = Hq // Hkv
    g = torch.Generator(device="cpu").manual_seed(1000 + c.seed)
    mk = lambda H: torch.randn(B, S, H, 128, generator=g)  # noqa: E731
    q, k, v, do = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    if c.kind == "counting":
        q = torch.zeros_like(q)
    elif c.kind in ("onehot", "decoy"):
        k = torch.where(k >= 0, 1.0, -1.0)
        idx = target_keys(c).view(B, S, 1, 1).expand(B, S, Hkv, 128)
        q = GAMMA * torch.gather(k, 1, idx).repeat_interleave(G, dim=2)
        if c.kind == "onehot":
            vt = torch.gather(v.to(torch.bfloat16).float(), 1, idx).repeat_interleave(G, dim=2)
            do = do.abs() * torch.where(vt >= 0, 1.0, -1.0)
    return tuple(t.to(torch.bfloat16).contiguous() for t in (q, k, v, do))


@functools.lru_cache(maxsize=None)
def case_reference(c):
    """attention_fp64 of a case, computed once and shared (callers must not modify it)."""
    return attention_fp64(*case_inputs(c), c.scale, case_mask(c))
