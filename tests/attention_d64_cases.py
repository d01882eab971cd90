"""Inputs and case lists for the head-dim-64 flash-attention kernels (csrc/kernels/attention_d64.hip),
on top of tests/attention_refs.py: its fp64 reference, bounds and rounding model are head-dim
generic, only its input builder is written for 128.  tests/test_attention_d64_cpu.py runs the
rounding model through every case below, tests/test_attention_d64_gpu.py the kernels.

One-hot and decoy queries are GAIN = 3 times the target key (attention_refs.GAMMA = 2 at D = 128):
with 64 entries of +-1 a gain of 2 leaves up to 2.15e-3 of a row outside its target key in the fp64
reference ((1, 512, 8, 2), "reverse"), over the 1e-3 the one-hot tests allow; 3 leaves 6.1e-5, and
3 * +-1 is exact in bf16.
"""
import functools
import math

import torch

from attention_refs import Case, attention_fp64, case_mask, target_keys

D64 = 64
SCALE64 = 1 / math.sqrt(D64)
GAIN = 3.0


def case64(kind, shape, mask, scale=SCALE64, pmap=None, seed=0):
    return Case(kind, shape, mask, scale, pmap, seed)


SHAPES = [  # B, S, Hq, Hkv
    (1, 128, 2, 2),   # one block everywhere
    (3, 256, 6, 3),   # two query and key blocks; B and Hkv no powers of two; G = 2
    (2, 384, 3, 1),   # three query and key blocks; G = 3
    (1, 512, 8, 2),   # four blocks, heaviest-first order under the causal mask; G = 4
]
DOC_SHAPES = [(1, 128, 2, 2), (2, 256, 8, 2), (1, 384, 4, 1)]
DOC_LAYOUTS = [(s, lay) for s in DOC_SHAPES for lay in ("dense", "last", "mixed")]
ONEHOT_SHAPES = [(3, 256, 6, 3), (1, 512, 8, 2)]
MAPS = ("diag", "first", "tile", "tile-1")  # the target key of row i: see attention_refs.target_keys

GAUSSIAN = [case64("gaussian", s, m) for s in SHAPES for m in ("causal", "full")]
GAUSSIAN_DOC = [case64("gaussian", s, lay) for s, lay in DOC_LAYOUTS]
COUNTING = [case64("counting", s, m, seed=1) for s in SHAPES for m in ("causal", "full")]
COUNTING_DOC = [case64("counting", s, lay, seed=1) for s, lay in DOC_LAYOUTS]
ONEHOT = ([case64("onehot", s, "causal", pmap=p, seed=2) for s in ONEHOT_SHAPES for p in MAPS]
          + [case64("onehot", s, "full", pmap="reverse", seed=2) for s in ONEHOT_SHAPES])
DECOY = [case64("decoy", s, "causal", seed=3) for s in ONEHOT_SHAPES]
DECOY_DOC = [case64("decoy", (2, 256, 8, 2), lay, seed=3) for lay in ("dense", "mixed")]
SCALES = [case64("gaussian", (3, 256, 6, 3), "causal", scale=sc, seed=4) for sc in (0.05, 0.2)]
PLAIN_CASES = GAUSSIAN + COUNTING + ONEHOT + DECOY + SCALES   # pto_attn_fwd / pto_attn_bwd
DOC_CASES = GAUSSIAN_DOC + COUNTING_DOC + DECOY_DOC           # pto_attn_doc_fwd / pto_attn_doc_bwd
ALL_CASES = PLAIN_CASES + DOC_CASES


@functools.lru_cache(maxsize=None)
def case_inputs64(c):
    """attention_refs.case_inputs at head dim 64: q, k, v, dO as bf16 CPU tensors from a seeded CPU
    generator, so a CPU test and a GPU test of one case see the same values.  The kinds are the
    same (gaussian, counting: q = 0, onehot: q_i = GAIN * k_pi(i) with k entries +-1 and dO_i =
    |gaussian| * sign(v_pi(i)), decoy: the one-hot construction aimed at a key row i must not see)."""
    B, S, Hq, Hkv = c.shape
    G = Hq // Hkv
    g = torch.Generator(device="cpu").manual_seed(6400 + c.seed)
    mk = lambda H: torch.randn(B, S, H, D64, generator=g)  # noqa: E731
    q, k, v, do = mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)
    if c.kind == "counting":
        q = torch.zeros_like(q)
    elif c.kind in ("onehot", "decoy"):
        k = torch.where(k >= 0, 1.0, -1.0)
        idx = target_keys(c).view(B, S, 1, 1).expand(B, S, Hkv, D64)
        q = GAIN * torch.gather(k, 1, idx).repeat_interleave(G, dim=2)
        if c.kind == "onehot":
            vt = torch.gather(v.to(torch.bfloat16).float(), 1, idx).repeat_interleave(G, dim=2)
            do = do.abs() * torch.where(vt >= 0, 1.0, -1.0)
    return tuple(t.to(torch.bfloat16).contiguous() for t in (q, k, v, do))


@functools.lru_cache(maxsize=None)
def case_reference64(c):
    """attention_fp64 of a case, computed once and shared (callers must not modify it)."""
    return attention_fp64(*case_inputs64(c), c.scale, case_mask(c))


def onehot_rest(c):
    """[B, S, Hq]: the share of each row the fp64 reference leaves outside the row's target key."""
    B, S, Hq, _ = c.shape
    p = case_reference64(c)["p"]
    pi = target_keys(c)
    return 1 - torch.gather(p, 3, pi.view(B, 1, S, 1).expand(B, Hq, S, 1)).squeeze(-1).transpose(1, 2)
