#!/usr/bin/env python3
"""Attention kernel timing at Llama-3 shapes: HIP flash attention vs the library SDPA.

usage: python tools/attn_bench.py [--batch 4] [--seq 2048] [--hq 32] [--hkv 8] [--head-dim 128] [--reps 20]
                                  [--json-out F] [--doc-len-mean N]

--head-dim 64 is the Llama-3.2 1B shape (the 4-wave kernels of attention_d64.hip).

Times forward alone and forward+backward (CUDA events, median of reps); FLOPs count the
causal half: fwd 2 products, bwd 5 products (the HIP backward does 7: see attention.hip).

--doc-len-mean N packs documents of mean length N into every sequence (boundaries drawn per
position with probability 1/N from a fixed seed) and also times, on the same tensors, the HIP
document path (the attn_doc_* kernels of attention.hip: "hip_doc"), that path with one document
per sequence ("hip_doc_one": the price of its plain 4-wave passes) and SDPA with the dense boolean
mask ("sdpa_doc").  "visited_tile_fraction" is the share of the causal (query block, key tile)
pairs the document path's forward / dQ passes visit, and of the (key block, query tile) pairs its
dK/dV pass visits, counted on the host from doc_start.
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def visited_fractions(doc_start):
    """(forward / dQ, dK/dV) visited share of the plain causal passes' tiles; doc_start [B, S] on the host."""
    from pytorch_operator_amd.ops.attention import doc_ends
    BM, BN, BK, QT = 128, 64, 128, 32  # attention_common.h
    ds, de = doc_start.long(), doc_ends(doc_start).long()
    S = ds.shape[1]
    qb = torch.arange(S // BM)
    fwd_all = ((qb * BM + BM) // BN).sum() * ds.shape[0]
    fwd = ((qb * BM + BM) // BN - torch.minimum(ds[:, ::BM], qb * BM) // BN).sum()
    kb = torch.arange(S // BK)
    qt0 = kb * BK // QT
    bwd_all = (S // QT - qt0).sum() * ds.shape[0]
    qtend = ((de[:, BK - 1::BK] + QT - 1) // QT).clamp(max=S // QT)
    bwd = (torch.maximum(qtend, qt0 + 1) - qt0).sum()
    return float(fwd) / float(fwd_all), float(bwd) / float(bwd_all)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--seq", type=int, default=2048)
    p.add_argument("--hq", type=int, default=32)
    p.add_argument("--hkv", type=int, default=8)
    p.add_argument("--head-dim", type=int, default=128)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--causal", type=int, default=1)
    p.add_argument("--impl", default="hip,sdpa")
    p.add_argument("--doc-len-mean", type=int, default=0)
    p.add_argument("--json-out", default=None)
    a = p.parse_args()
    from pytorch_operator_amd.ops.attention import flash_attention, sdpa_bshd, validate_doc_start
    B, S, Hq, Hkv, D = a.batch, a.seq, a.hq, a.hkv, a.head_dim
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    k = torch.randn(B, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    v = torch.randn(B, S, Hkv, D, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    do = torch.randn(B, S, Hq, D, device="cuda", generator=g).to(torch.bfloat16)
    frac = 0.5 if a.causal else 1.0
    fwd_flop = 4 * B * Hq * S * S * D * frac
    res = {"shape": {"B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "causal": bool(a.causal)}}
    impls = [("hip", flash_attention), ("sdpa", sdpa_bshd)]
    doc_frac = frac
    if a.doc_len_mean > 0:
        if not a.causal:
            raise SystemExit("--doc-len-mean needs --causal 1")
        cut = torch.rand(B, S, generator=torch.Generator().manual_seed(0)) < 1.0 / a.doc_len_mean
        cut[:, 0] = False
        idx = torch.arange(S).expand(B, S)
        ds_host = torch.cummax(torch.where(cut, idx, torch.zeros_like(idx)), dim=1).values.to(torch.int32)
        validate_doc_start(ds_host)
        ds, one = ds_host.cuda(), torch.zeros(B, S, dtype=torch.int32, device="cuda")
        f_fwd, f_bwd = visited_fractions(ds_host)
        res["doc"] = {"doc_len_mean": a.doc_len_mean, "docs_per_seq": round(float(cut.sum()) / B + 1, 2),
                      "visited_tile_fraction": {"fwd_dq": round(f_fwd, 4), "dkdv": round(f_bwd, 4)}}
        # FLOPs of the document rows count the visible (query, key) pairs only
        doc_frac = float((idx - ds_host.long() + 1).sum()) / (B * S * S)
        res["doc"]["visible_pair_fraction"] = round(doc_frac, 4)
        print("doc", res["doc"], flush=True)
        impls += [("hip_doc", lambda q, k, v, c: flash_attention(q, k, v, c, doc_start=ds)),
                  ("hip_doc_one", lambda q, k, v, c: flash_attention(q, k, v, c, doc_start=one)),
                  ("sdpa_doc", lambda q, k, v, c: sdpa_bshd(q, k, v, c, doc_start=ds))]
    want = a.impl.split(",")
    for name, fn in impls:
        if name.replace("_doc_one", "").replace("_doc", "") not in want:
            continue
        with torch.no_grad():
            fn(q, k, v, bool(a.causal))
            t_f = timed(lambda: fn(q, k, v, bool(a.causal)), a.reps)

        def fb():
            o = fn(q, k, v, bool(a.causal))
            o.backward(do)
        fb()
        t_fb = timed(fb, a.reps)
        t_b = t_fb - t_f
        flop = fwd_flop * (doc_frac / frac if name in ("hip_doc", "sdpa_doc") else 1.0)
        res[name] = {"fwd_us": round(t_f, 1), "fwd_bwd_us": round(t_fb, 1), "bwd_us": round(t_b, 1),
                     "fwd_tflops": round(flop / t_f / 1e6, 1),
                     "bwd_tflops": round(2.5 * flop / t_b / 1e6, 1)}
        print(name, res[name], flush=True)
        q.grad = k.grad = v.grad = None
    if "hip" in res and "sdpa" in res:
        res["speedup_fwd_bwd"] = round(res["sdpa"]["fwd_bwd_us"] / res["hip"]["fwd_bwd_us"], 2)
    if "hip_doc" in res:
        # times of the document path over: itself with one document, the default causal kernels
        # (which ignore the documents), SDPA with the dense mask
        for other in ("hip_doc_one", "hip", "sdpa_doc"):
            if other in res:
                res["doc"][f"fwd_bwd_vs_{other}"] = round(res["hip_doc"]["fwd_bwd_us"] / res[other]["fwd_bwd_us"], 3)
                res["doc"][f"fwd_vs_{other}"] = round(res["hip_doc"]["fwd_us"] / res[other]["fwd_us"], 3)
    print(json.dumps(res))
    if a.json_out:
        Path(a.json_out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
