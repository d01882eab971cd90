#!/usr/bin/env python3
"""Decode attention timing at Llama-3 shapes: the HIP kernels vs the library path over the same cache.

usage: python tools/decode_bench.py [--batch 1,8] [--keys 512,2048,8192] [--head-dim 64,128] [--hq 32] [--hkv 8]
                                    [--reps 200] [--json-out F]
       python tools/decode_bench.py --e2e [--model llama3-1b,llama3-8b] [--batch 1,8] [--prompt 128] [--tokens 128]
                                    [--decode-linear lib,hip,hip-fp8]
       python tools/decode_bench.py --queries 2,4 [--batch 1,8] [--keys 512,2048,8192] [--head-dim 64,128]
       python tools/decode_bench.py --e2e --queries 2,4 [--model llama3-1b,llama3-8b] [--batch 1,2,4,8] [--prompt 128]
       python tools/decode_bench.py --queries 1,2,4 --kv fp8 [--e2e] [...]
       python tools/decode_bench.py --linear [--rows 1,8,16] [--reps 200] [--decode-linear hip-fp4,hip-fp8,hip,lib]
                                             [--fp8-tiles 1,2,4]

Kernel mode: one ``decode_attention`` call per cache layer, ``--reps`` calls back to back between two
device events, every row at the full length n.  The calls walk over enough layers that K + V of all
of them exceed 512 MiB (at most 64 layers), as the layers of a model do: "footprint_mb" says how much
that is -- below 256 MB the caches stay in the Infinity Cache and the rate is not an HBM rate.  "hip"
and "sdpa" (``impl="sdpa"``: zero the rows past the lengths, then SDPA with a length mask) alternate,
two runs each; "sdpa_raw" is SDPA with the mask alone, without the pass that makes NaN rows safe.
"gbps" = K + V bytes of the valid rows / time.  "*_host_us" is the host's clock around the loop that
issues the calls, per call, taken before any wait: where it equals the device figure, the calls are
bound by the host issuing them, not by the kernels.

--e2e: ``Llama.generate`` tokens/s (bf16 matmul weights, random init), HIP against SDPA decode attention,
alternating, two runs each; the prefill runs the HIP flash attention both times.  With --decode-linear lib,hip
the attention stays on the HIP kernels and the decode step's projections change sides instead (the library
GEMMs + a SwiGLU launch against ``ops.skinny.linear_rows``), each run checked by ``TNLinear.rows_calls``.

--kv fp8: the e4m3 cache of ``csrc/kernels/decode_attention_fp8.hip`` against the bf16 cache.  Kernel mode: "fp8"
and "hip" (the bf16 kernel) alternate, two runs each, over caches of equal shape; each side's "gbps" counts its own
bytes, the fp8 side's scales included, and the layers are sized so that the e4m3 caches alone exceed 512 MiB.
--e2e --kv fp8: ``Llama.generate`` with ``kv_dtype=torch.float8_e4m3fn`` against the bf16 cache, with the peak of
``torch.cuda.max_memory_allocated`` per side ("*_peak_mb").

--queries S,..: the multi-query kernel of ``csrc/kernels/decode_attention_multi.hip``.  Kernel mode: one
``attend_rows`` call over S queries per sequence ("rows") against S back-to-back ``decode_attention`` calls over the
same cache ("single", the S calls counted as one) and against ``attend_rows(impl="sdpa")`` ("sdpa"), alternating, two
runs each, with the layers and the host's issue time as above; "rows_vs_single" is the ratio of the best device
times.  --e2e --queries: one ``Llama.decode_steps`` over S tokens per sequence against one ``decode_step``, ms per
step on a cache of --prompt rows (the lengths are put back before every step), for every --batch with B * S <= 16,
projections by --decode-linear's first side (default hip); "steps_vs_step" is what S tokens cost relative to one.
That ratio is the result: the models are randomly initialised, so how many drafted tokens a target would accept,
and with it any speculative tokens/s, means nothing here and is not reported.

--queries S,.. --kv fp8: the e4m3 multi-query kernel of ``csrc/kernels/decode_attention_multi_fp8.hip``.  Kernel
mode, three sides alternating, two runs each: one e4m3 ``attend_rows`` call ("rows8"), S back-to-back e4m3
``decode_attention`` calls ("single8") and the bf16 ``attend_rows`` call over a bf16 cache of the same shape
("rows"); layers as with --kv fp8 alone, "rows8_gbps" counts the e4m3 side's own bytes, scales included;
"rows8_vs_single8" and "rows8_vs_rows" are ratios of the best device times.  With --e2e: ``decode_steps`` against
``decode_step`` as above, both on an e4m3 cache.

--linear: ``ops.skinny.linear_rows`` against ``F.linear`` (+ ``swiglu_packed`` for w13) on the same tensors, at
the five projection shapes of llama3-8b and llama3-1b and M = --rows.  The calls cycle through enough copies
of the weight to exceed 512 MiB, so every call streams its weight from HBM ("gbps" = bytes of W / time, "peak"
= that over 8 TB/s); sides alternate, two runs each, with the host's issue time beside the device's as above.
With hip-fp8 among --decode-linear, ``ops.skinny.linear_rows_fp8`` on ``quantize_rows`` of the same weights is a
third side ("fp8": its "gbps" counts its own, one-byte weights), and the copies are sized so that the e4m3 ones
alone exceed 512 MiB.  hip-fp4 adds ``ops.skinny.linear_rows_fp4`` on ``quantize_rows_fp4`` of the same weights in
the same way ("fp4": its "gbps" counts its codes and scale bytes, 17 / 32 of a byte a weight).  --fp8-tiles adds one side per forced accumulator count ("fp8_t1", ...), where "fp8" is the
library's own choice ("tiles").

--linear --fuse-norm: each call of ``csrc/kernels/skinny_gemm_fused.hip`` ("fused") against the launches it replaces
("unfused"): see ``fused_linear_bench``.  --e2e --fuse-norm [--decode-linear hip,hip-fp8]: ``Llama.generate`` with
``TNLinear.rows_fuse_norm`` off and on, alternating, two runs each, every run checked by ``TNLinear.rows_calls``.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, layers, reps):
    """(device, host) us per call: ``reps`` calls over the layers in turn, between two events; the host
    figure is its clock around the issuing loop alone, before any wait for the device."""
    for i in range(min(layers, reps)):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i % layers)
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps


def kernel_fp8_bench(a):
    from pytorch_operator_amd.ops.decode import FP8, KVCache, decode_attention, quantize_kv
    out = []
    for D in a.head_dim:
        for B in a.batch:
            for n in a.keys:
                own = {"hip": 2 * B * n * a.hkv * D * 2, "fp8": 2 * B * n * a.hkv * (D + 4)}
                L = max(1, min(64, -(-(512 << 20) // own["fp8"])))
                cache, cache8 = KVCache(L, B, n, a.hkv, D, torch.bfloat16, "cuda"), KVCache(L, B, n, a.hkv, D, FP8, "cuda")
                for i in range(L):
                    cache.k[i].normal_()
                    cache.v[i].normal_()
                    quantize_kv(cache.k[i], cache.v[i], cache8.k[i], cache8.v[i], cache8.k_scale[i], cache8.v_scale[i])
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                q = torch.randn(B, a.hq, D, device="cuda").to(torch.bfloat16)
                fns = {"hip": lambda i: decode_attention(q, cache.k[i], cache.v[i], lens),
                       "fp8": lambda i: decode_attention(q, cache8.k[i], cache8.v[i], lens, k_scale=cache8.k_scale[i],
                                                         v_scale=cache8.v_scale[i])}
                row = {"B": B, "n": n, "Hq": a.hq, "Hkv": a.hkv, "D": D, "layers": L,
                       "footprint_mb": round(L * own["hip"] / 1e6, 1), "fp8_footprint_mb": round(L * own["fp8"] / 1e6, 1)}
                for name in ("fp8", "hip", "fp8", "hip"):
                    dev_us, host_us = timed(fns[name], L, a.reps)
                    row.setdefault(name + "_us", []).append(round(dev_us, 2))
                    row.setdefault(name + "_host_us", []).append(round(host_us, 2))
                for name in ("fp8", "hip"):
                    row[name + "_gbps"] = round(own[name] / min(row[name + "_us"]) / 1e3, 1)
                print(json.dumps(row), flush=True)
                out.append(row)
                del cache, cache8
    return out


def kernel_bench(a):
    from pytorch_operator_amd.ops.decode import KVCache, decode_attention
    out = []
    for D in a.head_dim:
        for B in a.batch:
            for n in a.keys:
                per_layer = 2 * B * n * a.hkv * D * 2
                L = max(1, min(64, -(-(512 << 20) // per_layer)))
                cache = KVCache(L, B, n, a.hkv, D, torch.bfloat16, "cuda")
                cache.k.normal_()
                cache.v.normal_()
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                q = torch.randn(B, a.hq, D, device="cuda").to(torch.bfloat16)
                mask = torch.ones(B, 1, 1, n, dtype=torch.bool, device="cuda")

                def raw(i):
                    return F.scaled_dot_product_attention(q.view(B, a.hkv, a.hq // a.hkv, D),
                                                          cache.k[i].transpose(1, 2), cache.v[i].transpose(1, 2),
                                                          attn_mask=mask)
                fns = {"hip": lambda i: decode_attention(q, cache.k[i], cache.v[i], lens),
                       "sdpa": lambda i: decode_attention(q, cache.k[i], cache.v[i], lens, impl="sdpa"),
                       "sdpa_raw": raw}
                row = {"B": B, "n": n, "Hq": a.hq, "Hkv": a.hkv, "D": D, "layers": L,
                       "footprint_mb": round(L * per_layer / 1e6, 1)}
                for name in ("hip", "sdpa", "hip", "sdpa", "sdpa_raw"):
                    dev_us, host_us = timed(fns[name], L, a.reps)
                    row.setdefault(name + "_us", []).append(round(dev_us, 2))
                    row.setdefault(name + "_host_us", []).append(round(host_us, 2))
                for name in ("hip", "sdpa", "sdpa_raw"):
                    row[name + "_gbps"] = round(per_layer / min(row[name + "_us"]) / 1e3, 1)
                print(json.dumps(row), flush=True)
                out.append(row)
                del cache
    return out


def queries_bench(a):
    from pytorch_operator_amd.ops.decode import KVCache, attend_rows, decode_attention
    out = []
    for D in a.head_dim:
        for B in a.batch:
            for n in a.keys:
                per_layer = 2 * B * n * a.hkv * D * 2
                L = max(1, min(64, -(-(512 << 20) // per_layer)))
                cache = KVCache(L, B, n, a.hkv, D, torch.bfloat16, "cuda")
                cache.k.normal_()
                cache.v.normal_()
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                for S in a.queries:
                    if S * (a.hq // a.hkv) > 16:
                        continue
                    q = torch.randn(B, S, a.hq, D, device="cuda").to(torch.bfloat16)
                    qs = [q[:, s].contiguous() for s in range(S)]

                    def single(i):
                        for s in range(S):
                            decode_attention(qs[s], cache.k[i], cache.v[i], lens)
                    fns = {"rows": lambda i: attend_rows(q, cache.k[i], cache.v[i], lens), "single": single,
                           "sdpa": lambda i: attend_rows(q, cache.k[i], cache.v[i], lens, impl="sdpa")}
                    row = {"B": B, "n": n, "S": S, "Hq": a.hq, "Hkv": a.hkv, "D": D, "layers": L,
                           "footprint_mb": round(L * per_layer / 1e6, 1)}
                    for name in ("rows", "single", "sdpa") * 2:
                        dev_us, host_us = timed(fns[name], L, a.reps)
                        row.setdefault(name + "_us", []).append(round(dev_us, 2))
                        row.setdefault(name + "_host_us", []).append(round(host_us, 2))
                    row["rows_gbps"] = round(per_layer / min(row["rows_us"]) / 1e3, 1)
                    row["rows_vs_single"] = round(min(row["rows_us"]) / min(row["single_us"]), 3)
                    print(json.dumps(row), flush=True)
                    out.append(row)
                del cache
    return out


def queries_fp8_bench(a):
    from pytorch_operator_amd.ops.decode import FP8, KVCache, attend_rows, decode_attention, quantize_kv
    out = []
    for D in a.head_dim:
        for B in a.batch:
            for n in a.keys:
                own = {"rows": 2 * B * n * a.hkv * D * 2, "rows8": 2 * B * n * a.hkv * (D + 4)}
                L = max(1, min(64, -(-(512 << 20) // own["rows8"])))
                cache, cache8 = KVCache(L, B, n, a.hkv, D, torch.bfloat16, "cuda"), KVCache(L, B, n, a.hkv, D, FP8, "cuda")
                for i in range(L):
                    cache.k[i].normal_()
                    cache.v[i].normal_()
                    quantize_kv(cache.k[i], cache.v[i], cache8.k[i], cache8.v[i], cache8.k_scale[i], cache8.v_scale[i])
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                for S in a.queries:
                    if S * (a.hq // a.hkv) > 16:
                        continue
                    q = torch.randn(B, S, a.hq, D, device="cuda").to(torch.bfloat16)
                    qs = [q[:, s].contiguous() for s in range(S)]

                    def single8(i):
                        for s in range(S):
                            decode_attention(qs[s], cache8.k[i], cache8.v[i], lens, k_scale=cache8.k_scale[i],
                                             v_scale=cache8.v_scale[i])
                    fns = {"rows8": lambda i: attend_rows(q, cache8.k[i], cache8.v[i], lens, k_scale=cache8.k_scale[i],
                                                          v_scale=cache8.v_scale[i]),
                           "single8": single8, "rows": lambda i: attend_rows(q, cache.k[i], cache.v[i], lens)}
                    row = {"B": B, "n": n, "S": S, "Hq": a.hq, "Hkv": a.hkv, "D": D, "layers": L,
                           "footprint_mb": round(L * own["rows"] / 1e6, 1),
                           "fp8_footprint_mb": round(L * own["rows8"] / 1e6, 1)}
                    for name in ("rows8", "single8", "rows") * 2:
                        dev_us, host_us = timed(fns[name], L, a.reps)
                        row.setdefault(name + "_us", []).append(round(dev_us, 2))
                        row.setdefault(name + "_host_us", []).append(round(host_us, 2))
                    for name in ("rows8", "rows"):
                        row[name + "_gbps"] = round(own[name] / min(row[name + "_us"]) / 1e3, 1)
                    row["rows8_vs_single8"] = round(min(row["rows8_us"]) / min(row["single8_us"]), 3)
                    row["rows8_vs_rows"] = round(min(row["rows8_us"]) / min(row["rows_us"]), 3)
                    print(json.dumps(row), flush=True)
                    out.append(row)
                del cache, cache8
    return out


def steps_bench(a):
    """ms per step: one ``decode_steps`` over S tokens per sequence against one ``decode_step``."""
    from pytorch_operator_amd.models.llama import CONFIGS, Attention, Llama, TNLinear
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    out = []
    for name in a.model:
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = Llama(CONFIGS[name]).eval()
        to_bf16_matmul_weights(model)
        for p in model.parameters():
            if hasattr(p, "_pto_master"):
                del p._pto_master
        V, n_layers = model.cfg.vocab_size, model.cfg.n_layers
        for S in a.queries:
            for B in [b for b in a.batch if b * S <= 16]:
                prompts = torch.randint(0, V, (B, a.prompt), device="cuda")
                toks = torch.randint(0, V, (B, S), device="cuda")
                row = {"model": name, "B": B, "S": S, "keys": a.prompt, "linear": (a.decode_linear or ["hip"])[0],
                       "kv": a.kv}
                TNLinear.rows_impl = row["linear"]
                try:
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                        cache = model.new_cache(B, a.prompt + S, torch.float8_e4m3fn if a.kv == "fp8" else None)
                        lens0 = torch.full((B,), a.prompt, dtype=torch.int32, device="cuda")
                        model.prefill(prompts, lens0, cache)

                        def step(i):
                            cache.lens = lens0
                            model.decode_step(toks[:, 0], cache)

                        def steps(i):
                            cache.lens = lens0
                            model.decode_steps(toks, cache)
                        Attention.decode_calls.clear()
                        for side, fn in (("step", step), ("steps", steps)) * 2:
                            dev_us, host_us = timed(fn, 1, a.reps)
                            row.setdefault(side + "_ms", []).append(round(dev_us / 1e3, 3))
                            row.setdefault(side + "_host_ms", []).append(round(host_us / 1e3, 3))
                finally:
                    TNLinear.rows_impl = "lib"
                # both sides ran the HIP attention: 2 runs of (1 warm-up + reps) steps over every layer, each
                sfx = "-fp8" if a.kv == "fp8" else ""
                assert dict(Attention.decode_calls) == {"hip" + sfx: 2 * (a.reps + 1) * n_layers,
                                                        "hip-rows" + sfx: 2 * (a.reps + 1) * n_layers}, Attention.decode_calls
                row["steps_vs_step"] = round(min(row["steps_ms"]) / min(row["step_ms"]), 3)
                print(json.dumps(row), flush=True)
                out.append(row)
                del cache
        del model
        torch.cuda.empty_cache()
    return out


def linear_shapes():
    """(model, projection, N, K, swiglu) of the decode step's five GEMMs per model."""
    from pytorch_operator_amd.models.llama import CONFIGS
    for name in ("llama3-8b", "llama3-1b"):
        c = CONFIGS[name]
        qkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
        yield from ((name, "wqkv", qkv, c.dim, False), (name, "wo", c.dim, c.dim, False),
                    (name, "w13", 2 * c.ffn_hidden, c.dim, True), (name, "w2", c.dim, c.ffn_hidden, False),
                    (name, "output", c.vocab_size, c.dim, False))


def linear_bench(a):
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.llm import swiglu_packed
    from pytorch_operator_amd.ops.skinny import (linear_rows, linear_rows_fp4, linear_rows_fp8, quantize_rows,
                                                 quantize_rows_fp4)
    fp8, fp4 = "hip-fp8" in (a.decode_linear or []), "hip-fp4" in (a.decode_linear or [])
    sides = [{"hip-fp8": "fp8", "hip-fp4": "fp4"}.get(s, s) for s in (a.decode_linear or ["hip", "lib"])]
    sides = sides[:1] + [f"fp8_t{t}" for t in a.fp8_tiles if fp8] + sides[1:]
    lib = _native.load()
    out = []
    for name, proj, N, K, swiglu in linear_shapes():
        wbytes = N * K * 2
        own = {"fp4": wbytes * 17 // 64, "fp8": wbytes // 2}   # fp4: half a byte a weight and a scale byte per 32
        copies = max(2, -(-(512 << 20) // (own["fp4"] if fp4 else own["fp8"] if fp8 else wbytes)))
        ws = torch.empty(copies, N, K, dtype=torch.bfloat16, device="cuda")
        for i in range(copies):  # a copy at a time: the fp32 draw of all of them would be 4 bytes a weight
            ws[i] = torch.randn(N, K, device="cuda") * 0.02
        if fp8:
            qs = [quantize_rows(ws[i]) for i in range(copies)]
        if fp4:
            q4 = [quantize_rows_fp4(ws[i]) for i in range(copies)]
        for M in a.rows:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            fns = {"hip": lambda i: linear_rows(x, ws[i], swiglu),
                   "lib": (lambda i: swiglu_packed(F.linear(x, ws[i]))) if swiglu else (lambda i: F.linear(x, ws[i])),
                   "fp8": lambda i: linear_rows_fp8(x, *qs[i], swiglu),
                   "fp4": lambda i: linear_rows_fp4(x, *q4[i], swiglu)}
            for t in a.fp8_tiles:
                fns[f"fp8_t{t}"] = lambda i, t=t: linear_rows_fp8(x, *qs[i], swiglu, t)
            row = {"model": name, "proj": proj, "M": M, "N": N, "K": K, "swiglu": swiglu, "copies": copies,
                   "footprint_mb": round(copies * wbytes / 1e6, 1), "waves": int(lib.pto_skinny_waves(K))}
            if fp8:
                row.update(fp8_footprint_mb=round(copies * wbytes / 2e6, 1),
                           tiles=int(lib.pto_skinny_fp8_tiles(M, N, int(swiglu))))
            if fp4:
                row.update(fp4_footprint_mb=round(copies * own["fp4"] / 1e6, 1))
            with torch.no_grad():
                for side in sides * 2:
                    dev_us, host_us = timed(fns[side], copies, a.reps)
                    row.setdefault(side + "_us", []).append(round(dev_us, 2))
                    row.setdefault(side + "_host_us", []).append(round(host_us, 2))
            for side in sides:
                mine = own.get(side[:3], wbytes)
                row[side + "_gbps"] = round(mine / min(row[side + "_us"]) / 1e3, 1)
                row[side + "_peak"] = round(row[side + "_gbps"] / 8000.0, 3)
            print(json.dumps(row), flush=True)
            out.append(row)
        del ws
        torch.cuda.empty_cache()
    return out


def fused_linear_bench(a):
    """Each call of csrc/kernels/skinny_gemm_fused.hip against the launches it replaces, at the decode step's
    shapes: wo and w2 with the residual epilogue against ``linear_rows`` + ``add_rms_norm`` (two launches), wqkv,
    w13 + SwiGLU and the lm-head with the row-scale epilogue against ``linear_rows`` alone (the norm they no longer
    wait for is on the producer's side of the ledger).  bf16 and e4m3 weights, an fp32 residual stream (what
    ``generate`` carries under autocast), both sides alternating in one process, two runs each."""
    from pytorch_operator_amd.ops import skinny as S
    from pytorch_operator_amd.ops.norm import add_rms_norm
    out = []
    for name, proj, N, K, swiglu in linear_shapes():
        wbytes = N * K * 2
        copies = max(2, -(-(512 << 20) // (wbytes // 2)))
        ws = torch.empty(copies, N, K, dtype=torch.bfloat16, device="cuda")
        for i in range(copies):
            ws[i] = torch.randn(N, K, device="cuda") * 0.02
        qs = [S.quantize_rows(ws[i]) for i in range(copies)]
        gamma = 1 + 0.1 * torch.randn(N, device="cuda")
        for M in a.rows:
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            resid, ss = torch.randn(M, N, device="cuda"), 8 + 16 * torch.rand(M, K // 16, device="cuda")
            for fmt in ("bf16", "e4m3"):
                wa = (lambda i: (ws[i],)) if fmt == "bf16" else (lambda i: qs[i])
                sfx = "" if fmt == "bf16" else "_fp8"
                plain = getattr(S, "linear_rows" + sfx)
                if proj in ("wo", "w2"):
                    add = getattr(S, "linear_rows_add_norm" + sfx)
                    fns = {"fused": lambda i: add(x, *wa(i), resid, gamma),
                           "unfused": lambda i: add_rms_norm(resid, plain(x, *wa(i)), gamma, 1e-5, torch.bfloat16)}
                else:
                    scaled = getattr(S, "linear_rows_scaled" + sfx)
                    fns = {"fused": lambda i: scaled(x, *wa(i), ss, 1e-5, swiglu),
                           "unfused": lambda i: plain(x, *wa(i), swiglu)}
                row = {"model": name, "proj": proj, "epilogue": "residual" if proj in ("wo", "w2") else "row-scale",
                       "weights": fmt, "M": M, "N": N, "K": K, "swiglu": swiglu, "copies": copies}
                with torch.no_grad():
                    for side in ("fused", "unfused") * 2:
                        dev_us, host_us = timed(fns[side], copies, a.reps)
                        row.setdefault(side + "_us", []).append(round(dev_us, 2))
                        row.setdefault(side + "_host_us", []).append(round(host_us, 2))
                print(json.dumps(row), flush=True)
                out.append(row)
        del ws, qs
        torch.cuda.empty_cache()
    return out


def e2e_fused_bench(a):
    """tokens/s of ``Llama.generate`` with ``TNLinear.rows_fuse_norm`` off (the path without the fused kernels)
    and on, alternating, for each of --decode-linear's sides (default hip)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama, TNLinear
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    impls = a.decode_linear or ["hip"]
    out = []
    for name in a.model:
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = Llama(CONFIGS[name])
        to_bf16_matmul_weights(model)
        for p in model.parameters():
            if hasattr(p, "_pto_master"):
                del p._pto_master
        if "hip-fp8" in impls:
            model.quantize_decode_weights(snap=True)
        L, steps = model.cfg.n_layers, a.tokens - 1
        for B in a.batch:
            prompts = torch.randint(0, model.cfg.vocab_size, (B, a.prompt), device="cuda")
            for impl in impls:
                row = {"model": name, "linear": impl, "B": B, "prompt": a.prompt, "new_tokens": a.tokens}
                for side in ("warm", "off", "on", "off", "on"):
                    TNLinear.rows_impl, TNLinear.rows_fuse_norm = impl, side != "off"
                    TNLinear.rows_calls.clear()
                    try:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        toks = model.generate(prompts, max_new_tokens=a.tokens)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                    finally:
                        TNLinear.rows_impl, TNLinear.rows_fuse_norm = "lib", False
                    want = {impl: steps * (4 * L + 1) + 1} if side == "off" else \
                        {impl: steps + 1, impl + "-scaled": steps * 2 * L, impl + "-add-norm": steps * 2 * L,
                         "rms-norm": steps}
                    assert dict(TNLinear.rows_calls) == want, TNLinear.rows_calls  # every step took its side's path
                    if side != "warm":
                        row.setdefault(side + "_tokens_per_s", []).append(round(B * a.tokens / dt, 1))
                        row.setdefault(side + "_ms_per_token", []).append(round(dt / a.tokens * 1e3, 3))
                assert toks.shape == (B, a.tokens)
                print(json.dumps(row), flush=True)
                out.append(row)
        del model
        torch.cuda.empty_cache()
    return out


def e2e_linear_bench(a):
    """tokens/s of ``Llama.generate`` with the decode step's projections on each side of --decode-linear."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama, TNLinear
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    out = []
    for name in a.model:
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = Llama(CONFIGS[name])
        to_bf16_matmul_weights(model)
        for p in model.parameters():
            if hasattr(p, "_pto_master"):
                del p._pto_master  # the fp32 copy an optimizer would take over: not needed here
        if "hip-fp8" in a.decode_linear:
            model.quantize_decode_weights(snap=True)  # every side then runs the same, quantised, model
        if "hip-fp4" in a.decode_linear:
            # alone, the same; beside hip-fp8 the weights stay the e4m3 model's and the fp4 side runs its own
            # quantisation of them: the time of a step does not depend on the values
            model.quantize_decode_weights(snap="hip-fp8" not in a.decode_linear, fmt="fp4")
        L = model.cfg.n_layers
        for B in a.batch:
            prompts = torch.randint(0, model.cfg.vocab_size, (B, a.prompt), device="cuda")
            row = {"model": name, "B": B, "prompt": a.prompt, "new_tokens": a.tokens}
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()  # after the quantisation's temporaries
            for i, side in enumerate(["warm"] + a.decode_linear * 2):
                TNLinear.rows_impl = a.decode_linear[0] if side == "warm" else side
                TNLinear.rows_calls.clear()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    toks = model.generate(prompts, max_new_tokens=a.tokens)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    want = TNLinear.rows_impl
                finally:
                    TNLinear.rows_impl = "lib"
                # every projection of the decode steps and every lm-head call took the side it is reported under
                # (hip: the fused w13 is one call; lib: w13 is one call as well, its SwiGLU a launch of its own)
                assert dict(TNLinear.rows_calls) == {want: (a.tokens - 1) * (4 * L + 1) + 1}, TNLinear.rows_calls
                if side != "warm":
                    row.setdefault(side + "_tokens_per_s", []).append(round(B * a.tokens / dt, 1))
                    row.setdefault(side + "_ms_per_token", []).append(round(dt / a.tokens * 1e3, 3))
            assert toks.shape == (B, a.tokens)
            row["peak_mem_mb"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)  # the weights of every side, and the caches
            print(json.dumps(row), flush=True)
            out.append(row)
        del model
        torch.cuda.empty_cache()
    return out


def e2e_bench(a):
    from pytorch_operator_amd.models.llama import CONFIGS, Attention, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    out = []
    for name in a.model:
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = Llama(CONFIGS[name])
        to_bf16_matmul_weights(model)
        for B in a.batch:
            prompts = torch.randint(0, model.cfg.vocab_size, (B, a.prompt), device="cuda")
            row = {"model": name, "B": B, "prompt": a.prompt, "new_tokens": a.tokens}
            other = "hip-fp8" if a.kv == "fp8" else "sdpa"
            for impl in ("warm", "hip", other, "hip", other):
                # the decode step alone changes sides: Attention.impl would move the prefill as well
                Attention.decode_impl = "sdpa" if impl == "sdpa" else None
                Attention.decode_calls.clear()
                torch.cuda.reset_peak_memory_stats()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    toks = model.generate(prompts, max_new_tokens=a.tokens,
                                          kv_dtype=torch.float8_e4m3fn if impl == "hip-fp8" else None)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    Attention.decode_impl = None
                # every decode step of the run took the side it is reported under
                want = "hip" if impl == "warm" else impl
                assert dict(Attention.decode_calls) == {want: (a.tokens - 1) * model.cfg.n_layers}, Attention.decode_calls
                if impl != "warm":
                    row.setdefault(impl + "_tokens_per_s", []).append(round(B * a.tokens / dt, 1))
                    row.setdefault(impl + "_ms_per_token", []).append(round(dt / a.tokens * 1e3, 3))
                    if a.kv == "fp8":
                        row.setdefault(impl + "_peak_mb", []).append(round(torch.cuda.max_memory_allocated() / 1e6, 1))
            assert toks.shape == (B, a.tokens) and Attention.impl == "auto"
            print(json.dumps(row), flush=True)
            out.append(row)
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=ints, default=[1, 8])
    p.add_argument("--keys", type=ints, default=[512, 2048, 8192])
    p.add_argument("--head-dim", type=ints, default=[64, 128])
    p.add_argument("--hq", type=int, default=32)
    p.add_argument("--hkv", type=int, default=8)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--model", type=lambda s: s.split(","), default=["llama3-1b", "llama3-8b"])
    p.add_argument("--prompt", type=int, default=128)
    p.add_argument("--tokens", type=int, default=128)
    p.add_argument("--linear", action="store_true", help="the skinny GEMM against F.linear at the decode step's shapes")
    p.add_argument("--rows", type=ints, default=[1, 8, 16], help="--linear: batch rows M")
    p.add_argument("--decode-linear", type=lambda s: s.split(","), default=None,
                   help="--e2e: the sides of the projection A/B, e.g. lib,hip or lib,hip,hip-fp8 (default: the "
                        "attention A/B); --linear: the sides in their order (default hip,lib)")
    p.add_argument("--fp8-tiles", type=ints, default=[], help="--linear with hip-fp8: also each forced tile count")
    p.add_argument("--fuse-norm", action="store_true",
                   help="--linear: each call of skinny_gemm_fused.hip against the launches it replaces; --e2e: "
                        "generate with the norms folded into the projections against the same without, for "
                        "--decode-linear's sides (hip and / or hip-fp8; default hip)")
    p.add_argument("--kv", choices=["bf16", "fp8"], default="bf16",
                   help="fp8: the e4m3 KV cache against the bf16 one (kernel mode and --e2e without --decode-linear); with "
                        "--queries: the e4m3 multi-query kernel")
    p.add_argument("--queries", type=ints, default=[],
                   help="S, ..: the multi-query kernel against S single-query calls (kernel mode), or with --e2e one "
                        "decode_steps over S tokens against one decode_step")
    p.add_argument("--json-out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    if a.decode_linear and (not (a.e2e or a.linear) or set(a.decode_linear) - {"lib", "hip", "hip-fp8", "hip-fp4"}):
        p.error("--decode-linear takes lib, hip, hip-fp8 and / or hip-fp4, with --e2e or --linear")
    if a.kv == "fp8" and (a.linear or a.decode_linear):
        p.error("--kv fp8 goes with the kernel mode or the attention --e2e")
    if set(a.fp8_tiles) - {1, 2, 4}:
        p.error("--fp8-tiles takes 1, 2 and / or 4")
    if a.queries and (a.linear or min(a.queries) < 1):
        p.error("--queries takes positive counts, in the kernel mode or with --e2e")
    if a.fuse_norm and (not (a.e2e or a.linear) or a.queries or set(a.decode_linear or []) - {"hip", "hip-fp8"}):
        p.error("--fuse-norm goes with --linear or --e2e, and --decode-linear hip and / or hip-fp8")
    if a.fuse_norm:
        res = {"fused_linear": fused_linear_bench(a)} if a.linear else {"e2e_fused": e2e_fused_bench(a)}
    elif a.queries and a.e2e:
        res = {"steps": steps_bench(a)}
    elif a.queries:
        res = {"queries_fp8": queries_fp8_bench(a)} if a.kv == "fp8" else {"queries": queries_bench(a)}
    elif a.linear:
        res = {"linear": linear_bench(a)}
    elif a.e2e:
        res = {"e2e_linear": e2e_linear_bench(a)} if a.decode_linear else {"e2e": e2e_bench(a)}
    else:
        res = {"kernel_fp8": kernel_fp8_bench(a)} if a.kv == "fp8" else {"kernel": kernel_bench(a)}
    if a.json_out:
        Path(a.json_out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
