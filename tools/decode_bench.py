#!/usr/bin/env python3
"""Decode attention timing at Llama-3 shapes: the HIP kernels vs the library path over the same cache.

usage: python tools/decode_bench.py [--batch 1,8] [--keys 512,2048,8192] [--head-dim 64,128] [--hq 32] [--hkv 8]
                                    [--reps 200] [--json-out F]
       python tools/decode_bench.py --e2e [--model llama3-1b,llama3-8b] [--batch 1,8] [--prompt 128] [--tokens 128]

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
alternating, two runs each; the prefill runs the HIP flash attention both times.
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
            for impl in ("warm", "hip", "sdpa", "hip", "sdpa"):
                # the decode step alone changes sides: Attention.impl would move the prefill as well
                Attention.decode_impl = "sdpa" if impl == "sdpa" else None
                Attention.decode_calls.clear()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    toks = model.generate(prompts, max_new_tokens=a.tokens)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                finally:
                    Attention.decode_impl = None
                # every decode step of the run took the side it is reported under
                want = "sdpa" if impl == "sdpa" else "hip"
                assert dict(Attention.decode_calls) == {want: (a.tokens - 1) * model.cfg.n_layers}, Attention.decode_calls
                if impl != "warm":
                    row.setdefault(impl + "_tokens_per_s", []).append(round(B * a.tokens / dt, 1))
                    row.setdefault(impl + "_ms_per_token", []).append(round(dt / a.tokens * 1e3, 3))
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
    p.add_argument("--json-out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    res = {"e2e": e2e_bench(a)} if a.e2e else {"kernel": kernel_bench(a)}
    if a.json_out:
        Path(a.json_out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
