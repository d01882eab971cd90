#!/usr/bin/env python3
"""Do hipBLASLt's per-tensor-scaled FP8 GEMMs beat the bf16 TN GEMMs at the Llama-3 8B projection
shapes on MI355X, and what do the FP8 operands cost to make?

For M = 8192 tokens and each projection (N, K) it times, in one process and interleaved round by
round (every candidate once per round, the median of the rounds reported):

  forward  x.W^T, input gradient dy.W (fed W^T), weight gradient dy^T.x  -- each as the bf16 TN GEMM
  ``linear_tn`` issues (TunableOp winners of the committed table) and as ``torch._scaled_mm`` on
  e4m3 x and w and ``--grad-format`` dy, every operand K-contiguous;
  the two launches of ``ops.fp8.quantize`` (amax, cast with both outputs) on x, w and dy, and
  ``transpose2d`` on the same tensors -- the pass the cast replaces.

The bandwidth kernels run over a ring of buffers larger than the 256 MB Infinity Cache, so their
GB/s are HBM figures: bytes = what the algorithm needs (amax: one read; cast: one read + two FP8
writes; transpose: one read + one write).  Output: one JSON document (``--out``).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_operator_amd.ops import _native, fp8  # noqa: E402
from pytorch_operator_amd.ops.llm import transpose2d  # noqa: E402

SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w13": (28672, 4096), "w2": (4096, 14336)}
RING_BYTES = 640 << 20


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us


def interleaved(cands, rounds, iters):
    """{name: median us} of callables fn(i), every one run once per round."""
    for fn in cands.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    seen = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            seen[k].append(timed(fn, iters))
    return {k: round(statistics.median(v), 2) for k, v in seen.items()}, \
           {k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in seen.items()}


class Caster:
    """The two launches of ops.fp8.quantize on preallocated outputs, one ring of inputs."""

    def __init__(self, ring, fmt):
        self.lib, self.ring = _native.load(), ring
        self.code, _, dt = fp8.FORMATS[fmt]
        R, C = ring[0].shape
        self.R, self.C = R, C
        dev = ring[0].device
        self.q = torch.empty((R, C), device=dev, dtype=dt)
        self.qT = torch.empty((C, R), device=dev, dtype=dt)
        self.inv = torch.empty((), device=dev, dtype=torch.float32)
        self.nparts = self.lib.pto_fp8_amax_parts(R * C)
        self.ws = torch.empty(self.nparts, device=dev, dtype=torch.float32)
        self.stream = ctypes.c_void_p(_native.current_stream_ptr(dev))

    def amax(self, i):
        x = self.ring[i % len(self.ring)]
        _native.check(self.lib.pto_fp8_amax(x.data_ptr(), self.R, self.C, self.ws.data_ptr(), self.nparts,
                                            self.stream), "fp8_amax")

    def cast(self, i):
        x = self.ring[i % len(self.ring)]
        _native.check(self.lib.pto_fp8_cast(x.data_ptr(), self.R, self.C, self.code, self.ws.data_ptr(),
                                            self.nparts, None, self.q.data_ptr(), self.qT.data_ptr(),
                                            self.inv.data_ptr(), self.stream), "fp8_cast")


def ring_of(t):
    n = max(2, -(-RING_BYTES // (t.numel() * t.element_size())))
    return [t] + [t.clone() for _ in range(n - 1)]


def probe_shape(name, M, N, K, grad_format, rounds, iters):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, generator=g)
    w = torch.randn(N, K, device=dev, dtype=torch.bfloat16, generator=g) * 0.02
    dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16, generator=g) * 0.01
    wT, dyT, xT = transpose2d(w), transpose2d(dy), transpose2d(x)
    x8, x8T, sx = fp8.quantize(x, "e4m3")
    w8, w8T, sw = fp8.quantize(w, "e4m3")
    d8, d8T, sd = fp8.quantize(dy, grad_format)

    def smm(a, bt, sa, sb):
        return torch._scaled_mm(a, bt.t(), scale_a=sa, scale_b=sb, out_dtype=torch.bfloat16, use_fast_accum=False)

    gemms = {"fwd_bf16": lambda i: F.linear(x, w), "fwd_fp8": lambda i: smm(x8, w8, sx, sw),
             "dgrad_bf16": lambda i: F.linear(dy, wT), "dgrad_fp8": lambda i: smm(d8, w8T, sd, sw),
             "wgrad_bf16": lambda i: F.linear(dyT, xT), "wgrad_fp8": lambda i: smm(d8T, x8T, sd, sx)}
    # the FP8 results agree with the bf16 ones to FP8 accuracy (a wrong layout would not)
    check = {}
    for k in ("fwd", "dgrad", "wgrad"):
        a, b = gemms[k + "_fp8"](0).float(), gemms[k + "_bf16"](0).float()
        check[k + "_rel_err"] = round(float((a - b).norm() / b.norm()), 4)
    us, spread = interleaved(gemms, rounds, iters)
    rec = {"linear": name, "M": M, "N": N, "K": K, "grad_format": grad_format, "gemm_us": us,
           "gemm_spread": spread, "fp8_vs_bf16": check,
           "gemm_tflops": {k: round(2.0 * M * N * K / v / 1e6, 1) for k, v in us.items()}}
    del wT, dyT, xT, x8, x8T, w8, w8T, d8, d8T
    rec["operands"] = {}
    for tag, t, fmt in (("x", x, "e4m3"), ("w", w, "e4m3"), ("dy", dy, grad_format)):
        ring = ring_of(t)
        c = Caster(ring, fmt)
        c.amax(0)
        cands = {"amax": c.amax, "cast_both": c.cast, "transpose2d": lambda i: transpose2d(ring[i % len(ring)])}
        us, spread = interleaved(cands, rounds, iters)
        nbytes = t.numel() * 2
        need = {"amax": nbytes, "cast_both": 2 * nbytes, "transpose2d": 2 * nbytes}
        rec["operands"][tag] = {"shape": list(t.shape), "format": fmt, "ring": len(ring), "us": us, "spread": spread,
                                "gb_per_s": {k: round(need[k] / us[k] / 1e3, 1) for k in us},
                                "cast_over_transpose": round(us["cast_both"] / us["transpose2d"], 3)}
        del ring, c
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/fp8/gemm_probe.json")
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--grad-format", choices=sorted(fp8.FORMATS), default="e5m2")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--linears", default=",".join(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_gemm_probe: needs a GPU (a timing from anywhere else says nothing)")
    from pytorch_operator_amd.harness.ddp_train import parse_args, setup_gemm_tuning
    tuning = setup_gemm_tuning(parse_args(["--model", "llama3-8b"]), torch.device("cuda"))
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "bf16_gemm_tuning": tuning.get("mode"), "fp8_gemm_tuning": "library default",
           "rounds": args.rounds, "iters": args.iters, "timing": "device events, median of interleaved rounds",
           "shapes": []}
    for name in args.linears.split(","):
        N, K = SHAPES[name]
        rec = probe_shape(name, args.tokens, N, K, args.grad_format, args.rounds, args.iters)
        print(json.dumps(rec), flush=True)
        doc["shapes"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
