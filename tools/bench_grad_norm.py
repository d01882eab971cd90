"""pto_grad_sumsq + finish (csrc/kernels/gradclip.hip) against torch.linalg.vector_norm on one
1 GiB bf16 and one 1 GiB fp32 buffer, in one process, alternating (profiles/gradclip/README.md).

    python tools/bench_grad_norm.py [--out bench_norm.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_operator_amd.ops import _native  # noqa: E402

VP = ctypes.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    libs = {"pto_grad_sumsq+finish": _native.load()}
    ws = torch.empty(8192, dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    stream = VP(torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "bytes": 2 ** 30, "cases": {}}
    REPS, ROUNDS = 10, 12
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        n = 2 ** 30 // (2 if dtype == torch.bfloat16 else 4)
        g = torch.randn(n, dtype=dtype, device=dev)
        bf = 1 if dtype == torch.bfloat16 else 0

        def ours(lib):
            k = lib.pto_grad_sumsq_parts(n, bf)
            rc = lib.pto_grad_sumsq(g.data_ptr(), n, bf, 1.0, ws.data_ptr(), ws.numel(), stream)
            rc2 = lib.pto_grad_sumsq_finish(ws.data_ptr(), k, out.data_ptr(), stream)
            assert rc == 0 and rc2 == 0, (rc, rc2)

        fns = {k: (lambda lib=lib: ours(lib)) for k, lib in libs.items()}
        fns["torch.linalg.vector_norm"] = lambda: torch.linalg.vector_norm(g)
        if bf:
            fns["torch.linalg.vector_norm(dtype=float32)"] = lambda: torch.linalg.vector_norm(g, dtype=torch.float32)
        ref = float(torch.linalg.vector_norm(g, dtype=torch.float64))
        case = {"n": n, "ref_norm_fp64": ref, "ms": {}, "norm": {}}
        for k, fn in fns.items():  # warm up + values
            for _ in range(3):
                r = fn()
            torch.cuda.synchronize()
            case["norm"][k] = float(out[1]) if r is None else float(r)
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):  # alternate
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / REPS)
        for k, t in times.items():
            med = statistics.median(t)
            case["ms"][k] = {"median": round(med, 5), "min": round(min(t), 5), "max": round(max(t), 5),
                             "GBps_median": round(2 ** 30 / med / 1e6, 1)}
            print(name, k, case["ms"][k], "norm", case["norm"][k], "rel", abs(case["norm"][k] - ref) / ref, flush=True)
        res["cases"][name] = case
        del g
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
