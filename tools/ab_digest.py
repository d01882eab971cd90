#!/usr/bin/env python3
"""SHA-256 of every output of the elementwise kernels on seeded, NaN-free inputs: run it once per
build of libpto_hip.so (PTO_HIP_LIB selects a prebuilt one), each in a fresh process, and diff the
two files to see whether a kernel change altered any result bit.

    PTO_HIP_LIB=/path/to/other/libpto_hip.so python tools/ab_digest.py a.json
    python tools/ab_digest.py b.json && diff a.json b.json
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
from test_batchnorm_gpu import SHAPES  # noqa: E402
from test_llm_edges_gpu import ROWS, SCALAR_D, VECTOR_D  # noqa: E402  (every W = 1 / W = 4 RMSNorm width)

F32, BF16 = torch.float32, torch.bfloat16
PAIRS = {"x32-y32": (F32, F32), "xbf16-ybf16": (BF16, BF16), "x32-ybf16": (F32, BF16)}
# and 199: W = 1, P = 1 with both halves of every wave filled, so a lone product meets the block sum
RMS_D = SCALAR_D + [199] + VECTOR_D
EPS = 1e-5


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def unaligned(t):
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = base[1:].view(t.shape)
    v.copy_(t)
    return v


def rmsnorm_cases(out):
    from pytorch_operator_amd.ops.norm import add_rms_norm, rms_norm

    def one(key, rows, D, xdt, ydt, off):
        g = torch.Generator().manual_seed(1000 * D + rows)
        x = torch.randn(rows, D, generator=g).to(xdt)
        w = (1 + 0.1 * torch.randn(D, generator=g)).cuda().requires_grad_(True)
        dy = torch.randn(rows, D, generator=g).to(ydt).cuda()
        xg = (unaligned(x.cuda()) if off else x.cuda()).requires_grad_(True)
        y = rms_norm(xg, w, EPS, ydt)
        y.backward(dy)
        out[key] = {"y": sha(y), "dx": sha(xg.grad), "dw": sha(w.grad)}

    for name, (xdt, ydt) in PAIRS.items():
        for D in RMS_D:
            for rows in ROWS:
                one(f"rms_norm {name} D={D} rows={rows}", rows, D, xdt, ydt, False)
        one(f"rms_norm {name} D=1028 rows=9 unaligned x", 9, 1028, xdt, ydt, True)
        for D in (1028, 4100):
            for with_gs in (True, False):
                g = torch.Generator().manual_seed(8 + D)
                x = torch.randn(9, D, generator=g).to(xdt).cuda().requires_grad_(True)
                d = torch.randn(9, D, generator=g).to(ydt).cuda().requires_grad_(True)
                w = (1 + 0.1 * torch.randn(D, generator=g)).cuda().requires_grad_(True)
                gy = torch.randn(9, D, generator=g).to(ydt).cuda()
                gs = torch.randn(9, D, generator=g).to(xdt).cuda()
                s, y = add_rms_norm(x, d, w, EPS, ydt)
                torch.autograd.backward([y, s], [gy, gs]) if with_gs else y.backward(gy)
                out[f"add_rms_norm {name} D={D} gs={with_gs}"] = {
                    "s": sha(s), "y": sha(y), "dx": sha(x.grad), "dd": sha(d.grad), "dw": sha(w.grad)}


def batchnorm_cases(out):
    from pytorch_operator_amd.ops.batchnorm import batch_norm_act
    cl = dict(memory_format=torch.channels_last)
    for shape in (SHAPES[0], SHAPES[2]):
        for relu, res in [(False, False), (True, False), (True, True), (False, True)]:
            g = torch.Generator().manual_seed(0)
            C = shape[1]
            x = torch.randn(shape, generator=g).to(BF16).cuda().contiguous(**cl).requires_grad_(True)
            z = torch.randn(shape, generator=g).to(BF16).cuda().contiguous(**cl).requires_grad_(True) if res else None
            w = (0.5 + torch.rand(C, generator=g)).cuda().requires_grad_(True)
            b = (0.2 * torch.randn(C, generator=g)).cuda().requires_grad_(True)
            dy = torch.randn(shape, generator=g).to(BF16).cuda().contiguous(**cl)
            rm, rv = (0.1 * torch.randn(C, generator=g)).cuda(), (1 + torch.rand(C, generator=g)).cuda()
            nbt = torch.zeros((), dtype=torch.long, device="cuda")
            y = batch_norm_act(x, w, b, rm, rv, nbt, True, 0.1, 1e-5, relu, z, impl="hip")
            y.backward(dy)
            r = {"y": sha(y), "dx": sha(x.grad), "dw": sha(w.grad), "db": sha(b.grad), "rm": sha(rm), "rv": sha(rv)}
            if res:
                r["dz"] = sha(z.grad)
            out[f"batch_norm_act bf16 {shape} relu={relu} res={res}"] = r


def pool_cases(out):
    from pytorch_operator_amd.ops.pool import _MaxPool
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 8, 7, 9, generator=g).to(BF16).cuda().contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y = _MaxPool.apply(x)
    y.backward(torch.randn(y.shape, generator=g).to(BF16).cuda().contiguous(memory_format=torch.channels_last))
    out["max_pool_3x3_s2 (3, 8, 7, 9)"] = {"y": sha(y), "dx": sha(x.grad)}


def main():
    from pytorch_operator_amd.ops import _native
    _native.load()
    out = {}
    rmsnorm_cases(out)
    batchnorm_cases(out)
    pool_cases(out)
    torch.cuda.synchronize()
    text = json.dumps(out, indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(f"{len(out)} cases, digest of digests {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
