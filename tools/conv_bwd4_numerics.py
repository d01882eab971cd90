#!/usr/bin/env python3
"""conv_bwd4 against an fp64 CPU reference (round 8).

One conv_bwd4 launch + slab reduction per batch size, on the kernel's own inputs (a1 / idx1 / xn
from conv1_fwd, a random pooled dz2), compared with the four conv gradients computed in fp64 on
the CPU from exactly those inputs.  tests/test_conv_bwd4_2b_gpu.py imports the cases and the
reference from here; run as a script it records, for the loaded library (PTO_HIP_LIB selects a
variant), each gradient's max error relative to the reference's max magnitude and a sha256 of its
bytes:

    python tools/conv_bwd4_numerics.py --json profiles/r8_bwd4_2b/numerics.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

BATCHES = (1, 4, 5, 64)  # lone non-full chunk; one full chunk; 1 valid + 3 zero-filled; the training batch
NAMES = ("conv2.weight", "conv2.bias", "conv1.weight", "conv1.bias")
SHAPES = {"conv2.weight": (50, 500), "conv2.bias": (50,), "conv1.weight": (20, 25), "conv1.bias": (20,)}


def make_case(B: int, co_only=None, seed: int = 0):
    """CPU inputs of one launch: image bytes, labels, pooled dz2 [B, 800] and its argmax codes.
    ``co_only``: the output channels whose dz2 is non-zero (None: all 50)."""
    g = torch.Generator().manual_seed(8000 + 16 * B + seed)
    x = torch.randint(0, 256, (B, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    dpool = torch.randn((B, 50, 16), generator=g)
    idx2 = torch.randint(0, 4, (B, 800), generator=g, dtype=torch.uint8)
    if co_only is not None:
        keep = torch.zeros(50, dtype=torch.bool)
        keep[list(co_only)] = True
        dpool = dpool * keep.view(1, 50, 1)
    return x, y, dpool.reshape(B, 800).contiguous(), idx2


def unpool(v: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """[B, C, h, w] values at 2 x 2 argmax codes (dy * 2 + dx) -> [B, C, 2h, 2w], zeros elsewhere."""
    B, C, h, w = v.shape
    out = torch.zeros((B, C, h, 2, w, 2), dtype=v.dtype)
    c = code.long()
    for dy in range(2):
        for dx in range(2):
            out[:, :, :, dy, :, dx] = torch.where(c == dy * 2 + dx, v, torch.zeros_like(v))
    return out.reshape(B, C, 2 * h, 2 * w)


def reference(dpool, idx2, w2, a1, idx1, xn, absolute: bool = False) -> dict:
    """The four conv gradients in fp64 on the CPU.  ``absolute``: every product replaced by its
    magnitude (the sum an a-priori rounding bound scales with)."""
    B = dpool.shape[0]
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    dz2 = unpool(dpool.double().view(B, 50, 4, 4), idx2.view(B, 50, 4, 4))
    a1d = a1.double().view(B, 20, 12, 12)
    col = F.unfold(ab(a1d), 5)  # [B, 500, 64], rows (ci, kh, kw)
    out = {"conv2.weight": torch.einsum("bjp,bkp->jk", ab(dz2).view(B, 50, 64), col),
           "conv2.bias": ab(dz2).sum((0, 2, 3))}
    da1 = F.conv_transpose2d(ab(dz2), ab(w2.double().view(50, 20, 5, 5)))  # [B, 20, 12, 12]
    da1 = torch.where(a1d > 0, da1, torch.zeros_like(da1))
    dz1 = unpool(da1, idx1.view(B, 20, 12, 12))  # [B, 20, 24, 24]
    xcol = F.unfold(ab(xn.double().view(B, 1, 28, 28)), 5)  # [B, 25, 576]
    out["conv1.weight"] = torch.einsum("bcp,bkp->ck", dz1.view(B, 20, 576), xcol)
    out["conv1.bias"] = dz1.sum((0, 2, 3))
    return out


def run_case(case, seed: int = 8):
    """conv1_fwd -> conv_bwd4 -> slab_reduce on the GPU.  Returns ({name: fp32 CPU gradient}, the
    kernel inputs on the CPU for reference())."""
    from pytorch_operator_amd.models.mnist import flat_layout, reference_init
    from pytorch_operator_amd.ops import mnist as K
    x, y, dpool, idx2 = case
    B = x.shape[0]
    dev = torch.device("cuda")
    p = {k: v.to(dev).contiguous() for k, v in reference_init(seed).items()}
    src = K.BatchSource(x.to(dev), y.to(dev))
    a1, idx1, xn, _ = K.conv1_fwd(src, p["conv1.weight"], p["conv1.bias"], B)
    lay = flat_layout()
    ce = lay.conv_end
    slab = torch.full((B, ce), float("nan"), device=dev)  # every element read has one writer
    K.conv_bwd4(dpool.to(dev), idx2.to(dev), p["conv2.weight"], a1, idx1, xn, slab, lay.offsets, B)
    got = torch.empty(ce, device=dev)
    K.slab_reduce(slab, B, got, big=K.conv_bwd4_rows(B, lay.offsets))
    torch.cuda.synchronize()
    got = got.cpu()
    grads = {n: got[lay.offsets[n]:lay.offsets[n] + torch.Size(SHAPES[n]).numel()].view(SHAPES[n]).clone()
             for n in NAMES}
    return grads, (dpool, idx2, p["conv2.weight"].cpu(), a1.cpu(), idx1.cpu(), xn.cpu())


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from pytorch_operator_amd.ops import _native
    rec = {"library": _native.library_path().name, "batches": {}}
    for B in BATCHES:
        grads, inputs = run_case(make_case(B))
        ref = reference(*inputs)
        rec["batches"][str(B)] = {"max_rel_err": {n: rel_err(grads[n], ref[n]) for n in NAMES},
                                  "sha256": {n: digest(grads[n]) for n in NAMES}}
        print(B, json.dumps(rec["batches"][str(B)]))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rec, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
