"""float64 forward of the MNIST CNN's conv / pool stages, with what an elementwise bound needs:
per output the sum of the absolute values of the terms of its dot product, the pool argmax in
the kernels' in-window code (dy * 2 + dx), and the relative gap between each window's two
largest values (an argmax between values closer than fp32 rounding has no stable answer).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

U = 2.0 ** -24   # fp32 unit roundoff
FWD_K = 8        # a1 / a2: |got - ref| <= FWD_K * U * sum |terms|
GAP = 1e-5       # pool windows whose top two float64 values are closer (relative) are not compared


@dataclass
class PoolRef:
    out: torch.Tensor      # relu(max over the 2x2 window), float64
    abs_sum: torch.Tensor  # the window's largest sum |terms| (|max a - max b| <= max |a_i - b_i|)
    code: torch.Tensor     # argmax as dy * 2 + dx, uint8
    clear: torch.Tensor    # bool: the window's top two differ by more than GAP (relative)


def _windows(z: torch.Tensor) -> torch.Tensor:
    B, C, H, W = z.shape
    return z.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def conv_pool_ref(x64: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> PoolRef:
    """relu(maxpool2(conv(x64, w) + b)) in float64 from fp32 weights."""
    w, b = w.detach().cpu().double(), b.detach().cpu().double()
    z = _windows(F.conv2d(x64, w, b))
    a = _windows(F.conv2d(x64.abs(), w.abs(), b.abs()))
    top, code = z.max(dim=4)
    two = z.topk(2, dim=4).values
    gap = (two[..., 0] - two[..., 1]) / two[..., 0].abs().clamp_min(1e-300)
    return PoolRef(F.relu(top), a.max(dim=4).values, code.to(torch.uint8), gap > GAP)


def normalize_ref(x: torch.Tensor, scale: float, shift: float) -> torch.Tensor:
    """x * scale + shift in float64, scale / shift as the fp32 values the kernel receives."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    return x.detach().cpu().double().reshape(-1, 784) * f32(scale) + f32(shift)


def forward_ref(xn64: torch.Tensor, params: dict):
    """(conv1 stage, conv2 stage) PoolRefs of normalised images xn64 [B, 784]."""
    p1 = conv_pool_ref(xn64.view(-1, 1, 28, 28), params["conv1.weight"], params["conv1.bias"])
    p2 = conv_pool_ref(p1.out, params["conv2.weight"], params["conv2.bias"])
    return p1, p2


def check_stage(got: torch.Tensor, idx: torch.Tensor, ref: PoolRef, what: str) -> float:
    """Activations within FWD_K * U * sum |terms| elementwise; argmax codes equal on every clear
    window, of which there must be more than 99 %.  Returns the worst error in units of U * sum."""
    B = ref.out.shape[0]
    g = got.detach().cpu().double().reshape(ref.out.shape)
    r = ((g - ref.out).abs() / (U * ref.abs_sum)).max().item()
    assert r <= FWD_K, f"{what}: {r:.3g} x 2^-24 x sum|terms| from the float64 reference (bound {FWD_K})"
    unclear = 1.0 - ref.clear.double().mean().item()
    assert unclear < 0.01, f"{what}: {unclear:.4f} of the reference's windows have no clear argmax"
    code = idx.detach().cpu().reshape(ref.code.shape)
    bad = (code != ref.code) & ref.clear
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} argmax codes differ from the reference (B={B})"
    return r
