"""fp64 references and derived error bounds for the Llama norm and optimizer kernels
(csrc/kernels/rmsnorm.hip, adamw.hip).  Plain arithmetic on the values the kernels read:
nothing here calls the project's own fallback paths.  tests/test_adamw_reference_cpu.py
proves the AdamW rule equal to torch.optim.AdamW."""
import math

import torch

BF16_O = 2.0 ** -8   # one RNE rounding to bf16 (8-bit significand): half an ulp, at most 2^-8 relative;
                     # the fp32 error before the rounding is carried by the FP32_E term of each bound
FP32_E = 1e-5        # bound on the kernels' accumulated fp32 error (tests state the chain)


def out_o(dtype) -> float:
    return BF16_O if dtype == torch.bfloat16 else 0.0


def rmsnorm_fp64(x, w, dy, eps, stats_from=None):
    """y, dx, dw of y = x * rsqrt(mean(x^2) + eps) * w in fp64, and the error bound of each.

    x, dy: [rows, D] (any float dtype, read as they are), w: [D].  Returns a dict of fp64
    tensors: y, dx, dw and the bound magnitudes ymag, dxmag, dwmag with
      |y  - y64|  <= o*|y64|  + FP32_E * ymag          ymag  = |y64|
      |dx - dx64| <= o*|dx64| + FP32_E * dxmag         dxmag = |r w g| + |x| (sum|g w x|) r^3 / D
      |dw - dw64| <=            FP32_E * dwmag         dwmag = sum_rows |g x r|
    dxmag bounds the two products and the row sum before they cancel.

    stats_from: the tensor r = rsqrt(mean(.^2) + eps) is taken from, when it is not x itself: the
    residual-fused forward normalises the unrounded sum x + delta and saves that r, while its
    backward reads the sum as it was stored (rounded to the residual stream's dtype)."""
    x, w, g = x.double(), w.double(), dy.double()
    D = x.shape[-1]
    r = ((x if stats_from is None else stats_from.double()).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = x * r * w
    c = (g * w * x).sum(-1, keepdim=True) * r.pow(3) / D
    dx = r * w * g - x * c
    dxmag = (r * w * g).abs() + x.abs() * (g * w * x).abs().sum(-1, keepdim=True) * r.pow(3) / D
    return dict(y=y, dx=dx, dw=(g * x * r).sum(0), ymag=y.abs(), dxmag=dxmag, dwmag=(g * x * r).abs().sum(0))


def worst_ratio(got, want, bound) -> float:
    """max |got - want| / bound (0/0 counts as 0, err/0 as inf); NaN anywhere gives inf."""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


def adamw_step_fp64(p, m, v, g, *, lr, b1, b2, eps, wd, step, grad_scale=1.0, sumsq=None, max_norm=None):
    """One AdamW step in fp64 (the rule in adamw.hip's header; torch.optim.AdamW's).  The
    gradient is first multiplied by grad_scale and, when sumsq is given, by the clip
    coefficient min(1, max_norm / (sqrt(sumsq) + 1e-6)) of clip_grad_norm_ (a NaN norm
    propagates).  p, m, v: fp64 tensors; returns the new (p, m, v)."""
    g = g.double() * grad_scale
    if sumsq is not None:
        c = max_norm / (math.sqrt(sumsq) + 1e-6)
        g = g * (1.0 if c > 1.0 else c)
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** step) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v
