"""GPU: the edge paths of the kernels every Llama step runs -- rmsnorm.hip, llm_fused.hip
(cross-entropy, SwiGLU) and adamw.hip -- against fp64 arithmetic on the same values.

tests/test_llm_gpu.py checks these kernels at a few friendly shapes; this module walks the
branches those shapes never take: RMSNorm at one element per access (W = 1: odd D, unaligned
views) and every W / P instantiation, cross-entropy at the sizes that change its loop trip
count, with boundary targets and -inf (masked-vocabulary) logits, SwiGLU tails, saturating
inputs and the second grid-stride trip, all eight AdamW instantiations through the C entry
points with tail-only and grid-stride sizes, and the NaN rule of the bf16 rounding.  Inputs are
drawn on the CPU with a seeded generator and rounded to the kernel's input dtype first, so both
sides start from the same values; the references and the derived bounds are in
tests/llm_refs.py.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from llm_refs import FP32_E, adamw_step_fp64, out_o, rmsnorm_fp64, worst_ratio

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
_NAME = {F32: "fp32", BF16: "bf16"}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(values):
    """fp32 tensor with exactly these raw bit patterns."""
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).view(F32)


def _bf16_is_nan(t):
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    return (((b >> 7) & 0xff) == 0xff) & ((b & 0x7f) != 0)


def _unaligned(t):
    """The same values in a contiguous device tensor whose address is one element past a
    16-byte boundary (a view into a longer allocation)."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------- RMSNorm
PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16)]
PAIR_IDS = ["x32-y32", "xbf16-ybf16", "x32-ybf16"]
SCALAR_D = [3, 259, 515, 1027, 2051, 4099, 8191]  # W = 1: P = 1, 2, 4, 8, 16, 32 (twice)
VECTOR_D = [4, 1028, 2052, 4100]                   # W = 4: P = 1, 2, 4 and a mostly-empty 8
ROWS = [1, 9, 17]                                  # _ROWS_PER_BLOCK = 8: 1 row; 8 + 1; 8 + 8 + 1


def _rmsnorm_inputs(rows, D, xdt, ydt, seed):
    g = _gen(seed)
    x = torch.randn(rows, D, generator=g).to(xdt)
    w = 1 + 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g).to(ydt)
    return x, w, dy


def _rmsnorm_check(label, x, w, dy, xdt, ydt, xg=None, dyg=None):
    """rms_norm forward + backward on the device vs fp64 of the same values, at the bounds
    derived in llm_refs.rmsnorm_fp64.  fp32 error budget (FP32_E = 1e-5): y and dx take a tree
    sum of <= 32 per-lane + 6 wave + 4 LDS terms, rsqrtf and two or three products; dw's longest
    chain is <= 8 rows in a block plus <= 32 colsum slices, < 64 roundings = 3.8e-6."""
    from pytorch_operator_amd.ops.norm import rms_norm
    xg = (x.cuda() if xg is None else xg).requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    dyg = dy.cuda() if dyg is None else dyg
    y = rms_norm(xg, wg, EPS, ydt)
    seen = []
    y.register_hook(lambda grad: seen.append(grad.data_ptr()))
    y.backward(dyg)
    assert seen == [dyg.data_ptr()]  # the backward kernels read dy at the address the test chose
    assert y.dtype == ydt and xg.grad.dtype == xdt and wg.grad.dtype == F32
    ref = rmsnorm_fp64(x, w, dy, EPS)
    ry = worst_ratio(y.cpu(), ref["y"], (out_o(ydt) + FP32_E) * ref["ymag"])
    rdx = worst_ratio(xg.grad.cpu(), ref["dx"], out_o(xdt) * ref["dx"].abs() + FP32_E * ref["dxmag"])
    rdw = worst_ratio(wg.grad.cpu(), ref["dw"], FP32_E * ref["dwmag"])
    print(f"rmsnorm {label}: worst error/bound y {ry:.3f} dx {rdx:.3f} dw {rdw:.3f}")
    assert ry <= 1 and rdx <= 1 and rdw <= 1, (label, ry, rdx, rdw)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", SCALAR_D + VECTOR_D)
@pytest.mark.parametrize("xdt,ydt", PAIRS, ids=PAIR_IDS)
def test_rmsnorm_every_instantiation_matches_fp64(xdt, ydt, D, rows):
    """Odd D takes rmsnorm_fwd_kernel / rmsnorm_bwd_kernel at W = 1 (one D per P instantiation) and
    the scalar branch of colsum_kernel; D % 4 == 0 takes them at W = 4, P = 1, 2, 4, 8."""
    x, w, dy = _rmsnorm_inputs(rows, D, xdt, ydt, seed=1000 * D + rows)
    _rmsnorm_check(f"{_NAME[xdt]}->{_NAME[ydt]} D={D} rows={rows}", x, w, dy, xdt, ydt)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("which", ["x", "dy"])
@pytest.mark.parametrize("xdt,ydt", PAIRS, ids=PAIR_IDS)
def test_rmsnorm_unaligned_view_takes_scalar_kernels(xdt, ydt, which, rows):
    """D = 1028 is a multiple of 4, but a contiguous view one element off a 16-byte boundary
    cannot be read with 16-byte loads: an unaligned x sends forward and backward to the W = 1
    kernels (P = 8); an unaligned dy alone leaves the forward at W = 4."""
    D = 1028
    x, w, dy = _rmsnorm_inputs(rows, D, xdt, ydt, seed=77 + rows)
    xg = _unaligned(x) if which == "x" else x.cuda()
    dyg = _unaligned(dy) if which == "dy" else dy.cuda()
    assert (xg.data_ptr() % 16 != 0) == (which == "x") and (dyg.data_ptr() % 16 != 0) == (which == "dy")
    _rmsnorm_check(f"{_NAME[xdt]}->{_NAME[ydt]} D={D} rows={rows} unaligned {which}", x, w, dy, xdt, ydt,
                   xg=xg, dyg=dyg)


@pytest.mark.parametrize("with_gs", [True, False])
@pytest.mark.parametrize("D", [1028, 4100, 1027])
@pytest.mark.parametrize("xdt,ydt", [(F32, BF16), (F32, F32), (BF16, BF16)], ids=["x32-ybf16", "x32-y32", "xbf16-ybf16"])
def test_add_rms_norm_edge_widths(xdt, ydt, D, with_gs):
    """Residual-fused RMSNorm at P = 2 (D = 1028) and a partly filled P = 8 (D = 4100), and at
    D = 1027, where add_rms_norm falls back to the unfused add + rms_norm (W = 1 kernels); the
    tolerances of test_llm_gpu.test_add_rms_norm_matches_reference, dw at the derived bound."""
    from pytorch_operator_amd.ops.norm import add_rms_norm
    rows = 9
    g = _gen(8 + D)
    x = torch.randn(rows, D, generator=g).to(xdt)
    d = torch.randn(rows, D, generator=g).to(ydt)
    w = 1 + 0.1 * torch.randn(D, generator=g)
    gy = torch.randn(rows, D, generator=g).to(ydt)
    gs = torch.randn(rows, D, generator=g).to(xdt)
    xg, dg, wg = (t.cuda().requires_grad_(True) for t in (x, d, w))
    s, y = add_rms_norm(xg, dg, wg, EPS, ydt)
    assert s.dtype == xdt and y.dtype == ydt
    loss = (y.float() * gy.cuda().float()).sum() + ((s.float() * gs.cuda().float()).sum() if with_gs else 0)
    loss.backward()
    xr, dr, wr = (t.double().requires_grad_(True) for t in (x, d, w))
    sr = xr + dr
    yr = sr * (sr.pow(2).mean(-1, keepdim=True) + EPS).rsqrt() * wr
    ((yr * gy.double()).sum() + ((sr * gs.double()).sum() if with_gs else 0)).backward()
    lo = xdt == BF16 or ydt == BF16
    tol = dict(rtol=2e-2, atol=2e-2) if lo else dict(rtol=1e-4, atol=1e-4)
    for got, want in ((s, sr), (y, yr), (xg.grad, xr.grad), (dg.grad, dr.grad)):
        torch.testing.assert_close(got.double().cpu(), want.detach(), **tol)
    # dw: the backward reads the s the forward wrote (rounded to the dtype of x); the fused
    # forward took the statistics from the unrounded sum, the unfused fallback from s itself
    ref = rmsnorm_fp64(s.detach().cpu(), w, gy, EPS, stats_from=x.double() + d.double() if D % 4 == 0 else None)
    rdw = worst_ratio(wg.grad.cpu(), ref["dw"], FP32_E * ref["dwmag"])
    print(f"add_rms_norm {_NAME[xdt]}->{_NAME[ydt]} D={D} gs={with_gs}: worst error/bound dw {rdw:.3f}")
    assert rdw <= 1


@pytest.mark.parametrize("D", [8, 7], ids=["vector", "scalar"])
def test_rmsnorm_bf16_output_keeps_nan(D):
    """A NaN x element (payload all ones: the one a carry out of the mantissa would turn into
    bf16 +0.0) makes its whole row NaN in the bf16 y; the other row stays finite."""
    from pytorch_operator_amd.ops.norm import rms_norm
    x = torch.randn(2, D, generator=_gen(5))
    x.view(torch.int32)[0, 3] = -1  # bits 0xffffffff
    y = rms_norm(x.cuda(), torch.ones(D, device="cuda"), EPS, BF16).cpu()
    assert bool(_bf16_is_nan(y[0]).all()), y.view(torch.int16)
    assert bool(y[1].float().isfinite().all())


# ------------------------------------------------------------------------- cross-entropy
def _xent_check(x, t, overwrite, zero_cols=None):
    """cross_entropy on the device vs fp64 F.cross_entropy of the same logits, at the tolerances of
    test_llm_gpu.test_cross_entropy_matches_reference.  Returns (loss, d(logits)) on the CPU."""
    from pytorch_operator_amd.ops.llm import cross_entropy
    dtype = x.dtype
    xg = x.cuda().requires_grad_(True)
    y = xg * 1
    y_before = y.detach().clone()
    loss = cross_entropy(y, t.cuda(), overwrite_logits=overwrite)
    (loss * 3).backward()
    xr = x.double().requires_grad_(True)
    lr = F.cross_entropy(xr, t, ignore_index=-100)
    (lr * 3).backward()
    grad = xg.grad.cpu()
    assert bool(loss.isfinite()) and not bool(grad.isnan().any()), (float(loss), int(grad.isnan().sum()))
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == F32 else dict(rtol=1e-2, atol=1e-5)
    torch.testing.assert_close(loss.double().cpu(), lr.detach(), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(grad.double(), xr.grad, **tol)
    for row in (t == -100).nonzero().flatten().tolist():
        assert grad[row].abs().max().item() == 0
    if zero_cols is not None:
        assert grad[zero_cols].abs().max().item() == 0  # exactly 0 where the logit is -inf
    if not overwrite:
        assert torch.equal(y.detach().cpu(), y_before.cpu())
    else:
        assert y._version > y_before._version
    return loss.cpu(), grad


def _xent_sizes():
    for v in (8, 4096, 4104, 8200):
        for tgt in sorted({0, 7, 8, v - 1}):
            if tgt < v:
                yield v, tgt


@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("v,tgt", list(_xent_sizes()))
def test_cross_entropy_boundary_sizes_and_targets(dtype, v, tgt, overwrite):
    """V = 8: one lane has data and seven waves are empty; 4096: exactly one 8-element group per
    lane; 4104: lane 0 makes a second trip; 8200: a third.  Row 0's target sits at a boundary
    column (first, last of group 0, first of group 1, V-1), row 1 is ignored, row 2 is random."""
    g = _gen(7 + v)
    x = (torch.randn(3, v, generator=g) * 8).to(dtype)
    t = torch.tensor([tgt, -100, int(torch.randint(0, v, (1,), generator=g))])
    _xent_check(x, t, overwrite)


def _neg_inf_case(case):
    """(logits, targets, mask of -inf entries) of the -inf cases, built on randn * 8; every row's
    target column stays finite."""
    v = {"a4104": 4104, "a": 8200, "b": 8200, "c": 8200, "d": 4096}[case]
    g = _gen(11 + v)
    x = torch.randn(3, v, generator=g) * 8
    mask = torch.zeros(3, v, dtype=torch.bool)
    if case in ("a", "a4104"):   # the first groups of lanes 0 and 1
        mask[:, :16] = True
        t = torch.tensor([16, -100, v - 1])
    elif case == "b":            # the first group of every lane of wave 0
        mask[:, :512] = True
        t = torch.tensor([512, -100, v - 1])
    elif case == "c":            # everything but the target, which is in the last group
        t = torch.tensor([v - 1, v - 8, v - 3])
        mask[:] = True
        mask[torch.arange(3), t] = False
    else:                        # V = 4096: waves 0 and 1 hold nothing but -inf
        mask[:, :1024] = True
        t = torch.tensor([1024, -100, v - 1])
    x[mask] = -math.inf
    return x, t, mask


@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["a4104", "a", "b", "c", "d"])
def test_cross_entropy_neg_inf_logits(dtype, case, overwrite):
    """A padded or masked vocabulary: -inf logits have probability 0.  Loss and d(logits) equal
    the fp64 reference, the gradient is exactly 0 at every -inf column and nothing is NaN.  Case c
    leaves only the target finite: its rows' loss and whole gradient are exactly 0.  Case d (not in
    the per-lane loop alone: the block combine of two all -inf waves) empties waves 0 and 1.
    A row that is all -inf, or whose target is -inf, is undefined and not tested."""
    x, t, mask = _neg_inf_case(case)
    loss, grad = _xent_check(x.to(dtype), t, overwrite, zero_cols=mask)
    if case == "c":
        assert float(loss) == 0 and grad.abs().max().item() == 0


def test_cross_entropy_bf16_nan_upstream_gradient_stays_nan():
    """A NaN loss scale (payload all ones) reaches every logit gradient of a counted row as NaN
    in bf16 as well -- not as the +0.0 an unchecked round-to-nearest-even carry would give -- and
    an ignored row still gets exact zeros."""
    from pytorch_operator_amd.ops.llm import cross_entropy
    x = (torch.randn(3, 64, generator=_gen(3)) * 4).to(BF16).cuda().requires_grad_(True)
    t = torch.tensor([5, -100, 63]).cuda()
    cross_entropy(x * 1, t).backward(_bits([0xffffffff])[0].cuda())
    assert bool(_bf16_is_nan(x.grad[[0, 2]].cpu()).all())
    assert x.grad[1].abs().max().item() == 0


# -------------------------------------------------------------------------------- SwiGLU
def _swiglu_tol(ref, dtype):
    return out_o(dtype) * ref.abs() + 1e-6 * (1 + ref.abs())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 9, 15])
def test_swiglu_tails(dtype, n):
    """n < 8 is the scalar tail alone (n8 == 0); 9 and 15 are one vector plus a tail of 1 and 7."""
    from pytorch_operator_amd.ops.llm import swiglu
    g = _gen(3 + n)
    a, b, dy = ((s * torch.randn(n, generator=g)).to(dtype) for s in (2, 1, 1))
    ag, bg = (t.cuda().requires_grad_(True) for t in (a, b))
    y = swiglu(ag, bg)
    y.backward(dy.cuda())
    ar, br = (t.double().requires_grad_(True) for t in (a, b))
    yr = F.silu(ar) * br
    yr.backward(dy.double())
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == F32 else dict(rtol=1e-2, atol=2e-2)
    for got, want in ((y, yr), (ag.grad, ar.grad), (bg.grad, br.grad)):
        torch.testing.assert_close(got.double().cpu(), want.detach(), **tol)


@functools.lru_cache(maxsize=None)
def _extremes(dtype):
    """a x b x dy over a in {+-0, +-20, +-87, +-89, +-100, +-1e4, +-3e38} (|a| >= 88: __expf(-a)
    overflows to inf or underflows to 0), b in {0.5, -0.5}, dy in {1, -3}, rounded to dtype, and
    the fp64 silu(a) * b with its autograd gradients."""
    mags = [0.0, 20.0, 87.0, 89.0, 100.0, 1e4, 3e38]
    av = [s * m for m in mags for s in (1.0, -1.0)]
    a, b, dy = (torch.tensor(v).to(dtype) for v in zip(*[(x, y, z) for x in av for y in (0.5, -0.5)
                                                          for z in (1.0, -3.0)]))
    ar, br = (t.double().requires_grad_(True) for t in (a, b))
    yr = F.silu(ar) * br
    yr.backward(dy.double())
    return a, b, dy, yr.detach(), ar.grad, br.grad


def _assert_extreme(name, got, ref, dtype):
    """Within o*|ref| + 1e-6*(1 + |ref|) (the fp64 reference keeps tiny values where fp32 gives
    +-0: the absolute term covers them) and finite -- except where the exact result is beyond the
    dtype's largest finite value (db = dy * silu(a) at a = 3e38, dy = -3 is -9e38): there the only
    correct output is the infinity of that sign."""
    got = got.double().cpu()
    over = ref.abs() > torch.finfo(dtype).max
    assert torch.equal(got[over], torch.sign(ref[over]) * math.inf), name
    assert bool(got[~over].isfinite().all()), name
    err, bound = (got[~over] - ref[~over]).abs(), _swiglu_tol(ref[~over], dtype)
    assert bool((err <= bound).all()), (name, float((err / bound).max()))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_swiglu_extremes(dtype):
    from pytorch_operator_amd.ops.llm import swiglu
    a, b, dy, yr, dar, dbr = _extremes(dtype)
    assert a.numel() == 56 and int((yr.abs() > torch.finfo(dtype).max).sum()) == 0
    assert int((dbr.abs() > torch.finfo(dtype).max).sum()) == 2  # a = +3e38, dy = -3, b = +-0.5
    ag, bg = (t.cuda().requires_grad_(True) for t in (a, b))
    y = swiglu(ag, bg)
    y.backward(dy.cuda())
    for name, got, ref in (("y", y, yr), ("da", ag.grad, dar), ("db", bg.grad, dbr)):
        _assert_extreme(name, got.detach(), ref, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Fdim", [8, 16])
def test_swiglu_packed_extremes(dtype, Fdim):
    from pytorch_operator_amd.ops.llm import swiglu_packed
    a, b, dy, yr, dar, dbr = _extremes(dtype)
    pad = -a.numel() % Fdim  # F = 16: 56 values fill 3.5 rows; the rest is a = 0, b = 0, dy = 0
    a, b, dy = (torch.cat([t, torch.zeros(pad, dtype=dtype)]).view(-1, Fdim) for t in (a, b, dy))
    xg = torch.cat([a, b], dim=1).cuda().requires_grad_(True)
    y = swiglu_packed(xg)
    y.backward(dy.cuda())
    n = yr.numel()
    assert y.shape == (a.shape[0], Fdim)
    _assert_extreme("y", y.detach().flatten()[:n], yr, dtype)
    _assert_extreme("da", xg.grad[:, :Fdim].flatten()[:n], dar, dtype)
    _assert_extreme("db", xg.grad[:, Fdim:].flatten()[:n], dbr, dtype)
    for t in (y.detach().flatten()[n:], xg.grad[:, :Fdim].flatten()[n:], xg.grad[:, Fdim:].flatten()[n:]):
        assert t.abs().sum().item() == 0


def test_swiglu_packed_second_grid_trip():
    """Llama-3 8B's F = 14336 at 9400 tokens: 16 844 800 eight-element groups against the
    65 536 x 256 = 16 777 216 threads of the capped grid, so the first 67 584 threads take a second
    trip, starting inside row 9362.  Rows on both sides of the wrap and at both ends vs fp64."""
    from pytorch_operator_amd.ops.llm import swiglu_packed
    rows, Fdim = 9400, 14336
    assert rows * (Fdim // 8) > 65536 * 256 and 65536 * 256 // (Fdim // 8) == 9362
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(rows, 2 * Fdim, device="cuda", dtype=BF16, generator=gen).requires_grad_(True)
    dy = torch.randn(rows, Fdim, device="cuda", dtype=BF16, generator=gen)
    y = swiglu_packed(x)
    y.backward(dy)
    idx = torch.tensor([0, 1, 9361, 9362, 9363, 9364, 9398, 9399], device="cuda")
    xs, ys, gs, dxs = (t.detach()[idx].cpu() for t in (x, y, dy, x.grad))
    xr = xs.double().requires_grad_(True)
    yr = F.silu(xr[:, :Fdim]) * xr[:, Fdim:]
    yr.backward(gs.double())
    for name, got, ref in (("y", ys, yr.detach()), ("dx", dxs, xr.grad)):
        err, bound = (got.double() - ref).abs(), _swiglu_tol(ref, BF16)
        assert bool((err <= bound).all()), (name, float((err / bound).max()), (err > bound).nonzero()[:4])


def test_swiglu_bf16_keeps_nan():
    """NaN gate values stay NaN in y, da and db, in the vector part (n8 = 1) and in the tail."""
    from pytorch_operator_amd.ops.llm import swiglu
    a = torch.randn(9, generator=_gen(9)).to(BF16)
    av = a.view(torch.int16)
    av[2], av[5], av[8] = -1, 0x7fff, 0x7fc0  # bits 0xffff, 0x7fff, 0x7fc0
    nan = torch.tensor([k in (2, 5, 8) for k in range(9)])
    ag = a.cuda().requires_grad_(True)
    bg = torch.full((9,), 0.5, dtype=BF16, device="cuda", requires_grad=True)
    y = swiglu(ag, bg)
    y.backward(torch.ones(9, dtype=BF16, device="cuda"))
    for t in (y.detach(), ag.grad, bg.grad):
        assert torch.equal(_bf16_is_nan(t.cpu()), nan), t.cpu().view(torch.int16)


# --------------------------------------------------------------------------------- AdamW
HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
BIG = 8192 * 256 * 4 + 3075  # 8 391 683: past the 8192-block grid; the 3-element tail is block 3 / thread 0's second trip
THIRD = float(torch.tensor(1 / 3, dtype=F32))  # the fp32 the launcher receives
ADAM_PAIRS = [(BF16, True), (BF16, False), (F32, True), (F32, False)]
ADAM_IDS = ["gbf16-out", "gbf16-noout", "g32-out", "g32-noout"]


@functools.lru_cache(maxsize=4)
def _adam_inputs(n, gdt, steps):
    g = _gen(4 + n)
    w = torch.randn(n, generator=g)
    m0, v0 = 0.1 * torch.randn(n, generator=g), 0.1 * torch.rand(n, generator=g)
    return w, m0, v0, [torch.randn(n, generator=g).to(gdt) for _ in range(steps)]


def _adam_device(w, m0, v0, grads, out, first_step, grad_scale, clip=None):
    """The steps through pto_adamw_step_scaled / pto_adamw_step_clipped (clip = (device sumsq,
    max_norm)); returns CPU (master, m, v, bf16 weight or None)."""
    from pytorch_operator_amd.ops import _native
    lib = _native.load()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, m, v = w.cuda(), m0.cuda(), v0.cuda()
    wb = torch.zeros(w.numel(), dtype=BF16, device="cuda") if out else None
    for k, g in enumerate(grads):
        gg = g.cuda()
        args = (p.data_ptr(), m.data_ptr(), v.data_ptr(), gg.data_ptr(), wb.data_ptr() if out else None, w.numel(),
                1 if g.dtype == BF16 else 0, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], first_step + k,
                grad_scale)
        if clip is None:
            assert lib.pto_adamw_step_scaled(*args, s) == 0
        else:
            assert lib.pto_adamw_step_clipped(*args, clip[0].data_ptr(), clip[1], s) == 0
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), wb.cpu() if out else None


def _adam_fp64(w, m0, v0, grads, first_step, grad_scale, sumsq=None, max_norm=None):
    p, m, v = w.double(), m0.double(), v0.double()
    for k, g in enumerate(grads):
        p, m, v = adamw_step_fp64(p, m, v, g, step=first_step + k, grad_scale=grad_scale, sumsq=sumsq,
                                  max_norm=max_norm, **HP)
    return p, m, v


def _adam_assert(got, want):
    """m, v and master within rtol 1e-5 / atol 1e-6 of fp64 (attained by correct fp32 arithmetic:
    tests/test_adamw_reference_cpu.py); the bf16 weight is RNE of the kernel's own master."""
    p, m, v, wb = got
    for a, b in zip((m, v, p), (want[1], want[2], want[0])):
        torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-6)
    if wb is not None:
        assert torch.equal(wb.view(torch.int16), p.bfloat16().view(torch.int16))


@pytest.mark.parametrize("first_step", [1, 1000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25, THIRD], ids=["gs1", "gs0.25", "gs1/3"])
@pytest.mark.parametrize("gdt,out", ADAM_PAIRS, ids=ADAM_IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023])
def test_adamw_entry_matches_fp64(n, gdt, out, grad_scale, first_step):
    """All four (gradient dtype, bf16 weight) instantiations of the unclipped kernel, four steps:
    n < 4 is the scalar tail alone (n4 == 0), 4 one vector and an empty tail, 5 and 1023 both."""
    w, _, _, grads = _adam_inputs(n, gdt, 4)
    z = torch.zeros(n)
    got = _adam_device(w, z, z, grads, out, first_step, grad_scale)
    _adam_assert(got, _adam_fp64(w, z, z, grads, first_step, grad_scale))


@pytest.mark.parametrize("gdt,out,grad_scale,first_step",
                         [(BF16, True, 1.0, 1), (BF16, False, 0.25, 1000), (F32, True, THIRD, 1), (F32, False, THIRD, 1000)],
                         ids=ADAM_IDS)
def test_adamw_grid_stride_second_trip(gdt, out, grad_scale, first_step):
    """n = 8192 * 256 * 4 + 3075: threads 0..768 of the capped grid take a second trip and the
    3-element scalar tail is handled on one.  Two steps.  grad_scale and the step number are
    kernel arguments, not branches (crossed in full at the small sizes), so each instantiation
    runs one combination here."""
    assert BIG // 4 > 8192 * 256 and BIG % 4 == 3
    w, _, _, grads = _adam_inputs(BIG, gdt, 2)
    z = torch.zeros(BIG)
    got = _adam_device(w, z, z, grads, out, first_step, grad_scale)
    _adam_assert(got, _adam_fp64(w, z, z, grads, first_step, grad_scale))


@pytest.mark.parametrize("gdt,out", ADAM_PAIRS, ids=ADAM_IDS)
@pytest.mark.parametrize("sumsq", [0.81, 16.0, 0.0, math.inf, math.nan], ids=["below", "above", "zero", "inf", "nan"])
def test_adamw_clipped_entry(sumsq, gdt, out):
    """pto_adamw_step_clipped with max_norm = 1 and the device scalar sum(g^2) written by the test.
    Norm 0.9 and 0: the coefficient is exactly 1 and the result is the unclipped entry's, bit for
    bit.  Norm 4: scaled by 1 / (4 + 1e-6).  inf: finite gradients are scaled to 0, the moments
    only decay.  NaN: every output is NaN."""
    n, gs = 1023, 0.25
    w, m0, v0, grads = _adam_inputs(n, gdt, 4)
    sq = torch.tensor([sumsq], dtype=F32)
    got = _adam_device(w, m0, v0, grads, out, 1, gs, clip=(sq.cuda(), 1.0))
    if math.isnan(sumsq):
        assert all(bool(t.isnan().all()) for t in got[:3])
        assert got[3] is None or bool(_bf16_is_nan(got[3]).all())
        return
    assert all(bool(t.float().isfinite().all()) for t in got if t is not None)
    _adam_assert(got, _adam_fp64(w, m0, v0, grads, 1, gs, sumsq=float(sq), max_norm=1.0))
    if sumsq < 1:
        plain = _adam_device(w, m0, v0, grads, out, 1, gs)
        for a, b in zip(got, plain):
            assert a is None or torch.equal(a.view(torch.int16), b.view(torch.int16))
    if math.isinf(sumsq):
        assert torch.equal(got[1], _decay(m0, HP["b1"], 4)) and torch.equal(got[2], _decay(v0, HP["b2"], 4))


def _decay(t, b, steps):
    """t after `steps` of `t = b * t + (1 - b) * 0` in fp32, as the kernel computes it."""
    b = torch.tensor(b, dtype=F32)
    for _ in range(steps):
        t = b * t
    return t


def test_adamw_bf16_weight_keeps_nan():
    """fp32 gradient NaNs of every kind -- the default quiet NaN, payloads whose round-to-nearest
    carry would run out of the exponent (0x7fffffff -> bf16 -0.0, 0xffffffff -> +0.0), a signalling
    NaN, and a negative one with the smallest carrying low half -- leave the fp32 master NaN after
    one step, and the bf16 weight the matmuls read must be NaN there too."""
    n = 8
    g = torch.randn(n, generator=_gen(21))
    g.view(torch.int32)[[0, 1, 3, 4, 6]] = _bits([0x7fc00000, 0x7fffffff, 0xffffffff, 0x7f80ffff,
                                                  0xffff8001]).view(torch.int32)
    nan = torch.tensor([k in (0, 1, 3, 4, 6) for k in range(n)])
    w = torch.randn(n, generator=_gen(22))
    z = torch.zeros(n)
    p, m, v, wb = _adam_device(w, z, z, [g], True, 1, 1.0)
    assert torch.equal(p.isnan(), nan) and torch.equal(m.isnan(), nan) and torch.equal(v.isnan(), nan)
    assert torch.equal(_bf16_is_nan(wb), nan), ([hex(b & 0xffff) for b in wb.view(torch.int16).tolist()],
                                                [hex(b & 0xffffffff) for b in p.view(torch.int32).tolist()])
    assert torch.equal(wb[~nan].view(torch.int16), p[~nan].bfloat16().view(torch.int16))
