"""GPU: fused RMSNorm HIP kernels vs the fp32 reference, and the large-model DDP worker."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 64), (37, 4096), (5, 1000), (2, 3, 8192)])
def test_rmsnorm_matches_reference(dtype, shape):
    from pytorch_operator_amd.ops.norm import rms_norm, rms_norm_reference
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(*shape, generator=g).to("cuda", dtype).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(shape[-1], generator=g)).cuda().requires_grad_(True)
    dy = torch.randn(*shape, generator=g).to("cuda", dtype)
    y = rms_norm(x, w, 1e-5)
    (y.float() * dy.float()).sum().backward()
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    yr = rms_norm_reference(xr, wr, 1e-5)
    (yr * dy.float()).sum().backward()
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(y.float(), yr, **tol)
    torch.testing.assert_close(x.grad.float(), xr.grad, **tol)
    _assert_dw(w.grad, x.detach(), w.detach(), dy)


def _assert_dw(dw, x, w, dy, stats_from=None):
    """dw_j against fp64 of the values the backward kernel reads: |dw_j - dw64_j| <= 1e-5 *
    sum_rows |dy x rstd|.  Both sides start from the same values and the kernel accumulates in
    fp32 over <= 8 rows per block plus <= 32 column-sum slices: under 64 roundings, 3.8e-6."""
    from llm_refs import FP32_E, rmsnorm_fp64, worst_ratio
    D = x.shape[-1]
    ref = rmsnorm_fp64(x.cpu().reshape(-1, D), w.cpu(), dy.cpu().reshape(-1, D), 1e-5,
                       stats_from=None if stats_from is None else stats_from.reshape(-1, D))
    ratio = worst_ratio(dw.cpu(), ref["dw"], FP32_E * ref["dwmag"])
    print(f"dw worst error/bound {ratio:.3f}")
    assert ratio <= 1


@pytest.mark.parametrize("shape", [(37, 4096), (2, 3, 8192), (5, 1000)])
def test_rmsnorm_fp32_in_bf16_out(shape):
    """The autocast path: fp32 residual stream in, bf16 normalised output, bf16 dy back."""
    from pytorch_operator_amd.ops.norm import rms_norm, rms_norm_reference
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(*shape, generator=g).cuda().requires_grad_(True)
    w = (1 + 0.1 * torch.randn(shape[-1], generator=g)).cuda().requires_grad_(True)
    dy = torch.randn(*shape, generator=g).to("cuda", torch.bfloat16)
    y = rms_norm(x, w, 1e-5, torch.bfloat16)
    assert y.dtype == torch.bfloat16
    (y.float() * dy.float()).sum().backward()
    assert x.grad.dtype == torch.float32
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    (rms_norm_reference(xr, wr, 1e-5) * dy.float()).sum().backward()
    torch.testing.assert_close(y.float(), rms_norm_reference(x.detach(), w.detach(), 1e-5), rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(x.grad, xr.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(w.grad, wr.grad, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 32, 128), (1, 7, 3, 16), (3, 128, 8, 64)])
def test_rope_matches_reference(dtype, shape):
    from pytorch_operator_amd.models.llama import rope_tables
    from pytorch_operator_amd.ops.llm import rope, rope_reference
    g = torch.Generator(device="cpu").manual_seed(2)
    B, S, H, D = shape
    cos, sin = rope_tables(D, S, 500000.0, "cuda")
    x = torch.randn(*shape, generator=g).to("cuda", dtype).requires_grad_(True)
    dy = torch.randn(*shape, generator=g).to("cuda", dtype)
    y = rope(x, cos, sin)
    y.backward(dy)
    xr = x.detach().float().requires_grad_(True)
    yr = rope_reference(xr, cos, sin)
    yr.backward(dy.float())
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(y.float(), yr, **tol)
    torch.testing.assert_close(x.grad.float(), xr.grad, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [8, 4099, 2 * 14336 * 3])
def test_swiglu_matches_reference(dtype, n):
    from pytorch_operator_amd.ops.llm import swiglu
    g = torch.Generator(device="cpu").manual_seed(3)
    a = (2 * torch.randn(n, generator=g)).to("cuda", dtype).requires_grad_(True)
    b = torch.randn(n, generator=g).to("cuda", dtype).requires_grad_(True)
    dy = torch.randn(n, generator=g).to("cuda", dtype)
    y = swiglu(a, b)
    y.backward(dy)
    ar, br = (t.detach().float().requires_grad_(True) for t in (a, b))
    yr = torch.nn.functional.silu(ar) * br
    yr.backward(dy.float())
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=2e-2)
    torch.testing.assert_close(y.float(), yr, **tol)
    torch.testing.assert_close(a.grad.float(), ar.grad, **tol)
    torch.testing.assert_close(b.grad.float(), br.grad, **tol)


@pytest.mark.parametrize("n", [4096, 1001, 3 * 1024 * 1024 + 3])
@pytest.mark.parametrize("grad_dtype,param_dtype", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)])
def test_adamw_kernel_matches_reference(n, grad_dtype, param_dtype):
    from pytorch_operator_amd.ops.optim import MasterAdamW
    g0 = torch.Generator(device="cpu").manual_seed(4)
    w = torch.randn(n, generator=g0)
    pg = w.clone().to("cuda", param_dtype)
    pc = w.clone().to(param_dtype)
    og = MasterAdamW([pg], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    oc = MasterAdamW([pc], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    for _ in range(4):
        g = torch.randn(n, generator=g0).to(grad_dtype)
        pg.grad, pc.grad = g.cuda(), g.clone()
        og.step()
        oc.step()
    sg, sc = og.state[pg], oc.state[pc]
    for k in ("exp_avg", "exp_avg_sq"):
        torch.testing.assert_close(sg[k].cpu(), sc[k], rtol=1e-5, atol=1e-6)
    if param_dtype == torch.bfloat16:
        torch.testing.assert_close(sg["master"].cpu(), sc["master"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(pg.cpu().float(), sg["master"].cpu().bfloat16().float(), rtol=0, atol=0)
    else:
        torch.testing.assert_close(pg.cpu(), pc, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("xdt,ydt", [(torch.float32, torch.bfloat16), (torch.float32, torch.float32),
                                     (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("shape", [(37, 4096), (2, 3, 64)])
@pytest.mark.parametrize("with_gs", [True, False])
def test_add_rms_norm_matches_reference(xdt, ydt, shape, with_gs):
    """Residual-fused RMSNorm: s = x + delta, y = norm(s); backward dx = gs + d(norm) (also
    written as d(delta) in the branch dtype) and dw, vs fp32 autograd of the unfused ops."""
    from pytorch_operator_amd.ops.norm import add_rms_norm, rms_norm_reference
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(*shape, generator=g).to(xdt)
    d = torch.randn(*shape, generator=g).to(ydt)
    w = 1 + 0.1 * torch.randn(shape[-1], generator=g)
    gy = torch.randn(*shape, generator=g).to(ydt)
    gs = torch.randn(*shape, generator=g).to(xdt)
    xg, dg, wg = (t.cuda().requires_grad_(True) for t in (x, d, w))
    s, y = add_rms_norm(xg, dg, wg, 1e-5, ydt)
    assert s.dtype == xdt and y.dtype == ydt
    loss = (y.float() * gy.cuda().float()).sum() + ((s.float() * gs.cuda().float()).sum() if with_gs else 0)
    loss.backward()
    xr, dr, wr = (t.float().requires_grad_(True) for t in (x, d, w))
    sr = xr + dr
    yr = rms_norm_reference(sr, wr, 1e-5)
    lr = (yr * gy.float()).sum() + ((sr * gs.float()).sum() if with_gs else 0)
    lr.backward()
    lo = xdt == torch.bfloat16 or ydt == torch.bfloat16
    tol = dict(rtol=2e-2, atol=2e-2) if lo else dict(rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(s.float().cpu(), sr.detach(), **tol)
    torch.testing.assert_close(y.float().cpu(), yr.detach(), **tol)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, **tol)
    torch.testing.assert_close(dg.grad.float().cpu(), dr.grad, **tol)
    # the backward reads the s the forward stored (rounded to xdt) with the unrounded sum's statistics
    _assert_dw(wg.grad, s.detach(), w, gy, stats_from=x.double() + d.double())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 32, 8, 128), (1, 7, 4, 2, 16), (3, 33, 8, 8, 64)])
def test_rope_qkv_matches_reference(dtype, shape):
    """Fused QKV split + RoPE (and its packed backward) vs the fp32 split/rotate reference."""
    from pytorch_operator_amd.models.llama import rope_tables
    from pytorch_operator_amd.ops.llm import rope_qkv, rope_qkv_reference
    B, S, hq, hkv, D = shape
    W = (hq + 2 * hkv) * D
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(B, S, W, generator=g).to(dtype)
    cos, sin = rope_tables(D, S, 500000.0)
    dq, dk, dv = (torch.randn(B, S, h, D, generator=g).to(dtype) for h in (hq, hkv, hkv))
    xg = x.cuda().requires_grad_(True)
    outs = rope_qkv(xg, cos.cuda(), sin.cuda(), hq, hkv)
    sum((o.float() * d.cuda().float()).sum() for o, d in zip(outs, (dq, dk, dv))).backward()
    xr = x.float().requires_grad_(True)
    refs = rope_qkv_reference(xr, cos, sin, hq, hkv)
    sum((o * d.float()).sum() for o, d in zip(refs, (dq, dk, dv))).backward()
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-2)
    for o, r in zip(outs, refs):
        assert o.is_contiguous()
        torch.testing.assert_close(o.float().cpu(), r.detach(), **tol)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 2 * 14336), (7, 2 * 136), (3, 5, 32)])
def test_swiglu_packed_matches_reference(dtype, shape):
    from pytorch_operator_amd.ops.llm import swiglu_packed, swiglu_packed_reference
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(*shape, generator=g).to(dtype)
    dy = torch.randn(*shape[:-1], shape[-1] // 2, generator=g).to(dtype)
    xg = x.cuda().requires_grad_(True)
    y = swiglu_packed(xg)
    (y.float() * dy.cuda().float()).sum().backward()
    xr = x.float().requires_grad_(True)
    yr = swiglu_packed_reference(xr)
    (yr * dy.float()).sum().backward()
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(y.float().cpu(), yr.detach(), **tol)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, **tol)


@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,v", [(64, 256), (7, 1000), (5, 128256)])
def test_cross_entropy_matches_reference(dtype, n, v, overwrite):
    """Fused HIP cross-entropy (loss + d(logits), in place or into a new tensor) vs fp32
    F.cross_entropy, with ignored (-100) targets and large-magnitude logits (the online max
    must rescale).  The default keeps the caller's logits intact."""
    from pytorch_operator_amd.ops.llm import cross_entropy
    g = torch.Generator(device="cpu").manual_seed(7)
    x = (torch.randn(n, v, generator=g) * 8).to(dtype)
    t = torch.randint(0, v, (n,), generator=g)
    t[1] = -100
    xg = x.cuda().requires_grad_(True)
    y = xg * 1  # an intermediate (overwritten by the backward when overwrite=True)
    y_before = y.detach().clone()
    loss = cross_entropy(y, t.cuda(), overwrite_logits=overwrite)
    (loss * 3).backward()
    xr = x.float().requires_grad_(True)
    lr = torch.nn.functional.cross_entropy(xr, t, ignore_index=-100)
    (lr * 3).backward()
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=1e-5)
    torch.testing.assert_close(loss.cpu(), lr, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, **tol)
    assert xg.grad[1].abs().max().item() == 0
    if not overwrite:
        assert torch.equal(y.detach(), y_before)  # the caller may still read its logits
    else:
        assert y._version > y_before._version  # reuse of the overwritten logits is detectable


@pytest.mark.parametrize("shape", [(64, 128), (8192 // 8, 28672 // 8), (192, 64)])
def test_transpose2d_bf16(shape):
    from pytorch_operator_amd.ops.llm import transpose2d
    x = torch.randn(*shape, device="cuda").to(torch.bfloat16)
    assert torch.equal(transpose2d(x), x.t().contiguous())


@pytest.mark.parametrize("dims", [(2, 64, 128, 192), (1, 128, 256, 64), (3, 5, 24, 40)])
def test_linear_tn_matches_reference(dims):
    """TN-backward linear (transposed operand copies) vs fp32 autograd of x.W^T, bf16 in/out;
    the last shape is not a multiple of 64 (PyTorch transpose fallback)."""
    from pytorch_operator_amd.ops.llm import linear_tn
    B, S, fin, fout = dims
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(B, S, fin, generator=g).to(torch.bfloat16)
    w = (torch.randn(fout, fin, generator=g) * 0.05).to(torch.bfloat16)
    dy = torch.randn(B, S, fout, generator=g).to(torch.bfloat16)
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = linear_tn(xg, wg)
    y.backward(dy.cuda())
    xr, wr = x.float().requires_grad_(True), w.float().requires_grad_(True)
    yr = torch.nn.functional.linear(xr, wr)
    yr.backward(dy.float())
    torch.testing.assert_close(y.float().cpu(), yr.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad, rtol=2e-2, atol=5e-2)
    torch.testing.assert_close(wg.grad.float().cpu(), wr.grad, rtol=2e-2, atol=1e-1)
    assert xg.grad.dtype == wg.grad.dtype == torch.bfloat16


def test_master_adamw_overlap_matches_serial():
    """AdamW on a side stream overlapped with the next forward (per-module ready events) gives
    bit-identical weights and masters to the serial optimizer step."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import MasterAdamW, install_overlap, to_bf16_matmul_weights
    torch.manual_seed(0)
    tok = torch.randint(0, 256, (2, 65)).cuda()
    runs = []
    for overlap in (False, True):
        torch.manual_seed(3)
        m = Llama(CONFIGS["llama-tiny"]).cuda()
        to_bf16_matmul_weights(m)
        opt = MasterAdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, overlap=overlap)
        if overlap:
            assert install_overlap(m) > 0
        for _ in range(4):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m(tok[:, :-1], tok[:, 1:])
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        runs.append(([p.detach().clone() for p in m.parameters()],
                     [opt.state[p]["exp_avg"].clone() for p in m.parameters()]))
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert torch.equal(a, b)


def test_zero_adamw_matches_master_adamw_on_gpu():
    """ZeRO-1 optimizer (world 1: flat fp32 gradient buckets, HIP AdamW on the bucket shard,
    weights as views of flat bf16 buckets) gives bit-identical weights to MasterAdamW."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    tok = torch.randint(0, 256, (2, 65), generator=torch.Generator().manual_seed(0)).cuda()
    runs = []
    for zero in (False, True):
        torch.manual_seed(3)
        m = Llama(CONFIGS["llama-tiny"]).cuda()
        to_bf16_matmul_weights(m)
        if zero:
            opt = ZeroAdamW(m, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, bucket_mb=0.05)
            assert len(opt.buckets) > 2
        else:
            opt = MasterAdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
        for _ in range(4):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m(tok[:, :-1], tok[:, 1:])
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        runs.append([p.detach().clone() for p in m.parameters()])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


def test_llama_tiny_master_weights_trains_on_gpu():
    res = _run("--model", "llama-tiny", "--seq-len", "128", "--batch-size", "4", "--steps", "30", "--warmup", "2",
               "--lr", "3e-3", "--master-weights", "on")
    assert res["master_weights"] is True and res["loss"] < 5.0


def test_llama_tiny_fused_matches_eager_reference():
    """Whole-model check: the tiny Llama with the HIP kernels vs the same weights on CPU (fp32)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(0)
    cpu = Llama(CONFIGS["llama-tiny"])
    gpu = Llama(CONFIGS["llama-tiny"]).cuda()
    gpu.load_state_dict(cpu.state_dict())
    tok = torch.randint(0, 256, (2, 33))
    lc = cpu(tok[:, :-1], tok[:, 1:])
    lc.backward()
    lg = gpu(tok[:, :-1].cuda(), tok[:, 1:].cuda())
    lg.backward()
    torch.testing.assert_close(lg.cpu(), lc, rtol=1e-4, atol=1e-4)
    for (n, pc), pg in zip(cpu.named_parameters(), gpu.parameters()):
        torch.testing.assert_close(pg.grad.cpu(), pc.grad, rtol=2e-3, atol=2e-5, msg=n)


def _run(*args):
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", *args], capture_output=True,
                       text=True, timeout=600, cwd=ROOT, env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])


def test_llama_tiny_trains_on_gpu():
    res = _run("--model", "llama-tiny", "--seq-len", "128", "--batch-size", "4", "--steps", "30", "--warmup", "2",
               "--lr", "3e-3")
    assert res["loss"] < 5.0  # log(256) = 5.55 at init; memorising a fixed batch drives it down


@pytest.mark.parametrize("zero", ["0", "1"])
def test_llama_tiny_checkpoint_resume_on_gpu(tmp_path, zero):
    """GPU (HIP AdamW, bf16 weights + fp32 masters; ZeRO-1 shard state): 2 steps + checkpoint +
    2 resumed steps give the loss of 4 uninterrupted steps."""
    base = ["--model", "llama-tiny", "--seq-len", "64", "--batch-size", "2", "--warmup", "1", "--lr", "3e-3",
            "--zero", zero]
    full = _run(*base, "--steps", "3")
    ck = str(tmp_path / "ck")
    _run(*base, "--steps", "1", "--ckpt-dir", ck)
    res = _run(*base, "--steps", "1", "--ckpt-dir", ck)
    assert res["checkpoint_step"] == 4 and res["zero"] == int(zero)
    assert res["loss"] == full["loss"]


def test_resnet50_bf16_step_on_gpu():
    res = _run("--model", "resnet50", "--batch-size", "32", "--steps", "3", "--warmup", "1")
    assert res["value"] > 0 and res["loss"] == res["loss"]


def test_zero_grad_view_matches_master_adamw():
    """ZeRO-1 gradient-as-bucket-view at world 1 on the GPU: the TN-linear backward GEMMs write
    dW straight into the bf16 buckets (no .grad, no copy pass) and the result is bit-identical
    to MasterAdamW stepping autograd's bf16 .grad -- also with the AdamW grad scale path."""
    import copy
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    torch.manual_seed(0)
    with torch.device("cuda"):
        m1 = Llama(CONFIGS["llama-tiny"])
    m2 = copy.deepcopy(m1)
    to_bf16_matmul_weights(m1)
    to_bf16_matmul_weights(m2)
    o1 = MasterAdamW(m1.parameters(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1)
    o2 = ZeroAdamW(m2, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, bucket_mb=0.05)
    assert o2.sinks > 0 and all(b.unscaled for b in o2.buckets if b.gdt == torch.bfloat16)
    assert {b.gdt for b in o2.buckets} == {torch.bfloat16, torch.float32}
    x = torch.randint(0, 256, (2, 65), device="cuda")
    for _ in range(3):
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m(x[:, :-1], x[:, 1:])
            loss.backward()
            if o is o2:  # the sinks took every matmul weight's gradient: no .grad was materialised
                assert all(p.grad is None for p in m2.parameters())
            o.step()
    torch.cuda.synchronize()
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(a, b), n


@pytest.mark.timeout(300)
def test_zero_grad_view_matches_copy_path_at_world2(tmp_path):
    """ZeRO-1 grad_view at world 2 (two gloo ranks sharing the GPU, bf16 reduce-
    scatter): unscaled bucket sums + 1/W inside AdamW give bit-identical fp32 masters and bf16
    weights to the copy path that scales every deposit by 1/W (exact for power-of-two W)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        str(ROOT / "tools" / "zero_gv_check.py"), "--backend", "gloo", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=280, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=str(ROOT)))
    # per-rank files, not stdout: both ranks share one pipe and their lines interleave (round 4)
    lines = [json.loads((tmp_path / f"rank{k}.json").read_text()) for k in range(2)
             if (tmp_path / f"rank{k}.json").exists()]
    assert r.returncode == 0 and len(lines) == 2, r.stdout[-2000:] + r.stderr[-3000:]
    assert all(x["masters_equal"] and x["weights_equal"] and x["sinks"] > 0 for x in lines), lines
    assert lines[0]["digest"] == lines[1]["digest"], lines
