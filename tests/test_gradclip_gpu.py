"""Global-norm gradient clipping on the GPU: the sum-of-squares / finish kernels
(csrc/kernels/gradclip.hip), the clipped AdamW entry point (adamw.hip), and the two optimizers
and the worker that use them.  The CPU reference paths are pinned in tests/test_gradclip_cpu.py.
"""
import copy
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SIZES = [1, 3, 7, 8, 255, 256, 1001, 4096, 4099, 3 * 1024 * 1024 + 3]
DTYPES = [torch.bfloat16, torch.float32]


def _values(n, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    return torch.randn(n, generator=g).to(dtype)


def _ref_norm(pairs):
    """fp64 norm of the same values: sqrt(sum((scale * g)^2))."""
    return math.sqrt(sum(float((g.double() * s).pow(2).sum()) for g, s in pairs))


def _device_norm(pairs):
    from pytorch_operator_amd.ops.gradclip import DeviceGradNorm
    out = DeviceGradNorm().run(pairs)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq_matches_fp64(n, dtype, scale):
    """Sizes: scalar tail only (1, 3, 7 for bf16; 1, 3 for fp32), exactly one vector (8 bf16; 4 + 4
    fp32), tails of 1-3, one block (<= 256 vectors) and several, and a grid-stride run (fp32 at
    3M+3: 786432 vectors over the 2048-block cap, two strided vectors per thread; a second trip
    round the unrolled loop needs > 2M vectors: test_grad_sumsq_second_loop_trip).

    Tolerance 1e-5 on the norm.  The terms are non-negative, so the sum's relative error is at
    most (roundings on the longest chain) x 2^-24.  Longest chain of THIS kernel at these sizes:
    1 (scale) + 9 fused multiply-adds into one accumulator (bf16: the 8 elements of a thread's one
    vector, + 1 tail element; a grid-stride thread's second vector goes to another accumulator)
    + 2 (four accumulators, pairwise) + 6 wave steps + 2 (four waves, pairwise) + 1 (the finish
    kernel sums the partials in double and rounds once) = 21 roundings: <= 1.3e-6 on the sum, half
    of that on the root, plus the root's own rounding."""
    g = _values(n, dtype)
    out = _device_norm([(g.cuda(), scale)])
    want = _ref_norm([(g, scale)])
    print(f"n={n} {dtype} scale={scale}: norm {float(out[1])!r} want {want!r} rel {abs(float(out[1]) - want) / want:.2e}")
    assert abs(float(out[1]) - want) <= 1e-5 * want
    assert abs(float(out[0]) - want * want) <= 2e-5 * want * want
    assert abs(float(out[1]) - float(out[0].sqrt())) <= 2.0 ** -23 * float(out[1])  # the device sqrtf: 1 ulp


@pytest.mark.parametrize("dtype,n", [(torch.bfloat16, 17_000_005), (torch.float32, 9_000_003)], ids=["bf16", "fp32"])
def test_grad_sumsq_second_loop_trip(dtype, n):
    """More than 4 x 2048 x 256 vectors: some threads go round the 4-way unrolled grid-stride loop
    twice (the chain grows by one vector's 4 or 8 fused multiply-adds: still under 30 roundings)."""
    g = _values(n, dtype)
    assert n // (16 // g.element_size()) > 4 * 2048 * 256
    out = _device_norm([(g.cuda(), 1.0)])
    want = _ref_norm([(g, 1.0)])
    assert abs(float(out[1]) - want) <= 1e-5 * want


def test_two_buffers_in_consecutive_regions_finish_together():
    a, b = _values(4099, torch.bfloat16, 1), _values(3 * 1024 * 1024 + 3, torch.float32, 2)
    c = _values(7, torch.float32, 3)
    pairs = [(a, 1.0), (b, 0.25), (c, 1.0)]
    out = _device_norm([(t.cuda(), s) for t, s in pairs])
    want = _ref_norm(pairs)
    assert abs(float(out[1]) - want) <= 1e-5 * want


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [4099, 3 * 1024 * 1024 + 3])
def test_grad_sumsq_is_bitwise_reproducible(n, dtype):
    """No float atomics: the same buffer twice, and the same values at another 16-byte-aligned
    address, give the same bits."""
    from pytorch_operator_amd.ops.gradclip import DeviceGradNorm
    g = _values(n, dtype).cuda()
    norm = DeviceGradNorm()
    first = norm.run([(g, 1.0)]).clone()
    second = norm.run([(g, 1.0)]).clone()
    shift = 16 // g.element_size()  # one 16-byte step off the allocator's alignment
    moved = torch.empty(n + 3 * shift, dtype=dtype, device="cuda")[3 * shift:]
    moved.copy_(g)
    assert moved.data_ptr() % 16 == 0 and moved.data_ptr() != g.data_ptr()
    third = DeviceGradNorm().run([(moved, 1.0)]).clone()
    torch.cuda.synchronize()
    assert float(first[0]) > 0
    for other in (second, third):
        assert torch.equal(first.view(torch.int32), other.view(torch.int32))


def test_launchers_reject_bad_arguments():
    import ctypes
    from pytorch_operator_amd.ops import _native
    lib = _native.load()
    g = torch.ones(4096, device="cuda")
    ws = torch.zeros(64, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    parts = lib.pto_grad_sumsq_parts(4096, 0)
    assert parts == 4 and lib.pto_grad_sumsq_parts(3 * 1024 * 1024 + 3, 0) == 2048
    assert lib.pto_grad_sumsq(g.data_ptr(), 0, 0, 1.0, ws.data_ptr(), 64, s) == -1
    assert lib.pto_grad_sumsq(g.data_ptr() + 4, 4095, 0, 1.0, ws.data_ptr(), 64, s) == -2
    assert lib.pto_grad_sumsq(g.data_ptr(), 4096, 0, 1.0, ws.data_ptr(), parts - 1, s) == -3
    assert lib.pto_grad_sumsq_finish(ws.data_ptr(), 0, ws.data_ptr(), s) == -1
    m = torch.zeros(4096, device="cuda")
    assert lib.pto_adamw_step_clipped(m.data_ptr(), m.data_ptr(), m.data_ptr(), g.data_ptr(), None, 4096, 0,
                                      1e-3, 0.9, 0.95, 1e-8, 0.1, 1, 1.0, None, 1.0, s) == -2
    torch.cuda.synchronize()
    assert float(m.abs().sum()) == 0  # nothing was launched


@pytest.mark.parametrize("n", [1001, 4096])
@pytest.mark.parametrize("grad_dtype,param_dtype", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)])
def test_clipped_adamw_kernel_matches_reference(n, grad_dtype, param_dtype):
    """GPU MasterAdamW(max_grad_norm=c) against the CPU reference path.  Unit-variance gradients
    have norm ~ sqrt(n) = c; scaled by 4 and 1/4 on alternate steps they clip and do not clip."""
    from pytorch_operator_amd.ops.optim import MasterAdamW
    c = math.sqrt(n)
    g0 = torch.Generator(device="cpu").manual_seed(4)
    w = torch.randn(n, generator=g0)
    pg = w.clone().to("cuda", param_dtype)
    pc = w.clone().to(param_dtype)
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_grad_norm=c)
    og, oc = MasterAdamW([pg], **kw), MasterAdamW([pc], **kw)
    norms = []
    for k in range(4):
        g = (torch.randn(n, generator=g0) * (4.0 if k % 2 == 0 else 0.25)).to(grad_dtype)
        pg.grad, pc.grad = g.cuda(), g.clone()
        og.step()
        oc.step()
        norms.append((float(og.last_grad_norm()), float(oc.last_grad_norm())))
    assert [a > c for a, _ in norms] == [True, False, True, False], (c, norms)
    for a, b in norms:
        assert abs(a - b) <= 1e-5 * b, norms
    sg, sc = og.state[pg], oc.state[pc]
    for k in ("exp_avg", "exp_avg_sq"):
        torch.testing.assert_close(sg[k].cpu(), sc[k], rtol=2e-5, atol=1e-6)
    if param_dtype == torch.bfloat16:
        torch.testing.assert_close(sg["master"].cpu(), sc["master"], rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(pg.cpu().float(), sg["master"].cpu().bfloat16().float(), rtol=0, atol=0)
    else:
        torch.testing.assert_close(pg.cpu(), pc, rtol=2e-5, atol=1e-6)


def _tiny_pair(c, grad_view):
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    torch.manual_seed(0)
    with torch.device("cuda"):
        m1 = Llama(CONFIGS["llama-tiny"])
    m2 = copy.deepcopy(m1)
    to_bf16_matmul_weights(m1)
    to_bf16_matmul_weights(m2)
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, max_grad_norm=c)
    o1 = MasterAdamW(m1.parameters(), **kw)
    o2 = ZeroAdamW(m2, bucket_mb=0.02, grad_view=grad_view, **kw)
    return (m1, o1), (m2, o2)


def _fwd_bwd(m, o, x):
    o.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = m(x[:, :-1], x[:, 1:])
    loss.backward()


@pytest.mark.parametrize("grad_view", [True, False])
def test_zero_adamw_clipped_matches_master_adamw_on_gpu(grad_view):
    c = 1e-3
    (m1, o1), (m2, o2) = _tiny_pair(c, grad_view)
    assert len(o2.buckets) > 2 and (o2.sinks > 0) == grad_view
    x = torch.randint(0, 256, (2, 65), generator=torch.Generator().manual_seed(0)).cuda()
    for _ in range(3):
        for m, o in ((m1, o1), (m2, o2)):
            _fwd_bwd(m, o, x)
            o.step()
        n1, n2 = float(o1.last_grad_norm()), float(o2.last_grad_norm())
        assert n1 > c, n1  # clipping was active
        assert abs(n1 - n2) <= 1e-5 * n1, (n1, n2)
    torch.cuda.synchronize()
    of = {id(p): b for b in o2.buckets for p in b.params}
    for (name, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        b, off = of[id(p2)], of[id(p2)].slot[id(p2)]
        ms2 = (b.master if b.master is not None else b.flat_w)[off:off + p2.numel()].view(p2.shape)
        ms1 = o1.state[p1]["master"] if o1.state[p1]["master"] is not None else p1
        torch.testing.assert_close(ms2, ms1.detach(), rtol=2e-5, atol=1e-6, msg=name)


def test_clipped_step_has_no_host_round_trip():
    """After one warm-up step (allocations), a clipped step() of either optimizer synchronises
    nothing: the norm stays on the device between the finish kernel and AdamW."""
    (m1, o1), (m2, o2) = _tiny_pair(1e-3, True)
    x = torch.randint(0, 256, (2, 65), generator=torch.Generator().manual_seed(0)).cuda()
    for m, o in ((m1, o1), (m2, o2)):
        _fwd_bwd(m, o, x)
        o.step()
        _fwd_bwd(m, o, x)
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            o.step()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        torch.cuda.synchronize()
        assert float(o.last_grad_norm()) > 1e-3


def test_worker_reports_grad_norm_on_gpu():
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", "--model", "llama-tiny",
                        "--seq-len", "128", "--batch-size", "2", "--steps", "2", "--warmup", "1",
                        "--max-grad-norm", "1e-3"], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    first = json.loads([ln for ln in r.stdout.splitlines() if '"first_step"' in ln][-1])
    assert res["master_weights"] is True and res["max_grad_norm"] == 1e-3
    assert res["grad_norm"] > res["max_grad_norm"] and first["grad_norm"] > res["max_grad_norm"]
    assert math.isfinite(res["loss"])
