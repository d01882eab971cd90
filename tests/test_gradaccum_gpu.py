"""Gradient accumulation on the GPU: the fold kernel (csrc/kernels/gradaccum.hip) against PyTorch,
bit for bit, and ``MasterAdamW`` / ``ZeroAdamW`` / the worker with ``grad_accum > 1``."""
import copy
import ctypes
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KW = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)


_CACHE = {}


def _values(n, dtype, seed):
    """Computed once per (n, dtype, seed) and shared; every caller gets its own device copy."""
    if (n, dtype, seed) not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(seed)
        # magnitudes over ten binades, so that adds round and bf16 roundings tie-break both ways
        x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-5, 5, (n,), generator=g).float())
        _CACHE[(n, dtype, seed)] = x.to(dtype)
    return _CACHE[(n, dtype, seed)].cuda()


def _sizes():
    from pytorch_operator_amd.ops.gradaccum import sweep
    return [1, 7, 8, 9, 2053, sweep() + 8 * 3 + 5]  # the last: a second loop trip and the tail


# out: none, a buffer of its own, or (bf16 g only) g itself
@pytest.mark.parametrize("dtype,out_kind", [(torch.bfloat16, "none"), (torch.bfloat16, "own"), (torch.bfloat16, "alias"),
                                            (torch.float32, "none"), (torch.float32, "own")],
                         ids=["bf16", "bf16-out", "bf16-alias", "fp32", "fp32-out"])
@pytest.mark.parametrize("first", [False, True], ids=["add", "first"])
def test_fold_kernel_is_bit_exact(dtype, first, out_kind):
    from pytorch_operator_amd.ops.gradaccum import fold
    for n in _sizes():
        g = _values(n, dtype, 1)
        want = g.float() if first else _values(n, torch.float32, 2) + g.float()
        acc = torch.full((n,), float("nan"), device="cuda") if first else _values(n, torch.float32, 2)
        out = {"none": None, "own": torch.zeros(n, dtype=torch.bfloat16, device="cuda"), "alias": g}[out_kind]
        fold(acc, g, first, out)
        torch.cuda.synchronize()
        assert not torch.isnan(acc).any(), n
        assert torch.equal(acc, want), n
        if out is not None:
            assert torch.equal(out, want.to(torch.bfloat16)), n


def test_fold_keeps_addends_a_bf16_sum_would_lose():
    """1.0 plus 64 addends of 2**-10, one by one: exactly 1.0625 in fp32; a bf16 running sum
    (ulp 2**-7 at 1.0) stays at 1.0."""
    from pytorch_operator_amd.ops.gradaccum import fold
    n = 1001
    acc = torch.empty(n, device="cuda")
    out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    fold(acc, torch.ones(n, dtype=torch.bfloat16, device="cuda"), True)
    small = torch.full((n,), 2.0 ** -10, dtype=torch.bfloat16, device="cuda")
    lossy = torch.ones(n, dtype=torch.bfloat16, device="cuda")
    for _ in range(64):
        fold(acc, small, False, out)
        lossy += small
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((n,), 1.0625, device="cuda"))
    assert torch.equal(out.float(), acc) and torch.equal(lossy.float(), torch.ones(n, device="cuda"))


def test_launcher_rejects_bad_arguments():
    from pytorch_operator_amd.ops import _native
    lib = _native.load()
    n = 4096
    acc = torch.zeros(n + 8, device="cuda")
    g = torch.ones(n + 8, device="cuda")
    gb = torch.ones(n + 8, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(n + 8, dtype=torch.bfloat16, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.pto_grad_accum(acc.data_ptr(), g.data_ptr(), out.data_ptr(), 0, 0, 0, s) == -1
    assert lib.pto_grad_accum(acc.data_ptr() + 4, g.data_ptr(), out.data_ptr(), n, 0, 0, s) == -2
    assert lib.pto_grad_accum(acc.data_ptr(), g.data_ptr() + 4, out.data_ptr(), n, 0, 0, s) == -2
    assert lib.pto_grad_accum(acc.data_ptr(), gb.data_ptr() + 4, out.data_ptr(), n, 1, 0, s) == -2
    assert lib.pto_grad_accum(acc.data_ptr(), g.data_ptr(), out.data_ptr() + 4, n, 0, 0, s) == -2
    assert lib.pto_grad_accum(None, g.data_ptr(), None, n, 0, 0, s) == -2
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0 and float(out.float().abs().sum()) == 0  # nothing was launched
    assert lib.pto_grad_accum_sweep() % 8 == 0 and lib.pto_grad_accum_sweep() > 0


# ---------------------------------------------------------------- MasterAdamW vs the hand-built sum
class Small(nn.Module):
    """Two bf16 linears (after ``to_bf16_matmul_weights``) and one fp32 parameter."""

    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(24, 16), nn.Tanh(), nn.Linear(16, 8))
        self.gain = nn.Parameter(torch.linspace(0.5, 1.5, 8))

    def forward(self, x):
        return (self.net(x.to(self.net[0].weight.dtype)).float() * self.gain).pow(2).mean()


@pytest.mark.parametrize("overlap", [False, True], ids=["inline", "overlap"])
@pytest.mark.parametrize("n", [2, 3])
def test_master_adamw_matches_hand_built_sum_on_gpu(n, overlap):
    """The reference forms ((g_1 + g_2) + g_3) * fp32(1/N) by hand from a twin model's autograd
    gradients and feeds it to an N = 1 MasterAdamW through the fp32-gradient hook."""
    from pytorch_operator_amd.ops.optim import MasterAdamW, install_overlap, to_bf16_matmul_weights
    torch.manual_seed(0)
    m = Small().cuda()
    ref = copy.deepcopy(m)
    to_bf16_matmul_weights(m)
    to_bf16_matmul_weights(ref)
    opt = MasterAdamW(m.parameters(), grad_accum=n, overlap=overlap, **KW)
    oref = MasterAdamW(ref.parameters(), **KW)
    if overlap:
        install_overlap(m)
    scale = torch.tensor(1.0 / n, dtype=torch.float32, device="cuda")
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        batches = [(torch.randn(8, 24, generator=gen) * 10.0 ** -k).cuda() for k in range(n)]
        opt.zero_grad(set_to_none=True)
        for k, x in enumerate(batches):
            m(x).backward()
            if k < n - 1:
                opt.accumulate()
        opt.step()
        total = {}
        for x in batches:
            for p in ref.parameters():
                p.grad = None
            ref(x).backward()
            for p in ref.parameters():
                total[p] = p.grad.float().clone() if p not in total else total[p] + p.grad.float()
        for p in ref.parameters():
            p._pto_grad32 = total[p] * scale
        oref.step()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    for (name, p), q in zip(m.named_parameters(), ref.parameters()):
        s, r = opt.state[p], oref.state[q]
        assert torch.equal(p, q) and torch.equal(s["exp_avg"], r["exp_avg"]), name
        assert torch.equal(s["exp_avg_sq"], r["exp_avg_sq"]), name
        if s["master"] is not None:
            assert torch.equal(s["master"], r["master"]), name


# ---------------------------------------------------------------- llama-mini: the HIP model kernels
def _mini(make_opt, n, steps=2, clip=False):
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-mini"])
    m = m.cuda()
    to_bf16_matmul_weights(m)
    opt = make_opt(m)
    x = torch.randint(0, 512, (1, 129), generator=torch.Generator().manual_seed(3)).cuda()
    for _ in range(steps):
        _mini_backwards(m, opt, x, n)
        opt.step()
    torch.cuda.synchronize()
    return m, opt


def _mini_backwards(m, opt, x, n):
    opt.zero_grad(set_to_none=True)
    for k in range(n):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m(x[:, :-1], x[:, 1:])
        loss.backward()
        if k < n - 1:
            opt.accumulate()


def _make(kind, **kw):
    from pytorch_operator_amd.ops.optim import MasterAdamW
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    base = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, **kw)
    if kind == "master":
        return lambda m: MasterAdamW(m.parameters(), **base)
    return lambda m: ZeroAdamW(m, bucket_mb=4.0, grad_view=kind == "zero-view", **base)


@pytest.mark.parametrize("kind", ["master", "zero-view", "zero-copy"])
def test_identical_micro_batches_equal_one_batch_on_llama_mini(kind):
    """head_dim 128: the HIP attention, norm, RoPE, SwiGLU and cross-entropy kernels produce the
    gradients; g + g and 1/2 are exact, so two copies of a batch train exactly as the batch."""
    m1, o1 = _mini(_make(kind), 1)
    m2, o2 = _mini(_make(kind, grad_accum=2), 2)
    for (name, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(a, b), name
    if kind == "master":
        for a, b in zip(m1.parameters(), m2.parameters()):
            for k in ("exp_avg", "exp_avg_sq", "master"):
                if o1.state[a][k] is not None:
                    assert torch.equal(o1.state[a][k], o2.state[b][k])
        assert len(o2._acc) == len(list(m2.parameters()))
    else:
        assert len(o2.buckets) > 2 and (o2.sinks > 0) == (kind == "zero-view")
        for a, b in zip(o1.buckets, o2.buckets):
            assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
            if a.master is not None:
                assert torch.equal(a.master, b.master)
            assert b.acc.numel() == b.npad and a.acc is None


@pytest.mark.parametrize("kind", ["master", "zero-view"])
def test_accumulated_clipped_step_has_no_host_round_trip(kind):
    """After one warm-up step (allocations), accumulate() and a clipped step() synchronise nothing."""
    m, o = _mini(_make(kind, grad_accum=2, max_grad_norm=1e-3), 2, steps=1)
    x = torch.randint(0, 512, (1, 129), generator=torch.Generator().manual_seed(3)).cuda()
    before = torch.cuda.get_sync_debug_mode()
    o.zero_grad(set_to_none=True)
    for k in range(2):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m(x[:, :-1], x[:, 1:])
        loss.backward()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            o.accumulate() if k == 0 else o.step()
        finally:
            torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert float(o.last_grad_norm()) > 1e-3


@pytest.mark.parametrize("kind", ["master", "zero-view"])
def test_no_accumulator_at_grad_accum_1(kind):
    """grad_accum=1 holds no accumulator and allocates what a construction without the argument
    does: ``memory_allocated`` and the allocator's ``requested_bytes`` both match.  Each
    construction allocates from a memory pool of its own: ``memory_allocated`` counts whole cached
    blocks, and in the shared pool the block a request is served from depends on what earlier
    tests freed (two constructions WITHOUT the argument measured 76566528 and 77060096 bytes)."""
    import gc
    pools = []

    def held(kw):
        gc.collect()
        torch.cuda.synchronize()
        req0 = torch.cuda.memory_stats()["requested_bytes.all.current"]
        blk0 = torch.cuda.memory_allocated()
        pools.append(torch.cuda.MemPool())
        with torch.cuda.use_mem_pool(pools[-1]):
            m, o = _mini(_make(kind, **kw), 1)
            o.zero_grad(set_to_none=True)
        if kind == "master":
            assert o._acc == {} and not o._live
        else:
            assert all(b.acc is None and b.rs_src is None and b._g is None for b in o.buckets)
        assert not [v for v in vars(o).values() if isinstance(v, torch.Tensor)]
        gc.collect()
        torch.cuda.synchronize()
        return (torch.cuda.memory_stats()["requested_bytes.all.current"] - req0, torch.cuda.memory_allocated() - blk0)

    used = [held(kw) for kw in ({}, {}, {"grad_accum": 1})]  # the first run pays the libraries' one-time allocations
    print("bytes (requested, memory_allocated) held:", used)
    assert used[1][0] == used[2][0] > 0 and used[1][1] == used[2][1] > 0, used


# ---------------------------------------------------------------- worker
@pytest.mark.parametrize("extra", [[], ["--zero", "1"], ["--linear-dtype", "fp8"], ["--doc-len-mean", "32"]],
                         ids=["default", "zero1", "fp8", "docs"])
def test_worker_accumulates_on_gpu(extra):
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", "--model", "llama-mini",
                        "--seq-len", "128", "--batch-size", "1", "--steps", "2", "--warmup", "1",
                        "--grad-accum", "2", *extra], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert res["grad_accum"] == 2 and res["master_weights"] is True and math.isfinite(res["loss"])
    assert res["zero"] == (1 if "--zero" in extra else 0)
    assert res["value"] == pytest.approx(2 * 128 / (res["ms_per_step"] / 1e3), rel=1e-3)
