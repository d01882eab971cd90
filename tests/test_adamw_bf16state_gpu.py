"""bf16 AdamW moments with stochastic rounding on the GPU: the ``pto_adamw_bf16state_*`` entry
points of csrc/kernels/adamw.hip through the shared checker (tests/bf16state_refs.py: an fp64 step
from the widened old moments, then the rounding rule from its own numpy hash), determinism, the
shard property ZeRO relies on, the decay of ``v`` that round-to-nearest would freeze, the plumbing
of ``MasterAdamW`` / ``ZeroAdamW`` (``state_dtype=bf16``) and the worker's ``--opt-state``.
"""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16state_refs as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BF16, F32 = torch.bfloat16, torch.float32
HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
# n / 8 vectors of eight elements, one per thread, on a grid capped at 8192 blocks of 256: threads
# 0..768 take a second trip, and the 5-element scalar tail is handled on one
BIG = 8192 * 256 * 8 + 769 * 8 + 5
WRAP = 2 ** 32 - 3  # the counter's low word wraps at element 3, inside the first thread's vector


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _lib():
    from pytorch_operator_amd.ops import _native
    return _native.load()


@functools.lru_cache(maxsize=2)
def _inputs(n, gdt):
    """Master, non-zero bf16 moments (v >= 0) and one gradient, on the CPU."""
    g = _gen(40 + n % 1000)
    w = torch.randn(n, generator=g)
    m0 = (0.1 * torch.randn(n, generator=g)).to(BF16)
    v0 = (0.1 * torch.rand(n, generator=g)).to(BF16)
    return w, m0, v0, torch.randn(n, generator=g).to(gdt)


def _launch(p, m, v, g, wb, n, step, gs, key, base, clip=None, hp=HP):
    """One pass through pto_adamw_bf16state_scaled / _clipped (clip = (device sumsq, max_norm)) on
    device tensors, in place; returns the entry point's code."""
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), None if wb is None else wb.data_ptr(), n,
            1 if g.dtype == BF16 else 0, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step, gs)
    if clip is None:
        return _lib().pto_adamw_bf16state_scaled(*args, key, base, s)
    return _lib().pto_adamw_bf16state_clipped(*args, clip[0].data_ptr(), clip[1], key, base, s)


def _one_step(n, gdt, out, clipped, step, base, gs=1.0, key=None, cuts=()):
    """One step over the inputs of size n, as one launch or (cuts) as one launch per range, each on
    views of the same device tensors with the range's first counter; CPU (master, m, v, weight or None)."""
    w, m0, v0, g = _inputs(n, gdt)
    p, m, v, gg = w.cuda(), m0.cuda(), v0.cuda(), g.cuda()
    wb = torch.zeros(n, dtype=BF16, device="cuda") if out else None
    clip = (torch.tensor([16.0], device="cuda"), 1.0) if clipped else None
    key = R.sr_key(7, step) if key is None else key
    edges = [0, *cuts, n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert 0 <= lo < hi <= n
        assert _launch(p[lo:hi], m[lo:hi], v[lo:hi], gg[lo:hi], None if wb is None else wb[lo:hi], hi - lo, step, gs,
                       key, base + lo, clip) == 0
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), None if wb is None else wb.cpu()


CASES = [  # n, gradient dtype, bf16 weight, clipped, step, rng_base, grad_scale
    (5, BF16, True, False, 1, 0, 1.0),            # below a vector: the scalar tail alone
    (5, F32, False, True, 1000, WRAP, 0.25),
    (1024, F32, True, True, 1, 5 * 10 ** 9, 1.0),  # whole vectors, an empty tail
    (1024, BF16, False, False, 1000, 0, 0.25),
    (1029, BF16, True, True, 1000, WRAP, 1.0),    # vectors and a tail
    (1029, F32, False, False, 1, 5 * 10 ** 9, 1.0),
    (4101, BF16, True, False, 1, WRAP, 0.25),
    (4101, F32, True, True, 1000, 5 * 10 ** 9, 1.0),
    (4101, BF16, False, True, 1, 0, 1.0),
    (4101, F32, False, False, 1000, WRAP, 1.0),
    (BIG, BF16, True, False, 1000, 2 ** 32 - 16_000_003, 1.0),  # the low word wraps in the second half
    (BIG, F32, False, True, 1, 5 * 10 ** 9, 0.25),
]


@pytest.mark.parametrize("n,gdt,out,clipped,step,base,gs", CASES,
                         ids=[f"n{c[0]}-{'gbf16' if c[1] == BF16 else 'g32'}-{'out' if c[2] else 'noout'}-"
                              f"{'clip' if c[3] else 'plain'}-t{c[4]}-base{c[5]}" for c in CASES])
def test_entry_point_follows_the_rule(n, gdt, out, clipped, step, base, gs):
    assert (n == BIG) == (n // 8 > 8192 * 256)
    w, m0, v0, g = _inputs(n, gdt)
    got = _one_step(n, gdt, out, clipped, step, base, gs)
    coef = 1.0 / (4.0 + 1e-6) if clipped else 1.0  # sum(g^2) = 16, max_norm = 1
    R.check_step(f"n{n}", (w, m0, v0), g, got, HP, step, R.sr_key(7, step), base, gs * coef)


def test_entry_point_return_codes():
    p, m, v, g = (torch.zeros(24, device="cuda"), torch.zeros(24, dtype=BF16, device="cuda"),
                  torch.zeros(24, dtype=BF16, device="cuda"), torch.zeros(24, device="cuda"))
    sq = torch.ones(1, device="cuda")
    assert _launch(p, m, v, g, None, 0, 1, 1.0, 1, 0) == -1
    assert _launch(p, m, v, g, None, 8, 0, 1.0, 1, 0) == -1
    assert _launch(p, m[4:], v, g, None, 8, 1, 1.0, 1, 0) == -2   # 8 bytes into a 16-byte unit
    assert _launch(p, m, v[1:], g, None, 8, 1, 1.0, 1, 0) == -2
    assert _launch(p[1:], m, v, g, None, 8, 1, 1.0, 1, 0) == -2
    assert _launch(p, m, v, g, None, 8, 1, 1.0, 1, 0, clip=(sq, 0.0)) == -1
    assert _launch(p, m, v, g, None, 8, 1, 1.0, 1, 0) == 0
    torch.cuda.synchronize()


def test_same_launch_same_bits_other_key_or_base_other_bits():
    n = 4101
    a = _one_step(n, BF16, True, False, 3, 100)
    b = _one_step(n, BF16, True, False, 3, 100)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    for other in (_one_step(n, BF16, True, False, 3, 100, key=R.sr_key(8, 3)), _one_step(n, BF16, True, False, 3, 101)):
        assert torch.equal(_bits(a[0]), _bits(other[0])) and torch.equal(_bits(a[3]), _bits(other[3]))  # not the master
        flips = int((_bits(a[1]) != _bits(other[1])).sum()) + int((_bits(a[2]) != _bits(other[2])).sum())
        assert flips > n // 4, flips  # about half of the 2 n roundings change


@pytest.mark.parametrize("gdt,out,clipped", [(BF16, True, False), (F32, False, True)], ids=["gbf16-out", "g32-clip"])
def test_two_shard_launches_equal_one(gdt, out, clipped):
    """[0, k) with base and [k, n) with base + k give the bits of one launch over [0, n): an
    element's random bits depend on its counter alone (k a multiple of 8: aligned shard pointers)."""
    n, k, base = 4101, 1032, WRAP
    whole = _one_step(n, gdt, out, clipped, 2, base)
    split = _one_step(n, gdt, out, clipped, 2, base, cuts=(k,))
    for x, y in zip(whole, split):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y))
    assert not torch.equal(_bits(whole[1]), _bits(_inputs(n, gdt)[1]))  # and the moments did move


def test_v_decays_under_zero_gradient_through_the_kernel():
    """As tests/test_adamw_bf16state_cpu.py: b2 = 0.999, zero gradient, 500 launches.  The mean of
    v_T / (v_0 * 0.999^500) is within 1 % of 1 (standard error 0.0002); round-to-nearest gives 1 / 0.606."""
    n, T, b2 = 65536, 500, 0.999
    hp = dict(lr=0.0, b1=0.9, b2=b2, eps=1e-8, wd=0.0)
    v0 = torch.exp(torch.randn(n, generator=_gen(2))).to(BF16)
    p, m, v = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=BF16, device="cuda"), v0.cuda()
    g = torch.zeros(n, dtype=BF16, device="cuda")
    for t in range(1, T + 1):
        assert _launch(p, m, v, g, None, n, t, 1.0, R.sr_key(3, t), 0, hp=hp) == 0
    torch.cuda.synchronize()
    ratio = v.cpu().double() / (v0.double() * b2 ** T)
    print("mean ratio", float(ratio.mean()), "std", float(ratio.std()))
    assert abs(float(ratio.mean()) - 1) < 0.01
    assert not bool(m.any()) and not bool(p.any())


# --------------------------------------------------------------------------------- MasterAdamW
OPT = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
SEED, MAX_NORM, ACCUM, STEPS = 21, 1.0, 2, 3


def _mini_model():
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-mini"]).cuda()
    to_bf16_matmul_weights(m)
    return m


def _mini_grads(params, step, micro):
    g = torch.Generator(device="cuda").manual_seed(1000 + 10 * step + micro)
    return [torch.randn(p.shape, generator=g, device="cuda").to(p.dtype) for p in params]


@functools.lru_cache(maxsize=None)
def _mini_by_hand():
    """llama-mini's parameters, three steps of two seeded micro-batch gradients each, driven by hand:
    the fp32 sum of the two, DeviceGradNorm over the sums (scale 1/2) in parameter order, then
    pto_adamw_bf16state_clipped per parameter with key = mix(seed + 0x9E3779B9 * step) and base =
    the number of elements of the parameters before it.  CPU (master, m, v, weight) per parameter."""
    from pytorch_operator_amd.ops.gradclip import DeviceGradNorm
    live = list(_mini_model().parameters())
    params = [p.detach() for p in live]
    # a bf16 weight's exact fp32 initial value, as MasterAdamW takes it over
    master = [p.detach().clone() if p.dtype == F32 else p._pto_master.clone() for p in live]
    wb = [p.clone() if p.dtype == BF16 else None for p in params]
    m = [torch.zeros(p.shape, dtype=BF16, device="cuda") for p in params]
    v = [torch.zeros(p.shape, dtype=BF16, device="cuda") for p in params]
    bases = np.cumsum([0] + [p.numel() for p in params])
    norm = DeviceGradNorm()
    for step in range(1, STEPS + 1):
        acc = [a.float() + b.float() for a, b in zip(_mini_grads(params, step, 0), _mini_grads(params, step, 1))]
        out = norm.run([(a.reshape(-1), 1.0 / ACCUM) for a in acc])
        for i, a in enumerate(acc):
            assert _launch(master[i], m[i], v[i], a, wb[i], a.numel(), step, 1.0 / ACCUM, R.sr_key(SEED, step),
                           int(bases[i]), (out, MAX_NORM), hp=dict(lr=OPT["lr"], b1=0.9, b2=0.95, eps=1e-8, wd=0.1)) == 0
        torch.cuda.synchronize()
    assert float(out[1]) > MAX_NORM  # the clip acts
    return [(master[i].cpu(), m[i].cpu(), v[i].cpu(), None if wb[i] is None else wb[i].cpu()) for i in range(len(params))]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_master_adamw_equals_hand_driven_entry_point_on_llama_mini(overlap):
    from pytorch_operator_amd.ops.optim import MasterAdamW
    want = _mini_by_hand()
    model = _mini_model()
    params = list(model.parameters())
    opt = MasterAdamW(params, overlap=overlap, max_grad_norm=MAX_NORM, grad_accum=ACCUM, state_dtype=BF16,
                      state_seed=SEED, **OPT)
    for step in range(1, STEPS + 1):
        for k in range(ACCUM):
            for p, g in zip(params, _mini_grads(params, step, k)):
                p.grad = g
            if k < ACCUM - 1:
                opt.accumulate()
        opt.step()
    torch.cuda.synchronize()
    assert {p.dtype for p in params} == {BF16, F32} and len(params) > 10
    for i, p in enumerate(params):
        st = opt.state[p]
        ms, mom, var, wb = want[i]
        assert st["step"] == STEPS and st["exp_avg"].dtype == BF16 and st["exp_avg_sq"].dtype == BF16
        assert (st["master"] is None) == (wb is None)
        assert torch.equal(_bits((p if wb is None else st["master"]).detach().cpu()), _bits(ms)), i
        assert torch.equal(_bits(st["exp_avg"].cpu()), _bits(mom)), i
        assert torch.equal(_bits(st["exp_avg_sq"].cpu()), _bits(var)), i
        assert bool(st["exp_avg_sq"].any()), i
        if wb is not None:
            assert torch.equal(_bits(p.detach().cpu()), _bits(wb)), i


# --------------------------------------------------------------------------------- ZeroAdamW, world 1
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(48, 64, bias=False)
        self.scale = nn.Parameter(torch.ones(64))
        self.b = nn.Linear(64, 33, bias=False)


def _zero():
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    torch.manual_seed(5)
    m = _Tiny().cuda()
    to_bf16_matmul_weights(m)
    return m, ZeroAdamW(m, bucket_mb=0.01, grad_view=False, state_dtype=BF16, state_seed=9, max_grad_norm=1.0, **OPT)


def _zero_step(m, opt, step):
    g = _gen(100 + step)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype).cuda()
    opt.step()


def _zero_bits(m, opt):
    out = [_bits(p.data).cpu() for p in m.parameters()]
    for b in opt.buckets:
        out += [_bits(b.exp_avg).cpu(), _bits(b.exp_avg_sq).cpu()] + ([] if b.master is None else [_bits(b.master).cpu()])
    return out


def test_zero_adamw_bf16_state_resumes_bit_identically(tmp_path):
    from pytorch_operator_amd.utils import train_ckpt
    m, opt = _zero()
    assert len(opt.buckets) == 3 and all(b.exp_avg.dtype == BF16 and b.exp_avg_sq.dtype == BF16 for b in opt.buckets)
    # master 4 + m 2 + v 2 bytes per (padded) bf16-weight element; fp32 parameters are their own
    # master and hold the two bf16 moments
    pad16 = sum(b.npad for b in opt.buckets if b.dtype == BF16)
    pad32 = sum(b.npad for b in opt.buckets if b.dtype == F32)
    assert opt.state_bytes() == 8 * pad16 + 4 * pad32
    for step in (1, 2):
        _zero_step(m, opt, step)
    d = str(tmp_path / "ck")
    train_ckpt.save(d, 2, m, opt, rank=0, world=1)
    _zero_step(m, opt, 3)
    torch.cuda.synchronize()
    m2, opt2 = _zero()
    assert train_ckpt.load(d, m2, opt2, rank=0, world=1, device=torch.device("cuda")) == 2
    _zero_step(m2, opt2, 3)
    torch.cuda.synchronize()
    want, got = _zero_bits(m, opt), _zero_bits(m2, opt2)
    assert len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(want, got))
    assert all(bool(b.exp_avg_sq.any()) for b in opt2.buckets)


# --------------------------------------------------------------------------------- the worker
@functools.lru_cache(maxsize=None)
def _worker(opt_state, seed):
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", "--model", "llama-mini",
                        "--seq-len", "128", "--batch-size", "1", "--steps", "8", "--warmup", "1", "--seed", str(seed),
                        "--opt-state", opt_state], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])


# |final loss with bf16 moments - with fp32 moments| after 1 + 8 steps of the worker on llama-mini,
# measured on an MI355X for seeds 1 and 2 (profiles/optstate/README.md): LOSS_DIFFS; the bound is
# 4 x the larger one, a margin for the seed-to-seed spread of a quantity whose scale is set by the
# bf16 rounding noise in the moments
LOSS_DIFFS = (0.0002983212471008301, 0.000347137451171875)
LOSS_BOUND = 4 * max(LOSS_DIFFS)


def test_worker_runs_with_bf16_optimizer_state():
    lo, hi = _worker("bf16", 1), _worker("fp32", 1)
    assert lo["opt_state"] == "bf16" and hi["opt_state"] == "fp32"
    assert 0 < lo["optimizer_state_bytes"] < hi["optimizer_state_bytes"]
    assert math.isfinite(lo["loss"]) and math.isfinite(hi["loss"])
    diff = abs(lo["loss"] - hi["loss"])
    print("final losses", lo["loss"], hi["loss"], "difference", diff)
    assert diff <= LOSS_BOUND, (diff, LOSS_BOUND)
