"""Host-side plumbing of ``MasterAdamW`` and ``ZeroAdamW`` on the GPU, bit for bit: which entry point
of csrc/kernels/adamw.hip each update reaches, with which step count, gradient and norm.  Only the
constructors, ``step()``, ``last_grad_norm()``, the optimizer state, the two C entry points and
``DeviceGradNorm`` are used, so the file says the same about any commit that keeps those.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HP = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
STEPS = 3
# (shape, dtype): a vector body, a 231-element body + scalar tail, fp32 parameters that are their
# own master (one of them a single element: tail only), a parameter that never gets a gradient,
# and one whose gradient is a view one element into a larger buffer (the optimizer must copy it)
SPECS = [((64, 48), BF16), ((33, 7), BF16), ((64,), F32), ((1,), F32), ((8, 8), BF16), ((40,), BF16)]
LAGS, NEVER, MISALIGNED = 2, 4, 5  # SPECS[LAGS] gets no gradient on step 2
CLIPS = [None, 1.0, 1e30]          # 1.0 is far below the norm (~ sqrt(3400) = 58), asserted below


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _inputs():
    """Initial values and per-step gradients (None: no gradient), on the CPU, from one seed."""
    gen = torch.Generator(device="cpu").manual_seed(11)
    init = [torch.randn(shape, generator=gen).to(dt) for shape, dt in SPECS]
    grads = []
    for step in range(1, STEPS + 1):
        row = [torch.randn(shape, generator=gen).to(dt) for shape, dt in SPECS]
        row[NEVER] = None
        if step == 2:
            row[LAGS] = None
        grads.append(row)
    return init, grads


@functools.lru_cache(maxsize=None)
def _expected(max_norm):
    """The three steps driven by hand through pto_adamw_step_scaled / pto_adamw_step_clipped (after
    DeviceGradNorm.run over the same gradients in the same order); CPU (master, m, v, weight) per
    parameter, the step counts and the last norm."""
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops.gradclip import DeviceGradNorm
    lib = _native.load()
    init, grads = _inputs()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    master = [w.float().cuda() for w in init]
    wb = [w.cuda() if w.dtype == BF16 else None for w in init]
    m = [torch.zeros_like(x) for x in master]
    v = [torch.zeros_like(x) for x in master]
    count = [0] * len(init)
    norm, out = DeviceGradNorm(), None
    for row in grads:
        live = [(i, g.cuda()) for i, g in enumerate(row) if g is not None]
        if max_norm is not None:
            out = norm.run([(g.reshape(-1), 1.0) for _, g in live])
        for i, g in live:
            count[i] += 1
            assert g.data_ptr() % 16 == 0 and g.is_contiguous()
            args = (master[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), g.data_ptr(),
                    None if wb[i] is None else wb[i].data_ptr(), g.numel(), 1 if g.dtype == BF16 else 0,
                    HP["lr"], *HP["betas"], HP["eps"], HP["weight_decay"], count[i], 1.0)
            if max_norm is None:
                assert lib.pto_adamw_step_scaled(*args, s) == 0
            else:
                assert lib.pto_adamw_step_clipped(*args, out.data_ptr(), max_norm, s) == 0
        torch.cuda.synchronize()  # the gradients of this step stay alive until its launches ran
    cpu = [(master[i].cpu(), m[i].cpu(), v[i].cpu(), None if wb[i] is None else wb[i].cpu()) for i in range(len(init))]
    return cpu, count, None if out is None else float(out[1])


def _set_grads(params, row):
    for i, (p, g) in enumerate(zip(params, row)):
        if g is None:
            p.grad = None
        elif i == MISALIGNED:
            buf = torch.empty(g.numel() + 1, dtype=g.dtype, device="cuda")
            buf[1:].copy_(g.reshape(-1))
            p.grad = buf[1:].view(g.shape)
            assert p.grad.data_ptr() % 16 != 0
        else:
            p.grad = g.cuda()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("max_norm", CLIPS, ids=["noclip", "clip1", "clip1e30"])
def test_master_adamw_equals_hand_driven_entry_points(max_norm, overlap):
    from pytorch_operator_amd.ops.optim import MasterAdamW
    init, grads = _inputs()
    want, count, want_norm = _expected(max_norm)
    params = [w.cuda() for w in init]
    opt = MasterAdamW(params, overlap=overlap, max_grad_norm=max_norm, **HP)
    for row in grads:
        _set_grads(params, row)
        opt.step()
    torch.cuda.synchronize()
    if max_norm is None:
        assert opt.last_grad_norm() is None
    else:
        assert float(opt.last_grad_norm()) == want_norm
        assert (want_norm > max_norm) == (max_norm == 1.0), want_norm
    for i, p in enumerate(params):
        if i == NEVER:
            assert torch.equal(_bits(p.cpu()), _bits(init[i])) and not opt.state[p]
            continue
        st = opt.state[p]
        assert st["step"] == count[i] == (STEPS - 1 if i == LAGS else STEPS)
        ms, mom, var, wb = want[i]
        assert (st["master"] is None) == (wb is None)
        got_master = p if wb is None else st["master"]
        assert torch.equal(_bits(got_master.cpu()), _bits(ms)), i
        assert torch.equal(_bits(st["exp_avg"].cpu()), _bits(mom.view(p.shape))), i
        assert torch.equal(_bits(st["exp_avg_sq"].cpu()), _bits(var.view(p.shape))), i
        if wb is not None:
            assert torch.equal(_bits(p.cpu()), _bits(wb)), i


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(48, 64, bias=False)
        self.scale = nn.Parameter(torch.ones(64))
        self.b = nn.Linear(64, 33, bias=False)


def _tiny_model_steps(make_opt):
    """Three steps with the same seeded gradients assigned to .grad; returns (model, optimizer)."""
    from pytorch_operator_amd.ops.optim import to_bf16_matmul_weights
    torch.manual_seed(5)
    m = _Tiny().cuda()
    to_bf16_matmul_weights(m)
    opt = make_opt(m)
    gen = torch.Generator(device="cpu").manual_seed(6)
    for _ in range(STEPS):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=gen).to(p.dtype).cuda()
        opt.step()
    torch.cuda.synchronize()
    return m, opt


def _holds_device_norm(opt):
    """A DeviceGradNorm among the optimizer's attributes or those of its helper objects."""
    from pytorch_operator_amd.ops.gradclip import DeviceGradNorm
    held = list(vars(opt).values())
    for x in list(held):
        if hasattr(x, "__dict__") and not isinstance(x, (torch.Tensor, nn.Module)):
            held += list(vars(x).values())
    return any(isinstance(x, DeviceGradNorm) for x in held)


def test_huge_max_grad_norm_is_bit_identical_to_none_master_adamw_gpu():
    from pytorch_operator_amd.ops.optim import MasterAdamW
    m0, o0 = _tiny_model_steps(lambda m: MasterAdamW(m.parameters(), **HP))
    m1, o1 = _tiny_model_steps(lambda m: MasterAdamW(m.parameters(), max_grad_norm=1e30, **HP))
    assert o0.last_grad_norm() is None and float(o1.last_grad_norm()) > 0
    for p0, p1 in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(_bits(p0.data), _bits(p1.data))
        s0, s1 = o0.state[p0], o1.state[p1]
        assert s0["step"] == s1["step"] == STEPS
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(s0[k]), _bits(s1[k]))
        assert (s0["master"] is None) == (s1["master"] is None) == (p0.dtype == F32)
        if s0["master"] is not None:
            assert torch.equal(_bits(s0["master"]), _bits(s1["master"]))


def test_huge_max_grad_norm_is_bit_identical_to_none_zero_adamw_gpu():
    """World 1, gradients deposited from .grad by step() (grad_view=False), each Linear weight in a
    bucket of its own (cap 2621 elements) and the fp32 parameter in a third."""
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    kw = dict(bucket_mb=0.01, grad_view=False, **HP)
    m0, o0 = _tiny_model_steps(lambda m: ZeroAdamW(m, **kw))
    m1, o1 = _tiny_model_steps(lambda m: ZeroAdamW(m, max_grad_norm=1e30, **kw))
    assert o0.last_grad_norm() is None and float(o1.last_grad_norm()) > 0
    assert len(o0.buckets) == len(o1.buckets) >= 2 and o0.sinks == 0
    for p0, p1 in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(_bits(p0.data), _bits(p1.data))
    for b0, b1 in zip(o0.buckets, o1.buckets):
        for k in ("exp_avg", "exp_avg_sq", "flat_w"):
            assert torch.equal(_bits(getattr(b0, k)), _bits(getattr(b1, k)))
        assert (b0.master is None) == (b1.master is None)
        if b0.master is not None:
            assert torch.equal(_bits(b0.master), _bits(b1.master))
    assert not torch.equal(m0.scale.data.cpu(), torch.ones(64))  # and the weights did move


@pytest.mark.parametrize("kind", ["master", "zero"])
def test_no_norm_state_without_max_grad_norm(kind):
    """max_grad_norm=None: no norm is reported and no DeviceGradNorm (workspace, result floats) hangs
    off the optimizer; with a value, one does -- which also shows that the search finds it."""
    from pytorch_operator_amd.ops.optim import MasterAdamW
    from pytorch_operator_amd.parallel.zero import ZeroAdamW

    def make(clip):
        if kind == "master":
            return lambda m: MasterAdamW(m.parameters(), max_grad_norm=clip, **HP)
        return lambda m: ZeroAdamW(m, bucket_mb=0.01, grad_view=False, max_grad_norm=clip, **HP)
    _, off = _tiny_model_steps(make(None))
    assert off.last_grad_norm() is None and not _holds_device_norm(off)
    _, on = _tiny_model_steps(make(1.0))
    assert float(on.last_grad_norm()) > 1.0 and _holds_device_norm(on)
