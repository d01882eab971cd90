"""The fp64 AdamW rule the GPU edge tests compare adamw.hip with (tests/llm_refs.py):
equal to torch.optim.AdamW on fp64 tensors, and a tolerance that correct fp32 arithmetic
(MasterAdamW._step_reference) attains against it."""
import math

import pytest
import torch

from llm_refs import adamw_step_fp64

HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
# tests/test_llm_edges_gpu.py: the sizes below 8.39 M elements, first steps and step counts
SIZES = [1, 2, 3, 4, 5, 1023]


def _inputs(n, steps, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]


@pytest.mark.parametrize("n", [1, 5, 1023])
def test_fp64_rule_equals_torch_adamw(n):
    w, grads = _inputs(n, 6)
    p = torch.nn.Parameter(w.double())
    opt = torch.optim.AdamW([p], lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    q, m, v = w.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k, g in enumerate(grads):
        p.grad = g.double()
        opt.step()
        q, m, v = adamw_step_fp64(q, m, v, g, step=k + 1, **HP)
        st = opt.state[p]
        torch.testing.assert_close(q, p.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-12)


def test_fp64_rule_scale_and_clip_equal_clip_grad_norm():
    """grad_scale and the clip coefficient against clip_grad_norm_ + torch.optim.AdamW."""
    n = 257
    w, grads = _inputs(n, 4, seed=1)
    for max_norm in (1.0, 1e3):  # clips (norm ~ 4), does not clip
        p = torch.nn.Parameter(w.double())
        opt = torch.optim.AdamW([p], lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"],
                                weight_decay=HP["wd"])
        q, m, v = w.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for k, g in enumerate(grads):
            p.grad = g.double() * 0.25
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            opt.step()
            sumsq = float((g.double() * 0.25).pow(2).sum())
            q, m, v = adamw_step_fp64(q, m, v, g, step=k + 1, grad_scale=0.25, sumsq=sumsq, max_norm=max_norm,
                                      **HP)
            torch.testing.assert_close(q, p.detach(), rtol=1e-12, atol=1e-12)


def test_fp64_rule_clip_edges():
    one = torch.ones(3, dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    g = torch.tensor([1.0, -2.0, 0.5])
    plain = adamw_step_fp64(one, z, z, g, step=1, **HP)
    for sumsq in (0.0, 0.81):  # norm 0 and 0.9 < max_norm: the coefficient is exactly 1
        got = adamw_step_fp64(one, z, z, g, step=1, sumsq=sumsq, max_norm=1.0, **HP)
        assert all(torch.equal(a, b) for a, b in zip(got, plain))
    p, m, v = adamw_step_fp64(one, one, one, g, step=1, sumsq=math.inf, max_norm=1.0, **HP)
    assert torch.equal(m, HP["b1"] * one) and torch.equal(v, HP["b2"] * one)  # the moments only decay
    p, m, v = adamw_step_fp64(one, one, one, g, step=1, sumsq=math.nan, max_norm=1.0, **HP)
    assert all(bool(t.isnan().all()) for t in (p, m, v))


@pytest.mark.parametrize("first_step", [1, 1000])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g32", "gbf16"])
@pytest.mark.parametrize("n", SIZES)
def test_fp32_step_reference_within_gpu_tolerance_of_fp64(n, gdt, first_step):
    """rtol 1e-5 / atol 1e-6 on m, v and the master, the GPU tests' tolerance, is attained by
    correct fp32 arithmetic at the same inputs and step counts: the bound is not taken from
    the kernel's own output."""
    from pytorch_operator_amd.ops.optim import MasterAdamW
    w, grads = _inputs(n, 4)
    grads = [g.to(gdt) for g in grads]
    p32 = w.clone()
    st = dict(step=first_step - 1, exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n))
    q, m, v = w.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k, g in enumerate(grads):
        st["step"] += 1
        MasterAdamW._step_reference(p32, g, p32, st, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"])
        q, m, v = adamw_step_fp64(q, m, v, g, step=first_step + k, **HP)
    torch.testing.assert_close(st["exp_avg"].double(), m, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st["exp_avg_sq"].double(), v, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(p32.double(), q, rtol=1e-5, atol=1e-6)
