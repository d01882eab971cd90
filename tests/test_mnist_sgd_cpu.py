"""The SGD reference of tests/mnist_sgd_refs.py, checked without a GPU: it is torch.optim.SGD
(in float64), a faithful fp32 chain stays inside the bound, and four wrong chains do not."""
import numpy as np
import pytest
import torch

import mnist_sgd_refs as R


def _inputs(n, seed):
    g = np.random.default_rng(seed)
    return tuple(g.standard_normal(n).astype(np.float32) for _ in range(3))


@pytest.mark.parametrize("hy", R.OPS_CONFIGS, ids=lambda h: h.id)
def test_sgd_ref_is_torch_sgd_in_float64(hy):
    """Three steps of sgd_ref from a zero buffer, ``first`` as the trainer passes it (only with
    dampening, only on step 0), against torch.optim.SGD on float64 tensors with the same
    fp32-valued hyper-parameters.  grad_scale: torch gets the scaled gradient.  Tolerance: float64
    rounding (the two evaluate the same expression in another order), 64 x 2^-53 x abs_sum."""
    n = 4096
    p0, _, _ = _inputs(n, 1)
    grads = [_inputs(n, 10 + s)[2] for s in range(3)]
    tp = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.SGD([tp], lr=R.f32(hy.lr), momentum=R.f32(hy.momentum), dampening=R.f32(hy.dampening),
                          weight_decay=R.f32(hy.weight_decay), nesterov=hy.nesterov)
    p, m = R.to64(p0), np.zeros(n)
    for s, g in enumerate(grads):
        tp.grad = torch.from_numpy(g).double() * R.f32(hy.grad_scale)
        opt.step()
        p, m, a_p, a_m = R.sgd_ref(p, m, g, hy, first=(s == 0 and hy.dampening != 0))
        tol = 64 * 2.0 ** -53
        assert np.all(np.abs(p - tp.detach().numpy()) <= tol * a_p), s
        if hy.momentum != 0:
            buf = opt.state[tp]["momentum_buffer"].numpy()
            assert np.all(np.abs(m - buf) <= tol * a_m), s
        else:
            assert not np.any(m) and "momentum_buffer" not in opt.state[tp]


def test_fp32_chain_stays_inside_the_bound():
    """The kernel's chain emulated with one fp32 rounding per operation, 2^18 random elements per
    configuration, steady-state and first step: every element within K x 2^-24 x abs_sum."""
    worst = 0.0
    for i, hy in enumerate(R.OPS_CONFIGS):
        p, m, g = _inputs(1 << 18, 100 + i)
        for first in (False, True):
            pr, mr, a_p, a_m = R.sgd_ref(p, m, g, hy, first)
            pe, me = R.kernel_emulation(p, m, g, hy, first)
            wp = R.assert_within_bound(pe, pr, a_p, f"p {hy.id} first={first}")
            wm = R.assert_within_bound(me, mr, a_m, f"m {hy.id} first={first}")
            if hy.momentum == 0:
                assert np.array_equal(me, R.to64(m))
            worst = max(worst, wp, wm)
    print(f"\nworst emulated deviation: {worst:.3f} x 2^-24 x abs_sum (bound K = {R.K})")
    assert worst < R.K


@pytest.mark.parametrize("variant,hy,first", [
    ("scale_on_decay", R.CONFIGS[1].scaled(0.5), False),
    ("first_ignored", R.CONFIGS[2], True),
    ("no_dampening", R.CONFIGS[2], False),
    ("nesterov_old_buffer", R.CONFIGS[1], False),
], ids=lambda v: v if isinstance(v, str) else None)
def test_bound_rejects_wrong_update(variant, hy, first):
    """Each wrong chain puts more than half of p's or m's elements outside the bound."""
    p, m, g = _inputs(1 << 16, 7)
    pr, mr, a_p, a_m = R.sgd_ref(p, m, g, hy, first)
    pe, me = R.kernel_emulation(p, m, g, hy, first, variant=variant)
    share_p = float((R.ratio(pe, pr, a_p) > R.K).mean())
    share_m = float((R.ratio(me, mr, a_m) > R.K).mean())
    print(f"\n{variant}: share outside the bound p {share_p:.3f}, m {share_m:.3f}")
    assert max(share_p, share_m) > 0.5
    with pytest.raises(AssertionError):
        R.assert_within_bound(pe, pr, a_p, "p")
        R.assert_within_bound(me, mr, a_m, "m")


def test_ratio_is_elementwise_and_exact_where_the_terms_vanish():
    ref, a = np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    assert R.ratio(np.array([1.0, 0.0, 0.0]), ref, a).max() == 0
    assert np.isinf(R.ratio(np.array([1.0, 0.0, 1e-30]), ref, a)[2])
    r = R.ratio(np.array([1.0 + 8 * R.U, 0.0, 0.0]), ref, a)
    assert r[0] == 8 and r[1] == 0
