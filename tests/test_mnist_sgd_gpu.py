"""Every place the MNIST step applies SGD, held to the elementwise bound of tests/mnist_sgd_refs.py.

The optimizer is isolated from the forward pass: each step stores its gradients, and the new
parameters / momentum are compared with ``sgd_ref(p_before, m_before, stored gradient)`` over the
whole flat vector -- whether each site applied the stated update to the gradient it stored.  (The
gradients' own accuracy: tests/test_kernels_gpu.py, tests/test_torch_parity_gpu.py.)
"""
import numpy as np
import pytest
import torch

import mnist_sgd_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
_ids = lambda h: h.id  # noqa: E731


def _layout():
    from pytorch_operator_amd.models.mnist import PARAM_SPECS, flat_layout
    lay = flat_layout()
    pad = torch.ones(lay.total, dtype=torch.bool)
    for name, shape in PARAM_SPECS:
        o = lay.offsets[name]
        pad[o:o + int(torch.Size(shape).numel())] = False
    return lay, pad


def _check_update(p0, m0, g, p1, m1, hy, first, what):
    """p1 / m1 against sgd_ref(p0, m0, g) elementwise; momentum 0: the buffer bit-identical."""
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite gradient"
    pr, mr, a_p, a_m = R.sgd_ref(p0, m0, g, hy, first)
    R.assert_within_bound(p1, pr, a_p, f"{what}: params")
    if hy.momentum == 0:
        assert torch.equal(m1, m0), f"{what}: momentum 0 must leave the buffer untouched"
    else:
        R.assert_within_bound(m1, mr, a_m, f"{what}: momentum")


# ------------------------------------------------------------------ the trainer's step forms
_FORMS = {
    "tail": {},                               # tail_: fc1 / fc2 tiles + the slab columns
    "slab_w1": {"fuse_head": False},          # slab_reduce_sgd_w1 + the plain range (fc2)
    "slab_extra": {"w1_tail": False},         # slab_reduce_sgd, every fc parameter in the plain range
    "sgd_momentum": None,                     # forward_backward() + optimizer_step()
}


def _trainer(B, hy, seed, knobs=None, n=500, cursor0=5):
    from pytorch_operator_amd.models.mnist import FusedMnistTrainer
    from pytorch_operator_amd.ops import mnist as K
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    cur = torch.full((1,), cursor0, dtype=torch.int32, device=DEV)
    src = K.BatchSource(x.to(DEV), y.to(DEV), perm=perm.to(DEV), cursor=cur)
    tr = FusedMnistTrainer(batch_size=B, source=src, seed=seed, **hy.trainer_kwargs())
    tr.materialize_fc1_grad = True
    for k, v in (knobs or {}).items():
        setattr(tr, k, v)
    return tr


@pytest.mark.parametrize("hy", R.CONFIGS, ids=_ids)
@pytest.mark.parametrize("form,B", [("tail", 37), ("tail", 64), ("slab_w1", 37), ("slab_extra", 37),
                                    ("sgd_momentum", 37)])
def test_step_forms_apply_the_stated_update(form, B, hy):
    """Three steps per form and configuration.  ``first`` follows torch's semantics (the first
    step with dampening initialises the buffer undamped), not the trainer's flag.  The padding of
    the flat layout stays exactly 0 in parameters and momentum."""
    lay, pad = _layout()
    tr = _trainer(B, hy, seed=11 + B, knobs=_FORMS[form])
    pad = pad.to(DEV)
    assert not bool(tr.flat_params[pad].any())
    for s in range(3):
        p0, m0 = tr.flat_params.clone(), tr.flat_momentum.clone()
        if form == "sgd_momentum":
            tr.forward_backward()
            tr.optimizer_step()
        else:
            tr.train_step()
        torch.cuda.synchronize()
        assert int(tr.cursor.item()) == 5 + s + 1
        _check_update(p0, m0, tr.flat_grads, tr.flat_params, tr.flat_momentum, hy,
                      first=(s == 0 and hy.dampening != 0), what=f"{form} B={B} step {s}")
        assert bool(tr.flat_grads[: lay.conv_end].any()) and bool(tr.flat_grads[lay.conv_end:].any())
    assert not bool(tr.flat_params[pad].any()) and not bool(tr.flat_momentum[pad].any())
    assert not bool(tr.flat_grads[pad].any())


def test_captured_step_clears_first_step():
    """Dampening: the first step is special.  One eager step, then capture + two replays, lands on
    the bits of three eager steps -- the captured launch does not carry first_step."""
    hy = R.CONFIGS[2]
    a, b = _trainer(37, hy, seed=3), _trainer(37, hy, seed=3)
    a.train_step()
    g = a.capture(steps_per_graph=1)
    g.replay()
    g.replay()
    for _ in range(3):
        b.train_step()
    torch.cuda.synchronize()
    assert int(a.cursor.item()) == int(b.cursor.item()) == 8
    assert torch.equal(a.flat_params, b.flat_params)
    assert torch.equal(a.flat_momentum, b.flat_momentum)


# ------------------------------------------------------------------ the ops, directly
_GUARD = 64


def _guarded(n, gen, fill):
    t = torch.full((n + _GUARD,), fill, device=DEV)
    t[:n] = torch.randn(n, generator=gen).to(DEV)
    return t


@pytest.mark.parametrize("hy", [h.scaled(0.5) for h in R.CONFIGS], ids=_ids)
@pytest.mark.parametrize("n", [1, 3, 4, 7, 1029])
def test_sgd_momentum_scalar_tail_and_guards(n, hy):
    """sgd_momentum_ at n < 4 and n % 4 != 0 (the scalar tail), grad_scale 0.5: the bound on every
    element, the step counter + 1 per launch, nothing written past n."""
    from pytorch_operator_amd.ops import mnist as K
    gen = torch.Generator().manual_seed(n)
    p, m, g = _guarded(n, gen, 7.0), _guarded(n, gen, -3.0), _guarded(n, gen, 5.0)
    counter = torch.full((1,), 41, dtype=torch.int32, device=DEV)
    for s in range(2):
        first = s == 0 and hy.dampening != 0
        p0, m0 = p.clone(), m.clone()
        K.sgd_momentum_(p[:n], g[:n], m[:n], first_step=first, step_counter=counter, **hy.kwargs())
        torch.cuda.synchronize()
        assert int(counter.item()) == 42 + s
        _check_update(p0[:n], m0[:n], g[:n], p[:n], m[:n], hy, first, f"n={n} launch {s}")
        assert torch.equal(p[n:], p0[n:]) and torch.equal(m[n:], m0[n:])
        assert bool((g[n:] == 5.0).all())


def _tail_inputs(B, seed):
    lay, pad = _layout()
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    p, m = rnd(lay.total), rnd(lay.total)
    p[pad] = 0
    m[pad] = 0
    rows = (B + 3) // 4
    lo = lay.offsets["conv2.weight"]
    slab = rnd(8, lay.conv_end)
    valid = slab.clone()
    slab[B:] = float("nan")                       # rows no sample wrote
    slab[rows:, lo:lo + 25000] = float("nan")     # conv2.weight: only the chunk rows hold partials
    valid[B:] = 0
    valid[rows:, lo:lo + 25000] = 0
    act = dict(dh=rnd(B, 500), a2=rnd(B, 800), dlog=rnd(B, 10), h=rnd(B, 500), per_sample=rnd(B, 2).abs())
    g_fc = rnd(lay.total)                          # gradients of the plain range (given, not computed)
    g_fc[pad] = 0
    g_fc[:lay.conv_end] = 0
    to = lambda t: t.to(DEV)  # noqa: E731
    return lay, to(p), to(m), to(slab), valid.double(), {k: to(v) for k, v in act.items()}, to(g_fc)


@pytest.mark.parametrize("hy,first", [(R.CONFIGS[1].scaled(0.125), False), (R.CONFIGS[2].scaled(0.125), True),
                                      (R.CONFIGS[2].scaled(0.125), False), (R.CONFIGS[3].scaled(0.125), False)],
                         ids=lambda v: v.id if isinstance(v, R.Hyper) else f"first{int(v)}")
@pytest.mark.parametrize("form", ["tail", "slab_w1", "slab_extra"])
def test_tail_and_slab_reduce_sgd_with_grad_scale(form, hy, first):
    """grad_scale 0.125 (DDP and the xGMI fallback pass it; the trainer never does) on a synthetic
    slab at B = 5 with conv_bwd4's chunk rows.  The slab holds NaN in every cell the reduction must
    not sum: conv2.weight columns of rows >= ceil(B / 4), every row >= B."""
    from pytorch_operator_amd.ops import mnist as K
    B = 5
    lay, p, m, slab, valid, act, g = _tail_inputs(B, seed=17)
    ce, o = lay.conv_end, lay.offsets
    o2w, o2b = o["fc2.weight"], o["fc2.bias"]
    p0, m0 = p.clone(), m.clone()
    big = K.conv_bwd4_rows(B, o)
    assert big == (2, o["conv2.weight"], o["conv2.weight"] + 25000)
    stats = torch.zeros(16, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(first_step=first, step_counter=counter, big=big, **hy.kwargs())
    w1 = (act["dh"], act["a2"], p[ce:o2w], m[ce:o2w], g[ce:o2w])
    if form == "tail":
        K.tail_(slab, B, g[:ce], p[:ce], m[:ce], w1=w1,
                fc2=(act["dlog"], act["h"], act["per_sample"], stats, 1.0 / B, p[o2w:o2b], m[o2w:o2b],
                     g[o2w:o2b], p[o2b:], m[o2b:], g[o2b:]), **kw)
    elif form == "slab_w1":
        K.slab_reduce_sgd_(slab, B, g[:ce], p[:ce], m[:ce], extra=(p[o2w:], g[o2w:], m[o2w:]), w1=w1, **kw)
    else:
        K.slab_reduce_sgd_(slab, B, g[:ce], p[:ce], m[:ce], extra=(p[ce:], g[ce:], m[ce:]), **kw)
    torch.cuda.synchronize()
    assert int(counter.item()) == 1
    _check_update(p0, m0, g, p, m, hy, first, form)
    # the reduced conv gradient: the float64 sum of the valid cells; a sum of r terms in any order
    # is within (r - 1) x 2^-24 x sum |terms| (first order)
    rows = torch.full((ce,), B - 1.0, dtype=torch.float64)
    rows[big[1]:big[2]] = big[0] - 1.0
    R.assert_within_bound(g[:ce], valid.sum(0).numpy(), (rows * valid.abs().sum(0)).numpy(), f"{form}: conv grads",
                          k=1.0 + 1e-6)


# ------------------------------------------------------------------ the xGMI exchange's copy
@pytest.mark.parametrize("hy", [R.CONFIGS[1], R.CONFIGS[2]], ids=_ids)
def test_xgmi_exchange_sgd(hy):
    """xgmi_allreduce.hip's sgd4 at world 2 (emulated on one device), four steps, no slab: the
    summed gradient is exactly fp32(g0 + g1) and grad_scale 1 / 2 is exact, so the bound applies
    unchanged.  Replicas bit-identical, no protocol error."""
    from pytorch_operator_amd.parallel.xgmi import XgmiEmulation
    lay, _ = _layout()
    L, world = lay.total, 2
    gen = torch.Generator().manual_seed(23)
    emu = XgmiEmulation(world, L, nblk=128)
    try:
        p_init = torch.randn(L, generator=gen).to(DEV)
        ps = [p_init.clone() for _ in range(world)]
        ms = [torch.zeros(L, device=DEV) for _ in range(world)]
        shard = emu.npad // world
        owned = lambda: torch.cat([ms[r][r * shard:min(L, (r + 1) * shard)] for r in range(world)])  # noqa: E731
        hs = hy.scaled(1.0 / world)
        for s in range(4):
            first = s == 0 and hy.dampening != 0
            grads = [torch.randn(L, generator=gen).to(DEV) for _ in range(world)]
            p0, m0 = ps[0].clone(), owned()
            emu.configure(1, grads, ps, ms, first_step=first, **hy.trainer_kwargs())
            emu.launch()
            torch.cuda.synchronize()
            _check_update(p0, m0, grads[0] + grads[1], ps[0], owned(), hs, first, f"xgmi step {s}")
            assert torch.equal(ps[1], ps[0])
        assert emu.error() == 0
    finally:
        emu.close()
