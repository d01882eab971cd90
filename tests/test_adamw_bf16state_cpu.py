"""bf16 AdamW moments with stochastic rounding, on the CPU: the rounding rule of
``ops/optim.py`` against the checker's own numpy copy (tests/bf16state_refs.py), the decay of ``v``
that round-to-nearest would freeze, ``MasterAdamW(state_dtype=bf16)`` through the shared checker,
determinism, checkpoints of both optimizers, and the worker's ``--opt-state`` flag.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import bf16state_refs as R

BF16, F32 = torch.bfloat16, torch.float32
HP = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
HPK = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)  # the same, as the checker names them
BASES = [0, 2 ** 32 - 3, 5 * 10 ** 9]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


# --------------------------------------------------------------------------------- the rule
def test_key_and_hash_equal_the_checkers():
    from pytorch_operator_amd.ops.optim import sr_bits, sr_key
    for seed, step in [(0, 1), (1, 1), (1, 1000), (2 ** 31 + 5, 7), (12345, 2 ** 20)]:
        assert sr_key(seed, step) == R.sr_key(seed, step)
    assert R.sr_key(0, 1) != R.sr_key(0, 2) != R.sr_key(1, 2)
    for base in BASES:  # the middle one wraps the counter's low word at i = 3
        for key in (0, R.sr_key(1, 1), 0xFFFFFFFF):
            got = sr_bits(key, base, 1000).numpy().astype(np.uint64)
            assert np.array_equal(got, R.sr_hash(key, base, 1000)), (base, key)
    h = R.sr_hash(7, 2 ** 32 - 3, 8)
    assert len(set(h.tolist())) == 8  # and the wrap does not repeat counters


def test_rounding_equals_the_checkers_on_random_values():
    from pytorch_operator_amd.ops.optim import sr_round_bf16
    g = _gen(1)
    n = 1 << 16
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-60, 60, (n,), generator=g).float())
    r = torch.randint(0, 65536, (n,), generator=g)
    got = R.bf16_bits(sr_round_bf16(x, r))
    assert np.array_equal(got, R.sr(x.numpy(), r.numpy()))
    # unbiased: the mean of the rounded values is the mean of the inputs (both signs), where
    # round-down alone would lose half an ulp, 2^-9 relative
    y = torch.rand(n, generator=g) + 1.0
    y = torch.cat([y, -y])
    r2 = torch.randint(0, 65536, (2 * n,), generator=g)
    out = sr_round_bf16(y, r2).double()
    assert abs(float((out[:n] / y[:n].double()).mean()) - 1) < 1e-4
    assert abs(float((out[n:] / y[n:].double()).mean()) - 1) < 1e-4


def test_rounding_edges():
    from pytorch_operator_amd.ops.optim import sr_round_bf16
    inf, fmax = float("inf"), float(np.finfo(np.float32).max)
    den = 2.0 ** -130  # a denormal that bf16 represents (its smallest is 2^-133)
    den_odd = np.array([0x00018001], dtype=np.uint32).view(np.float32)[0]  # one that it does not
    rep = [1.0, -1.5, 0.0, -0.0, inf, -inf, den, -den, 3.140625, 2.0 ** -126]
    for r in (0, 1, 0x7FFF, 0xFFFF):
        x = torch.tensor(rep, dtype=F32)
        out = sr_round_bf16(x, torch.full((len(rep),), r))
        assert torch.equal(_bits(out.float()), _bits(x)), r  # representable values never change, -0 stays -0
        assert np.array_equal(R.bf16_bits(out), R.sr(x.numpy(), np.full(len(rep), r)))
    x = torch.tensor([fmax, -fmax, float(den_odd), 1.0 + 2.0 ** -16], dtype=F32)
    down = sr_round_bf16(x, torch.zeros(4, dtype=torch.int64))
    up = sr_round_bf16(x, torch.full((4,), 0xFFFF))
    assert down.float().tolist() == [R.BF16_MAX, -R.BF16_MAX, 2.0 ** -133, 1.0]
    assert up.float().tolist() == [inf, -inf, 2.0 ** -132, 1.0 + 2.0 ** -7]
    for r in (0, 0xFFFF):
        assert np.array_equal(R.bf16_bits(sr_round_bf16(x, torch.full((4,), r))), R.sr(x.numpy(), np.full(4, r)))
    # NaNs of every kind stay NaN, quiet, with their sign; the carry never reaches the exponent
    nan_bits = np.array([0x7FC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001, 0xFF80FFFF], dtype=np.uint32)
    nans = torch.from_numpy(nan_bits.view(np.float32).copy())
    for r in (0, 0xFFFF):
        out = R.bf16_bits(sr_round_bf16(nans, torch.full((5,), r)))
        assert np.array_equal(out, R.sr(nans.numpy(), np.full(5, r)))
        assert ((out & 0x7FFF) > 0x7F80).all() and ((out & 0x40) != 0).all()
        assert np.array_equal(out >> 15, (nan_bits >> 31).astype(np.uint16))


# --------------------------------------------------------------------------------- decay of v
def test_v_decays_under_zero_gradient():
    """lr = 0, wd = 0, b2 = 0.999, zero gradient: v_T = v_0 * 0.999^T.  The per-step change (0.1 %) is
    below half a bf16 ulp, so round-to-nearest leaves v_T / v_0 at exactly 1 (a ratio of 1 / 0.606 to
    the expectation); stochastic rounding is unbiased.  Per-element standard deviation at T = 500:
    0.048, so the standard error of the mean over 65 536 elements is 0.0002 and the bound is 1 %."""
    from pytorch_operator_amd.ops.optim import MasterAdamW, sr_key
    n, T, b2 = 65536, 500, 0.999
    v0 = torch.exp(torch.randn(n, generator=_gen(2))).to(BF16)
    p = torch.zeros(n)
    st = {"step": 0, "exp_avg": torch.zeros(n, dtype=BF16), "exp_avg_sq": v0.clone()}
    g = torch.zeros(n)
    for t in range(1, T + 1):
        st["step"] = t
        MasterAdamW._step_reference(p, g, p, st, 0.0, 0.9, b2, 1e-8, 0.0, (sr_key(3, t), 0))
    ratio = st["exp_avg_sq"].double() / (v0.double() * b2 ** T)
    print("mean ratio", float(ratio.mean()), "std", float(ratio.std()))
    assert abs(float(ratio.mean()) - 1) < 0.01
    assert not bool(st["exp_avg"].any()) and not bool(p.any())


# --------------------------------------------------------------------------------- MasterAdamW
SPECS = [((64, 48), BF16), ((33, 7), BF16), ((64,), F32), ((1,), F32), ((4101,), BF16)]
STEPS = 3


def _params():
    g = _gen(11)
    return [torch.randn(shape, generator=g).to(dt) for shape, dt in SPECS]


def _grads(accum):
    g = _gen(12)
    return [[[torch.randn(shape, generator=g).to(dt) for shape, dt in SPECS] for _ in range(accum)]
            for _ in range(STEPS)]


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p)
        if not st:
            out.append((p.detach().float().clone(), torch.zeros(p.shape, dtype=BF16), torch.zeros(p.shape, dtype=BF16)))
            continue
        master = st["master"] if st["master"] is not None else p
        out.append((master.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def _run_master(max_norm, accum, seed=5, check=True, **kw):
    from pytorch_operator_amd.ops.optim import MasterAdamW
    params = _params()
    opt = MasterAdamW(params, max_grad_norm=max_norm, grad_accum=accum, state_dtype=BF16, state_seed=seed, **HP, **kw)
    bases = np.cumsum([0] + [p.numel() for p in params])
    for step, micro in enumerate(_grads(accum), start=1):
        old = _snapshot(opt, params)
        for k, row in enumerate(micro):
            for p, g in zip(params, row):
                p.grad = g.clone()
            if k < accum - 1:
                opt.accumulate()
        opt.step()
        if not check:
            continue
        gs = 1.0 / accum
        if max_norm is not None:
            gs *= min(1.0, max_norm / (float(opt.last_grad_norm()) + 1e-6))
            assert float(opt.last_grad_norm()) > max_norm
        for i, p in enumerate(params):
            st = opt.state[p]
            assert st["step"] == step and st["exp_avg"].dtype == BF16 and st["exp_avg_sq"].dtype == BF16
            gsum = sum(row[i].float() for row in micro)
            master = st["master"] if st["master"] is not None else p
            R.check_step(f"step{step}.p{i}", old[i], gsum, (master, st["exp_avg"], st["exp_avg_sq"],
                                                         p if p.dtype == BF16 else None),
                         HPK, step, R.sr_key(seed, step), int(bases[i]), gs)
    return opt, params


@pytest.mark.parametrize("accum", [1, 2], ids=["accum1", "accum2"])
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip1"])
def test_master_adamw_bf16_state_steps_follow_the_rule(max_norm, accum):
    _run_master(max_norm, accum)


def test_master_adamw_default_state_is_fp32_and_unchanged():
    from pytorch_operator_amd.ops.optim import MasterAdamW
    params = _params()
    opt = MasterAdamW(params, **HP)
    assert opt.state_dtype == F32
    for p, g in zip(params, _grads(1)[0][0]):
        p.grad = g
    opt.step()
    for p in params:
        assert set(opt.state[p]) == {"step", "master", "exp_avg", "exp_avg_sq"}
        assert opt.state[p]["exp_avg"].dtype == F32 and opt.state[p]["exp_avg_sq"].dtype == F32
    with pytest.raises(TypeError):
        MasterAdamW(_params(), state_dtype=torch.float16, **HP)


def test_adamw_launch_rng_goes_with_bf16_moments():
    from pytorch_operator_amd.ops.optim import adamw_launch
    p, g = torch.zeros(8), torch.zeros(8)
    with pytest.raises(ValueError):
        adamw_launch(p, torch.zeros(8, dtype=BF16), torch.zeros(8, dtype=BF16), g, None, 8, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0)
    with pytest.raises(ValueError):
        adamw_launch(p, torch.zeros(8), torch.zeros(8), g, None, 8, 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, rng=(1, 0))


def test_master_adamw_bf16_state_is_deterministic_and_seeded():
    a, pa = _run_master(None, 1, seed=5, check=False)
    b, pb = _run_master(None, 1, seed=5, check=False)
    c, pc = _run_master(None, 1, seed=6, check=False)
    differs = 0
    for x, y, z in zip(pa, pb, pc):
        assert torch.equal(_bits(x.data), _bits(y.data))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(a.state[x][k]), _bits(b.state[y][k]))
            differs += int((_bits(a.state[x][k]) != _bits(c.state[z][k])).sum())
    assert differs > 100  # of 2 * 7673 stored moments about half the inexact ones flip


# --------------------------------------------------------------------------------- checkpoints
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(48, 64, bias=False)
        self.scale = nn.Parameter(torch.ones(64))
        self.b = nn.Linear(64, 33, bias=False)


def _make(kind, state_dtype):
    from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    torch.manual_seed(5)
    m = _Tiny()
    to_bf16_matmul_weights(m)
    if kind == "master":
        return m, MasterAdamW(m.parameters(), state_dtype=state_dtype, state_seed=9, **HP)
    return m, ZeroAdamW(m, bucket_mb=0.01, grad_view=False, state_dtype=state_dtype, state_seed=9, **HP)


def _tiny_step(m, opt, step):
    g = _gen(100 + step)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype)
    opt.step()


def _state_bits(kind, m, opt):
    out = [_bits(p.data).clone() for p in m.parameters()]
    if kind == "master":
        for p in m.parameters():
            st = opt.state[p]
            out += [_bits(st["exp_avg"]).clone(), _bits(st["exp_avg_sq"]).clone()]
            if st["master"] is not None:
                out.append(_bits(st["master"]).clone())
    else:
        for b in opt.buckets:
            out += [_bits(b.exp_avg).clone(), _bits(b.exp_avg_sq).clone()]
            if b.master is not None:
                out.append(_bits(b.master).clone())
    return out


@pytest.mark.parametrize("kind", ["master", "zero"])
def test_checkpoint_resume_is_bit_identical(kind, tmp_path):
    from pytorch_operator_amd.utils import train_ckpt
    m, opt = _make(kind, BF16)
    for step in (1, 2):
        _tiny_step(m, opt, step)
    d = str(tmp_path / "ck")
    train_ckpt.save(d, 2, m, opt, rank=0, world=1)
    _tiny_step(m, opt, 3)
    want = _state_bits(kind, m, opt)
    m2, opt2 = _make(kind, BF16)
    assert train_ckpt.load(d, m2, opt2, rank=0, world=1, device="cpu") == 2
    _tiny_step(m2, opt2, 3)
    got = _state_bits(kind, m2, opt2)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    moments = [b.exp_avg for b in opt2.buckets] if kind == "zero" else [opt2.state[p]["exp_avg"] for p in m2.parameters()]
    assert all(t.dtype == BF16 for t in moments) and any(bool(t.any()) for t in moments)


@pytest.mark.parametrize("kind", ["master", "zero"])
@pytest.mark.parametrize("saved,built", [(F32, BF16), (BF16, F32)], ids=["fp32-into-bf16", "bf16-into-fp32"])
def test_checkpoint_of_the_other_state_dtype_is_refused(kind, saved, built, tmp_path):
    from pytorch_operator_amd.utils import train_ckpt
    m, opt = _make(kind, saved)
    _tiny_step(m, opt, 1)
    d = str(tmp_path / "ck")
    train_ckpt.save(d, 1, m, opt, rank=0, world=1)
    m2, opt2 = _make(kind, built)
    with pytest.raises(ValueError) as e:
        train_ckpt.load(d, m2, opt2, rank=0, world=1, device="cpu")
    assert "fp32" in str(e.value) and "bf16" in str(e.value)


def test_checkpoint_without_the_field_is_fp32():
    from pytorch_operator_amd.utils import train_ckpt
    m, opt = _make("master", F32)
    _tiny_step(m, opt, 1)
    blob = train_ckpt.optimizer_state(opt)
    assert blob.pop("state_dtype") == "fp32"
    m2, opt2 = _make("master", F32)
    train_ckpt.load_optimizer_state(opt2, blob)
    m3, opt3 = _make("master", BF16)
    with pytest.raises(ValueError):
        train_ckpt.load_optimizer_state(opt3, blob)
    mz, oz = _make("zero", F32)
    _tiny_step(mz, oz, 1)
    sd = oz.shard_state_dict()
    assert sd.pop("state_dtype") == "fp32"
    _make("zero", F32)[1].load_shard_state_dict(sd)
    with pytest.raises(ValueError):
        _make("zero", BF16)[1].load_shard_state_dict(sd)


def test_zero_state_bytes_count_the_element_size():
    n16, n32 = 48 * 64 + 64 * 33, 64
    for dt, per16, per32 in ((F32, 12, 8), (BF16, 8, 4)):
        _, opt = _make("zero", dt)
        pad16 = sum(b.npad for b in opt.buckets if b.dtype == BF16)
        pad32 = sum(b.npad for b in opt.buckets if b.dtype == F32)
        assert pad16 >= n16 and pad32 >= n32
        assert opt.state_bytes() == per16 * pad16 + per32 * pad32


# --------------------------------------------------------------------------------- the worker's flag
def test_opt_state_flag():
    from pytorch_operator_amd.harness.ddp_train import parse_args
    assert parse_args([]).opt_state == "fp32"
    assert parse_args(["--model", "llama-mini"]).opt_state == "fp32"
    assert parse_args(["--model", "llama-mini", "--opt-state", "bf16"]).opt_state == "bf16"
    for bad in (["--model", "llama-mini", "--opt-state", "bf16", "--master-weights", "off"],
                ["--model", "resnet50", "--opt-state", "bf16"],
                ["--model", "llama-mini", "--opt-state", "bf16", "--dtype", "fp32"],
                ["--model", "llama-mini", "--opt-state", "fp8"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
