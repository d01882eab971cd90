"""Gradient accumulation (``grad_accum=N`` / ``--grad-accum N``) -- CPU paths and the worker flag.

The step's gradient is ``A = ((g_1 + g_2) + ... + g_N)``: each micro-batch's autograd gradient
widened to fp32, summed sequentially, and consumed as ``A * fp32(1/(N*W))``.  The reference side
forms that by hand (autograd on a twin model, an fp32 sum in order) and feeds it to an N = 1
``MasterAdamW`` through ``p._pto_grad32``, the existing fp32-gradient hook.  The HIP fold kernel
(csrc/kernels/gradaccum.hip) is checked in tests/test_gradaccum_gpu.py.
"""
import copy
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights  # noqa: E402

WORKER = "pytorch_operator_amd.harness.ddp_train"
KW = dict(lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(cmd, world, cwd, timeout=240):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(r),
                   PYTHONPATH=str(ROOT), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *cmd], cwd=cwd, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=timeout)
        outs.append((p.returncode, out))
    return outs


def _worker(args, world, cwd):
    return _launch(["-m", WORKER, *args], world, cwd)


def _json_lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


def _scale(n):
    return torch.tensor(1.0 / n, dtype=torch.float32)


class Small(nn.Module):
    """Two bf16 linears (after ``to_bf16_matmul_weights``) and one fp32 parameter."""

    def __init__(self):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(17, 9), nn.Tanh(), nn.Linear(9, 5))
        self.gain = nn.Parameter(torch.linspace(0.5, 1.5, 5))

    def forward(self, x):
        return (self.net(x.to(self.net[0].weight.dtype)).float() * self.gain).pow(2).mean()


def _pair():
    torch.manual_seed(0)
    m = Small()
    ref = copy.deepcopy(m)
    to_bf16_matmul_weights(m)
    to_bf16_matmul_weights(ref)
    return m, ref


def _hand_sum(ref, batches, loss_of=lambda m, x: m(x)):
    """((g_1 + g_2) + ...) per parameter of ``ref``: fp32, in order, the first term stored."""
    total = {}
    for x in batches:
        for p in ref.parameters():
            p.grad = None
        loss_of(ref, x).backward()
        for p in ref.parameters():
            if p.grad is not None:
                g = p.grad.float()
                total[p] = g.clone() if p not in total else total[p] + g
    return total


def _feed(ref, total, scale):
    """Hand the reference optimizer ``A * scale`` through the fp32-gradient hook."""
    for p in ref.parameters():
        p.grad = None
        if p in total:
            p.grad = torch.zeros_like(p)  # (only marks the parameter as having a gradient)
            p._pto_grad32 = total[p] * scale


def _accum_step(m, opt, batches, loss_of=lambda m, x: m(x)):
    opt.zero_grad(set_to_none=True)
    for k, x in enumerate(batches):
        loss_of(m, x).backward()
        if k < len(batches) - 1:
            opt.accumulate()
    opt.step()


def _assert_same_state(m, opt, ref, oref, exact=True):
    for (name, p), q in zip(m.named_parameters(), ref.parameters()):
        s, r = opt.state[p], oref.state[q]
        assert s["step"] == r["step"], name
        pairs = [(s["exp_avg"], r["exp_avg"]), (s["exp_avg_sq"], r["exp_avg_sq"]), (p.detach(), q.detach())]
        assert (s["master"] is None) == (r["master"] is None)
        if s["master"] is not None:
            pairs.append((s["master"], r["master"]))
        for a, b in pairs:
            if exact:
                assert torch.equal(a, b), name
            else:
                torch.testing.assert_close(a.float(), b.float(), rtol=2e-5, atol=1e-6, msg=name)


# ---------------------------------------------------------------- 1. hand-built reference
@pytest.mark.parametrize("n", [2, 3])
def test_master_adamw_matches_hand_built_sum(n):
    m, ref = _pair()
    opt, oref = MasterAdamW(m.parameters(), grad_accum=n, **KW), MasterAdamW(ref.parameters(), **KW)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        batches = [torch.randn(4, 17, generator=g) * (10.0 ** -k) for k in range(n)]
        _accum_step(m, opt, batches)
        _feed(ref, _hand_sum(ref, batches), _scale(n))
        oref.step()
        _assert_same_state(m, opt, ref, oref)
    assert all(p.grad is None for p in m.parameters())
    assert not any(isinstance(k, str) and "acc" in k for st in opt.state.values() for k in st)
    assert set(opt.state_dict()["state"][0]) == {"step", "master", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("n", [2, 3])
def test_master_adamw_clipped_matches_hand_built_sum(n):
    c = 1e-3
    m, ref = _pair()
    opt = MasterAdamW(m.parameters(), grad_accum=n, max_grad_norm=c, **KW)
    oref = MasterAdamW(ref.parameters(), max_grad_norm=c, **KW)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        batches = [torch.randn(4, 17, generator=g) for _ in range(n)]
        _accum_step(m, opt, batches)
        _feed(ref, _hand_sum(ref, batches), _scale(n))
        oref.step()
        assert float(oref.last_grad_norm()) > c  # clipping was active
        torch.testing.assert_close(opt.last_grad_norm(), oref.last_grad_norm(), rtol=1e-5, atol=0)
    for p, q in zip(m.parameters(), ref.parameters()):
        a = opt.state[p]["master"] if opt.state[p]["master"] is not None else p.detach()
        b = oref.state[q]["master"] if oref.state[q]["master"] is not None else q.detach()
        torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-6)


# ---------------------------------------------------------------- 2. identical micro-batches
def _llama_tiny(make_opt, n, steps=3, batches=None):
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-tiny"])
    to_bf16_matmul_weights(m)
    opt = make_opt(m)
    gen = torch.Generator().manual_seed(5)
    for _ in range(steps):
        xs = batches(gen) if batches else [torch.randint(0, 256, (2, 17), generator=gen)] * n
        opt.zero_grad(set_to_none=True)
        for k, x in enumerate(xs):
            with torch.autocast("cpu", dtype=torch.bfloat16):
                loss = m(x[:, :-1], x[:, 1:])
            loss.backward()
            if k < n - 1:
                opt.accumulate()
        opt.step()
    return m, opt


def _zero_masters(m, opt):
    """Each parameter's fp32 master, read through its bucket slot (world 1)."""
    of = {id(p): b for b in opt.buckets for p in b.params}
    out = []
    for p in m.parameters():
        b, off = of[id(p)], of[id(p)].slot[id(p)]
        out.append((b.master if b.master is not None else b.flat_w)[off:off + p.numel()].view(p.shape))
    return out


def _master_masters(m, opt):
    return [opt.state[p]["master"] if opt.state[p]["master"] is not None else p.detach() for p in m.parameters()]


@pytest.mark.parametrize("n", [2, 4])
def test_identical_micro_batches_equal_one_batch(n):
    """g + g (+ g + g) and the power-of-two 1/N are exact: N copies of a batch train as the batch."""
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1)
    m1, o1 = _llama_tiny(lambda m: MasterAdamW(m.parameters(), **kw), 1)
    mn, on = _llama_tiny(lambda m: MasterAdamW(m.parameters(), grad_accum=n, **kw), n)
    for a, b in zip(_master_masters(m1, o1), _master_masters(mn, on)):
        assert torch.equal(a, b)
    z1, p1 = _llama_tiny(lambda m: ZeroAdamW(m, bucket_mb=0.02, **kw), 1)
    zn, pn = _llama_tiny(lambda m: ZeroAdamW(m, bucket_mb=0.02, grad_accum=n, **kw), n)
    assert len(pn.buckets) > 2
    for a, b, c in zip(_zero_masters(z1, p1), _zero_masters(zn, pn), _master_masters(m1, o1)):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(z1.parameters(), zn.parameters()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 3. ZeroAdamW vs MasterAdamW, world 1
@pytest.mark.parametrize("grad_view", [True, False])
@pytest.mark.parametrize("n", [2, 3])
def test_zero_adamw_accum_matches_master_adamw_accum_world_1(n, grad_view):
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, grad_accum=n)

    def batches(gen):
        return [torch.randint(0, 256, (2, 17), generator=gen) for _ in range(n)]
    m0, o0 = _llama_tiny(lambda m: MasterAdamW(m.parameters(), **kw), n, batches=batches)
    m1, o1 = _llama_tiny(lambda m: ZeroAdamW(m, bucket_mb=0.02, grad_view=grad_view, **kw), n, batches=batches)
    assert len(o1.buckets) > 2 and all(b.acc is not None and b.acc.numel() == b.npad for b in o1.buckets)
    for a, b in zip(_master_masters(m0, o0), _zero_masters(m1, o1)):
        assert torch.equal(a, b)
    for a, b in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. two gloo ranks
def _rank_batches(rank, n, step):
    gen = torch.Generator().manual_seed(1000 + 100 * step + 10 * rank)
    return [torch.randint(0, 256, (2, 17), generator=gen) for _ in range(n)]


def _llama_loss(m, x):
    with torch.autocast("cpu", dtype=torch.bfloat16):
        return m(x[:, :-1], x[:, 1:])


def _gloo_rank_main(n, reduce_name):
    """One of two gloo ranks: ZeroAdamW(grad_accum=n) against the hand reference every rank can
    form alone (all ranks' micro-batches come from seeds)."""
    import torch.distributed as dist
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    rdt = getattr(torch, reduce_name)
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-tiny"])
    ref = copy.deepcopy(m)
    to_bf16_matmul_weights(m)
    to_bf16_matmul_weights(ref)
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1)
    opt = ZeroAdamW(m, bucket_mb=0.02, reduce_dtype=rdt, grad_accum=n, **kw)
    oref = MasterAdamW(ref.parameters(), **kw)
    assert all(b.gdt == b.dtype and b.unscaled for b in opt.buckets)
    for step in range(2):
        _accum_step(m, opt, _rank_batches(rank, n, step), _llama_loss)
        sums = [_hand_sum(ref, _rank_batches(r, n, step), _llama_loss) for r in range(world)]
        total = {}
        for p in ref.parameters():
            if rdt == torch.bfloat16:
                total[p] = (sums[0][p].bfloat16() + sums[1][p].bfloat16()).float()
            else:
                total[p] = sums[0][p] + sums[1][p]
        _feed(ref, total, _scale(n * world))
        oref.step()
    opt.synchronize()
    want = dict(zip((id(p) for p in m.parameters()), _master_masters(ref, oref)))
    for b in opt.buckets:
        shard = b.master if b.master is not None else b.w_shard().float()
        full = torch.zeros(b.npad, dtype=torch.float32)
        dist.all_gather_into_tensor(full, shard.contiguous())
        for p in b.params:
            off = b.slot[id(p)]
            assert torch.equal(full[off:off + p.numel()].view(p.shape), want[id(p)].float()), (rank, tuple(p.shape))
    for a, b in zip(m.parameters(), ref.parameters()):
        assert torch.equal(a, b)
    dist.barrier()
    dist.destroy_process_group()
    print("GLOO_RANK_OK", flush=True)


@pytest.mark.parametrize("reduce_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("n", [2, 3])
def test_two_gloo_ranks_match_hand_built_sum(tmp_path, n, reduce_name):
    outs = _launch([str(Path(__file__).resolve()), "gloo-rank", str(n), reduce_name], 2, tmp_path)
    for rc, out in outs:
        assert rc == 0 and "GLOO_RANK_OK" in out, out


# ---------------------------------------------------------------- 5. gradients in some micro-batches only
class Gated(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(8, 8)
        self.b = nn.Linear(8, 8)       # in the graph of the second micro-batch only
        self.unused = nn.Linear(8, 8)  # never in the graph
        self.c = nn.Linear(8, 4)

    def forward(self, x, use_b):
        h = torch.relu(self.a(x))
        if use_b:
            h = h + self.b(h)
        return self.c(h).square().mean()


@pytest.mark.parametrize("kind", ["master", "zero"])
def test_gradient_in_one_of_two_micro_batches(kind):
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    torch.manual_seed(1)
    m = Gated()
    ref = copy.deepcopy(m)
    opt = MasterAdamW(m.parameters(), grad_accum=2, **KW) if kind == "master" else \
        ZeroAdamW(m, bucket_mb=1.0, grad_accum=2, **KW)
    oref = MasterAdamW(ref.parameters(), **KW)
    before = m.unused.weight.detach().clone()
    gen = torch.Generator().manual_seed(2)
    for _ in range(3):
        xs = [torch.randn(5, 8, generator=gen) for _ in range(2)]
        opt.zero_grad(set_to_none=True)
        m(xs[0], False).backward()
        opt.accumulate()
        m(xs[1], True).backward()
        opt.step()
        total = {}
        for k, x in enumerate(xs):
            for p in ref.parameters():
                p.grad = None
            ref(x, k == 1).backward()
            for p in ref.parameters():
                if p.grad is not None:
                    total[p] = p.grad.clone() if p not in total else total[p] + p.grad
        assert ref.b.weight in total and ref.unused.weight not in total
        _feed(ref, total, _scale(2))
        oref.step()
    for (name, p), q in zip(m.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(m.unused.weight, before) and not torch.equal(m.b.weight, before * 0)
    if kind == "master":
        assert m.unused.weight not in opt.state and opt.state[m.b.weight]["step"] == 3


# ---------------------------------------------------------------- 6. miscounts
@pytest.mark.parametrize("kind", ["master", "zero"])
def test_miscounted_calls_raise(kind):
    from pytorch_operator_amd.parallel.zero import ZeroAdamW

    def make(n):
        torch.manual_seed(0)
        m = nn.Linear(8, 4)
        kw = dict(KW, **({"grad_accum": n} if n else {}))
        return m, (MasterAdamW(m.parameters(), **kw) if kind == "master" else ZeroAdamW(m, **kw))
    x = torch.randn(3, 8)
    m, o = make(3)
    m(x).sum().backward()
    o.accumulate()
    m(x).sum().backward()
    with pytest.raises(RuntimeError, match="accumulate"):
        o.step()  # too few
    o.accumulate()
    m(x).sum().backward()
    with pytest.raises(RuntimeError, match="accumulate"):
        o.accumulate()  # too many
    o.step()  # the count is right now
    for n in (0, 1):
        m, o = make(n)
        m(x).sum().backward()
        with pytest.raises(RuntimeError, match="grad_accum"):
            o.accumulate()
        o.step()
    with pytest.raises(ValueError):
        make(-1)


def test_second_backward_without_grad_accum_still_raises_in_zero_adamw():
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    m = nn.Linear(8, 4)
    o = ZeroAdamW(m, **KW)
    x = torch.randn(3, 8)
    m(x).sum().backward()
    with pytest.raises(RuntimeError, match=r"a second backward before step\(\)"):
        m(x).sum().backward()


# ---------------------------------------------------------------- 7. worker
BASE = ["--model", "llama-tiny", "--seq-len", "32", "--batch-size", "2", "--steps", "2", "--warmup", "1"]


def test_worker_flag_parses_defaults_to_1_and_refuses_resnet(capsys):
    from pytorch_operator_amd.harness.ddp_train import parse_args
    assert parse_args([]).grad_accum == 1
    assert parse_args(["--model", "llama-tiny", "--grad-accum", "4"]).grad_accum == 4
    for bad in (["--model", "resnet-tiny", "--grad-accum", "2"], ["--model", "llama-tiny", "--grad-accum", "0"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert "--grad-accum" in capsys.readouterr().err


@pytest.mark.parametrize("zero", ["0", "1"])
def test_worker_accumulates_with_master_weights_on_cpu(tmp_path, zero):
    args = BASE + ["--no-cuda", "--master-weights", "on", "--zero", zero]
    (rc, out), = _worker(args + ["--grad-accum", "2"], 1, tmp_path)
    assert rc == 0, out
    res = _json_lines(out, '"metric"')[-1]
    assert res["grad_accum"] == 2 and res["zero"] == int(zero) and math.isfinite(res["loss"])
    # value counts 2 * B sequences of 32 tokens per optimizer step
    assert res["value"] == pytest.approx(2 * 2 * 32 / (res["ms_per_step"] / 1e3), rel=1e-3)
    (rc, out), = _worker(args, 1, tmp_path)
    assert rc == 0, out
    plain = _json_lines(out, '"metric"')[-1]
    assert "grad_accum" not in plain
    assert set(res) - set(plain) == {"grad_accum"}


def test_worker_two_gloo_ranks_zero1_agree_and_ddp_is_refused(tmp_path):
    args = BASE + ["--backend", "gloo", "--master-weights", "on", "--zero-bucket-mb", "0.05", "--grad-accum", "2"]
    outs = _worker(args + ["--zero", "1"], 2, tmp_path)
    for rc, out in outs:
        assert rc == 0, out
    dig = [_json_lines(out, '"param_digest"')[-1] for _, out in outs]
    assert len({d["digest"] for d in dig}) == 1 and len({d["weights_digest"] for d in dig}) == 1, dig
    assert _json_lines(outs[0][1], '"metric"')[-1]["grad_accum"] == 2
    outs = _worker(args + ["--zero", "0"], 2, tmp_path)
    for rc, out in outs:
        assert rc != 0 and "--zero 1" in out, out


def test_worker_fp32_torch_optimizer_path_accumulates(tmp_path):
    (rc, out), = _worker(BASE + ["--dtype", "fp32", "--no-cuda", "--grad-accum", "2"], 1, tmp_path)
    assert rc == 0, out
    res = _json_lines(out, '"metric"')[-1]
    assert res["grad_accum"] == 2 and res["master_weights"] is False and math.isfinite(res["loss"])


# ---------------------------------------------------------------- 8. checkpoint / resume
def test_worker_checkpoint_resume_matches_uninterrupted(tmp_path):
    base = ["--model", "llama-tiny", "--seq-len", "32", "--batch-size", "2", "--warmup", "1", "--no-cuda",
            "--master-weights", "on", "--zero", "0", "--grad-accum", "2"]
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    ck = tmp_path / "b" / "ckpt"
    (ra, oa), = _worker(base + ["--steps", "3"], 1, tmp_path / "a")
    (r1, o1), = _worker(base + ["--steps", "1", "--ckpt-dir", str(ck), "--ckpt-every", "1"], 1, tmp_path / "b")
    (r2, o2), = _worker(base + ["--steps", "1", "--ckpt-dir", str(ck), "--ckpt-every", "1"], 1, tmp_path / "b")
    assert ra == r1 == r2 == 0, oa + o1 + o2
    assert '"event": "resumed", "step": 2' in o2  # --ckpt-every counts optimizer steps
    da, db = _json_lines(oa, '"param_digest"')[-1], _json_lines(o2, '"param_digest"')[-1]
    assert da["digest"] == db["digest"] and da["weights_digest"] == db["weights_digest"]
    assert _json_lines(o2, '"metric"')[-1]["checkpoint_step"] == 4
    blob = torch.load(ck / "step_4" / "optim.pt", weights_only=True)
    assert blob["kind"] == "master_adamw"
    for st in blob["state"]:
        assert set(st) == {"step", "master", "exp_avg", "exp_avg_sq"}  # no accumulator


if __name__ == "__main__":
    assert sys.argv[1] == "gloo-rank"
    _gloo_rank_main(int(sys.argv[2]), sys.argv[3])
