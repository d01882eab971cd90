"""Global-norm gradient clipping (``max_grad_norm``) -- CPU reference paths and the worker flag.

``MasterAdamW`` / ``ZeroAdamW`` own the gradients (fp32 comm-hook views, buckets, freed ``.grad``),
so clipping lives inside them; on CPU the same semantics run in PyTorch.  The HIP kernels
(csrc/kernels/gradclip.hip, adamw.hip) are checked against these paths in
tests/test_gradclip_gpu.py.
"""
import copy
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn as nn

from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights

ROOT = Path(__file__).resolve().parent.parent
WORKER = "pytorch_operator_amd.harness.ddp_train"


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(module, args, world, cwd, timeout=240):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(r),
                   PYTHONPATH=str(ROOT), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, "-m", module, *args], cwd=cwd, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=timeout)
        outs.append((p.returncode, out))
    return outs


def _json_lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


def test_fp32_params_match_torch_clip_grad_norm_and_adamw():
    """MasterAdamW(max_grad_norm=c) == clip_grad_norm_(c) + torch.optim.AdamW, for a c below every
    step's norm (always clips) and one above (never clips)."""
    for c, clips in ((1e-2, True), (1e4, False)):
        torch.manual_seed(0)
        a = nn.Linear(17, 9)
        b = nn.Linear(17, 9)
        b.load_state_dict(a.state_dict())
        oa = MasterAdamW(a.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1, max_grad_norm=c)
        ob = torch.optim.AdamW(b.parameters(), lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
        assert oa.last_grad_norm() is None
        for _ in range(5):
            x = torch.randn(4, 17)
            for m, o in ((a, oa), (b, ob)):
                o.zero_grad()
                m(x).pow(2).sum().backward()
            want = torch.nn.utils.clip_grad_norm_(b.parameters(), c)
            oa.step()
            ob.step()
            got = oa.last_grad_norm()
            assert got.dim() == 0 and got.dtype == torch.float32
            torch.testing.assert_close(got, want, rtol=1e-5, atol=0)
            assert (float(got) > c) if clips else (float(got) < c), (c, float(got))
        for pa, pb in zip(a.parameters(), b.parameters()):
            torch.testing.assert_close(pa, pb, rtol=1e-5, atol=1e-6)


def _llama_tiny_steps(make_opt, steps=3):
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    torch.manual_seed(0)
    m = Llama(CONFIGS["llama-tiny"])
    to_bf16_matmul_weights(m)
    opt = make_opt(m)
    x = torch.randint(0, 256, (2, 17))
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            loss = m(x[:, :-1], x[:, 1:])
        loss.backward()
        opt.step()
    return m, opt


def test_huge_max_grad_norm_is_bit_identical_to_none_master_adamw():
    """coef = min(1, 1e30 / norm) is exactly 1.0f, and g * 1.0f changes nothing."""
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1)
    m0, o0 = _llama_tiny_steps(lambda m: MasterAdamW(m.parameters(), **kw))
    m1, o1 = _llama_tiny_steps(lambda m: MasterAdamW(m.parameters(), max_grad_norm=1e30, **kw))
    assert o0.last_grad_norm() is None and float(o1.last_grad_norm()) > 0
    for p0, p1 in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p0, p1)
        s0, s1 = o0.state[p0], o1.state[p1]
        assert s0["step"] == s1["step"]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(s0[k], s1[k])
        assert (s0["master"] is None) == (s1["master"] is None)
        if s0["master"] is not None:
            assert torch.equal(s0["master"], s1["master"])


def test_huge_max_grad_norm_is_bit_identical_to_none_zero_adamw():
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, bucket_mb=0.02)
    m0, o0 = _llama_tiny_steps(lambda m: ZeroAdamW(m, **kw))
    m1, o1 = _llama_tiny_steps(lambda m: ZeroAdamW(m, max_grad_norm=1e30, **kw))
    assert o0.last_grad_norm() is None and float(o1.last_grad_norm()) > 0
    assert len(o0.buckets) == len(o1.buckets) > 2
    for p0, p1 in zip(m0.parameters(), m1.parameters()):
        assert torch.equal(p0, p1)
    for b0, b1 in zip(o0.buckets, o1.buckets):
        assert torch.equal(b0.exp_avg, b1.exp_avg) and torch.equal(b0.exp_avg_sq, b1.exp_avg_sq)
        assert (b0.master is None) == (b1.master is None)
        if b0.master is not None:
            assert torch.equal(b0.master, b1.master)


def test_zero_adamw_clipped_matches_master_adamw_clipped_on_cpu():
    """World 1: the per-bucket sum of squares equals the per-parameter one up to summation order."""
    from pytorch_operator_amd.parallel.zero import ZeroAdamW
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.1, max_grad_norm=1e-3)
    m0, o0 = _llama_tiny_steps(lambda m: MasterAdamW(m.parameters(), **kw))
    m1, o1 = _llama_tiny_steps(lambda m: ZeroAdamW(m, bucket_mb=0.02, **kw))
    assert float(o0.last_grad_norm()) > 1e-3  # clipping was active
    torch.testing.assert_close(o1.last_grad_norm(), o0.last_grad_norm(), rtol=1e-5, atol=0)
    # fp32 masters (the fp32 parameter itself where it is its own master): AdamW's 1e-5 plus the
    # norm's 1e-5, the bound of the GPU tests
    of = {id(p): b for b in o1.buckets for p in b.params}
    for p0, p1 in zip(m0.parameters(), m1.parameters()):
        b, off = of[id(p1)], of[id(p1)].slot[id(p1)]
        ms1 = (b.master if b.master is not None else b.flat_w)[off:off + p1.numel()].view(p1.shape)
        ms0 = o0.state[p0]["master"] if o0.state[p0]["master"] is not None else p0
        torch.testing.assert_close(ms1, ms0.detach(), rtol=2e-5, atol=1e-6)


def test_two_gloo_ranks_clip_identically(tmp_path):
    """ZeRO-1 and DDP + MasterAdamW with --max-grad-norm on two gloo ranks: replicas stay
    bit-identical within a run (every rank clips by the same factor), clipping is active, and
    both runs see the same first-step norm (same weights and data; only the partition of the sum
    of squares differs)."""
    base = ["--model", "llama-tiny", "--seq-len", "32", "--batch-size", "2", "--steps", "3", "--warmup", "1",
            "--backend", "gloo", "--master-weights", "on", "--zero-bucket-mb", "0.05", "--max-grad-norm", "1e-3"]
    first = {}
    for zero in ("1", "0"):
        cwd = tmp_path / f"z{zero}"
        cwd.mkdir()
        outs = _launch(WORKER, base + ["--zero", zero], 2, cwd)
        for rc, out in outs:
            assert rc == 0, out
        dig = [_json_lines(out, '"param_digest"')[-1] for _, out in outs]
        assert len({d["digest"] for d in dig}) == 1 and len({d["weights_digest"] for d in dig}) == 1, dig
        res = _json_lines(outs[0][1], '"metric"')[-1]
        assert res["zero"] == int(zero) and res["max_grad_norm"] == 1e-3
        assert res["grad_norm"] > res["max_grad_norm"], res
        assert res["loss"] == res["loss"]
        first[zero] = _json_lines(outs[0][1], '"first_step"')[-1]["grad_norm"]
        assert first[zero] > 1e-3
    assert abs(first["1"] - first["0"]) <= 1e-5 * abs(first["0"]), first


def test_worker_flag_parses_and_defaults_off():
    from pytorch_operator_amd.harness.ddp_train import parse_args
    assert parse_args([]).max_grad_norm == 0.0
    assert parse_args(["--max-grad-norm", "0.5"]).max_grad_norm == 0.5


@pytest.mark.parametrize("flag", [[], ["--max-grad-norm", "1e-3"]])
def test_plain_torch_optimizer_path_clips_with_torch(tmp_path, flag):
    """fp32 Llama (torch.optim.AdamW): the flag means clip_grad_norm_ before opt.step(); without
    it neither key appears in the output."""
    (rc, out), = _launch(WORKER, ["--model", "llama-tiny", "--seq-len", "32", "--batch-size", "2", "--steps", "2",
                                  "--warmup", "1", "--dtype", "fp32", "--no-cuda", *flag], 1, tmp_path)
    assert rc == 0, out
    res = _json_lines(out, '"metric"')[-1]
    first = _json_lines(out, '"first_step"')[-1]
    if flag:
        assert res["max_grad_norm"] == 1e-3 and res["grad_norm"] > 1e-3 and first["grad_norm"] > 1e-3
    else:
        assert "grad_norm" not in res and "max_grad_norm" not in res and "grad_norm" not in first
