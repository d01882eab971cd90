"""Sampling from the Llama worker on the CPU (``--sample-every``) and the stand-alone
``harness.generate``: sample events at the due steps and at the end, the same in two runs; training
itself (digests, result line) untouched by the flags; the checkpoint's weights alone reproduce the
worker's last sample.
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pytorch_operator_amd.harness.ddp_train import parse_args

ROOT = Path(__file__).resolve().parent.parent
V = 256
# what a wall clock or an allocator decides, not the training
TIMING = ("value", "ms_per_step", "tflops_per_gpu", "max_mem_gb")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(module, args, cwd):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), WORLD_SIZE="1", RANK="0",
               PYTHONPATH=str(ROOT), OMP_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-m", f"pytorch_operator_amd.harness.{module}", *args], cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return p.returncode, p.stdout


def _json_lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


def _training(out):
    res = _json_lines(out, '"metric"')[-1]
    dig = _json_lines(out, '"param_digest"')[-1]
    return {k: v for k, v in res.items() if k not in TIMING}, dig["digest"], dig["weights_digest"]


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """t -> (5 t + 3) % (V - 1) in documents closed by V - 1, as tests/test_tokendata_cpu.py builds them."""
    rng = np.random.default_rng(21)
    out = []
    while len(out) < 4000:
        t = int(rng.integers(0, V - 1))
        for _ in range(int(rng.geometric(1.0 / 40)) - 1):
            out.append(t)
            t = (5 * t + 3) % (V - 1)
        out.append(V - 1)
    path = tmp_path_factory.mktemp("tok") / "train.npy"
    np.save(path, np.array(out[:4000], dtype=np.uint16))
    return path


@pytest.mark.parametrize("opt", [[], ["--master-weights", "on", "--zero", "1"]], ids=["torch-adamw", "zero1"])
def test_worker_samples_without_disturbing_training(stream, tmp_path, opt):
    base = ["--model", "llama-tiny", "--no-cuda", "--data", str(stream), "--eos-id", str(V - 1), "--seq-len", "32",
            "--batch-size", "2", "--lr", "3e-3", "--warmup", "1", "--steps", "4", *opt]
    flags = ["--sample-every", "2", "--sample-tokens", "8"]
    outs = {}
    for name, extra in (("a", flags), ("b", flags), ("plain", [])):
        (tmp_path / name).mkdir()
        rc, outs[name] = _run("ddp_train", base + extra + ["--ckpt-dir", str(tmp_path / name / "ckpt")],
                              tmp_path / name)
        assert rc == 0, outs[name]
    ev = _json_lines(outs["a"], '"event": "sample"')
    assert [e["step"] for e in ev] == [2, 4, 5]          # the due steps, then the end
    first16 = [int(t) for t in np.load(stream)[:16]]
    for e in ev:
        assert e["prompt"] == first16
        assert len(e["tokens"]) == 8 and all(isinstance(t, int) and 0 <= t < V for t in e["tokens"])
    assert ev == _json_lines(outs["b"], '"event": "sample"')
    assert not _json_lines(outs["plain"], '"event": "sample"')
    assert _training(outs["a"]) == _training(outs["plain"])
    # the checkpoint's weights alone give the worker's last sample
    rc, out = _run("generate", ["--model", "llama-tiny", "--no-cuda", "--ckpt-dir", str(tmp_path / "a" / "ckpt"),
                                "--prompt", ",".join(map(str, first16)), "--tokens", "8"], tmp_path)
    assert rc == 0, out
    (g,) = _json_lines(out, '"event": "sample"')
    assert g == ev[-1]


def test_sampling_temperature_repeats_and_prompt_flag(stream, tmp_path):
    args = ["--model", "llama-tiny", "--no-cuda", "--dtype", "fp32", "--seq-len", "32", "--batch-size", "2",
            "--warmup", "1", "--steps", "1", "--sample-every", "5", "--sample-prompt", "3,1,4,1,5", "--sample-tokens", "6",
            "--sample-temperature", "0.8", "--sample-top-k", "40"]
    (rc1, o1), (rc2, o2) = _run("ddp_train", args, tmp_path), _run("ddp_train", args, tmp_path)
    assert rc1 == rc2 == 0, o1 + o2
    e1, e2 = _json_lines(o1, '"event": "sample"'), _json_lines(o2, '"event": "sample"')
    assert e1 == e2 and [e["step"] for e in e1] == [2] and e1[0]["prompt"] == [3, 1, 4, 1, 5]
    assert len(e1[0]["tokens"]) == 6
    # without --data and --sample-prompt the prompt is ids 1..--sample-prompt-len
    rc, out = _run("ddp_train", args[:args.index("--sample-prompt")] + ["--sample-prompt-len", "5", "--sample-tokens", "3"],
                   tmp_path)
    assert rc == 0, out
    (e,) = _json_lines(out, '"event": "sample"')
    assert e["prompt"] == [1, 2, 3, 4, 5] and len(e["tokens"]) == 3


def test_flags_are_refused_where_they_do_not_apply(capsys):
    assert parse_args(["--model", "llama-tiny"]).sample_every == 0
    for argv in (["--model", "resnet-tiny", "--sample-every", "2"], ["--model", "resnet-tiny", "--sample-tokens", "8"],
                 ["--model", "resnet-tiny", "--sample-prompt", "1,2"], ["--model", "resnet-tiny", "--sample-top-k", "5"],
                 ["--model", "llama-tiny", "--sample-every", "1", "--sample-prompt", "1,256"],
                 ["--model", "llama-tiny", "--sample-every", "1", "--sample-prompt", "-1"],
                 ["--model", "llama-tiny", "--sample-every", "1", "--sample-prompt", "a,b"],
                 ["--model", "llama-tiny", "--sample-every", "1", "--sample-prompt", ""],
                 # flags that would sample nothing without --sample-every
                 ["--model", "llama-tiny", "--sample-tokens", "8"], ["--model", "llama-tiny", "--sample-prompt", "1,2"],
                 ["--model", "llama-tiny", "--sample-temperature", "0.5"], ["--model", "llama-tiny", "--sample-top-k", "4"],
                 ["--model", "llama-tiny", "--sample-every", "1", "--sample-prompt", "1,2", "--sample-prompt-len", "4"],
                 ["--model", "llama-tiny", "--sample-every", "-1"], ["--model", "llama-tiny", "--sample-every", "1",
                                                                      "--sample-tokens", "0"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    capsys.readouterr()
    assert parse_args(["--model", "llama-tiny", "--sample-every", "3", "--sample-prompt", "1,255"]).sample_prompt_ids == [1, 255]


def test_generate_entry_refuses_a_missing_checkpoint_and_bad_ids(tmp_path):
    rc, out = _run("generate", ["--model", "llama-tiny", "--no-cuda", "--ckpt-dir", str(tmp_path), "--prompt", "1,2"],
                   tmp_path)
    assert rc == 2 and "no checkpoint" in out
    rc, out = _run("generate", ["--model", "llama-tiny", "--no-cuda", "--ckpt-dir", str(tmp_path), "--prompt", "1,999"],
                   tmp_path)
    assert rc == 2 and "vocabulary" in out
