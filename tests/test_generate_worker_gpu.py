"""Sampling from the Llama worker on the GPU: with ``--sample-every`` the worker prints sample events
(prefill on the HIP flash attention, decode on csrc/kernels/decode_attention.hip) and trains to the
same digests and result line as without, under the master-weight optimizer and under ZeRO-1.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
# what a wall clock or an allocator decides, not the training (the KV cache raises the allocator's peak)
TIMING = ("value", "ms_per_step", "tflops_per_gpu", "max_mem_gb")


def _run(args, cwd):
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", *args], capture_output=True,
                       text=True, timeout=300, cwd=cwd, env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


def _training(out):
    res = _lines(out, '"metric"')[-1]
    dig = _lines(out, '"param_digest"')[-1]
    return {k: v for k, v in res.items() if k not in TIMING}, dig["digest"], dig["weights_digest"]


@pytest.mark.parametrize("opt", [["--zero", "0"], ["--zero", "1"]], ids=["master-weights", "zero1"])
def test_sampling_leaves_the_digests_alone_on_gpu(tmp_path, opt):
    base = ["--model", "llama-mini", "--seq-len", "128", "--batch-size", "2", "--warmup", "1", "--steps", "4", *opt]
    plain = _run(base, tmp_path)
    sampled = _run(base + ["--sample-every", "2", "--sample-tokens", "8"], tmp_path)
    ev = _lines(sampled, '"event": "sample"')
    assert [e["step"] for e in ev] == [2, 4, 5] and not _lines(plain, '"event": "sample"')
    for e in ev:
        assert e["prompt"] == list(range(1, 17))
        assert len(e["tokens"]) == 8 and all(0 <= t < 512 for t in e["tokens"])
    assert _training(sampled)[0]["master_weights"] is True
    assert _training(sampled) == _training(plain)
