"""Token-file training data (``--data``): the memory-mapped reader and its window arithmetic
(data/tokens.py), the learning-rate schedule, the PyTorch composition that is the batch kernel's
reference (ops/token_batch.py), and the worker on the CPU -- convergence on a learnable stream,
checkpoint/resume, two gloo ranks, and the refusal of ids outside the vocabulary.  The HIP kernel
(csrc/kernels/token_batch.hip) is checked in tests/test_tokendata_gpu.py.
"""
import json
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent

from pytorch_operator_amd.data.tokens import TokenStream  # noqa: E402
from pytorch_operator_amd.harness.ddp_train import lr_at, parse_args  # noqa: E402

WORKER = "pytorch_operator_amd.harness.ddp_train"


def make_stream(n_tokens, vocab, seed, mean_len=40):
    """Documents of geometric length, a random first token, then t -> (5*t + 3) % (vocab - 1); each
    closed by the end-of-text id vocab - 1.  Learnable: the next token is a function of this one."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_tokens:
        t = int(rng.integers(0, vocab - 1))
        for _ in range(int(rng.geometric(1.0 / mean_len)) - 1):
            out.append(t)
            t = (5 * t + 3) % (vocab - 1)
        out.append(vocab - 1)
    return np.array(out[:n_tokens], dtype=np.uint32)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(args, world, cwd, timeout=300):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(r),
                   PYTHONPATH=str(ROOT), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, "-m", WORKER, *args], cwd=cwd, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        out, _ = p.communicate(timeout=timeout)
        outs.append((p.returncode, out))
    return outs


def _json_lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


# ---------------------------------------------------------------- 1. the reader
@pytest.mark.parametrize("dtype", ["uint16", "uint32", "int32"])
def test_npy_in_each_dtype(tmp_path, dtype):
    tok = np.random.default_rng(1).integers(0, 300, 101).astype(dtype)
    np.save(tmp_path / "a.npy", tok)
    st = TokenStream(str(tmp_path / "a.npy"), 300).bind(10, 2)
    assert st.n_tokens == 101 and st.n_windows == 10
    assert st.dtype == (np.uint16 if dtype == "uint16" else np.uint32)
    for k in range(10):
        assert np.array_equal(st.window(k), tok[10 * k:10 * k + 11])


@pytest.mark.parametrize("dtype, vocab, width", [("auto", 300, 2), ("auto", 65536, 2), ("auto", 65537, 4),
                                                 ("uint16", 100000, 2), ("uint32", 300, 4)])
def test_bin_in_both_widths(tmp_path, dtype, vocab, width):
    tok = np.random.default_rng(2).integers(0, 300, 64)
    tok.astype("<u2" if width == 2 else "<u4").tofile(tmp_path / "a.bin")
    st = TokenStream(str(tmp_path / "a.bin"), vocab, dtype).bind(7, 3)
    assert st.dtype.itemsize == width and st.n_tokens == 64 and st.n_windows == 9
    assert np.array_equal(st.window(8), tok[56:64])


def test_directory_of_three_files_stitches_a_window_across_a_boundary(tmp_path):
    tok = np.arange(1000, 1100, dtype=np.uint16)
    np.save(tmp_path / "b_second.npy", tok[35:70])
    tok[:35].tofile(tmp_path / "a_first.bin")
    np.save(tmp_path / "c_third.npy", tok[70:].astype(np.uint16))
    (tmp_path / "notes.txt").write_text("not a token file")
    st = TokenStream(str(tmp_path), 2000).bind(10, 3)
    assert [os.path.basename(f) for f in st.files] == ["a_first.bin", "b_second.npy", "c_third.npy"]
    assert st.n_tokens == 100 and st.n_windows == 9
    assert np.array_equal(st.window(3), tok[30:41])  # tokens 30..40 cross the boundary at 35
    assert np.array_equal(st.read(30, 75), tok[30:75])  # and this crosses both
    # step 1: windows 0..2 lie inside the first file -> one slice; step 2: windows 3..5 cross a file
    # boundary -> gathered rows
    span, stride = st.span(1, 0, 0)
    assert stride == 10 and np.array_equal(span, tok[0:31])
    span, stride = st.span(2, 0, 0)
    assert stride == 11 and np.array_equal(span.reshape(3, 11), np.stack([tok[30:41], tok[40:51], tok[50:61]]))


def test_mixed_widths_widen_to_uint32(tmp_path):
    np.save(tmp_path / "a.npy", np.arange(20, dtype=np.uint16))
    np.save(tmp_path / "b.npy", np.arange(20, 40, dtype=np.int32))
    st = TokenStream(str(tmp_path), 100).bind(6, 2)
    assert st.dtype == np.uint32
    assert np.array_equal(st.window(2), np.arange(12, 19))
    assert np.array_equal(st.window(3), np.arange(18, 25))


def test_the_wrap(tmp_path):
    tok = np.arange(500, 547, dtype=np.uint32)  # 47 tokens, S = 5: 9 windows, token 46 is never an input
    np.save(tmp_path / "a.npy", tok)
    st = TokenStream(str(tmp_path / "a.npy"), 1000).bind(5, 4)
    assert st.n_windows == 9
    span, stride = st.span(1, 0, 0)
    assert stride == 5 and np.array_equal(span, tok[0:21])
    span, stride = st.span(2, 0, 0)
    assert stride == 5 and np.array_equal(span, tok[20:41])
    span, stride = st.span(3, 0, 0)  # windows 8, 0, 1, 2
    assert stride == 6
    assert np.array_equal(span.reshape(4, 6), np.stack([tok[40:46], tok[0:6], tok[5:11], tok[10:16]]))
    assert [st.window_index(3, 0, 0, b) for b in range(4)] == [8, 0, 1, 2]


def test_every_refusal(tmp_path):
    np.save(tmp_path / "ok.npy", np.arange(10, dtype=np.uint16))
    np.save(tmp_path / "rank2.npy", np.zeros((4, 4), dtype=np.uint16))
    np.save(tmp_path / "int64.npy", np.arange(10))
    np.save(tmp_path / "float.npy", np.arange(10, dtype=np.float32))
    np.save(tmp_path / "empty.npy", np.zeros(0, dtype=np.uint16))
    (tmp_path / "empty.bin").write_bytes(b"")
    (tmp_path / "odd.bin").write_bytes(b"\0" * 7)
    (tmp_path / "tokens.txt").write_text("1 2 3")
    (tmp_path / "nothing").mkdir()
    for name in ("rank2.npy", "int64.npy", "float.npy", "empty.npy", "empty.bin", "tokens.txt", "nothing",
                 "missing.npy"):
        with pytest.raises(ValueError):
            TokenStream(str(tmp_path / name), 100)
    with pytest.raises(ValueError):
        TokenStream(str(tmp_path / "odd.bin"), 100000)  # 7 bytes of uint32
    with pytest.raises(ValueError):
        TokenStream(str(tmp_path / "ok.npy"), 100, dtype="int8")
    st = TokenStream(str(tmp_path / "ok.npy"), 100)
    st.bind(9, 1)
    with pytest.raises(ValueError):
        st.bind(10, 1)  # 10 tokens are one short of a window of 10 + 1
    with pytest.raises(ValueError):
        st.bind(4, 0)


# ---------------------------------------------------------------- 2. window arithmetic
def test_ranks_windows_are_disjoint_and_in_order(tmp_path):
    np.save(tmp_path / "a.npy", np.arange(8 * 19 + 1, dtype=np.uint16))  # 19 windows of 8
    W, N, B = 2, 2, 2
    st = TokenStream(str(tmp_path / "a.npy"), 1000).bind(8, B, N, W)
    assert st.n_windows == 19
    seen = []
    for t in (1, 2, 3):
        step = [[st.window_index(t, m, r, b) for m in range(N) for b in range(B)] for r in range(W)]
        assert not set(step[0]) & set(step[1])
        for m in range(N):
            for r in range(W):
                for b in range(B):
                    seen.append(st.window_index(t, m, r, b))
                    # and the span's rows are those windows
                    span, stride = st.span(t, m, r)
                    assert np.array_equal(span[b * stride:b * stride + 9], st.window(seen[-1]))
    assert seen == [k % 19 for k in range(3 * N * W * B)]


# ---------------------------------------------------------------- 3. the schedule
def test_schedule_matches_the_closed_form():
    lr, K, T, r = 3e-3, 10, 60, 0.1

    def ref(t):
        if t <= K:
            return lr * t / K
        if t >= T:
            return lr * r
        return lr * (r + (1 - r) * 0.5 * (1 + math.cos(math.pi * (t - K) / (T - K))))

    for t in (1, K, K + 1, (K + T) // 2, T, T + 5):
        assert lr_at(t, lr, "cosine", K, r, T) == ref(t)
    assert lr_at(K, lr, "cosine", K, r, T) == lr and lr_at(T, lr, "cosine", K, r, T) == lr * r
    assert lr_at((K + T) // 2, lr, "cosine", K, r, T) == pytest.approx(lr * (r + (1 - r) * 0.5))
    # constant: warm-up, then lr itself
    assert [lr_at(t, lr, "constant", 4) for t in (1, 2, 4, 5, 1000)] == [lr * 1 / 4, lr * 2 / 4, lr, lr, lr]
    assert lr_at(1, lr) == lr


def test_flags(capsys):
    a = parse_args(["--model", "llama-tiny"])
    assert a.data is None and a.lr_schedule == "constant" and a.lr_warmup_steps == 0 and a.log_every == 0
    assert a.lr_min_ratio == 0.1
    for bad in (["--model", "resnet-tiny", "--data", "x.npy"],
                ["--model", "llama-tiny", "--data", "x.npy", "--doc-len-mean", "8"],
                ["--model", "llama-tiny", "--lr-schedule", "cosine"],
                ["--model", "llama-tiny", "--lr-schedule", "cosine", "--lr-total-steps", "5", "--lr-warmup-steps", "5"],
                ["--model", "llama-tiny", "--eval-data", "x.npy"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2
    capsys.readouterr()


# ---------------------------------------------------------------- 4. the kernel's reference
def test_reference_composition_on_a_hand_built_row():
    from pytorch_operator_amd.ops import token_batch
    eos = 9
    #            0  1  2  3  4  5 | last target
    row0 = [5, 9, 9, 3, 4, 9, 7]
    row1 = [1, 2, 3, 4, 5, 6, 9]
    src = torch.tensor(row0 + row1, dtype=torch.int32)
    x, y, ds, de, stats = token_batch.expand(src, 7, 2, 6, 10, eos)
    assert x.tolist() == [row0[:6], row1[:6]] and x.dtype == torch.int64
    assert y.tolist() == [[9, -100, -100, 4, 9, -100], [2, 3, 4, 5, 6, 9]]
    assert ds.tolist() == [[0, 0, 2, 3, 3, 3], [0] * 6] and ds.dtype == torch.int32
    assert de.tolist() == [[2, 2, 3, 6, 6, 6], [6] * 6] and de.dtype == torch.int32
    assert stats.tolist() == [9, 4, 0]
    # overlapping rows (row_stride = S), no eos, uint16 bits above 2^15, one id >= vocab
    src = torch.from_numpy(np.array([40000, 1, 2, 50001, 4, 5, 6], dtype=np.uint16).view(np.int16))
    x, y, ds, de, stats = token_batch.expand(src, 3, 2, 3, 50001)
    assert x.tolist() == [[40000, 1, 2], [50000, 4, 5]] and y.tolist() == [[1, 2, 50000], [4, 5, 6]]
    assert ds is None and de is None
    assert stats.tolist() == [6, 2, 2]  # the id at the seam is row 0's last target and row 1's first token
    with pytest.raises(ValueError):
        token_batch.expand(src, 3, 3, 3, 50001)  # 3 rows need 10 tokens
    with pytest.raises(TypeError):
        token_batch.expand(src.to(torch.int64), 3, 2, 3, 50001)


# ---------------------------------------------------------------- 5. the worker
V, EOS = 256, 255


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    np.save(d / "train.npy", make_stream(40000, V, seed=11).astype(np.uint16))
    np.save(d / "eval.npy", make_stream(4 * 8 * 64 + 1, V, seed=12).astype(np.uint16))
    return d


def _train_args(d, steps):
    return ["--model", "llama-tiny", "--no-cuda", "--data", str(d / "train.npy"), "--eos-id", str(EOS),
            "--seq-len", "64", "--batch-size", "8", "--lr", "3e-3", "--lr-schedule", "cosine",
            "--lr-warmup-steps", "10", "--lr-total-steps", "60", "--warmup", "1", "--steps", str(steps - 1)]


@pytest.mark.parametrize("opt", [["--dtype", "fp32"], ["--dtype", "bf16", "--master-weights", "on", "--zero", "0"],
                                 ["--dtype", "bf16", "--master-weights", "on", "--zero", "1"]],
                         ids=["fp32-torch-adamw", "master-weights", "zero1"])
def test_worker_learns_the_stream(streams, tmp_path, opt):
    """60 steps of cosine-scheduled training: the held-out loss at the end is below half the step-0
    loss (plain torch AdamW on this model and stream: 5.52 -> 0.60)."""
    args = _train_args(streams, 60) + ["--eval-data", str(streams / "eval.npy"), "--eval-batches", "4",
                                       "--log-every", "20", *opt]
    (rc, out), = _worker(args, 1, tmp_path)
    assert rc == 0, out
    evals = _json_lines(out, '"event": "eval"')
    assert [e["step"] for e in evals] == [0, 60]
    print("eval losses:", [(e["step"], round(e["loss"], 3)) for e in evals])
    assert evals[0]["tokens"] == evals[1]["tokens"] and 0 < evals[0]["tokens"] <= 4 * 8 * 64
    assert evals[-1]["loss"] < 0.5 * evals[0]["loss"], evals
    assert evals[-1]["ppl"] == pytest.approx(math.exp(evals[-1]["loss"]))
    res = _json_lines(out, '"metric"')[-1]
    assert res["data"] == "tokens" and res["attn_mask"] == "document" and res["lr_schedule"] == "cosine"
    assert res["eval_loss"] == evals[-1]["loss"]
    assert res["data_tokens"] == 40000 and res["data_windows"] == (40000 - 1) // 64
    assert res["data_epochs"] == pytest.approx(60 * 8 / res["data_windows"], abs=1e-3)
    assert res["docs_per_seq"] > 1.0
    logs = _json_lines(out, '"event": "train"')
    assert [e["step"] for e in logs] == [20, 40, 60]
    assert [e["lr"] for e in logs] == [lr_at(t, 3e-3, "cosine", 10, 0.1, 60) for t in (20, 40, 60)]


def test_worker_without_eos_is_plain_causal(streams, tmp_path):
    args = ["--model", "llama-tiny", "--no-cuda", "--dtype", "fp32", "--data", str(streams / "train.npy"),
            "--seq-len", "64", "--batch-size", "2", "--warmup", "1", "--steps", "1"]
    (rc, out), = _worker(args, 1, tmp_path)
    assert rc == 0, out
    res = _json_lines(out, '"metric"')[-1]
    assert res["data"] == "tokens" and "attn_mask" not in res and "eval_loss" not in res
    assert res["lr_schedule"] == "constant"


def test_worker_checkpoint_resume_matches_uninterrupted(streams, tmp_path):
    base = ["--model", "llama-tiny", "--no-cuda", "--data", str(streams / "train.npy"), "--eos-id", str(EOS),
            "--seq-len", "64", "--batch-size", "2", "--lr", "3e-3", "--lr-schedule", "cosine",
            "--lr-warmup-steps", "2", "--lr-total-steps", "6", "--warmup", "1", "--master-weights", "on",
            "--zero", "0", "--grad-accum", "2"]
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    ck = tmp_path / "b" / "ckpt"
    (ra, oa), = _worker(base + ["--steps", "5"], 1, tmp_path / "a")
    (r1, o1), = _worker(base + ["--steps", "2", "--ckpt-dir", str(ck)], 1, tmp_path / "b")
    (r2, o2), = _worker(base + ["--steps", "2", "--ckpt-dir", str(ck)], 1, tmp_path / "b")
    assert ra == r1 == r2 == 0, oa + o1 + o2
    assert '"event": "resumed", "step": 3' in o2
    da, db = _json_lines(oa, '"param_digest"')[-1], _json_lines(o2, '"param_digest"')[-1]
    assert da["digest"] == db["digest"] and da["weights_digest"] == db["weights_digest"]
    d1 = _json_lines(o1, '"param_digest"')[-1]
    assert d1["digest"] != da["digest"]
    assert _json_lines(o2, '"metric"')[-1]["checkpoint_step"] == 6


def test_worker_two_gloo_ranks_see_different_windows_and_agree(streams, tmp_path):
    args = ["--model", "llama-tiny", "--backend", "gloo", "--data", str(streams / "train.npy"), "--eos-id", str(EOS),
            "--seq-len", "64", "--batch-size", "2", "--warmup", "1", "--steps", "2", "--master-weights", "on",
            "--zero", "1", "--zero-bucket-mb", "0.05", "--log-every", "1", "--lr-schedule", "cosine",
            "--lr-warmup-steps", "1", "--lr-total-steps", "3"]
    outs = _worker(args, 2, tmp_path)
    for rc, out in outs:
        assert rc == 0, out
    dig = [_json_lines(out, '"param_digest"')[-1] for _, out in outs]
    assert len({d["digest"] for d in dig}) == 1 and len({d["weights_digest"] for d in dig}) == 1, dig
    first = [_json_lines(out, '"event": "train"')[0] for _, out in outs]
    assert [e["step"] for e in first] == [1, 1] and sorted(e["rank"] for e in first) == [0, 1]
    assert first[0]["loss"] != first[1]["loss"], first


def test_worker_refuses_ids_outside_the_vocabulary(tmp_path):
    tok = make_stream(2000, V, seed=13).astype(np.uint16)
    tok[[70, 300, 301]] = [256, 700, 65535]  # inside windows 1 and 4, none on a window seam
    np.save(tmp_path / "bad.npy", tok)
    args = ["--model", "llama-tiny", "--no-cuda", "--dtype", "fp32", "--data", str(tmp_path / "bad.npy"),
            "--eos-id", str(EOS), "--seq-len", "64", "--batch-size", "8", "--warmup", "1", "--steps", "1"]
    (rc, out), = _worker(args, 1, tmp_path)
    assert rc == 2, out
    assert "3 token id(s) >= the vocabulary size 256" in out, out
    assert '"metric"' not in out
