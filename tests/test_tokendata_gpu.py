"""Token-file training data on the GPU: the batch kernel (csrc/kernels/token_batch.hip) against the
PyTorch composition, exactly; attention with primed document bounds; the worker with ``--data``."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
B = 3
SIZES = [1, 7, 255, 256, 257, 2049, 4096]


def make_stream(n_tokens, vocab, seed, mean_len=40):
    """tests/test_tokendata_cpu.py's stream: geometric documents, t -> (5*t + 3) % (vocab - 1), eos = vocab - 1."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_tokens:
        t = int(rng.integers(0, vocab - 1))
        for _ in range(int(rng.geometric(1.0 / mean_len)) - 1):
            out.append(t)
            t = (5 * t + 3) % (vocab - 1)
        out.append(vocab - 1)
    return np.array(out[:n_tokens], dtype=np.uint32)


def _expand(tok, width, row_stride, nrows, S, vocab, eos, offset=0):
    """tok: int64 ids on the CPU.  Returns (GPU outputs, CPU reference outputs) of the same narrow span;
    ``offset``: the span starts that many tokens into its device allocation."""
    from pytorch_operator_amd.ops import token_batch
    narrow = torch.from_numpy(tok.numpy().astype(np.uint16 if width == 2 else np.uint32)
                              .view(np.int16 if width == 2 else np.int32))
    buf = torch.empty(narrow.numel() + offset, dtype=narrow.dtype, device="cuda")
    src = buf[offset:]
    src.copy_(narrow)
    assert src.data_ptr() == buf.data_ptr() + offset * width
    got = token_batch.expand(src, row_stride, nrows, S, vocab, eos)
    ref = token_batch.expand(narrow, row_stride, nrows, S, vocab, eos)
    return got, ref


def _assert_equal(got, ref):
    for name, g, r in zip(("x", "y", "doc_start", "doc_end", "stats"), got, ref):
        if r is None:
            assert g is None, name
            continue
        assert g.dtype == r.dtype and g.shape == r.shape, name
        if not torch.equal(g.cpu(), r):
            bad = (g.cpu() != r).nonzero()
            raise AssertionError(f"{name}: {bad.shape[0]} differ, first at {bad[0].tolist()}: "
                                 f"{g.cpu()[tuple(bad[0])]} vs {r[tuple(bad[0])]}")


@pytest.mark.parametrize("width", [2, 4], ids=["uint16", "uint32"])
@pytest.mark.parametrize("S", SIZES)
def test_expand_matches_the_composition(S, width):
    """B = 3: with uint16 and an odd S, rows 1 and 2 start off the 16-byte (and 4-byte) grid."""
    vocab = 50000 if width == 2 else 100000  # ids above 2^15 / 2^16: the narrow bits are unsigned
    g = torch.Generator().manual_seed(100 * S + width)
    for eos in (vocab - 3, None):
        for row_stride in (S, S + 1):
            for offset in (0, 1):
                n = (B - 1) * row_stride + S + 1
                tok = torch.randint(0, vocab, (n,), generator=g)
                tok[torch.rand(n, generator=g) < 1.0 / 16] = vocab - 3  # documents of ~16 tokens
                got, ref = _expand(tok, width, row_stride, B, S, vocab, eos, offset)
                _assert_equal(got, ref)
                assert int(got[4][2]) == 0


def _pattern_rows(S, eos, g):
    """Rows of S + 1 tokens with the end-of-text token where the kernel's edges are."""
    def row(eos_at=()):
        t = torch.randint(0, eos, (S + 1,), generator=g)
        for p in eos_at:
            if 0 <= p <= S:
                t[p] = eos
        return t
    rows = [row([0]), row([S - 1]), row([S]), row([S // 2, S // 2 + 1]), row(), torch.full((S + 1,), eos),
            row([5, S - 3]),  # one document from 6 to S - 3: over every chunk boundary in between
            row([0, 1, S - 2, S - 1, S]), row(range(0, S + 1, 2)), row([1023, 1024, 2047, 2048])]
    return torch.stack(rows)


@pytest.mark.parametrize("width", [2, 4], ids=["uint16", "uint32"])
@pytest.mark.parametrize("S", [7, 257, 4096])
def test_expand_rows_with_eos_at_the_edges(S, width):
    vocab, eos = 1000, 998
    rows = _pattern_rows(S, eos, torch.Generator().manual_seed(S))
    # gathered rows
    got, ref = _expand(rows.reshape(-1), width, S + 1, rows.shape[0], S, vocab, eos)
    _assert_equal(got, ref)
    assert ref[3][5].tolist() == list(range(1, S)) + [S]  # the all-eos row: every document is one token
    if S > 1024:
        assert ref[2][6, 6:S - 2].unique().tolist() == [6] and ref[3][6, 6:S - 2].unique().tolist() == [S - 2]
    # the same rows overlapping by one token (row_stride = S): row b's last target is row b + 1's first token
    flat = torch.cat([r[:S] for r in rows] + [rows[-1][S:]])
    got, ref = _expand(flat, width, S, rows.shape[0], S, vocab, eos, offset=1)
    _assert_equal(got, ref)


@pytest.mark.parametrize("width", [2, 4], ids=["uint16", "uint32"])
def test_ids_outside_the_vocabulary_are_clamped_and_counted(width):
    S, vocab, eos = 2049, 1000, 500
    g = torch.Generator().manual_seed(7)
    n = (B - 1) * S + S + 1  # overlapping rows
    tok = torch.randint(0, vocab, (n,), generator=g)
    tok[torch.rand(n, generator=g) < 1.0 / 32] = eos
    # position S is row 0's last target and row 1's first token: counted in both rows
    where = torch.tensor([0, 3, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 100, 3 * S])
    tok[where] = 1  # not the end-of-text token: clamping these moves no document
    clean, _ = _expand(tok, width, S, B, S, vocab, eos)
    bad = tok.clone()
    bad[where] = torch.tensor([vocab, vocab + 1, 65535, 40000, 1000, 1001, 2000, 3000, 1002, 1003])
    got, ref = _expand(bad, width, S, B, S, vocab, eos)
    _assert_equal(got, ref)
    seams = sum(1 for p in where.tolist() if p % S == 0 and 0 < p < B * S)
    assert int(got[4][2]) == where.numel() + seams and seams >= 1
    # nothing but the clamped ids moved
    x_pos = where[where < B * S]
    want_x = clean[0].clone().view(-1)
    want_x[x_pos] = vocab - 1
    assert torch.equal(got[0].view(-1), want_x)
    assert torch.equal(got[2], clean[2]) and torch.equal(got[3], clean[3])
    assert torch.equal(got[4][:2], clean[4][:2])
    moved = (got[1] != clean[1]).nonzero()
    assert all(int(got[1][i, j]) == vocab - 1 for i, j in moved.tolist()) and moved.shape[0] <= where.numel()


def test_launcher_rejects_bad_arguments():
    from pytorch_operator_amd.ops import _native, token_batch
    lib = _native.load()
    assert token_batch.chunk() == 1024
    src = torch.zeros(64, dtype=torch.int32, device="cuda")
    x = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    ds = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    ok = (src.data_ptr(), 4, 8, 2, 8, 100, 5, x.data_ptr(), x.data_ptr(), ds.data_ptr(), ds.data_ptr(), st.data_ptr(), None)

    def call(**kw):
        names = ("src", "width", "stride", "B", "S", "vocab", "eos", "x", "y", "ds", "de", "stats", "stream")
        a = dict(zip(names, ok), **kw)
        return lib.pto_token_batch(*[a[n] for n in names])

    assert call(width=3) != 0 and call(stride=7) != 0 and call(B=0) != 0 and call(S=0) != 0
    assert call(vocab=0) != 0 and call(vocab=2 ** 31) != 0 and call(eos=100) != 0
    assert call(ds=None) != 0 and call(eos=-1) != 0  # document outputs go with eos, and only with it
    assert call(src=src.data_ptr() + 2) != 0 and call(x=None) != 0 and call(stats=None) != 0
    torch.cuda.synchronize()
    assert int(st.sum()) == 0  # nothing was launched


@pytest.mark.parametrize("D", [64, 128])
def test_primed_bounds_are_bit_identical_and_skip_the_host_checks(D, monkeypatch):
    from pytorch_operator_amd.ops import attention as A
    Bq, S, Hq, Hkv = 2, 256, 4, 2
    g = torch.Generator().manual_seed(D)
    tok = torch.randint(0, 50, (Bq, S), generator=g).cuda()
    ds = A.doc_starts_from_tokens(tok, 7)
    de = A.doc_ends(ds)
    qkv = [torch.randn(Bq, S, h, D, generator=g).to("cuda", torch.bfloat16) for h in (Hq, Hkv, Hkv)]
    do = torch.randn(Bq, S, Hq, D, generator=g).to("cuda", torch.bfloat16)

    def run(doc_start):
        q, k, v = (t.clone().requires_grad_(True) for t in qkv)
        o = A.flash_attention(q, k, v, doc_start=doc_start)
        o.backward(do)
        return o.detach(), q.grad, k.grad, v.grad

    plain = run(ds.clone())
    primed_ds, primed_de = ds.clone(), de.clone()

    def boom(*a, **k):
        raise AssertionError("the primed call recomputed or validated the bounds")
    monkeypatch.setattr(A, "doc_ends", boom)
    monkeypatch.setattr(A, "validate_doc_start", boom)
    A.set_doc_bounds(primed_ds, primed_de)
    primed = run(primed_ds)
    for a, b in zip(plain, primed):
        assert torch.equal(a, b)
    with pytest.raises(AssertionError):
        run(ds.clone())  # another tensor is not the primed one: the bounds are rebuilt
    with pytest.raises(ValueError):
        A.set_doc_bounds(primed_ds.long(), primed_de)


# ---------------------------------------------------------------- the worker
V, EOS = 512, 511


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    np.save(d / "train.npy", make_stream(40000, V, seed=21).astype(np.uint16))
    np.save(d / "eval.npy", make_stream(4 * 2 * 256 + 1, V, seed=22).astype(np.uint16))
    return d


def _run(args, cwd):
    r = subprocess.run([sys.executable, "-m", "pytorch_operator_amd.harness.ddp_train", *args], capture_output=True,
                       text=True, timeout=300, cwd=cwd, env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _lines(out, key):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and key in ln]


def _args(d, model):
    return ["--model", model, "--data", str(d / "train.npy"), "--eos-id", str(EOS), "--seq-len", "256",
            "--batch-size", "2", "--lr", "3e-3", "--lr-schedule", "cosine", "--lr-warmup-steps", "5",
            "--lr-total-steps", "30", "--max-grad-norm", "1", "--grad-accum", "2", "--warmup", "1"]


# This configuration on the CPU in fp32 (--no-cuda --dtype fp32), 30 steps, held-out loss at step 0
# and step 30: llama-mini64 6.267 -> 0.424, llama-mini 6.348 -> 0.299.  The bf16 GPU run of the same
# training gets half the drop as margin: its final loss must lie below the midpoint.
CPU_EVAL = {"llama-mini64": (6.267, 0.424), "llama-mini": (6.348, 0.299)}


@pytest.mark.parametrize("model", ["llama-mini64", "llama-mini"])
def test_worker_learns_the_stream_on_gpu(streams, tmp_path, model):
    out = _run(_args(streams, model) + ["--steps", "29", "--eval-data", str(streams / "eval.npy"),
                                        "--eval-batches", "4", "--log-every", "10"], tmp_path)
    evals = _lines(out, '"event": "eval"')
    assert [e["step"] for e in evals] == [0, 30]
    print("eval losses:", [(e["step"], round(e["loss"], 3)) for e in evals])
    first, last = CPU_EVAL[model]
    assert evals[-1]["loss"] < 0.5 * (first + last), evals
    res = _lines(out, '"metric"')[-1]
    assert res["data"] == "tokens" and res["attn_mask"] == "document"
    assert res["lr_schedule"] == "cosine" and res["grad_accum"] == 2 and res["master_weights"] is True
    assert res["eval_loss"] == evals[-1]["loss"] and res["docs_per_seq"] > 1.0
    assert res["data_tokens"] == 40000 and res["data_windows"] == (40000 - 1) // 256
    logs = _lines(out, '"event": "train"')
    assert [e["step"] for e in logs] == [10, 20, 30] and all("grad_norm" in e for e in logs)


def test_worker_resume_is_bit_identical_on_gpu(streams, tmp_path):
    base = _args(streams, "llama-mini64")
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    ck = tmp_path / "b" / "ckpt"
    oa = _run(base + ["--steps", "3"], tmp_path / "a")
    _run(base + ["--steps", "1", "--ckpt-dir", str(ck)], tmp_path / "b")
    o2 = _run(base + ["--steps", "1", "--ckpt-dir", str(ck)], tmp_path / "b")
    assert '"event": "resumed", "step": 2' in o2
    da, db = _lines(oa, '"param_digest"')[-1], _lines(o2, '"param_digest"')[-1]
    assert da["digest"] == db["digest"] and da["weights_digest"] == db["weights_digest"]
