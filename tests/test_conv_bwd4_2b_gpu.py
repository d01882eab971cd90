"""conv_bwd4's 2b (round 8): dW_conv2 against an fp64 CPU reference computed from the launch's
own a1 / dz2 / xn, the other three gradients bit for bit against the round-7 kernel, the block
seams and rows co 48 / 49, and determinism.

The round-7 kernel's figures (max error relative to the reference's max magnitude, and a sha256
of every gradient) are the record in profiles/r8_bwd4_2b/numerics.json, written by
tools/conv_bwd4_numerics.py with the round-7 library loaded.  A regrouping of 2b's K sum may move
dW_conv2's error by a small factor -- every fixed order of a 256-term fp32 sum obeys the same
bound -- so dW_conv2 is held to twice the round-7 error; a wrong tile, K part or column moves it
by orders of magnitude.  (The kernel as merged keeps round 7's grouping; the shared-operand 2b
this was written for passed it too, profiles/r8_bwd4_2b/bit_identity.txt.)
"""
import json
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
RECORD = ROOT / "profiles" / "r8_bwd4_2b" / "numerics.json"


@pytest.fixture(scope="module")
def lib():
    from pytorch_operator_amd.ops import _native
    return _native.load()


@pytest.fixture(scope="module")
def num():
    import conv_bwd4_numerics
    return conv_bwd4_numerics


@pytest.fixture(scope="module")
def record():
    return json.loads(RECORD.read_text())["batches"]


@pytest.mark.parametrize("B", [1, 4, 5, 64])
def test_gradients_against_fp64_and_round7(lib, num, record, B):
    grads, inputs = num.run_case(num.make_case(B))
    ref = num.reference(*inputs)
    r7 = record[str(B)]
    for n in num.NAMES:
        err = num.rel_err(grads[n], ref[n])
        print(f"B={B} {n}: max rel err {err:.3e} (round 7: {r7['max_rel_err'][n]:.3e})")
    err = num.rel_err(grads["conv2.weight"], ref["conv2.weight"])
    assert err <= 2.0 * r7["max_rel_err"]["conv2.weight"], (B, err, r7["max_rel_err"]["conv2.weight"])
    for n in num.NAMES[1:]:  # only 2b's grouping changed
        assert num.digest(grads[n]) == r7["sha256"][n], (B, n)


# j columns at the block seams of every channel group cig: block r's columns start at
# jbase = 32 r - cig (clamped below 0 and at 125), its two j tiles 16 apart
def _seam_columns():
    cols = set()
    for cig in range(4):
        for j in (0, 124, 31, 32, 95, 96):
            cols.add(cig * 125 + j)
        for r in range(1, 4):
            for d in (-1, 0, 15, 16):
                cols.add(cig * 125 + 32 * r - cig + d)
    return sorted(cols)


@pytest.mark.parametrize("cos", [(48, 49), (0, 47)])
def test_edge_rows_and_seam_columns(lib, num, cos):
    """dz2 non-zero in two output channels only.  Every dW_conv2 element is a 256-term fp32 dot
    product (one 4-sample chunk; exact fp32 products on the matrix pipe and in the FMAs), so its
    error is at most gamma_n * sum |dz a1| with n = 256 terms + 2 combine adds + slack = 264,
    whatever the order; the rows of the other 48 channels are sums of exact zeros."""
    B = 4
    grads, inputs = num.run_case(num.make_case(B, co_only=cos, seed=1 + cos[0]))
    got = grads["conv2.weight"].double()
    ref = num.reference(*inputs)["conv2.weight"]
    mag = num.reference(*inputs, absolute=True)["conv2.weight"]
    bound = 264 * 2.0 ** -24 * mag
    other = [c for c in range(50) if c not in cos]
    assert torch.count_nonzero(got[other]) == 0
    cols = _seam_columns()
    for co in cos:  # the rows and columns under test carry signal
        assert int(torch.count_nonzero(ref[co, cols])) == len(cols), co
    bad = (got - ref).abs() > bound
    assert not bool(bad.any()), bad.nonzero()[:8].tolist()
    for co in cos:
        assert bool(((got[co, cols] - ref[co, cols]).abs() <= bound[co, cols]).all()), co


def _trainer(x, y, perm):
    from pytorch_operator_amd.models.mnist import FusedMnistTrainer
    from pytorch_operator_amd.ops import mnist as K
    dev = torch.device("cuda")
    cur = torch.zeros(1, dtype=torch.int32, device=dev)
    src = K.BatchSource(x.to(dev), y.to(dev), perm=perm.to(dev), cursor=cur)
    tr = FusedMnistTrainer(batch_size=64, source=src, seed=9)
    assert tr.conv_chunk == 4
    return tr


def _dataset(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1)).to(torch.int32)
    return x, y, perm


def test_three_steps_are_bit_reproducible(lib):
    x, y, perm = _dataset(256, 81)
    a, b = _trainer(x, y, perm), _trainer(x, y, perm)
    for tr in (a, b):
        for _ in range(3):
            tr.train_step()
    torch.cuda.synchronize()
    assert torch.equal(a.flat_params, b.flat_params)
    assert torch.equal(a.flat_momentum, b.flat_momentum)


def test_stream_launch_and_graph_replay_agree(lib):
    from pytorch_operator_amd.parallel.graphed_step import GraphedStep
    x, y, perm = _dataset(640, 82)
    a, b = _trainer(x, y, perm), _trainer(x, y, perm)
    ra = GraphedStep(a, mode="graph", steps_per_graph=1, launch="graph")
    rb = GraphedStep(b, mode="graph", steps_per_graph=1, launch="stream")
    for r in (ra, rb):
        r.warm(1)
        r.run(3)
    torch.cuda.synchronize()
    assert int(a.cursor.item()) == int(b.cursor.item())
    assert torch.equal(a.flat_params, b.flat_params)
    assert torch.equal(a.flat_momentum, b.flat_momentum)
