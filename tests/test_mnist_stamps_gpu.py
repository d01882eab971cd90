"""The debug-stamp path of the five-launch MNIST step (tools/phase_profile.py, tools/step_timeline.py).

With a debug buffer installed every block's thread 0 records wall_clock64() at phase boundaries
into dbg[slot][block][phase]; stamp 0 is the time read at kernel entry, stored once the kernel's
first loads are issued (round 7).  The stamps must not change what the step computes, every
launched block must have its stamp 0, and no block's stamp 0 may be later than its last stamp.
B = 37 is a multiple of neither 16 nor 4: clamped rows and a partial 4-sample chunk.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOT_U64 = 1024 * 16  # mnist_kernels.hip kDbgSlotU64
STEPS = 2


def _trainer(B, dev):
    from pytorch_operator_amd.data.synthetic import make_synthetic_mnist
    from pytorch_operator_amd.models.mnist import FusedMnistTrainer
    from pytorch_operator_amd.ops import mnist as K
    ds = make_synthetic_mnist(512, seed=5, device=dev)
    cur = torch.zeros(1, dtype=torch.int32, device=dev)
    src = K.BatchSource(ds.images, ds.labels, perm=ds.perm, cursor=cur)
    return FusedMnistTrainer(batch_size=B, source=src, lr=0.01, momentum=0.5, device=dev, seed=1)


def _run(B, dev, dbg):
    from pytorch_operator_amd.ops import mnist as K
    tr = _trainer(B, dev)
    K.set_debug_buffer(dbg)
    try:
        for _ in range(STEPS):
            tr.train_step()
        torch.cuda.synchronize()
    finally:
        K.set_debug_buffer(None)
    return tr


@pytest.mark.parametrize("B", [64, 37])
def test_stamps_do_not_change_the_step_and_cover_every_block(B):
    dev = torch.device("cuda", 0)
    dbg = torch.zeros(16 * SLOT_U64, dtype=torch.int64, device=dev)
    stamped = _run(B, dev, dbg)
    plain = _run(B, dev, None)
    assert torch.equal(stamped.flat_params, plain.flat_params)
    assert torch.equal(stamped.flat_momentum, plain.flat_momentum)

    # launched blocks of conv12_fwd, fc1_fwd<2>, fc1_bwd_head (tiles + staging), conv_bwd4, the tail
    # (fc1.weight tiles, fc2 tiles, 32-float4-column reduction blocks over the conv parameters)
    mt, ch = (B + 15) // 16, (B + 3) // 4
    conv_f4 = plain.layout.conv_end // 4
    expect = [4 * B, 32 * mt * 2, mt * 50 + ch, 4 * 4 * ch, 400 + 8 + (conv_f4 + 31) // 32]
    d = dbg.view(16, 1024, 16).cpu()
    used_slots = [k for k in range(16) if bool((d[k] != 0).any())]
    assert used_slots == list(range(5 * STEPS)), used_slots  # the five-launch step, twice
    for k in used_slots:
        wall = d[k, :, :8]
        touched = (d[k] != 0).any(1)
        n = expect[k % 5]
        print(f"B={B} slot {k}: {int(touched.sum())} blocks stamped, expected {n}")
        assert bool(touched[:n].all()) and not bool(touched[n:].any()), (k, int(touched.sum()), n)
        t0 = wall[:n, 0]
        assert bool((t0 > 0).all()), (k, int((t0 == 0).sum()))
        later = wall[:n, 1:]
        assert bool((later > 0).any(1).all()), k  # every block stamps at least one later phase
        assert bool((t0 <= later.max(1).values).all()), k
