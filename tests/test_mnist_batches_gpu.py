"""Which rows a step reads: batches that wrap from the end of the permutation to its start
(gathered through batch_row, staged one step ahead through batch_row_at), host-side cursor moves,
the host-side rejection of batches the row functions cannot wrap, and the float32 source.

With n = 200 and B = 64 the batches of steps 3, 6, 9, ... straddle the end of the permutation
(3 * 64 = 192 < 200 < 256), as the last step of every MNIST epoch does (60000 = 937 * 64 + 32).
"""
import numpy as np
import pytest
import torch

import mnist_fwd_refs as FR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N, B = 200, 64


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    return x, y, perm


def _rows(perm, step, n, b=B):
    return perm[(step * b + torch.arange(b)) % n].long()


def _straddles(step, n=N, b=B):
    return (step * b) % n + b > n


@pytest.fixture(scope="module")
def data():
    return _data(N, seed=61)


@pytest.fixture(scope="module")
def weights():
    from pytorch_operator_amd.models.mnist import reference_init
    return {k: v.to(DEV).contiguous() for k, v in reference_init(2).items()}


def _trainer(data, stage_batches, seed=9):
    from pytorch_operator_amd.models.mnist import FusedMnistTrainer
    from pytorch_operator_amd.ops import mnist as K
    x, y, perm = data
    cur = torch.zeros(1, dtype=torch.int32, device=DEV)
    src = K.BatchSource(x.to(DEV), y.to(DEV), perm=perm.to(DEV), cursor=cur)
    tr = FusedMnistTrainer(batch_size=B, source=src, seed=seed, lr=0.05, momentum=0.5)
    tr.stage_batches = stage_batches
    return tr


def _xn_of_rows(x, rows, weights):
    """The normalised batch of rows ``rows`` through a perm-less source that holds them
    contiguously: the same arithmetic, another gather."""
    from pytorch_operator_amd.ops import mnist as K
    src = K.BatchSource(x[rows].contiguous().to(DEV))
    return K.conv1_fwd(src, weights["conv1.weight"], weights["conv1.bias"], len(rows))[2]


def _check_batch(tr, data, step, weights, what):
    x, y, perm = data
    rows = _rows(perm, step, N)
    assert torch.equal(tr.lab.cpu(), y[rows]), f"{what}: labels of step {step}"
    assert torch.equal(tr.xn, _xn_of_rows(x, rows, weights)), f"{what}: pixels of step {step}"


def test_wrapping_batches_read_the_permutations_rows(data, weights):
    """8 steps from cursor 0 (steps 3 and 6 straddle), staged and gathered: after each step the
    labels and the normalised pixels are those of perm[(t * B + b) % n]; both trainers end on
    the same bits; the staged slot is tagged with the next step."""
    assert [t for t in range(8) if _straddles(t)] == [3, 6]
    staged, gathered = _trainer(data, True), _trainer(data, False)
    assert staged.stage is not None
    for t in range(8):
        for tr, what in ((staged, "staged"), (gathered, "gathered")):
            tr.train_step()
            torch.cuda.synchronize()
            assert int(tr.cursor.item()) == t + 1
            _check_batch(tr, data, t, weights, what)
    assert int(staged.stage.tag.item()) == int(staged.cursor.item()) == 8
    assert torch.equal(staged.flat_params, gathered.flat_params)
    assert torch.equal(staged.flat_momentum, gathered.flat_momentum)


def test_launch_forms_agree_across_the_wrap(data):
    """10 staged steps (3, 6 and 9 straddle) eagerly, as a replayed hipGraph and as the captured
    kernel list launched on the stream: bit-identical parameters, momentum and last batch."""
    from pytorch_operator_amd.parallel.graphed_step import GraphedStep
    x, y, perm = data
    eager, graph, stream = (_trainer(data, True) for _ in range(3))
    for _ in range(10):
        eager.train_step()
    rg = GraphedStep(graph, mode="graph", steps_per_graph=1, launch="graph")
    rs = GraphedStep(stream, mode="graph", steps_per_graph=1, launch="stream")
    assert rg.launch == "graph" and rs.launch == "stream"
    assert rg.internal_steps == rs.internal_steps == 0
    rg.run(10)
    rs.run(10)
    torch.cuda.synchronize()
    for tr in (graph, stream):
        assert int(tr.cursor.item()) == 10
        assert torch.equal(tr.flat_params, eager.flat_params)
        assert torch.equal(tr.flat_momentum, eager.flat_momentum)
        assert torch.equal(tr.lab, eager.lab)
    assert torch.equal(eager.lab.cpu(), y[_rows(perm, 9, N)])


def test_host_side_cursor_moves_on_straddling_steps(data, weights):
    """advance_cursor=False on a straddling step (the staging then re-stages the same batch) and a
    cursor set from the host onto a straddling step (the staged batch's tag no longer matches):
    the right rows each time, and the staged trainer stays bit-identical to the gathered one."""
    staged, gathered = _trainer(data, True), _trainer(data, False)
    assert _straddles(3) and _straddles(9)
    for tr, what in ((staged, "staged"), (gathered, "gathered")):
        for _ in range(3):
            tr.train_step()
        tr.train_step(advance_cursor=False)        # step 3, the cursor stays
        torch.cuda.synchronize()
        assert int(tr.cursor.item()) == 3
        _check_batch(tr, data, 3, weights, what)
        tr.train_step()                            # step 3 again
        torch.cuda.synchronize()
        _check_batch(tr, data, 3, weights, what)
        tr.cursor.fill_(9)                         # host move onto a straddling step
        tr.train_step()
        torch.cuda.synchronize()
        _check_batch(tr, data, 9, weights, what)
        tr.train_step()
        torch.cuda.synchronize()
        _check_batch(tr, data, 10, weights, what)
    assert int(staged.stage.tag.item()) == int(staged.cursor.item()) == 11
    assert torch.equal(staged.flat_params, gathered.flat_params)
    assert torch.equal(staged.flat_momentum, gathered.flat_momentum)


def test_conv12_host_offset_at_the_last_slot(data, weights):
    """host_offset = n - 1: every sample but the first wraps."""
    from pytorch_operator_amd.ops import mnist as K
    x, y, perm = data
    b, w = 13, weights
    src = K.BatchSource(x.to(DEV), y.to(DEV), perm=perm.to(DEV), host_offset=N - 1)
    a1, idx1, xn, lab = K.conv1_fwd(src, w["conv1.weight"], w["conv1.bias"], b)
    a2, idx2 = K.conv2_fwd(a1, w["conv2.weight"], w["conv2.bias"])
    f = K.conv12_fwd(src, w["conv1.weight"], w["conv1.bias"], w["conv2.weight"], w["conv2.bias"], b)
    torch.cuda.synchronize()
    rows = perm[(N - 1 + torch.arange(b)) % N].long()
    assert torch.equal(f[3].cpu(), y[rows]) and torch.equal(lab.cpu(), y[rows])
    assert torch.equal(f[2], _xn_of_rows(x, rows, weights)) and torch.equal(xn, f[2])
    assert torch.equal(f[0], a1) and torch.equal(f[1], idx1)
    assert torch.equal(f[4], a2) and torch.equal(f[5], idx2)


# ------------------------------------------------------------------ what the row functions cannot wrap
def _small_source(n=10, **kw):
    from pytorch_operator_amd.ops import mnist as K
    x, y, perm = _data(n, seed=5)
    return K.BatchSource(x.to(DEV), y.to(DEV), perm=perm.to(DEV), **kw)


def _forward_calls(src, b, w):
    from pytorch_operator_amd.ops import mnist as K
    return (lambda: K.conv1_fwd(src, w["conv1.weight"], w["conv1.bias"], b),
            lambda: K.conv12_fwd(src, w["conv1.weight"], w["conv1.bias"], w["conv2.weight"], w["conv2.bias"], b))


def _staging_calls(src, b, w):
    """fc1_bwd(stage=) and fc1_bwd_head(stage=) at batch ``b`` on uninitialised buffers (the calls
    under test must fail before anything is launched)."""
    from pytorch_operator_amd.ops import mnist as K
    e = lambda *s, dt=torch.float32: torch.empty(s, device=DEV, dtype=dt)  # noqa: E731
    stage = K.BatchStage(b, DEV)
    gw1, gb1, gw2, gb2 = e(500, 800), e(500), e(10, 500), e(10)
    dh, a2, idx2, dlog, h, ps = e(b, 500), e(b, 800), e(b, 800, dt=torch.uint8), e(b, 10), e(b, 500), e(b, 2)
    lab = torch.zeros(b, device=DEV, dtype=torch.int32)
    return (lambda: K.fc1_bwd(dh, a2, idx2, w["fc1.weight"], dlog, h, gw1, gb1, gw2, gb2, dpool=e(b, 800),
                              per_sample=ps, stats=e(16), src=src, stage=stage),
            lambda: K.fc1_bwd_head(e(2, b, 500), w["fc2.weight"], w["fc2.bias"], lab, a2, idx2, w["fc1.weight"],
                                   dz2=None, dpool=e(b, 800), h_out=h, dh_out=dh, dlog_out=dlog, per_sample=ps,
                                   grad_scale=1.0 / b, src=src, stage=stage))


def test_unwrappable_batches_raise_on_the_host(weights):
    """B > n_total with a permutation, and a host_offset outside [0, n_total): batch_row and
    batch_row_at subtract n_total at most once, so these would index perm[] and the pixels out
    of bounds.  ValueError from BatchSource.check_batch, before any launch."""
    cur = torch.zeros(1, dtype=torch.int32, device=DEV)
    for call in _forward_calls(_small_source(10), 13, weights):
        with pytest.raises(ValueError, match="larger than dataset"):
            call()
    for call in _forward_calls(_small_source(10, cursor=cur), 11, weights):
        with pytest.raises(ValueError, match="larger than dataset"):
            call()
    for off in (10, 11, -1):
        for call in _forward_calls(_small_source(10, host_offset=off), 4, weights):
            with pytest.raises(ValueError, match="host_offset"):
                call()
    for call in _staging_calls(_small_source(10, cursor=cur), 13, weights):
        with pytest.raises(ValueError, match="larger than dataset"):
            call()
    with pytest.raises(ValueError, match="larger than dataset"):
        _small_source(10).check_batch(11)
    _small_source(10, host_offset=9).check_batch(10)  # the largest batch and offset that wrap once


def test_c_entry_points_reject_unwrappable_batches(weights, monkeypatch):
    """The C entry points that take n_total return -1 for the same cases (here with the Python
    check switched off): a host-side shape error, nothing launched."""
    from pytorch_operator_amd.ops import _native
    from pytorch_operator_amd.ops import mnist as K
    monkeypatch.setattr(K.BatchSource, "check_batch", lambda self, b: None)
    cur = torch.zeros(1, dtype=torch.int32, device=DEV)
    calls = (_forward_calls(_small_source(10), 13, weights) +
             _forward_calls(_small_source(10, host_offset=10), 4, weights) +
             _forward_calls(_small_source(10, host_offset=-1), 4, weights) +
             _staging_calls(_small_source(10, cursor=cur), 13, weights))
    assert len(calls) == 8
    for call in calls:
        with pytest.raises(_native.NativeLibraryError, match="code -1"):
            call()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the float32 source
@pytest.mark.parametrize("normalize", [True, False])
def test_float32_source(weights, normalize):
    """x fp32 in [0, 1] (is_u8 = 0), B = 3: xn within 2 ulp of x * scale + shift in float64,
    a1 / a2 and the pool argmax against the float64 forward, fused and separate kernels
    bit-identical."""
    from pytorch_operator_amd.ops import mnist as K
    b, w = 3, weights
    x = torch.rand(b, 784, generator=torch.Generator().manual_seed(8))
    src = K.BatchSource(x.to(DEV), normalize=normalize)
    assert not src.is_u8
    assert (src.scale, src.shift) == ((1.0 / K.MNIST_STD, -K.MNIST_MEAN / K.MNIST_STD) if normalize else (1.0, 0.0))
    a1, idx1, xn, lab = K.conv1_fwd(src, w["conv1.weight"], w["conv1.bias"], b)
    a2, idx2 = K.conv2_fwd(a1, w["conv2.weight"], w["conv2.bias"])
    f = K.conv12_fwd(src, w["conv1.weight"], w["conv1.bias"], w["conv2.weight"], w["conv2.bias"], b)
    torch.cuda.synchronize()
    assert lab is None and f[3] is None
    assert torch.equal(f[0], a1) and torch.equal(f[1], idx1) and torch.equal(f[2], xn)
    assert torch.equal(f[4], a2) and torch.equal(f[5], idx2)
    ref = FR.normalize_ref(x, src.scale, src.shift)
    ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
    err = np.abs(xn.cpu().double().numpy() - ref.numpy())
    print(f"\nxn: worst {float((err / ulp).max()):.3f} ulp")
    assert np.all(err <= 2 * ulp)
    if not normalize:
        assert torch.equal(xn.cpu(), x)
    p1, p2 = FR.forward_ref(ref, w)
    r1 = FR.check_stage(a1, idx1, p1, "a1")
    r2 = FR.check_stage(a2, idx2, p2, "a2")
    print(f"a1 {r1:.3f}, a2 {r2:.3f} x 2^-24 x sum|terms| (bound {FR.FWD_K})")
