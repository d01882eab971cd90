"""FP8 projection path on the GPU: the cast kernels of csrc/kernels/fp8_cast.hip bit for bit against
the PyTorch reference, ``fp8_linear`` (hipBLASLt FP8 GEMMs) against its CPU emulation, and the
model switch."""
import functools

import pytest
import torch

from pytorch_operator_amd.ops import fp8

pytestmark = pytest.mark.gpu

FORMATS = ["e4m3", "e5m2"]


def _u8(t):
    return t.view(torch.uint8).cpu()


def _same(got, want):
    (q, qT, inv), (rq, rqT, rinv) = got, want
    assert torch.equal(_u8(q), _u8(rq))
    assert torch.equal(_u8(qT), _u8(rqT))
    assert torch.equal(inv.cpu().view(torch.int32), rinv.cpu().view(torch.int32)), (float(inv), float(rinv))


@functools.lru_cache(maxsize=None)
def _all_finite_bf16():
    bits = torch.arange(65536, dtype=torch.int32)
    bits = torch.where((bits & 0x7f80) == 0x7f80, torch.zeros_like(bits), bits)
    return bits.to(torch.uint16).view(torch.bfloat16).reshape(256, 256)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fixed_scale_cast_bit_exact(fmt):
    """Every finite bf16 value at scale 1: rounding ties, subnormals, saturation at +-fmax."""
    x = _all_finite_bf16()
    got = fp8.quantize(x.cuda(), fmt, scale=1.0)
    assert got[0].dtype == got[1].dtype == fp8.FORMATS[fmt][2] and got[1].shape == (256, 256)
    _same(got, fp8.quantize_reference(x, fmt, scale=1.0))


def _variants(shape):
    """Random bf16, the same with its largest-magnitude element first / last, and zeros."""
    g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
    x = (torch.randn(*shape, generator=g) * 2.5).to(torch.bfloat16)
    flat = x.flatten()
    i = int(flat.float().abs().argmax())
    out = [x]
    for j in (0, flat.numel() - 1):
        y = flat.clone()
        y[j], y[i] = flat[i], flat[j]
        out.append(y.reshape(shape))
    return out + [torch.zeros(shape, dtype=torch.bfloat16)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [(64, 64), (192, 64), (64, 192), (1024, 3584)])
def test_amax_and_cast_bit_exact(shape, fmt):
    for x in _variants(shape):
        xg = x.cuda()
        want = fp8.quantize_reference(x, fmt)
        got = fp8.quantize(xg, fmt)
        _same(got, want)
        q, none, inv = fp8.quantize(xg, fmt, transposed=False)
        assert none is None and torch.equal(_u8(q), _u8(want[0])) and float(inv) == float(want[2])
        none, qT, inv = fp8.quantize(xg, fmt, normal=False)
        assert none is None and torch.equal(_u8(qT), _u8(want[1])) and float(inv) == float(want[2])


def test_wrapper_handles_unaligned_and_strided_input_and_rejects_bad_shapes():
    g = torch.Generator().manual_seed(3)
    base = torch.randn(64 * 128 + 1, generator=g).to(torch.bfloat16)
    x = base[1:].reshape(64, 128)  # 2 bytes off 16-byte alignment on the device
    xg = base.cuda()[1:].reshape(64, 128)
    assert xg.data_ptr() % 16
    _same(fp8.quantize(xg, "e4m3"), fp8.quantize_reference(x, "e4m3"))
    wide = torch.randn(128, 256, generator=g).to(torch.bfloat16)
    _same(fp8.quantize(wide.cuda()[:, ::2], "e5m2"), fp8.quantize_reference(wide[:, ::2], "e5m2"))
    _same(fp8.quantize(wide.cuda().t(), "e4m3"), fp8.quantize_reference(wide.t(), "e4m3"))
    with pytest.raises(ValueError, match="96"):
        fp8.quantize(torch.zeros(96, 64, device="cuda", dtype=torch.bfloat16), "e4m3")
    with pytest.raises(ValueError):
        fp8.quantize(torch.zeros(64, 64, device="cuda"), "e4m3")


def test_launchers_validate():
    import ctypes
    from pytorch_operator_amd.ops import _native
    lib = _native.load()
    x = torch.zeros(128, 64, device="cuda", dtype=torch.bfloat16)
    q = torch.empty(128, 64, device="cuda", dtype=torch.uint8)
    ws = torch.zeros(8, device="cuda")
    s = ctypes.c_void_p(_native.current_stream_ptr(x.device))
    assert lib.pto_fp8_amax_parts(128 * 64) == 4 and lib.pto_fp8_amax_parts(1 << 30) == 1024
    assert lib.pto_fp8_amax(x.data_ptr(), 96, 64, ws.data_ptr(), 8, s) != 0
    assert lib.pto_fp8_amax(x.data_ptr(), 128, 64, ws.data_ptr(), 3, s) != 0      # workspace too small
    assert lib.pto_fp8_amax(x.data_ptr() + 2, 64, 64, ws.data_ptr(), 8, s) != 0   # unaligned
    assert lib.pto_fp8_cast(x.data_ptr(), 128, 96, 0, ws.data_ptr(), 4, None, q.data_ptr(), None, ws.data_ptr(), s) != 0
    assert lib.pto_fp8_cast(x.data_ptr(), 128, 64, 2, ws.data_ptr(), 4, None, q.data_ptr(), None, ws.data_ptr(), s) != 0
    assert lib.pto_fp8_cast(x.data_ptr(), 128, 64, 0, None, 0, None, q.data_ptr(), None, ws.data_ptr(), s) != 0
    assert lib.pto_fp8_cast(x.data_ptr(), 128, 64, 0, ws.data_ptr(), 4, None, None, None, ws.data_ptr(), s) != 0
    assert lib.pto_fp8_cast(x.data_ptr(), 128, 64, 0, ws.data_ptr(), 4, None, q.data_ptr() + 4, None, ws.data_ptr(), s) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", FORMATS)
def test_nonfinite_inputs_come_out_as_nan(fmt):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 128, generator=g).to(torch.bfloat16)
    x[3, 70], x[40, 5] = float("nan"), float("inf")
    q, qT, inv = fp8.quantize(x.cuda(), fmt)
    nan = torch.isnan(q.float().cpu())
    assert nan.sum() == 2 and nan[3, 70] and nan[40, 5]
    assert torch.equal(torch.isnan(qT.float().cpu()), nan.t())
    _same((q, qT, inv), fp8.quantize_reference(x, fmt))


def test_deterministic():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1024, 3584, generator=g).to(torch.bfloat16).cuda()
    a, b = fp8.quantize(x, "e4m3"), fp8.quantize(x, "e4m3")
    _same(a, b)


class _Sink:
    def __init__(self, like):
        self.view = torch.zeros_like(like)
        self.dtype, self.shape, self.calls = like.dtype, tuple(like.shape), 0

    def ready(self):
        self.calls += 1


@pytest.mark.parametrize("grad_format", FORMATS)
@pytest.mark.parametrize("dims", [(2, 64, 128, 192), (1, 128, 256, 64)])
def test_fp8_linear_matches_cpu_reference(dims, grad_format):
    """Same FP8 operands (bit-identical by the tests above) on both sides: only the accumulation order
    and the bf16 output rounding differ, so the bf16 tolerances of test_linear_tn_matches_reference."""
    B, S, fin, fout = dims
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(B, S, fin, generator=g).to(torch.bfloat16)
    w = (torch.randn(fout, fin, generator=g) * 0.05).to(torch.bfloat16)
    dy = torch.randn(B, S, fout, generator=g).to(torch.bfloat16)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = fp8.fp8_linear_reference(xr, wr, grad_format)
    yr.backward(dy)
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = fp8.fp8_linear(xg, wg, grad_format)
    y.backward(dy.cuda())
    assert y.dtype == xg.grad.dtype == wg.grad.dtype == torch.bfloat16 and y.shape == (B, S, fout)
    torch.testing.assert_close(y.float().cpu(), yr.detach().float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(xg.grad.float().cpu(), xr.grad.float(), rtol=2e-2, atol=5e-2)
    torch.testing.assert_close(wg.grad.float().cpu(), wr.grad.float(), rtol=2e-2, atol=1e-1)
    # the ZeRO gradient sink: dW lands in the sink's view, ready() once, no .grad
    ws = w.cuda().requires_grad_(True)
    ws._pto_grad_sink = sink = _Sink(ws.detach())
    xs = x.cuda().requires_grad_(True)
    fp8.fp8_linear(xs, ws, grad_format).backward(dy.cuda())
    assert sink.calls == 1 and ws.grad is None
    assert torch.equal(sink.view, wg.grad) and torch.equal(xs.grad, xg.grad)
    # the other way to the transposed weight gives the same bytes
    old, fp8.KEEP_W8T = fp8.KEEP_W8T, not fp8.KEEP_W8T
    try:
        xo, wo = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
        fp8.fp8_linear(xo, wo, grad_format).backward(dy.cuda())
    finally:
        fp8.KEEP_W8T = old
    assert torch.equal(xo.grad, xg.grad) and torch.equal(wo.grad, wg.grad)


def test_fp8_linear_autocast_and_bad_shapes():
    x = torch.randn(2, 64, 128, device="cuda")
    w = torch.randn(192, 128, device="cuda") * 0.05
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fp8.fp8_linear(x, w)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, fp8.fp8_linear(x.bfloat16(), w.bfloat16()))
    with pytest.raises(ValueError):
        fp8.fp8_linear(x, w)  # fp32 without autocast
    with pytest.raises(ValueError, match=r"\(3, 5, 24\)"):
        fp8.fp8_linear(torch.zeros(3, 5, 24, device="cuda", dtype=torch.bfloat16),
                       torch.zeros(40, 24, device="cuda", dtype=torch.bfloat16))


def _mini_losses(device):
    """llama-mini, B=2, S=128, one forward and backward: (tn loss, fp8 loss, fp8 model)."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama, TNLinear
    tok = torch.randint(0, 512, (2, 129), generator=torch.Generator().manual_seed(21)).to(device)
    out = []
    old = TNLinear.impl
    try:
        for impl in ("tn", "fp8"):
            torch.manual_seed(13)
            model = Llama(CONFIGS["llama-mini"]).to(device)  # initialised on the CPU: the same weights everywhere
            TNLinear.impl = impl
            with torch.autocast(device_type=device, dtype=torch.bfloat16):
                loss = model(tok[:, :-1], tok[:, 1:])
            loss.backward()
            out.append(float(loss.detach()))
    finally:
        TNLinear.impl = old
    return out[0], out[1], model


def test_model_fp8_against_tn():
    """|loss_fp8 - loss_tn| / loss_tn on the GPU is at most 1.5 x what the CPU emulation shows for
    the same comparison from the same seed (profiles/fp8/README.md records both)."""
    tn, f8, model = _mini_losses("cuda")
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    ctn, cf8, _ = _mini_losses("cpu")
    gpu_rel, cpu_rel = abs(f8 - tn) / tn, abs(cf8 - ctn) / ctn
    print(f"llama-mini loss tn {tn:.6f} fp8 {f8:.6f} rel {gpu_rel:.3e}; cpu tn {ctn:.6f} fp8 {cf8:.6f} rel {cpu_rel:.3e}")
    assert f8 == f8 and abs(f8) != float("inf")
    assert gpu_rel <= 1.5 * cpu_rel, (gpu_rel, cpu_rel)
