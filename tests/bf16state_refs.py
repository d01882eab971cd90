"""Checker for the AdamW pass with bf16 moments and stochastic rounding (csrc/kernels/adamw.hip,
``pto_adamw_bf16state_*``; ``MasterAdamW._step_reference`` on the CPU).  It holds its own numpy copy
of the rule and imports nothing from the package:

  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32, wrapping)
  key  = mix(seed + 0x9E3779B9 * step)
  h(c) = mix(mix(lo32(c) ^ key) + hi32(c)),  c = base + i (uint64), i the element's index in the launch
  r_m  = h & 0xffff,  r_v = h >> 16
  sr(x, r) = NaN -> quiet NaN of the same sign;  otherwise (bits(x) + r) >> 16

``check_step`` recomputes one step in fp64 from the widened old moments and asserts that every stored
moment is a bf16 neighbour of the fp64 value and, outside a window around the rounding threshold
that fp32 arithmetic cannot resolve (1e-5 * |x| / ulp + 2^-16: the rtol of
tests/test_adamw_reference_cpu.py in bf16 ulps), the neighbour the rule picks.  For ``m`` alone the
window is never below a tenth of that rtol of its two terms' magnitudes: where ``b1 m`` and
``(1 - b1) g`` cancel, fp32 and fp64 differ by far more than a bf16 ulp of the tiny result.
"""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """On uint64 arrays holding uint32 values (the products stay below 2^64)."""
    x = np.array(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def sr_key(seed: int, step: int) -> int:
    return int(mix((int(seed) + 0x9E3779B9 * int(step)) & 0xFFFFFFFF))


def sr_hash(key: int, base: int, n: int) -> np.ndarray:
    """h(base + i) for i in [0, n) as uint64 values below 2^32."""
    c = np.uint64(base) + np.arange(n, dtype=np.uint64)
    return mix((mix((c & M32) ^ np.uint64(key)) + (c >> np.uint64(32))) & M32)


def sr(x: np.ndarray, r: np.ndarray) -> np.ndarray:
    """fp32 array -> bf16 bits (uint16) by the rule."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    out = np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), (u + np.asarray(r, dtype=np.uint64)) >> np.uint64(16))
    return out.astype(np.uint16)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    """The bits of a bf16 tensor (any device) as a flat uint16 array."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1).view(np.uint16)


def bits_to_f64(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().numpy().reshape(-1)


def _neighbours(a: np.ndarray):
    """For magnitudes a >= 0 (fp64): the bf16 value at or below, the bf16 ulp there, and a's
    position between that value and the next one, in [0, 1)."""
    _, e = np.frexp(np.where(a > 0, a, 1.0))  # a = f * 2^e, f in [0.5, 1)
    e = np.maximum(e - 1, -126)               # exponent of the binade; denormals share the lowest
    ulp = np.ldexp(1.0, e - 7)                # 8 significant bits
    k = np.floor(a / ulp)                     # exact: ulp is a power of two
    return k * ulp, ulp, a / ulp - k


BF16_MAX = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])


def sr64(y, r):
    """The rule applied to an fp64 value: the bf16 neighbour below |y|, or the one above iff y's
    position between them is >= (65536 - r) / 65536; the sign is kept."""
    a = np.abs(y)
    lo, ulp, frac = _neighbours(a)
    out = lo + np.where(frac + np.asarray(r, dtype=np.float64) / 65536.0 >= 1.0, ulp, 0.0)
    out = np.where(out > BF16_MAX, np.inf, out)
    return np.copysign(out, y)


def check_rounding(name, x64, stored_bits, r, tol=None, cap=0.01):
    """x64: the fp64 value of each element before rounding; stored_bits: what the code under test
    stored; r: the element's 16 random bits; tol: how far the code's fp32 value may lie from x64
    (default 1e-5 * |x64|, the project's fp32-vs-fp64 AdamW rtol).

    The rule is monotone in the value, so what a correct fp32 computation may store is the range
    sr64(x64 - w) .. sr64(x64 + w), w = tol + 2^-16 ulp.  Where the two ends agree -- x64's position
    between its bf16 neighbours is further than w / ulp from the threshold (65536 - r) / 65536 --
    the stored value must be exactly the neighbour the rule picks from x64; elsewhere it may be
    either end.  The share of such undecided elements is capped (1 % for n >= 4096) and returned."""
    x64 = np.asarray(x64, dtype=np.float64)
    assert np.isfinite(x64).all(), name
    s = bits_to_f64(stored_bits)
    _, ulp, _ = _neighbours(np.abs(x64))
    w = (1e-5 * np.abs(x64) if tol is None else tol) + 2.0 ** -16 * ulp
    lo, hi = sr64(x64 - w, r), sr64(x64 + w, r)
    bad = ~((lo <= s) & (s <= hi))
    assert not bad.any(), (name, "not what the rule picks", np.flatnonzero(bad)[:4], x64[bad][:4], s[bad][:4],
                           lo[bad][:4], hi[bad][:4])
    share = float((lo != hi).mean())
    if x64.size >= 4096:
        assert share <= cap, (name, "share of elements the fp64 value does not decide", share)
    return share


def adamw_fp64(p, m, v, g, *, lr, b1, b2, eps, wd, step, gscale=1.0):
    """One AdamW step in fp64 numpy (torch.optim.AdamW's rule); gscale multiplies the gradient."""
    g = g.astype(np.float64) * gscale
    p = p.astype(np.float64) * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** step) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)
    return p, m, v


def check_step(name, old, grad, new, hp, step, key, base, gscale=1.0):
    """old = (master fp32, m bf16, v bf16) before the step, new = (master, m, v, bf16 weight or None)
    after it (torch tensors, any device); grad: the gradient the step consumed (fp32 or bf16
    tensor); hp: lr, b1, b2, eps, wd; gscale: grad_scale times the clip coefficient."""
    p0, m0, v0 = f32(old[0]), bits_to_f64(bf16_bits(old[1])), bits_to_f64(bf16_bits(old[2]))
    n = p0.size
    p64, m64, v64 = adamw_fp64(p0, m0, v0, f32(grad), step=step, gscale=gscale, **hp)
    h = sr_hash(key, base, n)
    # m = b1 m + (1 - b1) g can cancel: where |m| is far below its two terms, what fp32 arithmetic
    # resolves is set by the terms, not by the result.  The budget, relative to the gradient term:
    # the fp32 constant 1 - 0.9f against 0.1 (2.4e-7), the clip coefficient's sqrt, add and divide
    # (1.8e-7), and the roundings of g * gscale, (1 - b1) * g and the fma (6e-8 each): 6e-7; the
    # other term has b1's rounding and the fma's (9e-8).  1e-6 of both is that, rounded up.
    terms = np.abs(hp["b1"] * m0) + np.abs((1 - hp["b1"]) * f32(grad).astype(np.float64) * gscale)
    check_rounding(name + ".m", m64, bf16_bits(new[1]), h & np.uint64(0xFFFF),
                   tol=np.maximum(1e-5 * np.abs(m64), 1e-6 * terms))
    check_rounding(name + ".v", v64, bf16_bits(new[2]), h >> np.uint64(16))
    p1 = new[0].detach().cpu().float().reshape(-1)
    torch.testing.assert_close(p1.double(), torch.from_numpy(p64), rtol=1e-5, atol=1e-6)
    if new[3] is not None:
        wb = new[3].detach().cpu().reshape(-1)
        assert wb.dtype == torch.bfloat16
        assert torch.equal(wb.view(torch.int16), p1.bfloat16().view(torch.int16)), name + ".weight"
