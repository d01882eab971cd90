"""float64 reference of the MNIST step's SGD update, the bound the kernels are held to, and a
float64 emulation of the kernel's fp32 chain (with the wrong variants the bound must reject).

The kernels (``sgd_elem`` of csrc/kernels/mnist_kernels.hip, ``sgd4`` of xgmi_allreduce.hip)
compute, per element and in fp32,

    t  = fl(g * grad_scale)
    d  = fma(wd, p, t)
    m' = first ? d : fma(mom, m, fl(fl(1 - damp) * d))          (momentum != 0)
    e  = nesterov ? fma(mom, m', d) : m'                         (momentum == 0: e = d, m untouched)
    p' = fma(-lr, e, p)

``sgd_ref`` evaluates torch.optim.SGD's update of the same fp32 inputs in float64, with the
hyper-parameters as the fp32 values the kernel receives, and returns with each result the sum of
the absolute values of the terms of its expression:

    A_d = |wd p| + |gs g|
    A_m = |mom m| + |1 - damp| A_d                               (first: A_m = A_d)
    A_p = |p| + lr (nesterov ? |mom| A_m + A_d : A_m)            (momentum == 0: |p| + lr A_d)

The bound: ``|got - ref| <= K * 2^-24 * A`` per element (2^-24 = fp32's unit roundoff u under
round-to-nearest), never relative to a tensor's maximum.

K, from the roundings on the longest path (first order in u; every intermediate is bounded in
magnitude by its abs-sum, so a rounding of it costs at most u times that abs-sum):

    t, d      2 roundings                     |d  - d_ref|  <= 2 u A_d
    m'        + fl(1 - damp), the product's
              rounding, the fma's: 3          |m' - m_ref|  <= |1-damp| (2 + 2) u A_d + u A_m <= 5 u A_m
    e         Nesterov: the fma's, 1          |e  - e_ref|  <= |mom| 5 u A_m + 2 u A_d + u (|mom| A_m + A_d)
                                                            <= 6 u (|mom| A_m + A_d)
    p'        the fma's, 1                    |p' - p_ref|  <= lr 6 u (...) + u A_p <= 7 u A_p

Seven fp32 roundings lie on the path to p' with Nesterov momentum (six without, five to m'), so
K = 7 for every output; the terms of second order in u are below 1e-6 of the bound.  The
emulation below stays under 3 u A on random data (tests/test_mnist_sgd_cpu.py prints the figure).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

U = 2.0 ** -24   # fp32 unit roundoff
K = 7            # roundings on the longest path (module docstring)


def f32(x: float) -> float:
    """The fp32 value a kernel receives for the Python float ``x``, as a Python float."""
    return float(np.float32(x))


@dataclass(frozen=True)
class Hyper:
    lr: float
    momentum: float
    dampening: float
    weight_decay: float
    nesterov: bool
    grad_scale: float = 1.0

    def scaled(self, grad_scale: float) -> "Hyper":
        return replace(self, grad_scale=grad_scale)

    def kwargs(self) -> dict:
        """Keyword arguments of the ops' SGD launches (without ``first_step``)."""
        return dict(lr=self.lr, momentum=self.momentum, dampening=self.dampening,
                    weight_decay=self.weight_decay, nesterov=self.nesterov, grad_scale=self.grad_scale)

    def trainer_kwargs(self) -> dict:
        return dict(lr=self.lr, momentum=self.momentum, dampening=self.dampening,
                    weight_decay=self.weight_decay, nesterov=self.nesterov)

    @property
    def id(self) -> str:
        return (f"lr{self.lr}-mom{self.momentum}-damp{self.dampening}-wd{self.weight_decay}-"
                f"{'nesterov' if self.nesterov else 'plain'}-gs{self.grad_scale}")


# (lr, momentum, dampening, weight decay, nesterov)
CONFIGS = (
    Hyper(0.01, 0.5, 0.0, 0.0, False),     # what every other MNIST test runs
    Hyper(0.05, 0.9, 0.0, 5e-4, True),
    Hyper(0.05, 0.9, 0.1, 5e-4, False),    # dampening: the first step differs (first_step)
    Hyper(0.02, 0.0, 0.0, 1e-2, False),    # no momentum: the buffer must stay untouched
)
# ops level: the same with the gradient scales DDP (1 / world) and the xGMI fallback pass
OPS_CONFIGS = tuple(h.scaled(gs) for h in CONFIGS for gs in (1.0, 0.5, 0.125))


def to64(t) -> np.ndarray:
    """A torch tensor (any device) or array as a float64 numpy array."""
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def sgd_ref(p, m, g, hy: Hyper, first: bool):
    """torch.optim.SGD's update in float64 -> (p', m', A_p, A_m); see the module docstring.
    ``first``: this step initialises the momentum buffer (m' = d, no dampening)."""
    p, m, g = to64(p), to64(m), to64(g)
    lr, mom, damp, wd, gs = (f32(hy.lr), f32(hy.momentum), f32(hy.dampening), f32(hy.weight_decay),
                             f32(hy.grad_scale))
    d = wd * p + gs * g
    a_d = np.abs(wd * p) + np.abs(gs * g)
    if mom == 0.0:
        return p - lr * d, m.copy(), np.abs(p) + lr * a_d, np.abs(m)
    if first:
        m2, a_m = d, a_d
    else:
        m2 = mom * m + (1.0 - damp) * d
        a_m = np.abs(mom * m) + abs(1.0 - damp) * a_d
    if hy.nesterov:
        e, a_e = d + mom * m2, abs(mom) * a_m + a_d
    else:
        e, a_e = m2, a_m
    return p - lr * e, m2, np.abs(p) + lr * a_e, a_m


def ratio(got, ref, abs_sum) -> np.ndarray:
    """|got - ref| / (2^-24 * abs_sum) per element; where abs_sum is 0, 0 if equal, else inf."""
    err = np.abs(to64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / (U * abs_sum)
    return np.where(abs_sum == 0, np.where(err == 0, 0.0, np.inf), r)


def assert_within_bound(got, ref, abs_sum, what: str, k: float = K) -> float:
    r = ratio(got, ref, abs_sum)
    assert not np.isnan(r).any(), f"{what}: NaN"
    worst = float(r.max()) if r.size else 0.0
    if not worst <= k:
        i = int(r.argmax())
        raise AssertionError(f"{what}: element {i} is {worst:.3g} x 2^-24 x abs_sum from the float64 "
                             f"reference (bound {k}); {int((r > k).sum())} of {r.size} outside")
    return worst


def _r(x):
    """One fp32 rounding of a float64 value, returned as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


VARIANTS = ("scale_on_decay", "first_ignored", "no_dampening", "nesterov_old_buffer")


def kernel_emulation(p, m, g, hy: Hyper, first: bool, variant: Optional[str] = None):
    """The kernel's chain in float64 with one fp32 rounding per operation (the product inside an
    fma is exact in float64) -> (p', m').  ``variant``: one of the deliberately wrong VARIANTS."""
    assert variant is None or variant in VARIANTS
    p, m, g = to64(p), to64(m), to64(g)
    lr, mom, damp, wd, gs = (f32(hy.lr), f32(hy.momentum), f32(hy.dampening), f32(hy.weight_decay),
                             f32(hy.grad_scale))
    if variant == "scale_on_decay":
        d = _r(_r(wd * p + g) * gs)            # grad_scale on the weight-decay term too
    else:
        d = _r(wd * p + _r(g * gs))
    m2 = m.copy()
    if mom != 0.0:
        keep = 1.0 if variant == "no_dampening" else _r(1.0 - damp)
        if first and variant != "first_ignored":
            m2 = d
        else:
            m2 = _r(mom * m + _r(keep * d))
        buf = m if variant == "nesterov_old_buffer" else m2
        d = _r(mom * buf + d) if hy.nesterov else m2
    return _r(p - lr * d), m2
