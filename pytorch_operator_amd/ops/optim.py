"""Mixed-precision AdamW with fp32 master weights (``csrc/kernels/adamw.hip``).

``to_bf16_matmul_weights(model)`` turns every ``nn.Linear`` weight into bf16 -- the
tensors the bf16 autocast matmuls read directly, so the per-step fp32->bf16 weight casts
and bf16->fp32 gradient casts disappear -- and ``MasterAdamW`` keeps an fp32 master copy
of those weights plus fp32 moments.  Other parameters (embedding, RMSNorm weights) stay
fp32 and are their own master.  One fused HIP pass per parameter (``adamw_launch``) updates
master, m, v and rewrites the bf16 weight.  Update rule = ``torch.optim.AdamW`` (decoupled
decay, bias-corrected moments), applied to the fp32 master.  ``state_dtype=torch.bfloat16`` stores the
moments in bf16 with stochastic rounding (``sr_key`` / ``sr_bits`` / ``sr_round_bf16`` are the rule).

On CPU the same update runs in PyTorch (``MasterAdamW._step_reference``: CPU tests, gloo
plumbing).  ``parallel/zero.py`` applies both to its bucket shards.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _native


_M32 = 0xFFFFFFFF


def _mix32(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def sr_key(seed: int, step: int) -> int:
    """The 32-bit key of one AdamW pass with bf16 moments: ``mix(seed + 0x9E3779B9 * step)`` in
    wrapping uint32 arithmetic, ``step`` the pass's step count (>= 1)."""
    return _mix32(int(seed) + 0x9E3779B9 * int(step))


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    # x * c mod 2^32 on int64 tensors holding uint32 values, without leaving the int64 range
    return ((x & 0xFFFF) * c + ((((x >> 16) * c) & 0xFFFF) << 16)) & _M32


def _mix32_t(x: torch.Tensor) -> torch.Tensor:
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def sr_bits(key: int, base: int, n: int, device=None) -> torch.Tensor:
    """The kernel's 32 random bits of elements ``base .. base + n`` (csrc/kernels/adamw.hip,
    ``sr_bits``) as an int64 tensor: ``mix(mix(lo32(c) ^ key) + hi32(c))``."""
    c = torch.arange(n, dtype=torch.int64, device=device)
    lo = (c + (int(base) & _M32))          # < 2^33: the carry into the high word is bit 32
    hi = ((int(base) >> 32) + (lo >> 32)) & _M32
    return _mix32_t((_mix32_t((lo & _M32) ^ int(key)) + hi) & _M32)


def sr_round_bf16(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """fp32 ``x`` -> bf16, rounded away from zero with probability (its low 16 bits) / 65536 given
    ``r`` uniform in [0, 65535]: ``(bits(x) + r) >> 16``; a NaN becomes a quiet NaN of its sign.  A
    bf16-representable value (+-0, +-inf) never changes."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & _M32
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    b = torch.where(nan, (u >> 16) | 0x40, (u + r) >> 16)
    b = torch.where(b >= 0x8000, b - 0x10000, b)
    return b.to(torch.int16).view(torch.bfloat16)


def to_bf16_matmul_weights(model: nn.Module) -> int:
    """Cast ``nn.Linear`` weights (and biases) of ``model`` to bf16 in place; returns #params cast."""
    n = 0
    for mod in model.modules():
        if isinstance(mod, nn.Linear):
            for p in mod.parameters(recurse=False):
                if p.dtype == torch.bfloat16:
                    continue
                master = p.data.float()
                p.data = p.data.to(torch.bfloat16)
                p._pto_master = master  # exact fp32 init for MasterAdamW (dropped once it takes over)
                n += p.numel()
    return n


class MasterAdamW(torch.optim.Optimizer):
    """``overlap=True`` (GPU): ``step()`` enqueues the updates on a side stream, in parameter
    order, and returns at once; each parameter gets a ready event, and ``install_overlap
    (model)`` makes every module wait (on the compute stream) for its own parameters' events
    just before its forward.  The next step's forward then starts while the updates of the
    later layers are still streaming -- the memory-bound optimizer (~11 % of a Llama-3 8B
    step) runs under the compute-bound forward GEMMs instead of after them.

    ``max_grad_norm`` (default ``None``: off, nothing below runs): clip the gradients by their
    global L2 norm, ``torch.nn.utils.clip_grad_norm_``'s rule (``error_if_nonfinite=False``), over
    exactly the tensors the step consumes.  On the GPU that is one streaming sum-of-squares pass
    per gradient, one finish launch, and the AdamW launches reading the result on the device
    (``csrc/kernels/gradclip.hip``); the host never sees the norm unless it asks
    (``last_grad_norm()``).

    ``grad_accum=N`` (default 1: off, nothing below exists): N backward passes per step.  Call
    ``accumulate()`` after each of the first N-1 and ``step()`` after the last.  Every ``.grad`` is
    folded into an fp32 accumulator of the parameter's shape (``ops/gradaccum.py``: a sequential fp32
    sum, the first term stored) and freed; the norm pass and AdamW then read the accumulators with
    1/N as their gradient scale.  The accumulators (4 B per parameter, kept from step to step) are
    no optimizer state: they are empty at every step boundary and stay out of ``state_dict()``.
    Under ``DistributedDataParallel`` the comm hook would reduce only the last micro-batch: data
    parallelism with ``grad_accum > 1`` is ``ZeroAdamW``'s.

    ``state_dtype=torch.bfloat16`` (default fp32: nothing below exists): ``exp_avg`` / ``exp_avg_sq``
    are stored in bf16, 4 B per parameter instead of 8, and the update pass moves 20 B per
    bf16-weight element instead of 28.  Each pass widens them, updates the fp32 master from the fp32
    moments, and rounds the moments stochastically (round-to-nearest would freeze ``v``: its decay of
    ``1 - b2`` per step is below half a bf16 ulp).  The random bits are a hash of (``state_seed``,
    the parameter's step count, the element's index among all parameters in ``param_groups`` order),
    so a run is reproducible and a resumed one continues bit for bit.  ``ZeroAdamW`` counts elements
    by bucket, so the two optimizers do not agree bit for bit at bf16 state (they do at fp32); nor
    do the CPU and GPU paths."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, overlap=False,
                 max_grad_norm=None, grad_accum=1, state_dtype=torch.float32, state_seed=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if int(grad_accum) != grad_accum or grad_accum < 1:
            raise ValueError("grad_accum: a positive integer")
        if state_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("state_dtype: float32 or bfloat16")
        self.state_dtype = state_dtype
        self.state_seed = int(state_seed)
        self._base = None  # bf16 state: parameter -> index of its first element among all parameters
        self.grad_accum = int(grad_accum)
        self._micro = 0   # accumulate() calls since the last step()
        self._acc = {}    # grad_accum > 1: parameter -> its fp32 accumulator
        self._live = set()  # parameters whose accumulator holds a gradient of the current step
        self.overlap = overlap
        self._side = None
        self._clip = None  # gradclip.GlobalGradNorm: norm pass + result of the last clipped step
        if max_grad_norm is not None:
            from .gradclip import GlobalGradNorm
            self._clip = GlobalGradNorm(max_grad_norm)
        self.max_grad_norm = self._clip and self._clip.max_norm

    def last_grad_norm(self):
        """Global gradient norm of the last ``step()`` before clipping, as a 0-dim tensor on the
        parameters' device (``None`` without ``max_grad_norm`` or before the first step).  Does not
        synchronise: with ``overlap=True`` the value is written on the side stream."""
        return None if self._clip is None else self._clip.last_grad_norm()

    def set_lr(self, lr: float) -> None:
        """The learning rate of the next ``step()`` (a schedule sets it per step: the fused launch
        takes it as a host scalar)."""
        for group in self.param_groups:
            group["lr"] = lr

    def _state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            if p.dtype != torch.float32:
                st["master"] = getattr(p, "_pto_master", None)
                if st["master"] is None:
                    st["master"] = p.detach().float().clone()
                else:
                    del p._pto_master
            else:
                st["master"] = None
            st["exp_avg"] = torch.zeros(p.shape, dtype=self.state_dtype, device=p.device)
            st["exp_avg_sq"] = torch.zeros(p.shape, dtype=self.state_dtype, device=p.device)
        return st

    def _rng(self, p, step):
        """bf16 moments: (key, base) of parameter ``p``'s pass at its step count ``step``.  The bases
        follow ``param_groups`` order and are not checkpointed: a resumed run continues bit for bit
        only if it builds the optimizer with the same parameters in the same order (a group added
        later appends, and leaves the earlier bases alone)."""
        if self.state_dtype == torch.float32:
            return None
        if self._base is None or p not in self._base:
            self._base, off = {}, 0
            for group in self.param_groups:
                for q in group["params"]:
                    self._base[q] = off
                    off += q.numel()
        return sr_key(self.state_seed, step), self._base[p]

    @torch.no_grad()
    def accumulate(self):
        """End of one of the first N-1 backward passes of a step (``grad_accum=N``): fold every
        ``.grad`` into its accumulator, on the current stream, and free it."""
        if self.grad_accum == 1:
            raise RuntimeError("MasterAdamW.accumulate(): constructed with grad_accum=1")
        if self._micro >= self.grad_accum - 1:
            raise RuntimeError(f"MasterAdamW.accumulate(): called {self._micro + 1} times with grad_accum="
                               f"{self.grad_accum}; the last backward pass is followed by step()")
        self._fold_all()
        self._micro += 1

    def _fold_all(self):
        from .gradaccum import fold
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.dtype not in (torch.float32, torch.bfloat16):
                    raise TypeError(f"MasterAdamW: fp32/bf16 parameters only, got {p.dtype}")
                acc = self._acc.get(p)
                if acc is None:
                    acc = self._acc[p] = torch.empty(p.shape, dtype=torch.float32, device=p.device)
                if not self._live and self._side is not None:
                    # the first fold of a step overwrites what the last step's AdamW launches read
                    torch.cuda.current_stream(p.device).wait_stream(self._side)
                fold(acc, p.grad, p not in self._live)
                self._live.add(p)
                p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.grad_accum > 1:
            if self._micro != self.grad_accum - 1:
                raise RuntimeError(f"MasterAdamW.step(): {self._micro} accumulate() calls since the last step, "
                                   f"grad_accum={self.grad_accum} needs {self.grad_accum - 1}")
            self._fold_all()  # the last micro-batch, on the compute stream (the side stream waits for it)
        side = None
        for group in self.param_groups:
            for p in group["params"]:
                if self.overlap and p.is_cuda and (p.grad is not None or p in self._live):
                    if self._side is None:
                        self._side = torch.cuda.Stream(device=p.device)
                    side = self._side
                    side.wait_stream(torch.cuda.current_stream(p.device))  # gradients complete
                break
            if side is not None:
                break
        if side is None:
            self._step_all(None)
        else:
            with torch.cuda.stream(side):
                self._step_all(side)
        self._live.clear()  # the accumulators are empty again (their memory is kept)
        self._micro = 0
        return loss

    def _step_all(self, side):
        """The gradients this step consumes, in parameter order; with ``max_grad_norm`` their global
        norm; then AdamW per parameter (on the GPU all on the current stream -- the side stream
        under overlap)."""
        clip = self._clip
        scale = 1.0 / self.grad_accum  # the kernels round it to fp32
        work = []
        for group in self.param_groups:
            for p in group["params"]:
                if p in self._live:
                    g = self._acc[p]
                    if side is not None:
                        g.record_stream(side)
                    work.append((group, p, g))
                    continue
                if p.grad is None or self.grad_accum > 1:
                    continue
                if p.dtype not in (torch.float32, torch.bfloat16):
                    raise TypeError(f"MasterAdamW: fp32/bf16 parameters only, got {p.dtype}")
                # the DDP fp32 comm hook's reduced gradient (harness/ddp_train.py), else .grad
                g = getattr(p, "_pto_grad32", None)
                if g is not None:
                    del p._pto_grad32
                else:
                    g = p.grad
                if p.is_cuda:
                    if side is not None:
                        g.record_stream(side)  # the next backward may reuse the memory otherwise
                    if clip is not None:
                        g = self._hip_grad(p, g)  # fixed up once, read by both passes
                work.append((group, p, g))
        if clip is not None and work:
            if len({p.is_cuda for _, p, _ in work}) > 1:
                raise ValueError("MasterAdamW(max_grad_norm): parameters on the GPU and on the CPU in one optimizer")
            clip.run([(g, scale) for _, _, g in work if g.numel()])
        for group, p, g in work:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            st = self._state(p)
            st["step"] += 1
            master = st["master"] if st["master"] is not None else p
            rng = self._rng(p, st["step"])
            if p.is_cuda:
                if clip is None:
                    g = self._hip_grad(p, g)  # a fix-up copy lives until this launch only
                adamw_launch(master, st["exp_avg"], st["exp_avg_sq"], g, p if master is not p else None, p.numel(),
                             st["step"], lr, b1, b2, eps, wd, scale,
                             None if clip is None else (clip.out, clip.max_norm), rng)
                if side is not None:
                    ev = torch.cuda.Event()
                    ev.record(side)
                    p._pto_ready = ev
            else:
                if self.grad_accum > 1:
                    g = g * scale
                self._step_reference(p, g if clip is None else g.float() * clip.coef, master, st, lr, b1, b2, eps, wd,
                                     rng)

    @staticmethod
    def _step_reference(p, g, master, st, lr, b1, b2, eps, wd, rng=None):
        """``rng=(key, base)``: the moments in ``st`` are bf16 -- widened, updated in fp32 (the master
        from the fp32 moments), and stored back rounded stochastically with the kernel's hash."""
        g = g.float()
        t = st["step"]
        bf16_state = st["exp_avg"].dtype == torch.bfloat16
        if bf16_state != (rng is not None):
            raise ValueError("AdamW: rng=(key, base) goes with bf16 moments, and only with them")
        m, v = (st["exp_avg"].float(), st["exp_avg_sq"].float()) if bf16_state else (st["exp_avg"], st["exp_avg_sq"])
        master.mul_(1 - lr * wd)
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (v.sqrt() / math.sqrt(1 - b2 ** t)).add_(eps)
        master.addcdiv_(m, denom, value=-lr / (1 - b1 ** t))
        if bf16_state:
            h = sr_bits(rng[0], rng[1], m.numel(), m.device).view(m.shape)
            st["exp_avg"].copy_(sr_round_bf16(m, h & 0xFFFF))
            st["exp_avg_sq"].copy_(sr_round_bf16(v, h >> 16))
        if master is not p:
            p.copy_(master)

    @staticmethod
    def _hip_grad(p, g):
        """The gradient as the kernels read it: contiguous and 16-byte aligned."""
        if not g.is_contiguous() or g.data_ptr() % 16:
            g = g.contiguous().clone()
        if g.dtype not in (torch.float32, torch.bfloat16) or not p.is_contiguous():
            raise TypeError("MasterAdamW: contiguous fp32/bf16 parameters and gradients only")
        return g


def adamw_launch(master, exp_avg, exp_avg_sq, grad, out, n, step, lr, b1, b2, eps, wd, grad_scale=1.0, clip=None,
                 rng=None):
    """One fused AdamW pass (``csrc/kernels/adamw.hip``) over ``n`` elements on the current stream:
    the package's only call of the ``pto_adamw_*`` entry points.  ``out``: the bf16 weight to
    refresh (``None``: ``master`` is the parameter).  ``grad_scale`` multiplies the gradient first.
    ``clip=(norm_out, max_norm)``: also clip by the global norm whose sum of squares is the device
    float ``norm_out[0]`` (``gradclip.GlobalGradNorm``).  ``rng=(key, base)``: required with bf16
    moments (the stochastic-rounding kernels: ``key = sr_key(seed, step)``, ``base`` the counter of
    element 0), rejected with fp32 ones."""
    if exp_avg.dtype != exp_avg_sq.dtype or exp_avg.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("adamw_launch: both moments fp32, or both bf16")
    bf16_state = exp_avg.dtype == torch.bfloat16
    if bf16_state != (rng is not None):
        raise ValueError("adamw_launch: rng=(key, base) goes with bf16 moments, and only with them")
    lib = _native.load()
    args = (master.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.data_ptr(),
            None if out is None else out.data_ptr(), n, 1 if grad.dtype == torch.bfloat16 else 0, lr, b1, b2, eps, wd,
            step, grad_scale)
    stream = ctypes.c_void_p(torch.cuda.current_stream(master.device).cuda_stream)
    if bf16_state:
        key, base = int(rng[0]) & _M32, int(rng[1])
        if clip is None:
            _native.check(lib.pto_adamw_bf16state_scaled(*args, key, base, stream), "adamw_bf16state")
        else:
            _native.check(lib.pto_adamw_bf16state_clipped(*args, clip[0].data_ptr(), clip[1], key, base, stream),
                          "adamw_bf16state_clipped")
    elif clip is None:
        _native.check(lib.pto_adamw_step_scaled(*args, stream), "adamw_step")
    else:
        _native.check(lib.pto_adamw_step_clipped(*args, clip[0].data_ptr(), clip[1], stream), "adamw_step_clipped")


def install_overlap(model: nn.Module) -> int:
    """Forward pre-hooks: each module with parameters of its own makes the current stream wait
    for those parameters' optimizer-update events (``MasterAdamW(overlap=True)``); returns the
    number of hooked modules."""
    def hook(mod, _inputs):
        for p in mod.parameters(recurse=False):
            ev = getattr(p, "_pto_ready", None)
            if ev is not None:
                torch.cuda.current_stream(p.device).wait_event(ev)
    n = 0
    for mod in model.modules():
        if any(True for _ in mod.parameters(recurse=False)):
            mod.register_forward_pre_hook(hook)
            n += 1
    return n
