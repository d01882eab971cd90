"""ZeRO-1 data parallelism for bf16 master-weight training (the Llama DDP worker, ``--zero 1``).

The reference's DDP contract (``examples/mnist/mnist.py:136-138``: every replica steps the
same model on its own data, gradients averaged) is kept; what changes is where the optimizer
state lives.  ``DistributedDataParallel`` + ``MasterAdamW`` keeps, on EVERY rank, fp32
masters + both AdamW moments (12 B/param: 96 GB for Llama-3 8B) and runs the memory-bound
update over all of them (~40 ms of a 360 ms step on one MI355X,
``profiles/r2_llama3_8b_step_kernels.md``).  Here each rank owns 1/W of every bucket:

* backward: each gradient is copied (fp32) into its flat bucket as soon as autograd has
  accumulated it (post-accumulate hook; the bf16 ``.grad`` is freed right away), the bucket
  is scaled by 1/W and **reduce-scattered** (fp32 sum) asynchronously while backward goes on;
* ``step()``: fused HIP AdamW (``csrc/kernels/adamw.hip``) on the rank's shard only
  (master, m, v, grad shard -> new master + the bf16 weight shard, in place in the flat
  weight bucket), then an async in-place **all-gather** of the bucket's weights;
* next forward: a pre-hook per module waits (stream-side) for the all-gather of the buckets
  holding that module's weights, so later buckets' all-gathers run under earlier layers.

Bytes per rank and step over xGMI: reduce-scatter 4 B x (W-1)/W + all-gather 2 B x (W-1)/W
per parameter, against 2 x 4 B x (W-1)/W for the fp32 all-reduce it replaces; optimizer state
and update time are divided by W.  Buckets are large (``bucket_mb``, default 256 MB of
fp32 gradient): few collectives, each well into RCCL's bandwidth regime on point-to-point
xGMI links.

``reduce_dtype=torch.bfloat16`` (``--allreduce-dtype bf16``; at world 1, where nothing is
reduced, every bucket takes its parameters' dtype) halves the reduce-scatter bytes, like DDP's
``bf16_compress_hook``, and enables **gradient-as-bucket-view** (``grad_view``): every bf16
matmul weight gets a ``_pto_grad_sink`` whose view IS its bucket slot, and ``linear_tn``'s
backward GEMM writes dW there directly (``ops/llm.py``) -- no bf16 ``.grad`` allocation and no
deposit copy pass (the round-2 world-1 cost: 389 vs 365 ms/step and +30 GB).  Such buckets
hold the unscaled gradient sum; the 1/W rides on the AdamW kernel (exact for W = 2^k).

Numerics (fp32 reduction) equal ``DDP(fp32 comm hook) + MasterAdamW``: the same fp32 sum of the same
``grad / W`` terms, the same AdamW per element (tests/test_harness.py pins the parameter
digest of both paths equal on gloo).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from ..ops.optim import MasterAdamW, adamw_launch, sr_key

_ALIGN = 64  # shard lengths are multiples of this (16-byte aligned fp32 / bf16 shard pointers)


class _Sink:
    """Destination of a weight gradient written in place by a backward GEMM: its slot of the
    bucket (allocated when the bucket's first gradient arrives, see ``_Bucket.grad32``)."""
    __slots__ = ("bucket", "off", "shape", "dtype", "ready")

    def __init__(self, bucket, off: int, shape, ready):
        self.bucket, self.off, self.shape, self.ready = bucket, off, shape, ready
        self.dtype = bucket.gdt

    @property
    def view(self) -> torch.Tensor:
        n = 1
        for d in self.shape:
            n *= d
        return self.bucket.grad32[self.off:self.off + n].view(self.shape)


class _Bucket:
    def __init__(self, params: List[nn.Parameter], world: int, rank: int, reduce_dtype=torch.float32,
                 accum: bool = False, state_dtype=torch.float32, rng_base: int = 0):
        self.params = params
        self.rng_base = rng_base  # bf16 moments: elements (npad) of the buckets before this one
        self.dtype = params[0].dtype
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self.shard = -(-n // (world * _ALIGN)) * _ALIGN
        self.npad = self.shard * world
        self.lo = rank * self.shard
        self.flat_w = torch.zeros(self.npad, dtype=self.dtype, device=dev)
        # gradient bucket: the reduce dtype; at world 1 (nothing is reduced) the parameters' own
        # dtype, i.e. exactly the .grad autograd would have produced.  Under gradient accumulation
        # it is a per-backward staging buffer and takes the parameters' dtype as well: what is
        # reduced is the fp32 accumulator (or its bf16 rounding), of dtype rdt
        self.gdt = reduce_dtype if world > 1 and not accum else self.dtype
        self.rdt = reduce_dtype if accum else self.gdt
        # grad_accum > 1 only: the fp32 sum of the step's micro-batch gradients over the whole
        # bucket (allocated by the first fold, then kept), the number of folds into it this step,
        # the parameters that contributed to it, and the buffer a reduce-scatter in flight reads
        self.accum = accum
        self.acc: Optional[torch.Tensor] = None
        self.nfold = 0
        self.touched: set = set()
        self.rs_src: Optional[torch.Tensor] = None
        self.n = n
        self.world = world
        # the full gradient bucket lives only from its first gradient of a backward to the end of
        # its reduce-scatter (world 1: to the end of step()): allocated at the first arrival, then
        # released, so it never coexists with the forward's activation peak -- the peak memory of
        # a step stays that of .grad-based training (the caching allocator recycles the block)
        self._g: Optional[torch.Tensor] = None
        self._dev = dev
        self._gshard = None if world == 1 else torch.zeros(self.shard, dtype=self.rdt, device=dev)
        self.slot: Dict[int, int] = {}
        masters = torch.zeros(self.npad, dtype=torch.float32, device=dev) if self.dtype != torch.float32 else None
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                self.slot[id(p)] = off
                self.flat_w[off:off + k].copy_(p.detach().reshape(-1))
                if masters is not None:
                    init = getattr(p, "_pto_master", None)  # exact fp32 init (ops/optim.py)
                    masters[off:off + k].copy_((init if init is not None else p.detach()).reshape(-1))
                    if init is not None:
                        del p._pto_master
                p.data = self.flat_w[off:off + k].view(p.shape)
                off += k
        # fp32 master of the owned shard (None: fp32 weights are their own master)
        self.master = masters[self.lo:self.lo + self.shard].clone() if masters is not None else None
        del masters
        self.exp_avg = torch.zeros(self.shard, dtype=state_dtype, device=dev)
        self.exp_avg_sq = torch.zeros(self.shard, dtype=state_dtype, device=dev)
        self.pending = len(params)
        self.arrived: set = set()  # ids of the parameters whose gradient was deposited this step
        self.rs_work = None
        self.ag_work = None
        self.unscaled = False  # grad_view bucket: holds sum(g), AdamW applies 1/W

    def w_shard(self) -> torch.Tensor:
        return self.flat_w[self.lo:self.lo + self.shard]

    @property
    def grad32(self) -> torch.Tensor:
        if self._g is None:
            # every slot is written before use (gradient copy / in-place GEMM, or zeroed by
            # step() for a parameter without a gradient); only the alignment padding is cleared
            self._g = torch.empty(self.npad, dtype=self.gdt, device=self._dev)
            if self.npad > self.n:
                self._g[self.n:].zero_()
        return self._g

    @property
    def gshard(self) -> torch.Tensor:
        # world 1: the shard IS the bucket (no reduce-scatter, no copy) -- under gradient
        # accumulation, the accumulator
        if self.world > 1:
            return self._gshard
        return self.acc if self.accum else self.grad32

    def release_grad(self) -> None:
        self._g = None


class ZeroAdamW:
    """Replaces ``DDP(model) + MasterAdamW``: construct on the (unwrapped) model after
    ``to_bf16_matmul_weights``; call ``zero_grad`` / forward / backward / ``step`` as usual.
    Weights are broadcast from rank 0 at construction (DDP constructor semantics).

    ``max_grad_norm`` (default ``None``: off, ``step()`` is the single per-bucket loop): clip by the
    global L2 norm of the averaged gradient, ``torch.nn.utils.clip_grad_norm_``'s rule.  ``step()``
    then makes two passes.  Pass 1 waits for every bucket's reduce-scatter and launches the
    sum-of-squares kernel (``csrc/kernels/gradclip.hip``) over this rank's shard (1/W folded in
    for unscaled buckets; the zero padding adds nothing); one finish launch leaves the rank's
    sum in a device float, and at world > 1 one all-reduce (SUM) of that single fp32 gives every
    rank the same bytes, hence the same clip factor.  Pass 2 is the per-bucket AdamW + all-gather
    loop, its kernel reading the sum on the device.  The global norm needs every bucket reduced
    before the first update, so the first weight all-gather starts one gradient read later than
    without clipping; that is inherent to clipping by global norm.

    ``grad_accum=N`` (default 1: off, no accumulator exists): N backward passes per step, with
    ``accumulate()`` after each of the first N-1 and ``step()`` after the last.  Every bucket gets a
    persistent fp32 accumulator of the FULL bucket (``npad`` elements, 4 B per parameter on every
    rank -- not the 1/W shard: that is the price of one collective per bucket per step instead of
    one per micro-batch, DDP's ``no_sync``).  The per-backward bucket becomes a staging buffer in
    the parameters' dtype whatever the reduce dtype, so a deposit is an exact copy and gradient
    sinks serve every bf16 GPU bucket; when a micro-batch's last gradient of a bucket arrives, one
    launch folds staging into the accumulator (``ops/gradaccum.py``: sequential fp32 sum) and the
    staging buffer is released.  On the last micro-batch the accumulator is reduce-scattered (fp32
    reduce), or the bf16 rounding of it that the same fold wrote (bf16 reduce; in place in a bf16
    staging buffer); at world 1 the accumulator is the gradient shard.  The norm pass and AdamW
    apply 1/(N*W) as their gradient scale.

    ``state_dtype=torch.bfloat16`` (default fp32): the moments of every shard are bf16, rounded
    stochastically by each AdamW pass (``MasterAdamW``'s docstring has the rule).  An element's
    random bits are a hash of (``state_seed``, the pass's step count, its position: the ``npad`` of
    the buckets before its own plus its offset in the bucket), so a shard's bits do not depend on
    which launch updates it and a resumed run continues bit for bit.  The positions follow the
    bucket layout, which changes with the world size and differs from ``MasterAdamW``'s parameter
    order: at bf16 state the result equals neither another world size's nor ``MasterAdamW``'s bit
    for bit (the fp32-state identities above are unaffected)."""

    def __init__(self, model: nn.Module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 group=None, bucket_mb: float = 256.0, reduce_dtype=torch.float32, grad_view: bool = True,
                 max_grad_norm=None, grad_accum=1, state_dtype=torch.float32, state_seed=0):
        if int(grad_accum) != grad_accum or grad_accum < 1:
            raise ValueError("grad_accum: a positive integer")
        if state_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("state_dtype: float32 or bfloat16")
        self.state_dtype = state_dtype
        self.state_seed = int(state_seed)
        self.grad_accum = int(grad_accum)
        self._micro = 0  # accumulate() calls since the last step()
        accum = self.grad_accum > 1
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self._clip = None  # ops.gradclip.GlobalGradNorm: norm pass + result of the last clipped step
        if max_grad_norm is not None:
            from ..ops.gradclip import GlobalGradNorm
            self._clip = GlobalGradNorm(max_grad_norm, group, self.world)
        self.max_grad_norm = self._clip and self._clip.max_norm
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.t = 0
        # per-parameter AdamW step counts (bias correction), as MasterAdamW's st["step"]: at world 1
        # a parameter that gets no gradient skips the step and its count stays behind
        self.pstep: Dict[int, int] = {}
        if reduce_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("reduce_dtype: float32 or bfloat16")
        self.reduce_dtype = reduce_dtype
        params = [p for p in model.parameters() if p.requires_grad]
        if self.world > 1:
            with torch.no_grad():
                for p in params:
                    dist.broadcast(p.data, 0, group=group)
                    init = getattr(p, "_pto_master", None)
                    if init is not None:
                        dist.broadcast(init, 0, group=group)
        # buckets in backward order (reverse registration), <= bucket_mb of fp32 each; one open
        # bucket per dtype, so the small fp32 norm weights between the bf16 projections share
        # buckets instead of each cutting a bf16 run into a tiny collective
        cap = int(bucket_mb * 2 ** 20) // 4
        self.buckets: List[_Bucket] = []
        open_: Dict[torch.dtype, List[nn.Parameter]] = {}
        size: Dict[torch.dtype, int] = {}

        def close(cur):
            self.buckets.append(_Bucket(cur, self.world, self.rank, reduce_dtype, accum, state_dtype,
                                        sum(b.npad for b in self.buckets)))

        for p in reversed(params):
            cur = open_.setdefault(p.dtype, [])
            if cur and size[p.dtype] + p.numel() > cap:
                close(cur)
                cur = open_[p.dtype] = []
                size[p.dtype] = 0
            cur.append(p)
            size[p.dtype] = size.get(p.dtype, 0) + p.numel()
        for cur in open_.values():
            if cur:
                close(cur)
        self._of: Dict[int, _Bucket] = {id(p): b for b in self.buckets for p in b.params}
        for p in params:
            p.register_post_accumulate_grad_hook(self._on_grad)
        self.sinks = 0
        for b in self.buckets:
            b.unscaled = accum  # the accumulator holds the plain sum: AdamW applies 1/(N*W)
        if grad_view:
            for b in self.buckets:
                if b.gdt != b.dtype or not b.flat_w.is_cuda:
                    continue
                b.unscaled = True
                for p in b.params:
                    if p.dim() == 2:
                        p._pto_grad_sink = _Sink(b, b.slot[id(p)], tuple(p.shape),
                                                 lambda p=p, b=b: self._arrive(b, p))
                        self.sinks += 1
        self._hooked = 0
        for mod in model.modules():
            own = [self._of[id(p)] for p in mod.parameters(recurse=False) if id(p) in self._of]
            if own:
                uniq = list({id(b): b for b in own}.values())
                mod.register_forward_pre_hook(lambda _m, _i, bs=uniq: self._wait_weights(bs))
                self._hooked += 1

    # ------------------------------------------------------------------ backward side
    def _on_grad(self, p: torch.Tensor) -> None:
        if p.grad is None:
            # autograd runs post-accumulate hooks even when the backward returned no gradient
            # for the leaf -- the case of a weight whose gradient sink was written in place
            # (it arrived through _arrive already) or of no gradient at all (step() fills it)
            return
        b = self._of[id(p)]
        if b.pending < 0:
            raise RuntimeError(self._second_backward())
        off = b.slot[id(p)]
        self._deposit(b.grad32[off:off + p.numel()], p.grad.reshape(-1), b.unscaled)
        p.grad = None
        self._arrive(b, p)

    def _arrive(self, b: _Bucket, p: torch.Tensor) -> None:
        if b.pending < 0:
            raise RuntimeError(self._second_backward())
        if id(p) in b.arrived:
            raise RuntimeError("ZeroAdamW: a parameter received two gradients in one backward (a weight "
                               "used twice cannot write its gradient in place; construct with grad_view=False)")
        b.arrived.add(id(p))
        b.pending -= 1
        if b.pending == 0:
            if b.accum:
                self._fold(b)
            else:
                self._reduce_scatter(b)

    def _second_backward(self) -> str:
        if self.grad_accum > 1:
            return ("ZeroAdamW: a second backward before accumulate() / step() (grad_accum="
                    f"{self.grad_accum}: the bucket was already folded for this micro-batch)")
        return ("ZeroAdamW: a second backward before step() -- gradient accumulation "
                "across backward passes is not supported (the bucket was already reduced) "
                "without grad_accum > 1")

    def _fold(self, b: _Bucket) -> None:
        """grad_accum > 1: every gradient of this micro-batch is in the staging bucket -- fold it
        into the accumulator (one launch) and release it; on the last micro-batch start the
        bucket's one reduce-scatter of the step."""
        from ..ops.gradaccum import fold
        last = self._micro == self.grad_accum - 1
        stage = b.grad32
        if b.acc is None:
            b.acc = torch.empty(b.npad, dtype=torch.float32, device=stage.device)
        out = None
        if last and self.world > 1 and b.rdt == torch.bfloat16:
            # the bf16 reduce sends the rounded sum: in place in a bf16 staging bucket
            out = stage if stage.dtype == torch.bfloat16 else torch.empty_like(stage, dtype=torch.bfloat16)
        fold(b.acc, stage, b.nfold == 0, out)
        b.nfold += 1
        b.touched |= b.arrived
        b.release_grad()
        b.pending = -1  # folded for this micro-batch (accumulate() / step() reopen the bucket)
        if last and self.world > 1:
            b.rs_src = b.acc if out is None else out
            b.rs_work = dist.reduce_scatter_tensor(b._gshard, b.rs_src, group=self.group, async_op=True)

    def _fill_missing(self, b: _Bucket, force: bool) -> bool:
        """Staging slots of the parameters without a gradient from this backward: a ``.grad`` set
        outside backward is deposited, the rest zeroed.  A bucket no gradient reached at all is
        left alone (returns False) unless ``force``: then it is all zeros."""
        late = [p for p in b.params if id(p) not in b.arrived]
        if not force and not b.arrived and all(p.grad is None for p in late):
            return False
        for p in late:
            slot = b.grad32[b.slot[id(p)]:b.slot[id(p)] + p.numel()]
            if p.grad is None:
                slot.zero_()
            else:
                self._deposit(slot, p.grad.reshape(-1), b.unscaled)
                p.grad = None
                b.arrived.add(id(p))
        return True

    @torch.no_grad()
    def accumulate(self) -> None:
        """End of one of the first N-1 backward passes of a step (``grad_accum=N``): buckets that
        some parameter did not reach are folded with what arrived (a missing gradient adds
        nothing), and every bucket is reopened for the next micro-batch."""
        if self.grad_accum == 1:
            raise RuntimeError("ZeroAdamW.accumulate(): constructed with grad_accum=1")
        if self._micro >= self.grad_accum - 1:
            raise RuntimeError(f"ZeroAdamW.accumulate(): called {self._micro + 1} times with grad_accum="
                               f"{self.grad_accum}; the last backward pass is followed by step()")
        for b in self.buckets:
            if b.pending >= 0:
                if self._fill_missing(b, False):
                    self._fold(b)
            b.pending = len(b.params)
            b.arrived.clear()
        self._micro += 1

    def _deposit(self, dst: torch.Tensor, g: torch.Tensor, unscaled: bool = False) -> None:
        """dst = g / W in the bucket dtype -- the comm hooks' ``grad / W`` before the sum.  For a
        power-of-two W the scale is exact, so it rides on the cast copy (one pass).  ``unscaled``
        (grad_view buckets): plain copy, the 1/W is applied by AdamW."""
        w = self.world
        if w == 1 or unscaled:
            dst.copy_(g)
        elif w & (w - 1) == 0:
            src = g if dst.dtype == torch.float32 else g.to(dst.dtype)  # (out= never downcasts)
            torch.mul(src, 1.0 / w, out=dst)
        else:
            dst.copy_(g)
            dst.div_(w)

    def _reduce_scatter(self, b: _Bucket) -> None:
        if self.world == 1:
            b.rs_work = None
        else:
            b.rs_work = dist.reduce_scatter_tensor(b.gshard, b.grad32, group=self.group, async_op=True)
        b.pending = -1  # launched

    def zero_grad(self, set_to_none: bool = True) -> None:  # noqa: ARG002 -- grads never persist
        for b in self.buckets:
            for p in b.params:
                p.grad = None

    # ------------------------------------------------------------------ optimizer side
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._micro != self.grad_accum - 1:
            raise RuntimeError(f"ZeroAdamW.step(): {self._micro} accumulate() calls since the last step, "
                               f"grad_accum={self.grad_accum} needs {self.grad_accum - 1}")
        self.t += 1
        skip: Dict[int, set] = {}
        for b in self.buckets:
            if b.accum:
                # stragglers of the last micro-batch: fold what arrived (zeros where nothing ever
                # did, so the accumulator is defined); at world 1 a parameter without a gradient
                # in any micro-batch is left untouched
                if b.pending >= 0:
                    self._fill_missing(b, True)
                    self._fold(b)
                if self.world == 1:
                    missing = {id(p) for p in b.params} - b.touched
                    if missing:
                        skip[id(b)] = missing
            elif b.pending >= 0:
                # some parameter of this bucket got no gradient through the hook this step.  Only
                # the slots that never arrived are filled (zeros, or a gradient set outside
                # backward); deposited gradients are kept.  At world > 1 a missing gradient
                # contributes zeros to the sum (DDP's find_unused_parameters semantics); at world 1
                # a parameter without any gradient is left untouched, as MasterAdamW /
                # torch.optim.AdamW skip it.
                for p in b.params:
                    if id(p) in b.arrived:
                        continue
                    off = b.slot[id(p)]
                    if p.grad is None:
                        b.grad32[off:off + p.numel()].zero_()
                        if self.world == 1:
                            skip.setdefault(id(b), set()).add(id(p))
                    else:
                        self._deposit(b.grad32[off:off + p.numel()], p.grad.reshape(-1), b.unscaled)
                        p.grad = None
                self._reduce_scatter(b)
        if self._clip is not None:
            # pass 1 of a clipped step: global norm of the averaged gradient, left on the device
            self._clip.run([(self._reduced(b), self._gscale(b)) for b in reversed(self.buckets)])
        # forward order (the last bucket holds the first layers): their all-gathers go first
        for b in reversed(self.buckets):
            self._reduced(b)
            # parameters grouped by their step count after this step (world > 1: every parameter
            # steps -- a missing gradient is a zero contribution, DDP's semantics); each group is
            # one AdamW pass over the bucket with the other ranges saved and restored around it
            skipped = skip.get(id(b), set())
            groups: Dict[int, List[nn.Parameter]] = {}
            for p in b.params:
                if id(p) not in skipped:
                    t = self.pstep[id(p)] = self.pstep.get(id(p), self.t - 1) + 1
                    groups.setdefault(t, []).append(p)
            if self.world > 1 and len(groups) > 1:
                # _save_ranges / _restore_ranges index bucket-absolute offsets, valid only when the
                # shard is the whole bucket (world 1); at world > 1 every parameter steps together
                raise RuntimeError("ZeroAdamW: parameters of one bucket diverged in step count at world > 1")
            for t, members in groups.items():
                ids = {id(p) for p in members}
                keep = self._save_ranges(b, [(b.slot[id(p)], p.numel()) for p in b.params if id(p) not in ids])
                self._adamw(b, t)
                self._restore_ranges(b, keep)
            if self.world == 1:
                b.release_grad()
            if self.world > 1:
                src = b.w_shard() if b.flat_w.is_cuda else b.w_shard().clone()
                b.ag_work = dist.all_gather_into_tensor(b.flat_w, src, group=self.group, async_op=True)
            b.pending = len(b.params)
            b.arrived.clear()
            b.nfold = 0  # the accumulator is empty again (its memory is kept)
            b.touched.clear()
        self._micro = 0
        return loss

    def _gscale(self, b: _Bucket) -> float:
        """What the norm pass and AdamW multiply this bucket's gradient by: 1/(N*W) for a plain
        sum over micro-batches and ranks, 1 where the deposit scaled already."""
        return 1.0 / (self.grad_accum * self.world) if b.unscaled else 1.0

    def _reduced(self, b: _Bucket) -> torch.Tensor:
        """The bucket's gradient shard, its reduce-scatter waited for.  At world > 1 the full
        gradient bucket is released: the shard holds what the norm pass and AdamW need
        (stream-ordered after the wait)."""
        if b.rs_work is not None:
            b.rs_work.wait()
            b.rs_work = None
        if self.world > 1:
            b.release_grad()
            b.rs_src = None
        return b.gshard

    def last_grad_norm(self):
        """Global norm of the averaged gradient at the last ``step()``, before clipping, as a 0-dim
        tensor on the parameters' device (``None`` without ``max_grad_norm`` or before the first
        step).  Does not synchronise."""
        return None if self._clip is None else self._clip.last_grad_norm()

    def set_lr(self, lr: float) -> None:
        """The learning rate of the next ``step()`` (a schedule sets it per step: the fused launch
        takes it as a host scalar)."""
        self.lr = lr

    @staticmethod
    def _save_ranges(b: _Bucket, ranges) -> list:
        """Copies of the optimizer state + weights of the bucket ranges AdamW must not touch
        (world 1 only: the shard is the whole bucket)."""
        out = []
        for off, n in ranges:
            sl = slice(off, off + n)
            out.append((sl, b.flat_w[sl].clone(), b.exp_avg[sl].clone(), b.exp_avg_sq[sl].clone(),
                        b.master[sl].clone() if b.master is not None else None))
        return out

    @staticmethod
    def _restore_ranges(b: _Bucket, saved) -> None:
        for sl, w, m, v, ms in saved:
            b.flat_w[sl].copy_(w)
            b.exp_avg[sl].copy_(m)
            b.exp_avg_sq[sl].copy_(v)
            if ms is not None:
                b.master[sl].copy_(ms)

    def _adamw(self, b: _Bucket, t: int) -> None:
        b1, b2 = self.betas
        w = b.w_shard()
        master = b.master if b.master is not None else w
        clip = self._clip
        rng = None
        if self.state_dtype == torch.bfloat16:
            rng = (sr_key(self.state_seed, t), b.rng_base + b.lo)
        if w.is_cuda:
            adamw_launch(master, b.exp_avg, b.exp_avg_sq, b.gshard, w if b.master is not None else None, b.shard, t,
                         self.lr, b1, b2, self.eps, self.weight_decay, self._gscale(b),
                         None if clip is None else (clip.out, clip.max_norm), rng)
        else:
            st = {"step": t, "exp_avg": b.exp_avg, "exp_avg_sq": b.exp_avg_sq}
            g = b.gshard
            if b.accum:
                g = g.float() * self._gscale(b)
            if clip is not None:
                g = g.float() * clip.coef
            MasterAdamW._step_reference(w, g, master, st, self.lr, b1, b2, self.eps, self.weight_decay, rng)

    def _wait_weights(self, buckets) -> None:
        for b in buckets:
            if b.ag_work is not None:
                b.ag_work.wait()  # stream-side wait on GPU backends
                b.ag_work = None

    def synchronize(self) -> None:
        """Wait for every outstanding weight all-gather (before reading the weights)."""
        self._wait_weights(self.buckets)

    # ------------------------------------------------------------------ checkpoint (utils/train_ckpt.py)
    def shard_state_dict(self) -> dict:
        """This rank's optimizer shard: step count + fp32 master / moments of each bucket's slice
        (the weights themselves are in the model's state_dict)."""
        return {"t": self.t, "world": self.world, "rank": self.rank,
                "state_dtype": "bf16" if self.state_dtype == torch.bfloat16 else "fp32",
                "buckets": [{"npad": b.npad, "master": b.master, "exp_avg": b.exp_avg,
                             "exp_avg_sq": b.exp_avg_sq,
                             "pstep": [self.pstep.get(id(p), self.t) for p in b.params]} for b in self.buckets]}

    @torch.no_grad()
    def load_shard_state_dict(self, sd: dict) -> None:
        if sd["world"] != self.world or sd["rank"] != self.rank or len(sd["buckets"]) != len(self.buckets):
            raise ValueError("ZeRO shard checkpoint was written by a different world / rank / bucket layout")
        have = "bf16" if self.state_dtype == torch.bfloat16 else "fp32"
        got = sd.get("state_dtype", "fp32")  # checkpoints from before the field hold fp32 moments
        if got != have or any(s[k].dtype != self.state_dtype for s in sd["buckets"] for k in ("exp_avg", "exp_avg_sq")):
            raise ValueError(f"ZeRO shard checkpoint holds {got} moments, the optimizer was built with {have} "
                             "(state_dtype): they are never cast")
        for b, s in zip(self.buckets, sd["buckets"]):
            if s["npad"] != b.npad or (s["master"] is None) != (b.master is None):
                raise ValueError("ZeRO shard checkpoint bucket layout differs")
            if b.master is not None:
                b.master.copy_(s["master"])
            b.exp_avg.copy_(s["exp_avg"])
            b.exp_avg_sq.copy_(s["exp_avg_sq"])
            for p, n in zip(b.params, s.get("pstep") or [int(sd["t"])] * len(b.params)):
                self.pstep[id(p)] = int(n)
        self.t = int(sd["t"])

    # ------------------------------------------------------------------ inspection
    def state_bytes(self) -> int:
        """Optimizer-state bytes held by this rank (masters + moments of its shards)."""
        n = 0
        for b in self.buckets:
            n += b.exp_avg.numel() * b.exp_avg.element_size() + b.exp_avg_sq.numel() * b.exp_avg_sq.element_size()
            n += b.master.numel() * 4 if b.master is not None else 0
        return n

    def full_masters_digest(self) -> Optional[str]:
        """sha1 of every bucket's fp32 masters gathered in rank order (all ranks must call)."""
        import hashlib
        h = hashlib.sha1()
        for b in self.buckets:
            m = b.master if b.master is not None else b.w_shard().float()
            full = torch.zeros(b.npad, dtype=torch.float32, device=m.device)
            if self.world > 1:
                dist.all_gather_into_tensor(full, m.contiguous(), group=self.group)
            else:
                full.copy_(m)
            h.update(full.cpu().numpy().tobytes())
        return h.hexdigest()
