"""DDP training worker for the BASELINE's large-model job shapes (ResNet-50 / Llama-3 bf16).

The reference only ships the MNIST worker; BASELINE.json additionally names
"ResNet-50 DDP bf16" and "Llama-3 8B DDP bf16" (Master=1 Worker=7 on 8x MI355X).  This
entrypoint runs either shape under the same operator contract (env rendezvous, one
``amd.com/gpu`` per pod, ``--backend rccl``) with synthetic data and random-init
weights, and reports throughput as one JSON line (rank 0):

    python -m pytorch_operator_amd.harness.ddp_train --model resnet50 --batch-size 256
    python -m pytorch_operator_amd.harness.ddp_train --model llama3-8b --seq-len 2048 --batch-size 1

MI355X specifics: bf16 autocast (MFMA bf16 through hipBLASLt/MIOpen), fused RMSNorm / RoPE /
SwiGLU HIP kernels in the Llama blocks, bf16 matmul weights with fp32 masters updated by the
fused HIP AdamW (``--master-weights``, on by default on a GPU: no per-step weight/grad cast
kernels, fp32 all-reduce kept through a comm hook), DDP with flat gradient buckets sized for xGMI
(``--bucket-mb``, default 64: few, large RCCL collectives), ``gradient_as_bucket_view``
(no gradient copy), optional bf16 gradient compression (``--allreduce-dtype bf16``), and
the 288 GB HBM budget that lets Llama-3 8B train with plain DDP (whole fp32 model, grads
and AdamW state per GPU -- no sharding).

``--data PATH`` (Llama) trains on pre-tokenised files instead of the one synthetic batch: every
micro-step reads its own windows (``data/tokens.py``), expanded on the device by
``csrc/kernels/token_batch.hip``, with ``--lr-schedule`` / ``--lr-warmup-steps``, a held-out loss
(``--eval-data``) and ``--log-every``:

    python -m pytorch_operator_amd.harness.ddp_train --model llama3-8b --batch-size 4 --data shards/ \
        --eos-id 128001 --lr-schedule cosine --lr-warmup-steps 200 --lr-total-steps 10000 \
        --eval-data heldout.npy --eval-every 500 --log-every 50
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

MODELS = ("resnet50", "resnet-tiny", "llama3-8b", "llama3-1b", "llama-tiny", "llama-mini", "llama-mini64")


def parse_prompt(text, vocab_size: int):
    """'id,id,...' -> [ids] (None stays None); ValueError for anything but ids of the vocabulary."""
    if text is None:
        return None
    try:
        ids = [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise ValueError(f"token ids separated by commas, got {text!r}") from None
    if not ids:
        raise ValueError("at least one token id")
    bad = [i for i in ids if not 0 <= i < vocab_size]
    if bad:
        raise ValueError(f"ids {bad[:4]} are outside the {vocab_size}-token vocabulary")
    return ids


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="DDP training worker (ResNet-50 / Llama-3, synthetic data)")
    p.add_argument("--model", choices=MODELS, default="resnet50")
    p.add_argument("--batch-size", type=int, default=None, help="per-rank batch (default 256 / 1)")
    p.add_argument("--seq-len", type=int, default=2048)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--backend", default=None, choices=["gloo", "nccl", "rccl"])
    p.add_argument("--no-cuda", action="store_true")
    p.add_argument("--bucket-mb", type=float, default=64.0)
    p.add_argument("--allreduce-dtype", choices=["fp32", "bf16"], default="fp32")
    p.add_argument("--grad-checkpoint", action="store_true", help="Llama: recompute blocks in backward")
    p.add_argument("--master-weights", choices=["auto", "on", "off"], default="auto",
                   help="Llama: bf16 matmul weights + fp32 masters in the fused HIP AdamW (auto: on with a GPU)")
    p.add_argument("--conv-algo-search", choices=["on", "off"], default="on",
                   help="ResNet: let MIOpen benchmark conv algorithms per shape (torch.backends.cudnn.benchmark)")
    p.add_argument("--memory-format", choices=["channels_last", "contiguous"], default="channels_last",
                   help="ResNet activations/weights layout (NHWC maps to MIOpen's NHWC bf16 kernels)")
    p.add_argument("--bn", choices=["hip", "library"], default="hip",
                   help="ResNet: fused HIP batch-norm(+add)(+ReLU) kernels or PyTorch's BN/add/ReLU ops")
    p.add_argument("--bn-link", type=int, default=2, choices=[0, 1, 2],
                   help="ResNet: each bottleneck's bn3 backward also sums the next block's residual "
                        "gradient in-kernel (ops/batchnorm.py GradLink) instead of autograd's add pass (1); "
                        "2 also sums a stage's downsample-conv input gradient there (link_tap); 0: off")
    p.add_argument("--bn-mask", choices=["bits", "output"], default="bits",
                   help="ResNet: residual+ReLU BN backward masks from a 1-bit forward image, or re-read "
                        "from the BN output")
    p.add_argument("--pool", choices=["hip", "library"], default="hip",
                   help="ResNet stem max-pool: HIP kernels (1-byte taps, gather backward) or PyTorch's op")
    p.add_argument("--conv1x1", choices=["gemm", "library"], default="library",
                   help="ResNet: 1x1 convolutions as hipBLASLt GEMMs on the NHWC view, or MIOpen convs "
                        "(library: 30.5 vs 47.3 ms/step at B=256 -- hipBLASLt's picks for the K = N*H*W "
                        "weight-gradient GEMMs run at ~10%% of MIOpen's rate, profiles/r2_resnet_conv1x1_ab.md)")
    p.add_argument("--sgd", choices=["fused", "foreach"], default="fused",
                   help="ResNet SGD implementation (fused: one multi-tensor kernel per step)")
    p.add_argument("--attn", choices=["auto", "sdpa"], default="auto",
                   help="Llama attention: hand-written HIP flash attention where it applies, or SDPA")
    p.add_argument("--residual-norm", choices=["fused", "plain"], default="fused",
                   help="Llama: residual adds fused into the next RMSNorm (fwd and bwd) or plain add + norm")
    p.add_argument("--linear-bwd", choices=["tn", "autograd"], default="tn",
                   help="Llama projections: backward GEMMs with K-contiguous (transposed-copy) operands, "
                        "or autograd's dy.W / dy^T.x layouts")
    p.add_argument("--linear-dtype", choices=["bf16", "fp8"], default="bf16",
                   help="Llama, --dtype bf16: fp8 runs the wqkv / wo / w13 / w2 GEMMs (forward and both backward "
                        "ones) in per-tensor-scaled OCP FP8 (ops/fp8.py, csrc/kernels/fp8_cast.hip); the lm head "
                        "and the embedding stay bf16")
    p.add_argument("--fp8-grad-format", choices=["e5m2", "e4m3"], default="e5m2",
                   help="--linear-dtype fp8: format of the output gradients (activations and weights are e4m3)")
    p.add_argument("--opt-overlap", choices=["on", "off"], default="off",
                   help="Llama (master weights): AdamW updates on a side stream, overlapped with the next "
                        "forward (each module waits only for its own parameters' updates); measured neutral "
                        "(358-360 ms both ways, profiles/r2_llama3_8b_opt_overlap_ab.json): the forward "
                        "GEMMs hold every CU")
    p.add_argument("--zero", choices=["auto", "0", "1"], default="auto",
                   help="Llama (master weights): ZeRO-1 -- reduce-scatter fp32 gradients, AdamW on this "
                        "rank's 1/W shard, all-gather bf16 weights (parallel/zero.py) instead of DDP's "
                        "fp32 all-reduce + a full optimizer per rank; auto = on when world > 1")
    p.add_argument("--zero-bucket-mb", type=float, default=256.0)
    p.add_argument("--zero-grad-view", type=int, default=1,
                   help="ZeRO bf16 buckets: backward GEMMs write weight gradients into the bucket (1/0)")
    p.add_argument("--gemm-tuning", choices=["off", "use", "tune"], default="use",
                   help="PyTorch TunableOp over hipBLASLt/rocBLAS for the model's GEMM shapes: 'use' "
                        "replays the measured per-shape winners in --gemm-tuning-file (shapes not in "
                        "it take the library default), 'tune' benchmarks every candidate solution "
                        "during the first (untimed) step and writes the file, 'off' = library default")
    p.add_argument("--gemm-tuning-file", default=None,
                   help="TunableOp results CSV (default: pytorch_operator_amd/tuning/gemm_mi355x.csv)")
    p.add_argument("--ckpt-dir", default=None,
                   help="checkpoint directory (utils/train_ckpt.py): resume from it if it holds one, save "
                        "there at the end (and every --ckpt-every steps); shared by all ranks")
    p.add_argument("--ckpt-every", type=int, default=0)
    p.add_argument("--max-grad-norm", type=float, default=0.0,
                   help="clip gradients by their global L2 norm (torch.nn.utils.clip_grad_norm_'s rule) "
                        "before the optimizer step; 0 = off.  Master-weight / ZeRO Llama: computed on the "
                        "device inside the optimizer (csrc/kernels/gradclip.hip)")
    p.add_argument("--doc-len-mean", type=int, default=0,
                   help="Llama: pack documents into each sequence -- every position becomes the end-of-text "
                        "token with probability 1/N, attention stays inside each document (the document "
                        "kernels of csrc/kernels/attention.hip) and the target after an end-of-text token is "
                        "ignored; 0 = off (one document per sequence)")
    p.add_argument("--eos-id", type=int, default=None,
                   help="end-of-text token id for --doc-len-mean (default: the last vocabulary id); with --data: "
                        "turns the document mask on (no default)")
    p.add_argument("--grad-accum", type=int, default=1,
                   help="Llama: micro-batches of --batch-size sequences per optimizer step.  Master-weight / "
                        "ZeRO: their gradients are summed in fp32 accumulators (csrc/kernels/gradaccum.hip) and "
                        "reduced once per step; data parallelism needs --zero 1")
    p.add_argument("--opt-state", choices=["fp32", "bf16"], default="fp32",
                   help="Llama, master-weight / ZeRO: dtype of the AdamW moments.  bf16 halves them (4 B per "
                        "parameter instead of 8) and the update pass rounds them stochastically, seeded by --seed "
                        "(csrc/kernels/adamw.hip); the master weights stay fp32")
    p.add_argument("--data", default=None,
                   help="Llama: train on pre-tokenised data -- a .npy / .bin file of token ids or a directory of "
                        "them (data/tokens.py); every micro-step reads its own windows, expanded on the device "
                        "by csrc/kernels/token_batch.hip.  With --eos-id, documents are masked in attention and "
                        "the target after an end-of-text token is ignored; without it the stream is plain causal")
    p.add_argument("--data-dtype", choices=["auto", "uint16", "uint32"], default="auto",
                   help="--data: id width of .bin files (auto: uint16 when the vocabulary fits, else uint32)")
    p.add_argument("--lr-schedule", choices=["constant", "cosine"], default="constant")
    p.add_argument("--lr-warmup-steps", type=int, default=0,
                   help="linear warm-up: lr*t/K for the optimizer steps t <= K")
    p.add_argument("--lr-min-ratio", type=float, default=0.1,
                   help="--lr-schedule cosine: the floor, as a fraction of --lr, reached at --lr-total-steps")
    p.add_argument("--lr-total-steps", type=int, default=None,
                   help="--lr-schedule cosine: length of the whole run in optimizer steps (a resumed run's --steps "
                        "is not it)")
    p.add_argument("--eval-data", default=None,
                   help="--data: held-out token file(s); the eval loss is taken over its first "
                        "--eval-batches * world * --batch-size windows, before the first step, every --eval-every "
                        "steps and at the end")
    p.add_argument("--eval-every", type=int, default=0)
    p.add_argument("--eval-batches", type=int, default=8)
    p.add_argument("--log-every", type=int, default=0,
                   help="print a train event (step, loss, lr, grad_norm) every L optimizer steps; each one "
                        "synchronises with the device")
    p.add_argument("--sample-every", type=int, default=0,
                   help="Llama: every K optimizer steps and at the end, continue --sample-prompt by --sample-tokens "
                        "tokens (Llama.generate: KV cache + csrc/kernels/decode_attention.hip) and print a sample "
                        "event; every rank generates the same text, rank 0 prints it; 0 = off (a K above the run's "
                        "length samples at the end alone).  The other --sample-* flags need it")
    p.add_argument("--sample-tokens", type=int, default=32, help="--sample-every: new tokens per sample")
    p.add_argument("--sample-prompt", default=None,
                   help="--sample-every: token ids 'id,id,...' (default with --data: the first --sample-prompt-len "
                        "ids of the eval stream's first window, or the train stream's; without --data: ids "
                        "1..--sample-prompt-len, clamped to the vocabulary)")
    p.add_argument("--sample-prompt-len", type=int, default=16,
                   help="--sample-every: length of the default prompt (not with --sample-prompt)")
    p.add_argument("--sample-temperature", type=float, default=0.0, help="--sample-every: 0 = greedy")
    p.add_argument("--sample-top-k", type=int, default=0, help="--sample-every: 0 = the whole vocabulary")
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--json-out", default=None)
    args = p.parse_args(argv)
    sampling = [f for f, v, d in (("--sample-every", args.sample_every, 0), ("--sample-tokens", args.sample_tokens, 32),
                                  ("--sample-prompt", args.sample_prompt, None),
                                  ("--sample-prompt-len", args.sample_prompt_len, 16),
                                  ("--sample-temperature", args.sample_temperature, 0.0),
                                  ("--sample-top-k", args.sample_top_k, 0)) if v != d]
    if sampling and not args.model.startswith("llama"):
        p.error(f"{sampling[0]} is for the Llama models")
    args.sample_prompt_ids = None
    if sampling:
        if args.sample_every == 0:
            p.error(f"{sampling[0]} needs --sample-every K (K > 0): without it nothing is sampled")
        if args.sample_prompt is not None and args.sample_prompt_len != 16:
            p.error("--sample-prompt-len sets the length of the default prompt: not with --sample-prompt")
        from ..models.llama import CONFIGS
        try:
            args.sample_prompt_ids = parse_prompt(args.sample_prompt, CONFIGS[args.model].vocab_size)
        except ValueError as e:
            p.error(f"--sample-prompt: {e}")
        if args.sample_every < 0 or args.sample_tokens < 1 or args.sample_prompt_len < 1:
            p.error("--sample-every is not negative; --sample-tokens and --sample-prompt-len are positive")
        if args.sample_temperature < 0 or not 0 <= args.sample_top_k <= CONFIGS[args.model].vocab_size:
            p.error("--sample-temperature is not negative; --sample-top-k is between 0 and the vocabulary size")
    if args.data and not args.model.startswith("llama"):
        p.error("--data is for the Llama models")
    if args.data and args.doc_len_mean > 0:
        p.error("--doc-len-mean draws synthetic documents; with --data the documents are the stream's (--eos-id)")
    if args.eval_data and not args.data:
        p.error("--eval-data needs --data")
    if args.eval_data and args.eval_batches < 1:
        p.error("--eval-batches: a positive number of batches")
    if min(args.lr_warmup_steps, args.eval_every, args.log_every) < 0:
        p.error("--lr-warmup-steps, --eval-every and --log-every are not negative")
    if not 0.0 <= args.lr_min_ratio <= 1.0:
        p.error("--lr-min-ratio: between 0 and 1")
    if args.lr_schedule == "cosine" and (args.lr_total_steps is None or args.lr_total_steps <= args.lr_warmup_steps):
        p.error("--lr-schedule cosine needs --lr-total-steps, larger than --lr-warmup-steps")
    if args.linear_dtype == "fp8" and not (args.model.startswith("llama") and args.dtype == "bf16"):
        p.error("--linear-dtype fp8 is for the Llama models with --dtype bf16")
    if args.grad_accum < 1:
        p.error("--grad-accum: a positive number of micro-batches")
    if args.grad_accum > 1 and not args.model.startswith("llama"):
        p.error("--grad-accum is for the Llama models")
    if args.opt_state != "fp32" and (not args.model.startswith("llama") or args.dtype != "bf16"
                                     or args.master_weights == "off"):
        p.error("--opt-state bf16 is for the master-weight / ZeRO AdamW: a Llama model with --dtype bf16 and "
                "master weights")
    return args


def use_zero(args, device, world: int) -> bool:
    if not args.model.startswith("llama") or args.dtype != "bf16":
        return False
    if args.zero == "1":
        return True
    return args.zero == "auto" and world > 1 and use_master_weights(args, device)


def build(args, device, world: int = 1):
    import torch
    if args.model.startswith("resnet"):
        from ..models.resnet import (Bottleneck, resnet50, resnet_tiny, set_bn_impl, set_conv1x1_impl,
                                     set_pool_impl)
        model = set_bn_impl(resnet50() if args.model == "resnet50" else resnet_tiny(), args.bn)
        from ..ops import batchnorm as _bnm
        from ..ops.batchnorm import BatchNormAct2d
        _bnm.MASK_BITS = args.bn_mask == "bits"
        for m in model.modules():
            if isinstance(m, BatchNormAct2d) and m.link_output:
                m.link_output = bool(args.bn_link)
            if isinstance(m, Bottleneck):
                m.tap_downsample = args.bn_link >= 2
        set_pool_impl(model, args.pool)
        set_conv1x1_impl(model, args.conv1x1)
        fmt = torch.channels_last if args.memory_format == "channels_last" else torch.contiguous_format
        model = model.to(device=device, memory_format=fmt)
        if device.type == "cuda":
            torch.backends.cudnn.benchmark = args.conv_algo_search == "on"
        kw = {}
        if device.type == "cuda":
            kw = {"fused": True} if args.sgd == "fused" else {"foreach": True}
        opt = torch.optim.SGD(model.parameters(), lr=args.lr or 0.1, momentum=0.9, weight_decay=1e-4, **kw)
        return model, opt
    from ..models.llama import CONFIGS, Attention, Llama, RMSNorm, TNLinear
    Attention.impl = args.attn
    TNLinear.impl = "fp8" if args.linear_dtype == "fp8" else args.linear_bwd
    TNLinear.fp8_grad_format = args.fp8_grad_format
    RMSNorm.fuse_residual = args.residual_norm == "fused"
    with torch.device(device):
        model = Llama(CONFIGS[args.model], checkpoint_layers=args.grad_checkpoint)
    clip = {"max_grad_norm": args.max_grad_norm} if args.max_grad_norm > 0 else {}
    accum = {"grad_accum": args.grad_accum} if args.grad_accum > 1 else {}
    state = {"state_dtype": torch.bfloat16, "state_seed": args.seed} if args.opt_state == "bf16" else {}
    if state and not (use_zero(args, device, world) or use_master_weights(args, device)):
        raise SystemExit("error: --opt-state bf16 needs the master-weight optimizer (--master-weights on, or a GPU)")
    if use_zero(args, device, world):
        from ..ops.optim import to_bf16_matmul_weights
        from ..parallel.zero import ZeroAdamW
        to_bf16_matmul_weights(model)
        # bf16 gradient buckets with a bf16 reduce (at world 1 the buckets always take the
        # parameters' dtype): gradient-as-bucket-view then lets the backward GEMMs write dW
        # into the buckets directly
        opt = ZeroAdamW(model, lr=args.lr or 3e-4, betas=(0.9, 0.95), weight_decay=0.1,
                        bucket_mb=args.zero_bucket_mb,
                        reduce_dtype=torch.bfloat16 if args.allreduce_dtype == "bf16" else torch.float32,
                        grad_view=bool(args.zero_grad_view), **clip, **accum, **state)
        return model, opt
    if use_master_weights(args, device):
        from ..ops.optim import MasterAdamW, install_overlap, to_bf16_matmul_weights
        to_bf16_matmul_weights(model)
        overlap = args.opt_overlap == "on" and device.type == "cuda"
        opt = MasterAdamW(model.parameters(), lr=args.lr or 3e-4, betas=(0.9, 0.95), weight_decay=0.1,
                          overlap=overlap, **clip, **accum, **state)
        if overlap:
            install_overlap(model)
        return model, opt
    kw = {"fused": True} if device.type == "cuda" else {}
    try:
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr or 3e-4, betas=(0.9, 0.95), weight_decay=0.1, **kw)
    except (RuntimeError, TypeError):
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr or 3e-4, betas=(0.9, 0.95), weight_decay=0.1)
    return model, opt


def default_tuning_file() -> str:
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tuning",
                        "gemm_mi355x.csv")


def setup_gemm_tuning(args, device) -> dict:
    """TunableOp: each GEMM shape the model issues is dispatched to the hipBLASLt/rocBLAS
    solution measured fastest for it on MI355X (results CSV kept in-tree, validated by the
    library against the ROCm / hipBLASLt / gfx versions it was tuned on).  'tune' runs the
    search inside the first, untimed step; the timed steps only replay the winners."""
    if device.type != "cuda" or args.gemm_tuning == "off":
        return {"mode": "off"}
    import torch.cuda.tunable as tunable
    path = args.gemm_tuning_file or default_tuning_file()
    if args.gemm_tuning == "use" and not os.path.exists(path):
        return {"mode": "off", "missing": path}
    tunable.enable(True)
    tunable.tuning_enable(args.gemm_tuning == "tune")
    if args.gemm_tuning == "tune":
        if os.path.exists(path):
            tunable.read_file(path)  # keep the shapes tuned before; search only new ones
        tunable.set_max_tuning_duration(20)
        tunable.set_max_tuning_iterations(30)
        # the library appends the rank to the file name when it writes; keep ours explicit
        tunable.set_filename(path + ".tuning", False)
    elif not tunable.read_file(path):
        # validators differ (another ROCm / hipBLASLt / torch build): library defaults
        tunable.enable(False)
        print(f"warning: TunableOp rejected {path}; GEMMs use the library default", file=sys.stderr)
        return {"mode": "off", "rejected": path}
    return {"mode": args.gemm_tuning, "file": os.path.relpath(path, os.getcwd())}


def write_tuning_file(path: str) -> int:
    """Write TunableOp's in-memory results (validators first, then one line per tuned GEMM
    shape) in the CSV format ``read_file`` accepts; returns the number of shapes."""
    import torch.cuda.tunable as tunable
    rows = tunable.get_results()
    with open(path, "w") as f:
        vals = tunable.get_validators()
        for name, value in (vals.items() if isinstance(vals, dict) else vals):
            f.write(f"Validator,{name},{value}\n")
        for op, params, sol, ms in rows:
            f.write(f"{op},{params},{sol},{float(ms):.6f}\n")
    return len(rows)


def use_master_weights(args, device) -> bool:
    if not args.model.startswith("llama") or args.dtype != "bf16":
        return False
    return args.master_weights == "on" or (args.master_weights == "auto" and device.type == "cuda")


def optimizer_state_bytes(opt) -> int:
    """Bytes of optimizer state this rank holds: fp32 masters + both moments (``ZeroAdamW``: of its
    shards; ``MasterAdamW``: of every parameter that has stepped)."""
    if hasattr(opt, "state_bytes"):
        return opt.state_bytes()
    return sum(t.numel() * t.element_size() for st in opt.state.values()
               for t in (st.get("master"), st.get("exp_avg"), st.get("exp_avg_sq")) if t is not None)


def fp32_allreduce_hook(process_group, bucket):
    """DDP comm hook: all-reduce a bf16 gradient bucket in fp32 (``--allreduce-dtype fp32`` with
    bf16 master-weight training).  The fp32 mean is what the optimizer consumes: each
    parameter gets ``_pto_grad32``, a view into the reduced fp32 bucket, which ``MasterAdamW``
    reads instead of the bf16 ``.grad`` (also refreshed, rounded, for anything else)."""
    import torch.distributed as dist
    buf = bucket.buffer()
    group = process_group if process_group is not None else dist.group.WORLD
    t = buf.float().div_(dist.get_world_size(group))
    fut = dist.all_reduce(t, group=group, async_op=True).get_future()
    params, grads = bucket.parameters(), bucket.gradients()

    def done(f):
        red = f.value()[0]
        esz = buf.element_size()
        for p, g in zip(params, grads):
            off = (g.data_ptr() - buf.data_ptr()) // esz
            p._pto_grad32 = red[off:off + g.numel()].view(g.shape)
        buf.copy_(red)
        return buf
    return fut.then(done)


def param_digest(model, opt) -> str:
    """sha1 over every parameter and (MasterAdamW) fp32 master, in order: DDP replicas must agree."""
    import hashlib
    import torch
    h = hashlib.sha1()
    for p in model.parameters():
        h.update(p.detach().float().cpu().numpy().tobytes())
        st = opt.state.get(p) or {}
        if isinstance(st.get("master"), torch.Tensor):
            h.update(st["master"].detach().cpu().numpy().tobytes())
    return h.hexdigest()


def weights_digest(model) -> str:
    """sha1 over every parameter tensor as the model holds it (bf16 weights, fp32 norms)."""
    import hashlib
    h = hashlib.sha1()
    for p in model.parameters():
        h.update(p.detach().float().cpu().numpy().tobytes())
    return h.hexdigest()


def train_flops_per_sample(args) -> float:
    if args.model.startswith("resnet"):
        scale = (args.image_size / 224.0) ** 2
        return 3 * 4.09e9 * scale if args.model == "resnet50" else 0.0
    from ..models.llama import CONFIGS
    c = CONFIGS[args.model]
    n = c.num_params() - c.vocab_size * c.dim  # embedding lookup is not a matmul
    # causal attention per token: QK^T and PV over the (on average) S/2 visible keys = 2*S*d
    # forward FLOPs per layer, x3 for forward + backward = 6*L*d*S
    attn = 6 * c.n_layers * c.dim * args.seq_len
    return (6 * n + attn) * args.seq_len  # per sequence


def lr_at(t: int, lr: float, schedule: str = "constant", warmup: int = 0, min_ratio: float = 0.1,
          total: int = None) -> float:
    """Learning rate of optimizer step ``t`` (1-based): linear warm-up over the first ``warmup`` steps,
    then constant, or a cosine from ``lr`` down to ``lr * min_ratio`` at step ``total`` and held there.
    A pure function of the step: a resumed run needs no schedule state."""
    if t <= warmup:
        return lr * t / warmup
    if schedule != "cosine":
        return lr
    if t >= total:
        return lr * min_ratio
    return lr * (min_ratio + (1 - min_ratio) * 0.5 * (1 + math.cos(math.pi * (t - warmup) / (total - warmup))))


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch
    import torch.distributed as dist
    import torch.nn.functional as F
    from ..parallel.dist import init_from_env

    use_gpu = not args.no_cuda and torch.cuda.is_available()
    env = init_from_env(args.backend, use_gpu=use_gpu)
    dev, world, rank = env.device, env.world_size, env.rank
    torch.manual_seed(args.seed)
    is_llama = args.model.startswith("llama")
    B = args.batch_size or (1 if is_llama else (256 if use_gpu else 2))
    N = args.grad_accum
    zero = use_zero(args, dev, world)
    if N > 1 and world > 1 and not zero:
        # DDP's all-reduce would see only the last micro-batch's gradient
        print(f"error: --grad-accum {N} on {world} ranks needs the ZeRO-1 optimizer (--zero 1, with master "
              "weights): the DDP path reduces every backward pass", file=sys.stderr, flush=True)
        dist.destroy_process_group()
        return 2
    model, opt = build(args, dev, world)
    tuning = setup_gemm_tuning(args, dev)
    n_params = sum(p.numel() for p in model.parameters())
    if world > 1 and not zero:
        from torch.nn.parallel import DistributedDataParallel as DDP
        model = DDP(model, device_ids=[dev.index] if use_gpu else None, bucket_cap_mb=args.bucket_mb,
                    gradient_as_bucket_view=True, static_graph=True)
        if args.allreduce_dtype == "bf16":
            from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
            model.register_comm_hook(None, default_hooks.bf16_compress_hook)
        elif use_master_weights(args, dev):
            model.register_comm_hook(None, fp32_allreduce_hook)
    g = torch.Generator(device="cpu").manual_seed(args.seed + rank)
    feed = eval_feed = None
    if args.data:
        # token files: every micro-step takes its own windows (data/tokens.py, data/feed.py)
        from ..data.feed import TokenFeed
        from ..data.tokens import TokenStream
        from ..models.llama import CONFIGS
        V = CONFIGS[args.model].vocab_size
        try:
            if args.eos_id is not None and not 0 <= args.eos_id < V:
                raise ValueError(f"--eos-id {args.eos_id}: an id of the {V}-token vocabulary")
            feed = TokenFeed(TokenStream(args.data, V, args.data_dtype).bind(args.seq_len, B, N, world),
                             rank, dev, args.eos_id)
            if args.eval_data:
                eval_feed = TokenFeed(TokenStream(args.eval_data, V, args.data_dtype)
                                      .bind(args.seq_len, B, args.eval_batches, world), rank, dev, args.eos_id)
        except ValueError as e:
            print(f"error: {e}", file=sys.stderr, flush=True)
            if world > 1:
                dist.destroy_process_group()
            return 2
        doc_start = None
    elif is_llama:
        from ..models.llama import CONFIGS
        V = CONFIGS[args.model].vocab_size
        if args.doc_len_mean > 0:
            from ..ops.attention import doc_starts_from_tokens, validate_doc_start
            eos = V - 1 if args.eos_id is None else args.eos_id

        def draw():
            data = torch.randint(0, V, (B, args.seq_len + 1), generator=g).to(dev)
            doc_start = None
            if args.doc_len_mean > 0:
                # drawn after the tokens from the same generator: the default token stream is unchanged
                cut = torch.rand(B, args.seq_len + 1, generator=g) < 1.0 / args.doc_len_mean
                data = torch.where(cut.to(dev), torch.full_like(data, eos), data)
            x, y = data[:, :-1].contiguous(), data[:, 1:].contiguous()
            if args.doc_len_mean > 0:
                doc_start = doc_starts_from_tokens(x, eos)
                validate_doc_start(doc_start)
                y = y.masked_fill(x == eos, -100)  # that target would be the next document's first token
            return x, y, doc_start

        x, y, doc_start = draw()
        if args.doc_len_mean > 0:
            docs_per_seq = float((x[:, :-1] == eos).sum()) / B + 1.0
        # --grad-accum: micro-batches 2..N, drawn after everything above (the first is unchanged)
        micro = [(x, y, doc_start)] + [draw() for _ in range(N - 1)]
    else:
        H = args.image_size if args.model == "resnet50" else 32
        x = torch.randn(B, 3, H, H, generator=g).to(dev)
        if args.memory_format == "channels_last":
            x = x.to(memory_format=torch.channels_last)
        y = torch.randint(0, 1000 if args.model == "resnet50" else 10, (B,), generator=g).to(dev)
    amp = torch.autocast(device_type=dev.type, dtype=torch.bfloat16, enabled=args.dtype == "bf16")
    from ..utils import train_ckpt
    bare = model.module if hasattr(model, "module") else model
    gstep = train_ckpt.load(args.ckpt_dir, bare, opt, rank, world, dev)
    if gstep and rank == 0:
        print(json.dumps({"event": "resumed", "step": gstep, "dir": args.ckpt_dir}), flush=True)

    # gradient clipping: inside MasterAdamW / ZeroAdamW (they own the gradients), or torch's
    # clip_grad_norm_ in front of a plain torch optimizer
    clip = args.max_grad_norm if args.max_grad_norm > 0 else None
    torch_clip = clip is not None and not hasattr(opt, "last_grad_norm")
    torch_norm = None

    def grad_norm() -> float:
        return float(torch_norm if torch_clip else opt.last_grad_norm())

    own_accum = hasattr(opt, "accumulate")  # MasterAdamW / ZeroAdamW: fp32 accumulators

    def fed(f, t, k, n, last=None):
        """Micro-batch ``k`` of ``n`` of step ``t`` from a token feed, the next one copied ahead
        (``last``: the step after which nothing follows); the kernel's bounds go to attention."""
        then = (t, k + 1) if k + 1 < n else (None if t == last else (t + 1, 0))
        xk, yk, ds, de, stats = f.take(t, k, then)
        if ds is not None and use_gpu:
            from ..ops.attention import set_doc_bounds
            set_doc_bounds(ds, de)
        return xk, yk, ds, stats

    base_lr = args.lr or 3e-4
    scheduled = args.lr_schedule != "constant" or args.lr_warmup_steps > 0
    cur_lr = base_lr

    def set_lr(t):
        nonlocal cur_lr
        cur_lr = lr_at(t, base_lr, args.lr_schedule, args.lr_warmup_steps, args.lr_min_ratio, args.lr_total_steps)
        if hasattr(opt, "set_lr"):
            opt.set_lr(cur_lr)
        else:
            for group in opt.param_groups:
                group["lr"] = cur_lr

    def evaluate():
        """Token-weighted loss over the eval stream's first --eval-batches * world * B windows."""
        was_training = bare.training
        bare.eval()
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        with torch.no_grad():
            for k in range(args.eval_batches):
                xk, yk, dk, stats = fed(eval_feed, 1, k, args.eval_batches, last=1)
                with amp:
                    lk = bare(xk, yk) if dk is None else bare(xk, yk, doc_start=dk)
                acc[0] += lk.double() * stats[0]
                acc[1] += stats[0]
        bare.train(was_training)
        if world > 1:
            dist.all_reduce(acc)
        loss_sum, tokens = (float(v) for v in acc.cpu())
        ev = loss_sum / max(tokens, 1.0)
        if rank == 0:
            print(json.dumps({"event": "eval", "step": gstep, "loss": ev, "ppl": math.exp(min(ev, 700.0)),
                              "tokens": int(tokens)}), flush=True)
        return ev

    sampling = is_llama and args.sample_every > 0
    if sampling:
        # the same prompt and seed on every rank: each generates the same text, no collectives
        prompt_ids = args.sample_prompt_ids
        if prompt_ids is None and feed is not None:
            st = (eval_feed or feed).stream
            prompt_ids = [min(int(t), V - 1) for t in st.read(0, min(args.sample_prompt_len, st.seq_len))]
        elif prompt_ids is None:
            prompt_ids = [min(i, V - 1) for i in range(1, args.sample_prompt_len + 1)]
        if len(prompt_ids) + args.sample_tokens > bare.cfg.max_seq_len:
            print(f"error: a prompt of {len(prompt_ids)} ids and --sample-tokens {args.sample_tokens} exceed the "
                  f"model's {bare.cfg.max_seq_len} positions", file=sys.stderr, flush=True)
            if world > 1:
                dist.destroy_process_group()
            return 2
        sample_gen = torch.Generator(device=dev).manual_seed(args.seed) if args.sample_temperature > 0 else None

    def sample():
        """Continue the prompt (Llama.generate); touches neither the data generator, the feeds, the
        optimizer nor the gradients.  The KV cache lives for the call."""
        with amp:
            toks = bare.generate(torch.tensor([prompt_ids], dtype=torch.long, device=dev),
                                 max_new_tokens=args.sample_tokens, temperature=args.sample_temperature,
                                 top_k=args.sample_top_k, generator=sample_gen)
        if rank == 0:
            print(json.dumps({"event": "sample", "step": gstep, "prompt": prompt_ids, "tokens": toks[0].tolist()}),
                  flush=True)

    def bad_ids() -> int:
        """Ids >= the vocabulary seen so far, over all ranks (reads the device: call at a sync point)."""
        bad = torch.stack([f.total[2] for f in (feed, eval_feed) if f is not None]).sum()
        if world > 1:
            dist.all_reduce(bad)
        n = int(bad)
        if n:
            print(f"error: {n} token id(s) >= the vocabulary size {V} in the data (each was clamped to {V - 1}): "
                  "wrong --data-dtype, or files of another tokenizer", file=sys.stderr, flush=True)
            if world > 1:
                dist.destroy_process_group()
        return n

    def accum_backward():
        """N x (forward, backward); returns the mean of the micro-batch losses (on the device)."""
        total = None
        for k in range(N):
            xk, yk, dk = fed(feed, gstep, k, N)[:3] if feed is not None else micro[k]
            with amp:
                lk = model(xk, yk) if dk is None else model(xk, yk, doc_start=dk)
            if N == 1:
                lk.backward()
                return lk
            if own_accum:
                lk.backward()
                if k < N - 1:
                    opt.accumulate()
            else:
                (lk / N).backward()  # a plain torch optimizer: .grad accumulates the mean natively
            total = lk.detach() if total is None else total + lk.detach()
        return total / N

    def step():
        nonlocal gstep, torch_norm
        gstep += 1
        if args.ckpt_dir and args.ckpt_every and gstep % args.ckpt_every == 0:
            pending_ckpt.append(gstep)
        opt.zero_grad(set_to_none=True)
        if scheduled:
            set_lr(gstep)
        if N > 1 or feed is not None:
            loss = accum_backward()
        else:
            with amp:
                if is_llama and doc_start is not None:
                    loss = model(x, y, doc_start=doc_start)
                elif is_llama:
                    loss = model(x, y)
                else:
                    loss = F.cross_entropy(model(x).float(), y)
            loss.backward()
        if torch_clip:
            torch_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        if pending_ckpt:
            train_ckpt.save(args.ckpt_dir, pending_ckpt.pop(), bare, opt, rank, world)
        return loss

    pending_ckpt = []

    def sync():
        if use_gpu:
            torch.cuda.synchronize(dev)

    eval_loss = None

    def after_step(loss) -> int:
        """--log-every / --eval-every (the only added host syncs); non-zero: ids >= vocab, stop."""
        nonlocal eval_loss
        synced = False
        if args.log_every and gstep % args.log_every == 0:
            ev = {"event": "train", "rank": rank, "step": gstep, "loss": float(loss), "lr": cur_lr}
            if clip is not None:
                ev["grad_norm"] = grad_norm()
            print(json.dumps(ev), flush=True)
            synced = True
        if eval_feed is not None and args.eval_every and gstep % args.eval_every == 0:
            eval_loss = evaluate()
            synced = True
        if sampling and args.sample_every and gstep % args.sample_every == 0:
            sample()
            synced = True
        return 2 if synced and feed is not None and bad_ids() else 0

    if eval_feed is not None:
        eval_loss = evaluate()  # the starting point (step 0, or the checkpoint's step)
        if bad_ids():
            return 2
    t_start = time.time_ns()
    loss = step()
    sync()
    if feed is not None and bad_ids():
        return 2
    if rank == 0:
        first = {"event": "first_step", "rank": rank, "unix_ns": time.time_ns(),
                 "first_step_s": round((time.time_ns() - t_start) / 1e9, 3), "loss": float(loss)}
        if clip is not None:
            first["grad_norm"] = grad_norm()
        print(json.dumps(first), flush=True)
    if after_step(loss):
        return 2
    for _ in range(max(0, args.warmup - 1)):
        if after_step(step()):
            return 2
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
        if after_step(loss):
            return 2
    sync()
    if world > 1:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if eval_feed is not None and not (args.eval_every and gstep % args.eval_every == 0):
        eval_loss = evaluate()
    if sampling and not (args.sample_every and gstep % args.sample_every == 0):
        sample()
    if feed is not None and bad_ids():
        return 2
    samples = args.steps * B * world * N
    per_sample = train_flops_per_sample(args)
    unit_tokens = is_llama
    value = samples * (args.seq_len if unit_tokens else 1) / dt
    res = {"metric": f"{args.model.replace('-', '_')}_ddp_train_{'tokens' if unit_tokens else 'images'}_per_sec",
           "value": round(value, 1), "unit": "tokens/s" if unit_tokens else "images/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
           "dtype": args.dtype, "data": "tokens" if feed is not None else "synthetic", "params": n_params,
           "per_rank_batch": B,
           "seq_len": args.seq_len if is_llama else None, "loss": float(loss),
           "tflops_per_gpu": round(per_sample * samples / dt / world / 1e12, 1) if per_sample else None,
           "max_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1) if use_gpu else None,
           "parallelism": f"dp{world}", "bucket_mb": args.bucket_mb, "allreduce_dtype": args.allreduce_dtype,
           "master_weights": use_master_weights(args, dev) or zero, "zero": 1 if zero else 0}
    if zero:
        res.update(optimizer_state_gb_per_rank=round(opt.state_bytes() / 2 ** 30, 2), zero_buckets=len(opt.buckets),
                   zero_grad_sinks=opt.sinks, zero_grad_dtypes=sorted({str(b.gdt).replace("torch.", "") for b in opt.buckets}))
    res.update(gemm_tuning=tuning.get("mode"))
    if clip is not None:
        res.update(max_grad_norm=clip, grad_norm=grad_norm())
    if is_llama:
        res.update(attn=args.attn, residual_norm=args.residual_norm, linear_bwd=args.linear_bwd,
                   opt_overlap=args.opt_overlap if res["master_weights"] and not zero else None)
    if args.linear_dtype == "fp8":  # (the default's result line keeps its keys)
        res.update(linear_dtype=args.linear_dtype, grad_format=args.fp8_grad_format)
    if N > 1:
        res.update(grad_accum=N)
    if res["master_weights"]:
        res.update(opt_state=args.opt_state, optimizer_state_bytes=optimizer_state_bytes(opt))
    if is_llama and doc_start is not None:
        res.update(doc_len_mean=args.doc_len_mean, docs_per_seq=round(docs_per_seq, 2), attn_mask="document")
    if feed is not None:
        st = feed.stream
        res.update(data_tokens=st.n_tokens, data_windows=st.n_windows,
                   data_epochs=round(gstep * N * world * B / st.n_windows, 4), lr_schedule=args.lr_schedule)
        if args.eos_id is not None:
            res.update(attn_mask="document", docs_per_seq=round(float(feed.total[1]) / max(1, feed.batches * B), 2))
    if eval_loss is not None:
        res.update(eval_loss=eval_loss)
    if tuning.get("mode") == "tune" and rank == 0:
        import torch.cuda.tunable as tunable
        out = args.gemm_tuning_file or default_tuning_file()
        os.makedirs(os.path.dirname(out), exist_ok=True)
        write_tuning_file(out)
        res.update(gemm_tuning_file=out, gemm_tuned_shapes=len(tunable.get_results()))
    if not is_llama:
        res.update(memory_format=args.memory_format, conv_algo_search=args.conv_algo_search, sgd=args.sgd, bn=args.bn, bn_link=args.bn_link,
                   bn_mask=args.bn_mask, pool=args.pool,
                   conv1x1=args.conv1x1)
    if args.ckpt_dir:
        train_ckpt.save(args.ckpt_dir, gstep, bare, opt, rank, world)
        res.update(checkpoint_step=gstep)
    if zero:
        opt.synchronize()
        digest = opt.full_masters_digest()
    else:
        digest = param_digest(model.module if hasattr(model, "module") else model, opt)
    wdig = weights_digest(model.module if hasattr(model, "module") else model)
    print(json.dumps({"event": "param_digest", "rank": rank, "digest": digest, "weights_digest": wdig}),
          flush=True)
    if rank == 0:
        print(json.dumps(res), flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(json.dumps(res) + "\n")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
