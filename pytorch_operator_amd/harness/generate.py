"""Continue a prompt with a Llama checkpoint of the DDP worker (``ddp_train --ckpt-dir``):

    python -m pytorch_operator_amd.harness.generate --model llama3-8b --ckpt-dir ckpt/ \
        --prompt 128000,791,3938 --tokens 64 --temperature 0.8 --top-k 50

Loads the weights alone (``utils.train_ckpt.load_weights``: no optimizer state, any world size), runs
``Llama.generate`` (KV cache, ``csrc/kernels/decode_attention.hip`` on a GPU) and prints the worker's
sample event: ``{"event": "sample", "step": ..., "prompt": [...], "tokens": [...]}``.
"""
from __future__ import annotations

import argparse
import json
import sys


def parse_args(argv=None):
    from .ddp_train import MODELS
    p = argparse.ArgumentParser(description="generate from a Llama checkpoint of harness.ddp_train")
    p.add_argument("--model", choices=[m for m in MODELS if m.startswith("llama")], required=True)
    p.add_argument("--ckpt-dir", required=True)
    p.add_argument("--prompt", required=True, help="token ids 'id,id,...'")
    p.add_argument("--tokens", type=int, default=32)
    p.add_argument("--temperature", type=float, default=0.0, help="0 = greedy")
    p.add_argument("--top-k", type=int, default=0, help="0 = the whole vocabulary")
    p.add_argument("--eos-id", type=int, default=None, help="a sequence that emits it keeps emitting it")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16",
                   help="as the worker's: bf16 autocast around the model (a GPU always runs bf16 projections)")
    p.add_argument("--attn", choices=["auto", "sdpa"], default="auto",
                   help="HIP prefill and decode attention where they apply, or the library's")
    p.add_argument("--no-cuda", action="store_true")
    return p.parse_args(argv)


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch
    from ..models.llama import CONFIGS, Attention, Llama
    from ..utils import train_ckpt
    from .ddp_train import parse_prompt
    cfg = CONFIGS[args.model]
    try:
        prompt = parse_prompt(args.prompt, cfg.vocab_size)
        dev = torch.device("cuda" if not args.no_cuda and torch.cuda.is_available() else "cpu")
        Attention.impl = args.attn
        with torch.device(dev):
            model = Llama(cfg)
        step = train_ckpt.load_weights(args.ckpt_dir, model, dev)
        gen = torch.Generator(device=dev).manual_seed(args.seed) if args.temperature > 0 else None
        with torch.autocast(device_type=dev.type, dtype=torch.bfloat16, enabled=args.dtype == "bf16"):
            toks = model.generate(torch.tensor([prompt], dtype=torch.long, device=dev), max_new_tokens=args.tokens,
                                  temperature=args.temperature, top_k=args.top_k, eos_id=args.eos_id, generator=gen)
    except ValueError as e:
        print(f"error: {e}", file=sys.stderr, flush=True)
        return 2
    print(json.dumps({"event": "sample", "step": step, "prompt": prompt, "tokens": toks[0].tolist()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
