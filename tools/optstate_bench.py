#!/usr/bin/env python
"""The measurements of profiles/optstate/README.md that are not plain worker runs.

  adamw        the AdamW pass alone at the Llama-3 8B size, fp32 against bf16 moments
               -> adamw_bench.json
  convergence  llama-mini, one fixed batch, 200 steps with fp32 and with bf16 moments
               -> convergence_llama_mini.json
  sr-seed      the worker's Llama-3 8B run with bf16 moments, the data seed left at 1 and only the
               seed of the rounding bits set to --sr-seed S -> llama3_8b_b4_bf16_srseed<S>.json

Each writes its record into --out (default: the current directory).  One MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def adamw(out):
    """8 030 261 248 elements as 8 launches over one 1 003 782 656-element set of buffers (16 GB with
    fp32 moments, far beyond the caches), bf16 gradient and bf16 weight out.  Device events around
    the 8 launches, 2 warm-up passes, median of 7, three rounds alternating the two kernels."""
    from pytorch_operator_amd.ops.optim import adamw_launch, sr_key
    n, parts = 8030261248 // 8, 8
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    master = torch.randn(n, device=dev, generator=gen)
    grad = torch.randn(n, device=dev, generator=gen).bfloat16()
    w = master.bfloat16()
    state = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        state[name] = ((0.1 * torch.randn(n, device=dev, generator=gen)).to(dt),
                       (0.1 * torch.rand(n, device=dev, generator=gen)).to(dt))

    def one_pass(name, step):
        m, v = state[name]
        for k in range(parts):
            rng = (sr_key(1, step), k * n) if name == "bf16" else None
            adamw_launch(master, m, v, grad, w, n, step, 3e-4, 0.9, 0.95, 1e-8, 0.1, 1.0, None, rng)

    rows, step = [], 0
    for rnd in range(3):
        for name, nbytes in (("fp32", 28), ("bf16", 20)):
            times = []
            for it in range(9):
                step += 1
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                one_pass(name, step)
                b.record()
                torch.cuda.synchronize()
                if it >= 2:
                    times.append(a.elapsed_time(b))
            ms = statistics.median(times)
            row = {"round": rnd, "moments": name, "bytes_per_element": nbytes, "elements": n * parts, "launches": parts,
                   "ms_median_of_7": round(ms, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                   "TB_per_s": round(n * parts * nbytes / (ms * 1e-3) / 1e12, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    assert bool(torch.isfinite(master).all())
    with open(os.path.join(out, "adamw_bench.json"), "w") as f:
        json.dump(rows, f, indent=1)


def convergence(out):
    """4 x 128 tokens, MasterAdamW(lr=3e-4, betas=(0.9, 0.95), weight_decay=0.1), the same initial
    weights for both dtypes; the loss of the forward pass before steps 1, 10, 20, ..., 200."""
    from pytorch_operator_amd.models.llama import CONFIGS, Llama
    from pytorch_operator_amd.ops.optim import MasterAdamW, to_bf16_matmul_weights
    x = torch.randint(0, 512, (4, 129), generator=torch.Generator().manual_seed(3)).cuda()
    curves = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        m = Llama(CONFIGS["llama-mini"]).cuda()
        to_bf16_matmul_weights(m)
        opt = MasterAdamW(m.parameters(), lr=3e-4, betas=(0.9, 0.95), weight_decay=0.1, state_dtype=dt, state_seed=1)
        curve = []
        for step in range(1, 201):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m(x[:, :-1], x[:, 1:])
            loss.backward()
            opt.step()
            if step == 1 or step % 10 == 0:
                curve.append((step, round(float(loss), 6)))
        curves[name] = curve
        print(name, curve, flush=True)
    with open(os.path.join(out, "convergence_llama_mini.json"), "w") as f:
        json.dump({"model": "llama-mini", "batch": [4, 128], "steps": 200, "lr": 3e-4, "loss_before_step": curves}, f,
                  indent=1)


def sr_seed(out, seed):
    """ddp_train.main() of the README's bf16 run (--seed 1: weights and tokens), with the
    state_seed that build() passes to MasterAdamW replaced by `seed`."""
    from pytorch_operator_amd.harness import ddp_train
    from pytorch_operator_amd.ops import optim
    init = optim.MasterAdamW.__init__

    def patched(self, *a, **kw):
        if "state_seed" in kw:
            kw["state_seed"] = seed
        init(self, *a, **kw)

    optim.MasterAdamW.__init__ = patched
    return ddp_train.main(["--model", "llama3-8b", "--seq-len", "2048", "--batch-size", "4", "--steps", "20",
                           "--warmup", "5", "--opt-state", "bf16", "--json-out",
                           os.path.join(out, f"llama3_8b_b4_bf16_srseed{seed}.json")])


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("what", choices=["adamw", "convergence", "sr-seed"])
    p.add_argument("--out", default=".")
    p.add_argument("--sr-seed", type=int, default=2)
    args = p.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "adamw":
        adamw(args.out)
    elif args.what == "convergence":
        convergence(args.out)
    else:
        return sr_seed(args.out, args.sr_seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
