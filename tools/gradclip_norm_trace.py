"""Per-step loss and gradient norm of the clipped Llama-3 8B worker at --zero Z: the worker's own
build / data / step, plus a synchronise and a print per step (profiles/gradclip/README.md).

    python tools/gradclip_norm_trace.py Z out.jsonl
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_operator_amd.harness import ddp_train as W  # noqa: E402
from pytorch_operator_amd.models.llama import CONFIGS  # noqa: E402

zero, out = sys.argv[1], sys.argv[2]
args = W.parse_args(["--model", "llama3-8b", "--seq-len", "2048", "--batch-size", "4", "--zero", zero,
                     "--max-grad-norm", "1.0"])
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.manual_seed(args.seed)
model, opt = W.build(args, dev, 1)
W.setup_gemm_tuning(args, dev)
g = torch.Generator(device="cpu").manual_seed(args.seed + 0)
data = torch.randint(0, CONFIGS[args.model].vocab_size, (4, args.seq_len + 1), generator=g).to(dev)
x, y = data[:, :-1].contiguous(), data[:, 1:].contiguous()
rows = []
for step in range(11):
    opt.zero_grad(set_to_none=True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        loss = model(x, y)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    o = opt._clip.out.cpu()
    rows.append({"step": step + 1, "loss": float(loss.detach()), "sumsq": float(o[0]), "sumsq_bits": int(o[:1].view(torch.int32)),
                 "grad_norm": float(o[1])})
    print(json.dumps(rows[-1]), flush=True)
with open(out, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
