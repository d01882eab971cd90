"""Host time of ``MasterAdamW.step()`` alone (no synchronise inside the timed region) over 291 small
tensors, the tensor count of Llama-3 8B: what the Python loop and the launches cost the CPU.

    python tools/opt_step_host_time.py NAME [MAX_GRAD_NORM]

Prints one JSON line (profiles/adamw_unify/README.md).
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_operator_amd.ops.optim import MasterAdamW  # noqa: E402

name = sys.argv[1]
clip = float(sys.argv[2]) if len(sys.argv) > 2 else None
torch.manual_seed(0)
params = []
for layer in range(32):
    params += [torch.randn(64, 64, device="cuda").bfloat16() for _ in range(7)]
    params += [torch.ones(64, device="cuda") for _ in range(2)]
params += [torch.randn(256, 64, device="cuda"), torch.ones(64, device="cuda"), torch.randn(256, 64, device="cuda").bfloat16()]
opt = MasterAdamW(params, lr=1e-3, max_grad_norm=clip)
for p in params:
    p.grad = torch.randn_like(p)
times = []
for it in range(220):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.step()
    t1 = time.perf_counter()
    if it >= 20:
        times.append((t1 - t0) * 1e3)
torch.cuda.synchronize()
q = statistics.quantiles(times, n=10)
print(json.dumps({"run": name, "tensors": len(params), "max_grad_norm": clip,
                  "host_ms_median": round(statistics.median(times), 4), "host_ms_p10": round(q[0], 4),
                  "host_ms_p90": round(q[-1], 4), "host_ms_min": round(min(times), 4)}))
