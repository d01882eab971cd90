"""expand alone at B = 8, S = 8192, uint32, with eos, against the parent commit's composition
(doc_starts_from_tokens + validate_doc_start + masked_fill + doc_ends) on the same tokens.  Run from anywhere on a GPU; writes expand_bench.json beside this file."""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from pytorch_operator_amd.ops import attention as A  # noqa: E402
from pytorch_operator_amd.ops import token_batch  # noqa: E402

B, S, V = 8, 8192, 128256
eos = V - 1
rng = np.random.default_rng(5)
tok = rng.integers(0, V - 1, B * S + 1).astype(np.uint32)
tok[rng.random(B * S + 1) < 1.0 / 512] = eos
dev = torch.device("cuda")
src = torch.from_numpy(tok.view(np.int32)).to(dev)
# the parent's batch: int64 [B, S + 1] on the device (rows overlap by one token here, as the span's do)
idx = torch.arange(B).view(B, 1) * S + torch.arange(S + 1).view(1, S + 1)
data = torch.from_numpy(tok.astype(np.int64))[idx].to(dev)


def composition():
    x, y = data[:, :-1].contiguous(), data[:, 1:].contiguous()
    ds = A.doc_starts_from_tokens(x, eos)
    A.validate_doc_start(ds)
    y = y.masked_fill(x == eos, -100)
    de = A.doc_ends(ds)
    return x, y, ds, de


def composition_device_only():
    x, y = data[:, :-1].contiguous(), data[:, 1:].contiguous()
    ds = A.doc_starts_from_tokens(x, eos)
    y = y.masked_fill(x == eos, -100)
    de = A.doc_ends(ds)
    return x, y, ds, de


def kernel():
    return token_batch.expand(src, S, B, S, V, eos)


# same results first
kx, ky, kds, kde, kst = kernel()
cx, cy, cds, cde = composition()
assert torch.equal(kx, cx) and torch.equal(ky, cy) and torch.equal(kds, cds) and torch.equal(kde, cde)
print("outputs equal; stats", kst.tolist(), flush=True)


def timed(fn, iters):
    """us per call: host clock around iters calls closed by a synchronise, and device events around them."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, e0.elapsed_time(e1) / iters * 1e3


arms = {"expand": kernel, "composition": composition, "composition_no_validate": composition_device_only}
for fn in arms.values():
    for _ in range(20):
        fn()
rounds = {k: [] for k in arms}
for r in range(7):
    for name, fn in arms.items():
        rounds[name].append(timed(fn, 200))
out = {"B": B, "S": S, "vocab": V, "width_bytes": 4, "iters_per_round": 200, "rounds": 7}
for name, v in rounds.items():
    host, devt = [a for a, _ in v], [b for _, b in v]
    out[name] = {"host_us_median": round(statistics.median(host), 2), "host_us_min": round(min(host), 2),
                 "host_us_max": round(max(host), 2), "device_us_median": round(statistics.median(devt), 2),
                 "device_us_min": round(min(devt), 2), "device_us_max": round(max(devt), 2)}
out["ratio_host_median"] = round(out["composition"]["host_us_median"] / out["expand"]["host_us_median"], 2)
out["bytes_expand"] = B * S * 4 + B * S * (8 + 8 + 4 + 4)
print(json.dumps(out, indent=1))
with open(Path(__file__).with_name("expand_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
