"""conv_bwd4's dynamic LDS array starts behind the kernel's static LDS (the two wave-group arrival
counters).  Its float4 LDS accesses -- the W2-slice staging stores, the 2b partial tiles -- are
16-byte aligned only if that static part is a multiple of 16 bytes; at 8 bytes every one of them
was misaligned and the stage phase 0.5 us longer (profiles/r8_bwd4_2b/ab.txt).  Reads the AMDGPU
metadata of the built library, no GPU needed."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
LIB = ROOT / "pytorch_operator_amd" / "_lib" / "libpto_hip.so"


def test_conv_bwd4_dynamic_lds_starts_16_byte_aligned():
    if not LIB.exists():
        pytest.skip("libpto_hip.so not built")
    import isa_dump
    res = isa_dump.kernel_resources(LIB)
    hits = [v for k, v in res.items() if "conv_bwd4_kernel" in k]
    assert len(hits) == 1, hits
    assert hits[0]["lds"] > 0 and hits[0]["lds"] % 16 == 0, hits[0]
