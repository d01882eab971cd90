"""Kernel-argument preloading of the MNIST step kernels (round 7).

mnist_kernels.hip is built with ``-mllvm -amdgpu-kernarg-preload-count=16``: the command processor
writes the leading 14 argument dwords into user SGPRs at wave launch.  That covers only a leading
run of plain parameters -- it stops at the first by-value struct -- so the five kernels of the
single-GPU step keep what their first loads need in plain leading parameters.  Read from the
kernel descriptors of the built library (tools/isa_dump.py), no GPU needed.
"""
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
LIB = ROOT / "pytorch_operator_amd" / "_lib" / "libpto_hip.so"
MNIST_SRC = ROOT / "csrc" / "kernels" / "mnist_kernels.hip"

STEP_KERNELS = ["conv12_fwd_kernel", "fc1_fwd_kernelILi2", "fc1_bwd_head_kernel", "conv_bwd4_kernel",
                "slab_reduce_sgd_kernel"]


@pytest.fixture(scope="module")
def kd():
    if not LIB.exists():
        pytest.skip("libpto_hip.so not built")
    import isa_dump
    return isa_dump.kernel_descriptors(LIB)


def _find(kd, sub):
    hits = [k for k in kd if sub in k]
    assert len(hits) == 1, (sub, hits)
    return kd[hits[0]]


def test_descriptors_are_read(kd):
    # every kernel of the library has a descriptor with a plausible argument-block size
    assert len(kd) > 100
    assert all(0 < v["kernarg_size"] < 4096 for v in kd.values())


@pytest.mark.parametrize("name", STEP_KERNELS)
def test_step_kernels_preload_14_dwords(kd, name):
    d = _find(kd, name)
    assert d["kernarg_preload_length"] == 14 and d["kernarg_preload_offset"] == 0, (name, d)


def test_flag_is_scoped_to_the_mnist_kernels(kd):
    # the exchange kernels (xgmi_allreduce.hip) are built without the flag
    for name in ("xar_kernelENS", "xar_kernel_fcENS", "xar_prebarrier_kernel"):
        assert _find(kd, name)["kernarg_preload_length"] == 0, name
    # and so is every other translation unit, plain-parameter kernels included: a kernel that
    # preloads anything is one of mnist_kernels.hip's
    mnist = set(re.findall(r"void (\w+_kernel)\(", MNIST_SRC.read_text()))
    assert "conv12_fwd_kernel" in mnist
    others = [k for k, v in kd.items()
              if v["kernarg_preload_length"] and not any(re.search(r"\d" + m + r"(E|I)", k) for m in mnist)]
    assert not others, others
