"""BatchSource.check_batch rejects what the kernels' row functions cannot wrap (no GPU needed: the
check reads three integers of the source)."""
from types import SimpleNamespace

import pytest

from pytorch_operator_amd.ops.mnist import BatchSource


def _src(n_total, host_offset=0, perm=object()):
    return SimpleNamespace(n_total=n_total, host_offset=host_offset, perm=perm)


@pytest.mark.parametrize("perm", [object(), None], ids=["perm", "identity"])
def test_batch_larger_than_dataset_raises(perm):
    BatchSource.check_batch(_src(10, perm=perm), 10)
    with pytest.raises(ValueError, match="larger than dataset"):
        BatchSource.check_batch(_src(10, perm=perm), 11)


@pytest.mark.parametrize("off", [-1, 10, 11, 1 << 20])
def test_host_offset_outside_the_dataset_raises(off):
    with pytest.raises(ValueError, match="host_offset"):
        BatchSource.check_batch(_src(10, host_offset=off), 4)


def test_largest_wrapping_batch_passes():
    BatchSource.check_batch(_src(10, host_offset=9), 10)  # every sample but the first wraps
