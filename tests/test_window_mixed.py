"""A spec of every window family in one call, in four spec orders, on a CPU context: every column bit for
bit that of its spec alone, the trace counters independent of the order (window_mixed_utils)."""
import pytest

import window_mixed_utils as mx
from cylon_amd import CylonContext


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


@pytest.mark.parametrize("size", list(mx.SIZES))
def test_specs_of_one_call_do_not_affect_one_another(cpu, size):
    mx.check_mixed(cpu, "cpu", size)
