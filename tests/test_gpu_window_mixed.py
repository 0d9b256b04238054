"""A spec of every window family in one call, in four spec orders, on the MI355X and on a CPU context:
every column bit for bit that of its spec alone on the same context, the trace counters independent of
the order and the same on both contexts (window_mixed_utils)."""
import pytest

import window_mixed_utils as mx
from cylon_amd import CylonContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


@pytest.mark.parametrize("size", list(mx.SIZES))
def test_specs_of_one_call_do_not_affect_one_another(gpu, cpu, size):
    cg = mx.check_mixed(gpu, "gpu", size)
    cc = mx.check_mixed(cpu, "cpu", size)
    assert cg == cc, (cg, cc)
