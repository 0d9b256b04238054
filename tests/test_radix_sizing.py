"""The radix partitions' sizing rules (ops/radix_sizing.hpp), pinned on the CPU through their size
getters: C.radix_partition_bits(rows, cap) -- the partition bits of the LDS radix join
(ops/join_radix.cpp plan_radix_join), its bounded-memory first-pass chunks (ops/join_bounded.cpp)
and the semi join (ops/join_semi.cpp) -- and C.radix_slot_rows(rows, nparts), the slot of the
slot-mode partition passes.  semi_join_utils.semi_partition_bits is the independent statement of
the bit rule; the table holds values computed from the formulas before they were shared."""
import pytest

from cylon_amd._lib import C
from semi_join_utils import semi_partition_bits

CAPS = [4096, 4408, 4544]


@pytest.mark.parametrize("cap", CAPS)
def test_partition_bits_match_the_independent_rule(cap):
    for n in [0, 1, cap, cap + 1, 2**20, 3_000_000, 2**22, 200_000_000, 1_000_000_000]:
        assert C.radix_partition_bits(n, cap) == semi_partition_bits(n, cap), (n, cap)


BITS = [((10**9, 4544), 18), ((10**9, 4408), 18), ((2 * 10**8, 4544), 16), ((2**22, 4544), 11),
        ((3 * 10**6, 4544), 10), ((2**20, 4096), 9), ((4544, 4544), 1), ((1, 4544), 0), ((0, 4544), 0)]
SLOTS = [((10**9, 2**18), 4376), ((3 * 10**6, 2**12), 1016), ((0, 2**11), 64), ((1, 2**11), 64)]


@pytest.mark.parametrize("args,want", BITS)
def test_partition_bits_values(args, want):
    assert C.radix_partition_bits(*args) == want


@pytest.mark.parametrize("args,want", SLOTS)
def test_slot_rows_values(args, want):
    assert C.radix_slot_rows(*args) == want
