"""Engine-independent oracle for left semi / anti joins (docs/semantics.md "Semi / anti join").

The right table's key columns become a Python set of tuples (None for null, so null matches null);
expected semi = the left rows whose key tuple is in the set, in left order; expected anti = the rest."""
import numpy as np
import pyarrow as pa

M64 = (1 << 64) - 1


def fmix64(k: int) -> int:
    """hash.hpp fmix64 (the radix partition function takes its top bits)."""
    k &= M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def fmix64_inv(k: int) -> int:
    k &= M64
    k ^= k >> 33
    k = (k * 0x9cb4b2f8129337db) & M64
    k ^= k >> 33
    k = (k * 0x4f74430c22a54005) & M64
    k ^= k >> 33
    return k


def fmix64_np(k: np.ndarray) -> np.ndarray:
    k = k.astype(np.uint64)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def max_distinct_per_partition(keys: np.ndarray, bits: int) -> int:
    """Largest number of distinct keys in one partition of 2^bits (top bits of fmix64)."""
    u = np.unique(keys.astype(np.int64))
    if bits == 0:
        return len(u)
    return int(np.bincount((fmix64_np(u) >> np.uint64(64 - bits)).astype(np.int64)).max())


def semi_partition_bits(nr: int, cap: int = 4096) -> int:
    """ops/join.cpp: fewest bits with ceil(nr / 2^bits) + 8 sqrt(that) + 16 <= cap."""
    bits = 0
    while True:
        m = (nr + (1 << bits) - 1) >> bits
        if m + 8.0 * np.sqrt(m) + 16.0 <= cap:
            return bits
        bits += 1


def key_tuples(t: pa.Table, on):
    return list(zip(*[t.column(c).to_pylist() for c in on]))


def semi_mask(a: pa.Table, b: pa.Table, left_on, right_on=None) -> np.ndarray:
    """True where the left row's key tuple occurs among the right rows' key tuples."""
    keys = set(key_tuples(b, right_on or left_on))
    return np.fromiter((k in keys for k in key_tuples(a, left_on)), bool, a.num_rows)


def expected(a: pa.Table, b: pa.Table, how: str, left_on, right_on=None, prefix="") -> pa.Table:
    m = semi_mask(a, b, left_on, right_on)
    out = a.filter(pa.array(m if how == "semi" else ~m))
    return out.rename_columns([prefix + n for n in out.column_names])


def assert_same_rows(got: pa.Table, exp: pa.Table):
    """Same columns, same rows, same ORDER (no sorting: local paths keep left's order)."""
    assert got.column_names == exp.column_names
    assert got.num_rows == exp.num_rows
    for n in exp.column_names:
        assert got.column(n).to_pylist() == exp.column(n).to_pylist(), n


def canon(t: pa.Table):
    """Rows as a sorted list of tuples (distributed outputs: order unspecified)."""
    rows = list(zip(*[t.column(n).to_pylist() for n in t.column_names]))
    return sorted(rows, key=lambda r: tuple((x is None, x) for x in r))
