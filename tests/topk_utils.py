"""Engine-independent oracle for top-k (docs/semantics.md "Top-k").

expected = the first min(k, rows) rows of a numpy stable sort by, per order column, the tuple
(is-null, is-NaN, direction-adjusted value), then the row number: null after NaN after every
number in both directions, -0.0 == +0.0, ties to the lower row.  The direction-adjusted value is
the value's dense rank (np.unique), negated for descending, so no type's minimum overflows."""
import math

import numpy as np
import pyarrow as pa

from cylon_amd import Table
from cylon_amd._lib import C

D = 11  # kernels/topk.hip kTKDigitBits


def _plain(arr: pa.Array) -> pa.Array:
    """temporal -> its integer storage (full-range timestamps have no datetime)"""
    t = arr.type
    if pa.types.is_date32(t) or pa.types.is_time32(t):
        return arr.cast(pa.int32())
    if pa.types.is_temporal(t):
        return arr.cast(pa.int64())
    return arr


def _column_keys(col, asc):
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    arr = _plain(arr)
    isnull = np.asarray(arr.is_null().to_numpy(zero_copy_only=False), bool)
    if pa.types.is_string(arr.type) or pa.types.is_large_string(arr.type):
        vals = np.array(arr.fill_null("").to_pylist(), dtype=object)
        isnan = np.zeros(len(vals), bool)
    else:
        filled = arr.fill_null(0) if arr.null_count else arr  # before to_numpy: it turns null ints into NaN
        vals = np.array(filled.to_numpy(zero_copy_only=False))
        isnan = np.isnan(vals) if vals.dtype.kind == "f" else np.zeros(len(vals), bool)
        vals = np.where(isnan | isnull, vals.dtype.type(0), vals)
    _, rank = np.unique(vals, return_inverse=True)
    rank = rank.astype(np.int64)
    return isnull, isnan, rank if asc else -rank


def expected_rows(t: pa.Table, by, ascending, k: int) -> np.ndarray:
    by = [by] if isinstance(by, (str, int)) else list(by)
    asc = [ascending] * len(by) if isinstance(ascending, bool) else list(ascending)
    keys = [np.arange(t.num_rows)]  # np.lexsort: the LAST key is the primary one
    for name, a in reversed(list(zip(by, asc))):
        isnull, isnan, adj = _column_keys(t.column(name), a)
        keys += [adj, isnan, isnull]
    return np.lexsort(tuple(keys))[:max(0, k)]


def expected(t: pa.Table, by, ascending, k: int) -> pa.Table:
    return t.take(pa.array(expected_rows(t, by, ascending, k)))


def _cell(x):
    if isinstance(x, (float, np.floating)):
        return "nan" if x != x else repr(float(x))  # NaN equals NaN here; -0.0 differs from 0.0
    return x


def assert_same(got: pa.Table, exp: pa.Table):
    """Same columns, same rows, same ORDER, every column (payload included); nothing is re-sorted."""
    assert got.column_names == exp.column_names
    assert got.num_rows == exp.num_rows, (got.num_rows, exp.num_rows)
    for n in exp.column_names:
        g = [_cell(x) for x in _plain(got.column(n).combine_chunks()).to_pylist()]
        e = [_cell(x) for x in _plain(exp.column(n).combine_chunks()).to_pylist()]
        assert g == e, n


def traced(fn):
    """(result, trace counters of the call)"""
    C.trace_enable(True)
    C.trace_reset()
    try:
        out = fn()
        return out, dict(C.trace_counters())
    finally:
        C.trace_enable(False)


def check_topk(ctx, t: pa.Table, by, ascending, k, path="select"):
    """Table.topk on ctx against the oracle; asserts the path taken; returns the counters."""
    got, c = traced(lambda: Table(t, ctx).topk(k, by, ascending).to_arrow())
    print("topk", by, ascending, k, "rows", got.num_rows, c)
    assert_same(got, expected(t, by, ascending, k))
    if path == "select":
        assert c.get("topk.select", 0) == 1 and c.get("topk.sort_fallback", 0) == 0, c
        # the scan, one read per pass, the collect (none when every key is null)
        assert c["topk.key_reads"] in (c["topk.passes"] + 2, 1), c
    elif path == "fallback":
        assert c.get("topk.sort_fallback", 0) == 1 and c.get("topk.select", 0) == 0, c
    return c


def varying_bits(values: np.ndarray) -> int:
    """span of the bits that differ between the (non-negative integer) values"""
    v = values.astype(np.uint64)
    diff = int(np.bitwise_or.reduce(v)) ^ int(np.bitwise_and.reduce(v))
    return diff.bit_length() - ((diff & -diff).bit_length() - 1) if diff else 0


def max_passes(values: np.ndarray) -> int:
    return math.ceil(varying_bits(values) / D)


def clustered_int64(rng, n):
    """int64 keys spanning the full range whose k-th smallest lies in a dense cluster: INT64_MIN and
    INT64_MAX once each, everything else in [0, 2^20).  A D-bit pass over bits 63..53, 52..42, 41..31
    and 30..20 leaves the whole cluster in one bin, so a select of a row inside it needs several
    passes however small the candidate limit."""
    k = rng.integers(0, 1 << 20, n).astype(np.int64)
    k[n // 3] = np.iinfo(np.int64).min
    k[2 * n // 3] = np.iinfo(np.int64).max
    return k
