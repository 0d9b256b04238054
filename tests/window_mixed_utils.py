"""One window call with a spec of every family (ranking, running, shift, rolling on both paths, range,
pick, fill, dist, moment over ROWS and RANGE frames): the specs of a call must not affect one another.

Every output column of the mixed call, in four spec orders, is held bit for bit to the same column of a
call with that spec alone -- the specs share the sort, the flags, the rank scans, the dense values of a
column (gathered by whichever spec comes first), the RANGE bounds and the fill scans, and none of that
sharing may show in a result.  The trace counters of the mixed call do not depend on the order either.

Shapes: n in {1, 9, T + 1, 2 T + 77}, T = C.window_tile_rows(): a one-row table, one 8-block plus one,
a tile boundary, and a carry across more than one tile."""
import numpy as np
import pyarrow as pa

from cylon_amd import Table
from cylon_amd._lib import C
from window_utils import traced

T = C.window_tile_rows()
L = C.window_frame_lds_rows()
SIZES = {"1": 1, "9": 9, "T+1": T + 1, "2T+77": 2 * T + 77}

SPECS = {
    "rn": "row_number", "rk": "rank", "dr": "dense_rank",
    "cc": ("cumcount", "v"), "cs": ("cumsum", "v"), "cmin": ("cummin", "w"), "cmax": ("cummax", "v"),
    "lag": ("lag", "v", 2), "lead": ("lead", "s", 1),
    "rsum": ("rolling_sum", "v", 3, 0), "rcnt": ("rolling_count", "w", 1, 1),  # the LDS path
    "rmax": ("rolling_max", "v", L, L),                                        # the wide path
    "gsum": ("range_sum", "v", 2, 3), "gcnt": ("range_count", "v", 2, 3), "gmin": ("range_min", "w", None, 0),
    "fv": ("first_value", "v", True), "lv": ("last_value", "s"), "nth": ("nth_value", "v", 3),
    "ff": ("ffill", "v"), "bf": ("bfill", "v", 2), "ffs": ("ffill", "s"), "ffw": ("ffill", "w"),  # ffw: skipped
    "nt": ("ntile", 4), "pr": "percent_rank", "cd": "cume_dist",
    "rstd": ("rolling_std", "v", 3, 0),
    "gvar": ("range_var", "v", 2, 3),  # the bounds of gsum
}

# The window.* trace counters of the mixed call, copied from what the commit before the split of
# ops/window.cpp printed for each n (the same on both devices and in every spec order): the split code
# has to reproduce them.  At n = 1 and 9 the frame of rmax is cut to the table's rows and fits the LDS path.
_SHARED = {"window.sort": 1, "window.frame.moment": 2, "window.frame.range": 3, "window.moment.pyramids": 1,
           "window.range.bounds": 2}
_NULLS = dict(_SHARED, **{"window.nav.fill": 3, "window.nav.gather": 2, "window.nav.skipped": 1,
                          "window.range.pyramids": 3, "window.scan": 17})
COUNTERS = {
    # one row: no null in any column, so every fill is skipped and no count pyramid is built
    "1": dict(_SHARED, **{"window.frame.lds": 3, "window.nav.fill": 0, "window.nav.gather": 1, "window.nav.skipped": 4,
                          "window.range.pyramids": 2, "window.scan": 14, "window.tiles": 14}),
    "9": dict(_NULLS, **{"window.frame.lds": 3, "window.tiles": 17}),
    "T+1": dict(_NULLS, **{"window.frame.lds": 2, "window.frame.wide": 1, "window.tiles": 34}),
    "2T+77": dict(_NULLS, **{"window.frame.lds": 2, "window.frame.wide": 1, "window.tiles": 51}),
}


def make_table(n, seed=0):
    """g: int32 partitions of 1 .. 200 rows (they straddle the 8-blocks), o: int64 order key with ties of 2,
    v: float64 with 25 % nulls, w: int32 without nulls, s: string with nulls; rows shuffled"""
    rng = np.random.default_rng(seed + n)
    sizes = rng.integers(1, 201, n)
    k = int(np.searchsorted(np.cumsum(sizes), n)) + 1  # the partitions that the first n rows fall into
    ids = np.repeat(np.arange(k), sizes[:k])[:n]
    p = rng.permutation(n)
    v = 1e3 * rng.standard_normal(n)
    w = rng.integers(-1000, 1000, n).astype(np.int32)
    s = np.array(["s%d" % x for x in rng.integers(0, 50, n)], dtype=object)
    return pa.table({"g": ids[p].astype(np.int32), "o": (np.arange(n, dtype=np.int64) // 2)[p],
                     "v": pa.array(v[p], mask=(rng.random(n) < 0.25)[p]), "w": w[p],
                     "s": pa.array(s[p], mask=(rng.random(n) < 0.25)[p])})


def orders():
    """(label, spec names): as given, reversed, two seeded shuffles"""
    names = list(SPECS)
    out = [("given", names), ("reversed", names[::-1])]
    for seed in (1, 2):
        out.append(("shuffle%d" % seed, [names[i] for i in np.random.default_rng(seed).permutation(len(names))]))
    return out


def run(ctx, table, names):
    """(arrow result, window.* counters) of one call with the named specs"""
    got, c = traced(lambda: table.window("g", "o", True, {k: SPECS[k] for k in names}).to_arrow())
    return got, {k: v for k, v in c.items() if k.startswith("window.")}


def image(col):
    """(validity, the valid cells as raw bits): NaNs compare equal, -0.0 and 0.0 do not"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    valid = np.asarray(col.is_valid())
    if pa.types.is_string(col.type) or pa.types.is_large_string(col.type):
        cells = np.array([x for x in col.to_pylist() if x is not None], dtype=object)
        return valid, cells
    width = col.type.bit_width // 8
    raw = np.frombuffer(col.buffers()[1], dtype="u%d" % width, count=len(col) + col.offset)[col.offset:]
    return valid, raw[valid]


def same_bits(a, b):
    (va, ca), (vb, cb) = image(a), image(b)
    return a.type == b.type and np.array_equal(va, vb) and np.array_equal(ca, cb)


_alone = {}


def alone(ctx, key, table):
    """spec name -> its column from a call with that spec alone; computed once per (device, size)"""
    if key not in _alone:
        _alone[key] = {k: run(ctx, table, [k])[0].column(k) for k in SPECS}
    return _alone[key]


def check_mixed(ctx, device, size):
    """the assertions of the module docstring on one context and one size; returns the counters"""
    arrow = make_table(SIZES[size])
    table = Table(arrow, ctx)
    ref = alone(ctx, (device, size), table)
    counters = {}
    for label, names in orders():
        got, c = run(ctx, table, names)
        assert got.column_names == arrow.column_names + names, (label, got.column_names)
        for k in names:
            assert same_bits(got.column(k), ref[k]), "%s, n = %s, %s order: %s differs from the spec alone" % (
                device, size, label, k)
        counters[label] = c
    print("window_mixed counters", device, size, counters["given"])
    for label, c in counters.items():
        assert c == counters["given"], (device, size, label, c, counters["given"])
    assert counters["given"] == COUNTERS[size], (device, size, counters["given"], COUNTERS[size])
    return counters["given"]
