"""Window functions on the MI355X: the three-phase segmented scans of kernels/window.hip (k_win_tile /
k_win_carry / k_win_apply, the rank scan, k_win_shift) behind ops/window.cpp.  Every case runs on a GPU
context and on a CPU context and both are held to the engine-independent oracle (window_utils), in
input row order; window.scan > 0 on the GPU shows that the kernels ran (there is no other device path).

Shapes: wave (63 / 64 / 65), block (255 / 257), tile (T - 1 / T / T + 1, T = C.window_tile_rows()) and
multi-block (100 003 rows) edges; partition layouts that put heads on tile boundaries and runs of
whole tiles inside one partition; one case whose carry scan loops (the step lowered through the
binding's test-only argument)."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from window_utils import assert_window, check_window, expected, run_window

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
BIG = 100_003
SIZES = [1, 63, 64, 65, 255, 257, T - 1, T, T + 1, BIG]
FUNCS = {"rn": "row_number", "rk": "rank", "dr": "dense_rank", "cnt": ("cumcount", "v"), "s": ("cumsum", "v"),
         "lo": ("cummin", "v"), "hi": ("cummax", "v"), "prev": ("lag", "v", 1), "nxt": ("lead", "v", 3)}


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, t, part, order, asc, funcs, step=0):
    exp = expected(t, part, order, asc, funcs)  # once, for both contexts
    cg = check_window(gpu, t, part, order, asc, funcs, step, exp=exp)
    cc = check_window(cpu, t, part, order, asc, funcs, step, exp=exp)
    assert cg.get("window.scan", 0) == cc.get("window.scan", 0) and (not t.num_rows or cg["window.scan"] > 0), (cg, cc)
    return cg


def _partition_ids(layout, n, rng):
    """a partition id per row, non-decreasing (the rows are shuffled afterwards)"""
    if layout == "one":
        return np.zeros(n, np.int64)
    if layout == "each":
        return np.arange(n, dtype=np.int64)
    if layout == "random":
        sizes = rng.integers(1, 201, n)
        return np.repeat(np.arange(n), sizes)[:n].astype(np.int64)
    if layout == "tile_edges":
        # heads at a tile's first row (T), at a tile's last row (2T - 1), a partition that ends a tile
        # (the one before 3T), and every tile after 3T + 5 wholly inside one partition until a head in
        # the last tile: the tile pair's flag must stop that carry
        heads = [h for h in (T, 2 * T - 1, 3 * T, 3 * T + 5, n - 7) if 0 < h < n]
        ids = np.zeros(n, np.int64)
        for h in heads:
            ids[h:] += 1
        return ids
    raise ValueError(layout)


def _table(layout, n, seed, nullable=False):
    rng = np.random.default_rng(seed)
    ids = _partition_ids(layout, n, rng)
    p = rng.permutation(n)
    v = rng.integers(-1000, 1000, n)
    val = pa.array(v, mask=rng.random(n) < 0.25) if nullable else pa.array(v)
    # o: the position inside the sorted order with a few ties, so that peers exist
    return pa.table({"g": ids[p].astype(np.int32), "o": (np.arange(n) // 2)[p], "v": val})


@pytest.mark.parametrize("layout", ["one", "each", "random", "tile_edges"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_layouts(gpu, cpu, n, layout):
    if layout == "tile_edges" and n < T:
        layout = "random"  # no tile boundary to put a head on
    t = _table(layout, n, n * 7 + len(layout), nullable=n % 2 == 1)
    c = _both(gpu, cpu, t, "g", "o", True, FUNCS)
    assert c["window.tiles"] == c["window.scan"] * -(-n // T), c


def test_carry_scan_loops(gpu, cpu):
    """more tiles than one carry step covers: 49 tiles at 4 tiles per step, one partition across them
    all, then partitions of a tile and a half"""
    assert C.window_carry_tiles() >= 4
    n = BIG
    rng = np.random.default_rng(1)
    f = {"rn": "row_number", "s": ("cumsum", "v")}
    for ids in (np.zeros(n, np.int64), np.arange(n) // (T + T // 2)):
        p = rng.permutation(n)
        t = pa.table({"g": ids[p].astype(np.int32), "v": rng.integers(-(1 << 40), 1 << 40, n)})
        c = _both(gpu, cpu, t, "g", None, True, f, step=4)
        assert c["window.tiles"] == 2 * -(-n // T), c
        assert -(-n // T) > 4


def test_leading_nulls_keep_the_carry_empty(gpu, cpu):
    """the first rows of every partition are null, across a tile boundary for the long ones: nothing
    seen yet, so CUMMIN / CUMMAX stay null and the sums start at the first value"""
    n = 3 * T + 11
    rng = np.random.default_rng(2)
    ids = np.repeat(np.arange(8), -(-n // 8))[:n]
    pos = np.arange(n) - np.searchsorted(ids, ids)  # position inside the partition
    lead = np.array([0, 1, 5, 64, 300, T // 2, 700, 3])[ids]
    mask = pos < lead
    mask[: T + 9] = True  # the whole first tile and a little more
    for dt in (np.int64, np.float64):
        v = rng.integers(-500, 500, n).astype(dt)
        p = rng.permutation(n)
        t = pa.table({"g": ids[p], "o": pos[p], "v": pa.array(v[p], mask=mask[p])})
        _both(gpu, cpu, t, "g", "o", True, FUNCS)
        got = Table(t, gpu).window("g", "o", True, {"lo": ("cummin", "v"), "hi": ("cummax", "v")}).to_arrow()
        nulls = np.flatnonzero(mask[p])
        assert got["lo"].null_count == len(nulls) and got["hi"].null_count == len(nulls)


@pytest.mark.parametrize("dt", ["int8", "uint8", "int16", "int32", "uint32", "float32", "int64", "uint64", "float64"])
def test_value_widths(gpu, cpu, dt):
    n = T + 300
    rng = np.random.default_rng(len(dt))
    dt = np.dtype(dt)
    if dt.kind == "f":
        v = (rng.integers(-4000, 4000, n) / 16).astype(dt)
    else:
        v = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
    t = pa.table({"g": rng.integers(0, 5, n), "o": rng.integers(0, 99, n), "v": pa.array(v, mask=rng.random(n) < 0.2)})
    _both(gpu, cpu, t, "g", "o", False, FUNCS)


def test_nan_and_string_keys(gpu, cpu):
    n = T + 77
    rng = np.random.default_rng(3)
    o = rng.integers(0, 50, n).astype(np.float64)
    o[rng.random(n) < 0.1] = np.nan
    v = rng.standard_normal(n)
    v[rng.random(n) < 0.05] = np.nan
    t = pa.table({"s": pa.array([None if x == 0 else "k%d" % x for x in rng.integers(0, 9, n)]),
                  "o": pa.array(o, mask=rng.random(n) < 0.1), "i": rng.integers(0, 4, n),
                  "v": pa.array(v, mask=rng.random(n) < 0.1)})
    f = {"rn": "row_number", "rk": "rank", "dr": "dense_rank", "cnt": ("cumcount", "s"), "lo": ("cummin", "v"),
         "hi": ("cummax", "v"), "ps": ("lag", "s", 2), "si": ("cumsum", "i")}
    _both(gpu, cpu, t, "s", ["o", "i"], [False, True], f)
    _both(gpu, cpu, t, ["s", "i"], "o", True, f)


def test_sliced_column_starts_off_a_16_byte_boundary(gpu, cpu):
    n = T + 5
    rng = np.random.default_rng(4)
    t = pa.table({"g": rng.integers(0, 3, n + 3).astype(np.int32), "o": rng.integers(0, 500, n + 3),
                  "v": pa.array(rng.integers(-9, 9, n + 3), mask=rng.random(n + 3) < 0.2)})
    want = t.slice(3, n)
    for ctx in (gpu, cpu):
        got, c = run_window(ctx, want, "g", "o", True, FUNCS, table=Table(t, ctx).slice(3, n))
        assert_window(got, want, "g", "o", True, FUNCS)
        assert c["window.scan"] == 5, c


def test_float_cumsum_exact_and_under_cancellation(gpu, cpu):
    n = 2 * T + 99
    rng = np.random.default_rng(5)
    t = pa.table({"g": rng.integers(0, 3, n), "o": rng.permutation(n),
                  "v": rng.integers(0, 1 << 30, n).astype(np.float64)})  # every prefix < 2^53: exact in any order
    f = {"s": ("cumsum", "v")}
    want = [float(e[0]) for e in expected(t, "g", "o", True, f)["s"]]
    for ctx in (gpu, cpu):
        assert Table(t, ctx).window("g", "o", True, f).to_arrow()["s"].to_pylist() == want
    # a partition near 1e16 that spans more than a tile sorts immediately before a partition near 1
    nb, ns = T + T // 2, 900
    g = np.concatenate([np.zeros(nb, np.int64), np.ones(ns, np.int64)])
    v = np.concatenate([1e16 * (1 + rng.random(nb)), 1 + rng.random(ns)])
    p = rng.permutation(nb + ns)
    c = pa.table({"g": g[p], "o": rng.permutation(nb + ns), "v": v[p]})
    _both(gpu, cpu, c, "g", "o", True, f)
    w = pa.table({"g": c["g"], "o": c["o"], "w": pa.array(v[p].astype(np.float32))})
    _both(gpu, cpu, w, "g", "o", True, {"s": ("cumsum", "w")})


def _dist(ctx):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    g = _global()
    local = g.take(pa.array(np.arange(rank, g.num_rows, world)))
    C.trace_enable(True)
    C.trace_reset()
    out = Table(local, ctx).distributed_window("g", "o", True, DIST_FUNCS).to_arrow()
    return out, dict(C.trace_counters())


def _global():
    n = 3 * T + 17
    rng = np.random.default_rng(6)
    return pa.table({"g": rng.integers(0, 25, n), "o": rng.permutation(n),
                     "v": pa.array(rng.integers(-99, 99, n), mask=rng.random(n) < 0.1), "row": np.arange(n)})


DIST_FUNCS = {"rn": "row_number", "dr": "dense_rank", "s": ("cumsum", "v"), "hi": ("cummax", "v"),
              "p": ("lead", "v", 1)}


def test_distributed_window_on_device():
    res = run_distributed(_dist, 2, device="cuda:0")
    g = _global()
    on = [set(r[0]["g"].to_pylist()) for r in res]  # every partition on one rank
    assert on[0].isdisjoint(on[1])
    assert all(r[1].get("window.scan", 0) == 3 for r in res), [r[1] for r in res]
    assert_window(pa.concat_tables([r[0] for r in res]), g, "g", "o", True, DIST_FUNCS, row_id="row")
