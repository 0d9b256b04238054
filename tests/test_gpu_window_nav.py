"""Navigation and distribution window functions on the MI355X: the fill scan (k_nav_fill_tile /
k_win_carry / k_nav_fill_apply), k_nav_pick, k_nav_rank_heads and k_nav_dist of kernels/window_nav.hip
behind ops/window.cpp.  Every case runs on a GPU context and on a CPU context and both are held to the
engine-independent oracle (window_nav_utils), in input row order; window.scan > 0 on the GPU shows that
the kernels ran (there is no other device path).

Shapes: wave (63 / 64 / 65), block (255 / 257), tile (T - 1 / T / T + 1, T = C.window_tile_rows()),
several tiles (3T + 11) and multi-block (100 003 rows) edges; partition layouts that put heads on tile
boundaries and runs of whole tiles inside one partition; null runs longer than two tiles; fill limits
that end on either side of a tile boundary and of a thread's 8 items; one case whose carry scan loops."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext
from cylon_amd._lib import C
from window_nav_utils import check_nav, expected

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
BIG = 100_003
SIZES = [1, 63, 64, 65, 255, 257, T - 1, T, T + 1, 3 * T + 11, BIG]
NAV = {"ff": ("ffill", "v"), "bf": ("bfill", "v"), "ffl": ("ffill", "v", 3), "bfl": ("bfill", "v", 2),
       "fv": ("first_value", "v"), "lv": ("last_value", "v"), "fvi": ("first_value", "v", True),
       "lvi": ("last_value", "v", True), "nk": ("nth_value", "v", 5)}
DIST = {"nt": ("ntile", 4), "nt7": ("ntile", 7), "pr": "percent_rank", "cd": "cume_dist"}


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, t, part, order, asc, funcs, step=0, scans=True):
    exp = expected(t, part, order, asc, funcs)  # once, for both contexts
    cg = check_nav(gpu, t, part, order, asc, funcs, step, exp=exp)
    cc = check_nav(cpu, t, part, order, asc, funcs, step, exp=exp)
    assert cg.get("window.scan", 0) == cc.get("window.scan", 0), (cg, cc)
    assert not scans or not t.num_rows or cg["window.scan"] > 0, cg
    for k in ("window.nav.fill", "window.nav.gather", "window.nav.skipped"):
        assert cg[k] == cc[k], (cg, cc)
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


def _table(layout, n, seed, nulls, peers=2):
    rng = np.random.default_rng(seed)
    ids = _partition_ids(layout, n, rng)
    p = rng.permutation(n)
    v = pa.array(rng.integers(-1000, 1000, n), mask=rng.random(n) < nulls)
    # o: the position inside the sorted order in runs of `peers` ties
    return pa.table({"g": ids[p].astype(np.int32), "o": (np.arange(n) // peers)[p], "v": v})


@pytest.mark.parametrize("nulls", [0.25, 0.9])
@pytest.mark.parametrize("layout", ["one", "each", "random", "tile_edges"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_layouts(gpu, cpu, n, layout, nulls):
    if layout == "tile_edges" and n < T:
        layout = "random"  # no tile boundary to put a head on
    t = _table(layout, n, n * 7 + len(layout), nulls)
    c = _both(gpu, cpu, t, "g", "o", True, NAV)
    assert c["window.nav.gather"] == 0, c
    if t["v"].null_count:  # the two rank scans and one fill scan each way
        assert c["window.scan"] == 4 and c["window.nav.fill"] == 2, c
    else:  # a tiny table that drew no null
        assert c["window.scan"] == 2 and c["window.nav.fill"] == 0, c


@pytest.mark.parametrize("layout", ["one", "random", "tile_edges"])
@pytest.mark.parametrize("n", SIZES)
def test_distribution_functions(gpu, cpu, n, layout):
    """runs of 700 peers: they cross tile boundaries, and partition heads fall inside them"""
    if layout == "tile_edges" and n < T:
        layout = "random"
    t = _table(layout, n, n * 11 + len(layout), 0.25, peers=700 if n > 700 else 3)
    for asc in (True, False):
        c = _both(gpu, cpu, t, "g", "o", asc, DIST)
        assert c["window.scan"] == 2 and c["window.nav.fill"] == 0, c


def test_null_runs_across_whole_tiles(gpu, cpu):
    """a null run longer than 2T inside one partition: the carry crosses whole-null tiles; then a
    partition head inside an all-null tile: the tile flag stops it.  Forwards and reversed."""
    n = 6 * T
    head = 4 * T + 100
    g = (np.arange(n) >= head).astype(np.int64)
    live = np.zeros(n, bool)
    live[[5, 5 * T + 50, n - 6]] = True  # tiles 1 .. 4 hold no value at all
    rng = np.random.default_rng(1)
    p = rng.permutation(n)
    t = pa.table({"g": g[p], "o": np.arange(n)[p], "v": pa.array(np.arange(n)[p] * 10, mask=~live[p])})
    f = {"ff": ("ffill", "v"), "bf": ("bfill", "v"), "lvi": ("last_value", "v", True), "fvi": ("first_value", "v", True)}
    for asc in (True, False):
        c = _both(gpu, cpu, t, "g", "o", asc, f)
        assert c["window.nav.fill"] == 2, c
    from cylon_amd import Table
    got = Table(t, gpu).window("g", "o", True, f).to_arrow()
    o = np.asarray(t["o"])
    ff, bf = np.array(got["ff"].to_pylist(), object), np.array(got["bf"].to_pylist(), object)
    inside = (o > 5) & (o < head)
    assert set(ff[inside]) == {50} and set(bf[inside]) == {None}  # filled across tiles 1 .. 4; nothing ahead
    stopped = (o >= head) & (o < 5 * T + 50)
    assert set(ff[stopped]) == {None} and set(bf[stopped]) == {(5 * T + 50) * 10}


def test_limits_at_tile_and_thread_boundaries(gpu, cpu):
    """gaps of exactly `limit` and of `limit + 1` nulls that straddle a tile boundary and the boundary
    between two threads' 8 items"""
    n = 2 * T + 40
    live = np.ones(n, bool)
    for first in (6, T - 2, 2 * T - 4):  # 5 nulls: 6 .. 10 (items 8 | 8), T - 2 .. T + 2, 2T - 4 .. 2T
        live[first:first + 5] = False
    rng = np.random.default_rng(2)
    p = rng.permutation(n)
    t = pa.table({"o": np.arange(n)[p], "v": pa.array(np.arange(n)[p], mask=~live[p])})
    f = {"f5": ("ffill", "v", 5), "f4": ("ffill", "v", 4), "b5": ("bfill", "v", 5), "b4": ("bfill", "v", 4)}
    _both(gpu, cpu, t, None, "o", True, f)
    _both(gpu, cpu, t, None, "o", False, f)
    from cylon_amd import Table
    got = Table(t, gpu).window(None, "o", True, f).to_arrow()
    assert got["f5"].null_count == 0 and got["b5"].null_count == 0
    o = np.asarray(t["o"])
    for name, miss in (("f4", (10, T + 2, 2 * T)), ("b4", (6, T - 2, 2 * T - 4))):
        assert sorted(o[np.flatnonzero(got[name].is_null().to_numpy(zero_copy_only=False))]) == list(miss)


def test_carry_scan_loops(gpu, cpu):
    """more tiles than one carry step covers: 49 tiles at 4 tiles per step, one partition across them all"""
    assert C.window_carry_tiles() >= 4 and -(-BIG // T) > 4
    t = _table("one", BIG, 3, 0.9)
    f = {"ff": ("ffill", "v"), "bf": ("bfill", "v", 20), "lvi": ("last_value", "v", True),
         "fvi": ("first_value", "v", True), "cd": "cume_dist"}
    c = _both(gpu, cpu, t, "g", "o", True, f, step=4)
    assert c["window.scan"] == 4, c


@pytest.mark.parametrize("dt", ["bool", "int8", "uint16", "float32", "int32", "int64", "float64", "string"])
def test_value_and_source_mode(gpu, cpu, dt):
    n = T + 300
    rng = np.random.default_rng(len(dt))
    if dt == "string":
        v = pa.array(["s%d" % x for x in rng.integers(0, 99, n)], mask=rng.random(n) < 0.3)
    elif dt == "bool":
        v = pa.array(rng.integers(0, 2, n).astype(bool), mask=rng.random(n) < 0.3)
    elif np.dtype(dt).kind == "f":
        x = (rng.integers(-4000, 4000, n) / 16).astype(dt)
        x[rng.random(n) < 0.1] = np.nan  # a value: copied, and it stops a fill
        x[rng.random(n) < 0.1] = -0.0
        v = pa.array(x, mask=rng.random(n) < 0.3)
    else:
        info = np.iinfo(dt)
        v = pa.array(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True), mask=rng.random(n) < 0.3)
    t = pa.table({"g": rng.integers(0, 5, n), "o": rng.integers(0, 99, n), "v": v})
    for name, spec in NAV.items():
        c = _both(gpu, cpu, t, "g", "o", False, {name: spec})
        assert c["window.nav.gather"] == (1 if dt == "string" else 0), (name, c)


def test_columns_without_nulls_run_no_fill_scan(gpu, cpu):
    n = T + 9
    rng = np.random.default_rng(4)
    t = pa.table({"g": rng.integers(0, 5, n), "o": rng.permutation(n), "v": rng.integers(0, 9, n),
                  "s": pa.array(["s%d" % x for x in rng.integers(0, 9, n)])})
    f = {"ff": ("ffill", "v"), "bf": ("bfill", "s", 2)}
    c = _both(gpu, cpu, t, "g", "o", True, f, scans=False)
    assert c["window.scan"] == 0 and c["window.nav.fill"] == 0 and c["window.nav.skipped"] == 2, c
    c = _both(gpu, cpu, t, "g", "o", True, dict(f, lvi=("last_value", "s", True), fv=("first_value", "v", True)))
    assert c["window.scan"] == 2 and c["window.nav.fill"] == 0 and c["window.nav.gather"] == 1, c
