"""Framed aggregates on the MI355X: kernels/rolling.hip behind ops/window.cpp.  Every case runs on a GPU
context and on a CPU context and both are held to the engine-independent oracle (rolling_utils), in
input row order; the counters window.frame.lds / window.frame.wide show which path ran.

Shapes: wave (63 / 64 / 65), block (255 / 257), tile (T - 1 / T / T + 1, T = C.window_tile_rows()) and
multi-block (100 003 rows) edges; frames around the tile and around L = C.window_frame_lds_rows(),
where the path switches; unbounded frames; partition heads on tile edges."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from cylon_amd._lib import C
from rolling_utils import check_rolling, expected

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
L = C.window_frame_lds_rows()
BIG = 100_003
SIZES = [1, 63, 64, 65, 255, 257, T - 1, T, T + 1, BIG]


def five(v, p, f, minp=1):
    return {"c": ("rolling_count", v, p, f), "s": ("rolling_sum", v, p, f, minp), "m": ("rolling_mean", v, p, f, minp),
            "lo": ("rolling_min", v, p, f, minp), "hi": ("rolling_max", v, p, f, minp)}


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, t, part, order, asc, funcs):
    exp = expected(t, part, order, asc, funcs)  # once, for both contexts
    cg = check_rolling(gpu, t, part, order, asc, funcs, exp=exp, lds_rows=L)
    check_rolling(cpu, t, part, order, asc, funcs, exp=exp, lds_rows=L)
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
    if layout == "long":  # partitions longer than a tile among short ones
        sizes = rng.choice([1, 2, 70, 600, T + T // 2], n)
        return np.repeat(np.arange(n), sizes)[:n].astype(np.int64)
    if layout == "tile_edges":
        # heads at a tile's first row (T), at a tile's last row (2T - 1), a partition that ends a tile
        # (the one before 3T), and every tile after 3T + 5 wholly inside one partition until a head in
        # the last tile
        heads = [h for h in (T, 2 * T - 1, 3 * T, 3 * T + 5, n - 7) if 0 < h < n]
        ids = np.zeros(n, np.int64)
        for h in heads:
            ids[h:] += 1
        return ids
    raise ValueError(layout)


def _table(layout, n, seed, nullable=False, values=None):
    rng = np.random.default_rng(seed)
    ids = _partition_ids(layout, n, rng)
    p = rng.permutation(n)
    v = rng.integers(-1000, 1000, n) if values is None else values(rng, n)
    val = pa.array(v, mask=rng.random(n) < 0.25) if nullable else pa.array(v)
    # o: the position inside the sorted order with a few ties
    return pa.table({"g": ids[p].astype(np.int32), "o": (np.arange(n) // 2)[p], "v": val})


@pytest.mark.parametrize("layout", ["one", "each", "random", "tile_edges"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_layouts(gpu, cpu, n, layout):
    if layout == "tile_edges" and n < T:
        layout = "random"  # no tile boundary to put a head on
    t = _table(layout, n, n * 7 + len(layout), nullable=n % 2 == 1)
    f = five("v", 2, 3)
    f.update(lo=("rolling_min", "v", 64, 64), hi=("rolling_max", "v", 0, 70))
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.frame.lds"] == 5 and "window.frame.wide" not in c, c


def _split(w):
    """w rows split unevenly between preceding and following"""
    return ((w - 1) // 3, w - 1 - (w - 1) // 3)


FRAMES = [(0, 0), (1, 0), (0, 1), (2, 3), (63, 0), (64, 64), _split(T - 1), _split(T), _split(T + 1),
          _split(L - 1), _split(L), _split(L + 1), (L - 1, 0), (0, L), (None, 0), (0, None), (None, None),
          ("n+5", 2)]


@pytest.mark.parametrize("frame", FRAMES, ids=str)
def test_frames(gpu, cpu, frame):
    n = 3 * T + 11
    p, f = (n + 5 if x == "n+5" else x for x in frame)
    t = _table("long", n, 11, nullable=True)
    c = _both(gpu, cpu, t, "g", "o", True, five("v", p, f))
    w = min(n if p is None else p, n) + min(n if f is None else f, n) + 1
    assert c.get("window.frame.lds" if w <= L else "window.frame.wide") == 5, (w, c)
    one = _table("one", T + 300, 12, nullable=True)  # and one partition longer than every bounded frame but T's
    _both(gpu, cpu, one, "g", "o", False, {"s": ("rolling_sum", "v", p, f), "hi": ("rolling_max", "v", p, f)})


@pytest.mark.parametrize("layout", ["each", "random"])
def test_frames_wider_than_every_partition(gpu, cpu, layout):
    """partitions of length 1 and of at most 200 rows under frames of 301, L + 88 and all rows"""
    t = _table(layout, 2 * T + 5, 13, nullable=True)
    f = dict(five("v", 200, 100), ws=("rolling_sum", "v", L, 87), wl=("rolling_min", "v", 300, L),
             a=("rolling_mean", "v", None, None))
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.frame.lds"] == 5 and c["window.frame.wide"] == 3, c


@pytest.mark.parametrize("frame", [(5, 5), (0, 9), (9, 0), (300, 200), (L, L)])
def test_partition_heads_on_tile_edges(gpu, cpu, frame):
    """a head on the first and on the last position of a tile, with a frame reaching across it"""
    t = _table("tile_edges", 4 * T + 100, 14, nullable=True)
    _both(gpu, cpu, t, "g", "o", True, five("v", *frame))


@pytest.mark.parametrize("frame", [(2, 3), (40, 0), (400, 300)])
def test_min_periods(gpu, cpu, frame):
    w = frame[0] + frame[1] + 1
    t = _table("random", T + 500, 15, nullable=True)
    for minp in (1, 2, w):
        _both(gpu, cpu, t, "g", "o", True, five("v", frame[0], frame[1], minp))


def test_all_null_column_and_leading_nulls_across_a_tile_boundary(gpu, cpu):
    n = 3 * T + 11
    rng = np.random.default_rng(16)
    ids = np.repeat(np.arange(8), -(-n // 8))[:n]
    pos = np.arange(n) - np.searchsorted(ids, ids)  # position inside the partition
    lead = np.array([0, 1, 5, 64, 300, T // 2, 700, 3])[ids]
    mask = pos < lead
    mask[: T + 9] = True  # the whole first tile and a little more
    p = rng.permutation(n)
    for m in (mask, np.ones(n, bool)):
        t = pa.table({"g": ids[p], "o": pos[p], "v": pa.array(rng.integers(-500, 500, n)[p], mask=m[p])})
        for frame in ((3, 0), (0, 7), (600, 100), (None, 0)):
            _both(gpu, cpu, t, "g", "o", True, five("v", frame[0], frame[1], 2))
    got = Table(t, gpu).window("g", "o", True, five("v", 3, 3)).to_arrow()
    assert got["s"].null_count == n and got["c"].null_count == 0 and set(got["c"].to_pylist()) == {0}


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_float_columns(gpu, cpu, dt):
    t = _table("random", T + 300, 17, nullable=True,
               values=lambda rng, n: (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)).astype(dt))
    for frame in ((0, 0), (6, 0), (100, 100), (700, 0), (None, None)):
        _both(gpu, cpu, t, "g", "o", True, five("v", *frame))


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_large_partition_before_a_small_one(gpu, cpu, dt):
    """values near 1e16 sort immediately before a partition near 1: no digit of the second is lost"""
    rng = np.random.default_rng(18)
    nb, ns = T + T // 2, 900
    g = np.concatenate([np.zeros(nb, np.int64), np.ones(ns, np.int64)])
    v = np.concatenate([1e16 * (1 + rng.random(nb)), 1 + rng.random(ns)]).astype(dt)
    p = rng.permutation(nb + ns)
    t = pa.table({"g": g[p], "o": rng.permutation(nb + ns), "v": v[p]})
    for frame in ((6, 0), (3, 3), (250, 250), (1000, 0), (None, 0), (None, None)):
        _both(gpu, cpu, t, "g", "o", True, {"s": ("rolling_sum", "v", *frame), "m": ("rolling_mean", "v", *frame)})


def test_nan_and_inf_touch_only_their_frames(gpu, cpu):
    n = 2 * T + 99
    rng = np.random.default_rng(19)
    v = rng.standard_normal(n)
    v[T - 3], v[T + 700] = np.nan, np.inf  # sorted positions, in the one long partition
    p = rng.permutation(n)
    t = pa.table({"g": np.zeros(n, np.int8), "o": np.arange(n)[p], "v": v[p]})
    for frame in ((6, 0), (2, 5), (300, 300), (0, 600)):
        f = {"s": ("rolling_sum", "v", *frame), "m": ("rolling_mean", "v", *frame), "hi": ("rolling_max", "v", *frame)}
        _both(gpu, cpu, t, "g", "o", True, f)
        got = np.array(Table(t, gpu).window("g", "o", True, f).to_arrow()["s"].to_pylist())[np.argsort(p)]
        i = np.arange(n)
        has_nan = (i - frame[0] <= T - 3) & (T - 3 <= i + frame[1])
        has_inf = (i - frame[0] <= T + 700) & (T + 700 <= i + frame[1])
        assert (np.isnan(got) == has_nan).all() and (np.isinf(got) == (has_inf & ~has_nan)).all()


def test_mixed_with_ranking_running_and_shift_specs(gpu, cpu):
    t = _table("long", 2 * T + 77, 20, nullable=True)
    f = {"rn": "row_number", "r7": ("rolling_sum", "v", 6, 0), "cs": ("cumsum", "v"), "prev": ("lag", "v", 1),
         "wide": ("rolling_max", "v", 400, 400), "cnt": ("rolling_count", "v", 1, 1)}
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.frame.lds"] == 2 and c["window.frame.wide"] == 1 and c["window.sort"] == 1, c
    for ctx in (gpu, cpu):
        all_ = Table(t, ctx).window("g", "o", True, f).to_arrow()
        for name, spec in f.items():
            alone = Table(t, ctx).window("g", "o", True, {name: spec}).to_arrow()
            assert alone[name].equals(all_[name]), name


@pytest.mark.parametrize("dt", ["int8", "uint16", "int32", "uint64"])
def test_integer_widths_and_wrapping_sums(gpu, cpu, dt):
    dt = np.dtype(dt)
    info = np.iinfo(dt)
    t = _table("random", T + 300, 21 + dt.itemsize, nullable=True,
               values=lambda rng, n: rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))
    for frame in ((2, 3), (300, 300), (None, None)):
        f = five("v", *frame)
        del f["m"]
        _both(gpu, cpu, t, "g", "o", False, f)
