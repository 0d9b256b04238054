"""RANGE frames on the MI355X: kernels/frame_range.hip behind ops/window.cpp.  Every case runs on a GPU
context and on a CPU context and both are held to the engine-independent oracle (range_frame_utils), in
input row order.

Shapes: the edges of pyramid levels 1 - 5 (8, 64, 512, 4096 rows; 100 003 rows reach level 5) and of the
tile T = C.window_tile_rows().  The order key is mostly the sorted position itself (optionally with
ties), so an offset is a frame length: single rows, runs inside one 8-block, block-aligned frames, two
adjacent blocks, frames that climb every level, frames that reach further than the H =
C.window_range_halo() keys staged beside a tile (the bound is then found in global memory), and whole
partitions."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from cylon_amd._lib import C
from range_frame_utils import check_range, expected

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
H = C.window_range_halo()
R = C.window_range_radix()
BIG = 100_003
SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, T - 1, T, T + 1, 4095, 4096, 4097]


def five(v, p, f, minp=1):
    return {"c": ("range_count", v, p, f), "s": ("range_sum", v, p, f, minp), "m": ("range_mean", v, p, f, minp),
            "lo": ("range_min", v, p, f, minp), "hi": ("range_max", v, p, f, minp)}


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, t, part, order, asc, funcs):
    exp = expected(t, part, order, asc, funcs)  # once, for both contexts
    cg = check_range(gpu, t, part, order, asc, funcs, exp=exp)
    check_range(cpu, t, part, order, asc, funcs, exp=exp)
    return cg


def _partition_ids(layout, n, rng):
    """a partition id per sorted position, non-decreasing"""
    if layout == "one":
        return np.zeros(n, np.int64)
    if layout == "each":
        return np.arange(n, dtype=np.int64)
    if layout == "random":
        sizes = rng.integers(1, 201, n)
        return np.repeat(np.arange(n), sizes)[:n].astype(np.int64)
    if layout == "long":  # partitions longer than a tile and its halos among short ones
        sizes = rng.choice([1, 2, 70, 600, T + T // 2, 2 * T + 2 * H + 50], n)
        return np.repeat(np.arange(n), sizes)[:n].astype(np.int64)
    if layout == "tile_edges":  # heads on a tile's first and last row, and just inside the last tile
        heads = [h for h in (T, 2 * T - 1, 3 * T, 3 * T + 5, n - 7) if 0 < h < n]
        ids = np.zeros(n, np.int64)
        for h in heads:
            ids[h:] += 1
        return ids
    raise ValueError(layout)


def _table(layout, n, seed, nullable=False, ties=1, key=None, values=None):
    """rows shuffled; o = the sorted position // ties unless key(rng, n) gives the keys in sorted order"""
    rng = np.random.default_rng(seed)
    ids = _partition_ids(layout, n, rng)
    p = rng.permutation(n)
    v = rng.integers(-1000, 1000, n) if values is None else values(rng, n)
    val = pa.array(v, mask=rng.random(n) < 0.25) if nullable else pa.array(v)
    o = np.arange(n, dtype=np.int64) // ties if key is None else key(rng, n)
    o = o.take(pa.array(p)) if isinstance(o, pa.Array) else pa.array(o[p])
    return pa.table({"g": ids[p].astype(np.int32), "o": o, "v": val})


@pytest.mark.parametrize("layout", ["one", "each", "random", "tile_edges"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_layouts(gpu, cpu, n, layout):
    if layout == "tile_edges" and n <= T:
        layout = "random"  # no tile boundary to put a head on
    t = _table(layout, n, n * 7 + len(layout), nullable=n % 2 == 1)
    f = five("v", 2, 3)  # inside one block or across two
    f.update(one=("range_sum", "v", 0, 0), mn=("range_min", "v", 64, 64), mx=("range_max", "v", 0, 70),
             far=("range_sum", "v", H + 500, H + 77), all=("range_mean", "v", None, None))
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.range.bounds"] == 6 and c["window.frame.range"] == 10, c


# unique keys in one partition: (a, b) is the frame [i - a, i + b]
FRAMES = [(0, 0), (1, 0), (0, 1), (3, 4), (7, 0), (0, 7), (8, 8), (63, 64), (64, 0), (511, 0), (0, 512), (513, 513),
          (H - 1, H - 1), (H, H), (H + 1, H + 1), (T + H + 5, 0), (0, T + H + 5), (4096, 4095), (None, 0), (0, None),
          (None, None), (10 ** 12, 2)]


@pytest.mark.parametrize("frame", FRAMES, ids=str)
def test_frames(gpu, cpu, frame):
    n = 3 * T + 11
    t = _table("long", n, 11, nullable=True)
    _both(gpu, cpu, t, "g", "o", True, five("v", *frame))
    one = _table("one", 2 * T + 2 * H + 300, 12, nullable=True)  # a partition longer than every staged window
    _both(gpu, cpu, one, "g", "o", False, {"s": ("range_sum", "v", *frame), "hi": ("range_max", "v", *frame)})


@pytest.mark.parametrize("ties", [R, 64, 700, T + 2 * H + 100])
def test_runs_of_ties(gpu, cpu, ties):
    """ties of 8 in one partition are whole blocks: (0, 0) is one aligned block, (1, 0) two adjacent ones,
    (1, 1) three; the longer runs cross tile edges, the longest every staged window"""
    n = 3 * T + 11
    t = _table("one", n, 13 + ties, nullable=True, ties=ties)
    f = {"b1": ("range_sum", "v", 0, 0), "b2": ("range_sum", "v", 1, 0), "b3": ("range_min", "v", 1, 1),
         "c": ("range_count", "v", 0, 0), "m": ("range_mean", "v", 0, 2)}
    _both(gpu, cpu, t, "g", "o", True, f)
    if ties == R:
        got = Table(t, gpu).window("g", "o", True, {"n": ("range_count", "g", 0, 0)}).to_arrow()["n"].to_pylist()
        assert set(got) == {R, n % R}
    _both(gpu, cpu, _table("random", n, 14 + ties, ties=ties), "g", "o", False, f)


@pytest.mark.parametrize("n,frame", [(BIG, (40_000, 300)), (BIG, (None, None)), (BIG, (5, 33_000))], ids=str)
def test_every_pyramid_level(gpu, cpu, n, frame):
    """100 003 rows in one partition: levels of 12 501, 1 563, 196, 25 and 4 entries"""
    t = _table("one", n, 15, nullable=True)
    f = {"s": ("range_sum", "v", *frame), "lo": ("range_min", "v", *frame), "c": ("range_count", "v", *frame)}
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.range.pyramids"] == 3 and c["window.range.bounds"] == 1, c


def _tailed_keys(numbers, nans, nulls):
    def key(rng, n):
        k = np.sort(rng.integers(-300, 300, n) / 4.0)
        k[n - nans - nulls:] = np.nan
        mask = np.zeros(n, bool)
        mask[n - nulls:] = True
        assert numbers + nans + nulls == n
        return pa.array(k, mask=mask)
    return key


@pytest.mark.parametrize("asc", [True, False])
def test_nan_and_null_key_tails_across_a_tile_edge(gpu, cpu, asc):
    n = T + 600
    for numbers, nans in ((T - 40, 65), (T - 1, 1), (T, 300), (5, T + 20)):
        nulls = n - numbers - nans
        t = _table("one", n, 16, nullable=True, key=_tailed_keys(numbers, nans, nulls))
        for frame in ((1.5, 0.25), (0, None), (None, 2), (float("inf"), 0.0)):
            _both(gpu, cpu, t, "g", "o", asc, five("v", *frame))


def _float_keys(dt):
    def key(rng, n):
        k = np.sort(rng.integers(-4 * n, 4 * n, n) / 8.0).astype(dt)
        k[:3], k[-3:] = -np.inf, np.inf
        k[n // 2: n // 2 + 2] = [-0.0, 0.0]
        return np.sort(k)
    return key


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_float_keys_and_values(gpu, cpu, dt, asc):
    t = _table("random", T + 300, 17, nullable=True, key=_float_keys(dt),
               values=lambda rng, n: (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)).astype(dt))
    for frame in ((0.0, 0.0), (0.125, 3), (2, 0.7), (float("inf"), 1.0), (1e300, float("inf")), (None, 0.5)):
        _both(gpu, cpu, t, "g", "o", asc, five("v", *frame))


def _extreme_keys(dt):
    info = np.iinfo(dt)

    def key(rng, n):
        k = np.concatenate([info.min + rng.integers(0, 40, n // 2, dtype=np.uint64).astype(dt),
                            info.max - rng.integers(0, 40, n - n // 2, dtype=np.uint64).astype(dt)])
        return np.sort(k)
    return key


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("dt", ["int8", "uint16", "int32", "int64", "uint64"])
def test_integer_keys_at_their_extremes(gpu, cpu, dt, asc):
    """o - a and o + b never wrap: keys within 40 of both ends of the type"""
    t = _table("random", T + 300, 18, nullable=True, key=_extreme_keys(np.dtype(dt)))
    for frame in ((5, 5), (0, 100), ((1 << 63) - 2, 7), (None, 3)):
        _both(gpu, cpu, t, "g", "o", asc, five("v", *frame))


def test_timestamp_keys_and_integer_sums_that_wrap(gpu, cpu):
    n = T + 300
    t = _table("random", n, 19, nullable=True,
               key=lambda rng, n: pa.array(np.sort(rng.integers(0, 50 * n, n)) * 1_000_000, pa.timestamp("us")),
               values=lambda rng, n: rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64))
    for frame in ((5_000_000, 0), (60_000_000, 60_000_000), (None, None)):
        f = five("v", *frame)
        del f["m"]
        _both(gpu, cpu, t, "g", "o", True, f)


def test_min_periods(gpu, cpu):
    t = _table("random", T + 500, 20, nullable=True)
    for minp in (1, 3, 40):
        _both(gpu, cpu, t, "g", "o", True, five("v", 20, 20, minp))


def test_mixed_with_ranking_rolling_and_shift_specs(gpu, cpu):
    t = _table("long", 2 * T + 77, 21, nullable=True)
    f = {"rn": "row_number", "r7": ("range_sum", "v", 6, 0), "cs": ("cumsum", "v"), "prev": ("lag", "v", 1),
         "roll": ("rolling_max", "v", 400, 400), "cnt": ("range_count", "v", 6, 0), "o2": ("range_max", "o", 6, 0)}
    c = _both(gpu, cpu, t, "g", "o", True, f)
    assert c["window.frame.range"] == 3 and c["window.range.bounds"] == 1 and c["window.sort"] == 1, c
    for ctx in (gpu, cpu):
        all_ = Table(t, ctx).window("g", "o", True, f).to_arrow()
        for name, spec in f.items():
            alone = Table(t, ctx).window("g", "o", True, {name: spec}).to_arrow()
            assert alone[name].equals(all_[name]), name
