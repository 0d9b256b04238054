"""As-of joins on the MI355X: the segmented last-match scan of kernels/asof.hip (k_asof_tile / k_win_carry /
k_asof_apply, forwards and over the reversed order, and k_asof_pick) behind ops/asof.cpp.  Every case
runs on a GPU context and on a CPU context and both are held to the engine-independent oracle
(asof_utils), computed once; asof.scan > 0 on the GPU shows that the kernels ran (there is no other
device path).

Shapes: nl + nr on wave, block and tile edges (T - 1 / T / T + 1 / 2T, T = C.window_tile_rows()), a
multi-block count (2 x 100 003) and the two lopsided pairs; group layouts that put heads on tile
boundaries of the merged order; the carries a tile scan gets wrong (whole tiles of identity elements
between a candidate and its left rows, a left-only group that starts a tile, a right-only run longer
than a tile), forwards and reversed; one case whose carry scan loops."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from cylon_amd._lib import C
from asof_utils import DIRECTIONS, assert_asof, check_asof, expected
from dist_utils import run_distributed

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
BIG = 100_003
# (nl, nr): sums 2, 127, 320, 512, T - 1, T, T, T + 1, 2T, 2T, and multi-block counts
PAIRS = [(1, 1), (63, 64), (65, 255), (257, 255), (T - 1 - 257, 257), (1, T - 1), (T - 1, 1), (1, T), (T, T),
         (T + 1, T - 1), (T + 1, BIG), (BIG, BIG), (1, BIG), (BIG, 1)]


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, left, right, step=0, **kw):
    exp = expected(left, right, **kw)  # once, for both contexts
    cg = check_asof(gpu, left, right, step, exp=exp, **kw)
    cc = check_asof(cpu, left, right, step, exp=exp, **kw)
    assert cg.get("asof.scan", 0) == cc.get("asof.scan", 0), (cg, cc)
    if left.num_rows and right.num_rows:
        assert cg["asof.scan"] > 0 and cg["asof.tiles"] == cg["asof.scan"] * -(-(left.num_rows + right.num_rows) // T), cg
    return cg


def _group_ids(layout, n, rng):
    """a group id per position of the merged order, non-decreasing"""
    if layout == "one":
        return np.zeros(n, np.int64)
    if layout == "each":
        return np.arange(n, dtype=np.int64) // 2  # a pair per group: some hold both sides
    if layout == "random":
        return np.repeat(np.arange(n), rng.integers(1, 201, n))[:n].astype(np.int64)
    if layout == "tile_edges":
        # heads at a tile's first position (T), at a tile's last (2T - 1), a group that ends a tile, and
        # every tile after 3T + 5 wholly inside one group until a head in the last tile
        ids = np.zeros(n, np.int64)
        for h in (T, 2 * T - 1, 3 * T, 3 * T + 5, n - 7):
            if 0 < h < n:
                ids[h:] += 1
        return ids
    raise ValueError(layout)


def _split(ids, on, is_left, rng, payload=True):
    """the merged order (group ids, `on` values, side of every position) -> shuffled left and right tables"""
    li, ri = np.flatnonzero(is_left), np.flatnonzero(~is_left)
    li, ri = li[rng.permutation(len(li))], ri[rng.permutation(len(ri))]
    left = {"g": ids[li].astype(np.int32), "t": on[li]}
    right = {"g": ids[ri].astype(np.int32), "t": on[ri]}
    if payload:
        left["a"] = np.arange(len(li))
        right["b"] = pa.array(rng.integers(-99, 99, len(ri)), mask=rng.random(len(ri)) < 0.1)
    return pa.table(left), pa.table(right)


def _layout_pair(layout, nl, nr, seed):
    rng = np.random.default_rng(seed)
    n = nl + nr
    ids = _group_ids(layout, n, rng)
    is_left = np.zeros(n, bool)
    is_left[rng.permutation(n)[:nl]] = True
    return _split(ids, np.arange(n) // 2, is_left, rng)  # ties on `on`, also between the sides


@pytest.mark.parametrize("layout", ["one", "each", "random", "tile_edges"])
@pytest.mark.parametrize("nl,nr", PAIRS)
def test_sizes_and_group_layouts(gpu, cpu, nl, nr, layout):
    if layout == "tile_edges" and nl + nr <= T:
        layout = "random"  # no tile boundary to put a head on
    left, right = _layout_pair(layout, nl, nr, nl * 7 + nr + len(layout))
    if nl + nr > 4 * T:  # the large shapes: both scans, both concatenation orders, the tolerance
        _both(gpu, cpu, left, right, on="t", by="g", direction="backward")
        _both(gpu, cpu, left, right, on="t", by="g", direction="nearest", allow_exact_matches=False, tolerance=9)
        return
    for k, direction in enumerate(DIRECTIONS):
        _both(gpu, cpu, left, right, on="t", by="g", direction=direction, allow_exact_matches=True)
        _both(gpu, cpu, left, right, on="t", by="g", direction=direction, allow_exact_matches=False,
              tolerance=(None, 1, 30)[k])
    _both(gpu, cpu, left, right, on="t", direction="nearest")  # no `by`: one partition


def _sequence(runs, reverse, seed):
    """runs = [(group, 'L' | 'R', count)] in scan order -> tables whose merged order, read forwards
    (reverse = False) or backwards (reverse = True), is exactly that sequence"""
    g = np.concatenate([np.full(c, grp, np.int64) for grp, _, c in runs])
    is_left = np.concatenate([np.full(c, side == "L") for _, side, c in runs])
    on = np.arange(len(g), dtype=np.int64)
    if reverse:
        g, on = -g, -on
    return _split(g, on, is_left, np.random.default_rng(seed), payload=False)


CARRIES = {
    # one candidate, then more than two whole tiles of left rows: the carry crosses identity tiles
    "one_right_then_tiles_of_left": [(0, "R", 1), (0, "L", 2 * T + 50), (1, "R", 3), (1, "L", 5)],
    # a left-only group that starts a tile, right after a group rich in right rows: -1, not the neighbour's row
    "left_only_group_starts_a_tile": [(0, "R", T - 10), (0, "L", 10), (1, "L", 300), (2, "R", 7), (2, "L", 9)],
    # a right-only run longer than a tile before one left row
    "right_run_longer_than_a_tile": [(0, "L", 3), (0, "R", T + 100), (0, "L", 1), (1, "L", 2)],
}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", sorted(CARRIES))
def test_carries_across_tiles(gpu, cpu, case, reverse):
    left, right = _sequence(CARRIES[case], reverse, len(case))
    direction = "forward" if reverse else "backward"
    exp = expected(left, right, on="t", by="g", direction=direction)
    lg = np.abs(np.asarray(left["g"]))
    if case == "one_right_then_tiles_of_left":
        assert sum(e is not None for e in exp) == 2 * T + 55
    elif case == "left_only_group_starts_a_tile":
        assert all(e is None for e, grp in zip(exp, lg) if grp == 1) and sum(e is not None for e in exp) == 19
    else:
        assert sum(e is not None for e in exp) == 1
    _both(gpu, cpu, left, right, on="t", by="g", direction=direction)
    _both(gpu, cpu, left, right, on="t", by="g", direction="nearest")


@pytest.mark.parametrize("reverse", [False, True])
def test_carry_scan_loops(gpu, cpu, reverse):
    """more tiles than one carry step covers: 6 tiles at 2 tiles per step, one candidate carried across
    them all, then groups of a tile and a half"""
    assert C.window_carry_tiles() >= 2
    direction = "forward" if reverse else "backward"
    runs = [(0, "R", 1), (0, "L", 5 * T + 100)]
    left, right = _sequence(runs, reverse, 1)
    assert -(-(left.num_rows + right.num_rows) // T) >= 5
    c = _both(gpu, cpu, left, right, step=2, on="t", by="g", direction=direction)
    assert c["asof.matched"] == 5 * T + 100, c
    runs = []
    for grp in range(4):
        runs += [(grp, "R", 2), (grp, "L", T + T // 2 - 2)]
    left, right = _sequence(runs, reverse, 2)
    _both(gpu, cpu, left, right, step=2, on="t", by="g", direction=direction)
    _both(gpu, cpu, left, right, step=2, on="t", by="g", direction="nearest", allow_exact_matches=False)


@pytest.mark.parametrize("exact", [True, False])
def test_nearest_and_tolerance_across_tile_boundaries(gpu, cpu, exact):
    n = 3 * T + 17
    rng = np.random.default_rng(3)
    ids = np.arange(n) // (T // 2 + 33)  # groups that straddle every tile edge
    is_left = rng.random(n) < 0.6
    on = np.cumsum(rng.integers(0, 4, n))  # gaps of 0 .. 3: ties, and distances on both sides of the tolerance
    left, right = _split(ids, on, is_left, rng)
    for tol in (None, 0, 2):
        _both(gpu, cpu, left, right, on="t", by="g", direction="nearest", allow_exact_matches=exact, tolerance=tol)
    _both(gpu, cpu, left, right, on="t", by="g", direction="forward", allow_exact_matches=exact, tolerance=1)


@pytest.mark.parametrize("typ", ["float32", "float64"])
def test_float_on_with_nan_and_nulls_at_group_ends(gpu, cpu, typ):
    """NaN and null `on` values sort to the end of their group; the groups straddle the tile edges"""
    n = 3 * T + 40
    rng = np.random.default_rng(4)
    ids = np.arange(n) // (T + T // 2)
    is_left = rng.random(n) < 0.5
    on = (np.arange(n) // 3 / 4).astype(typ)
    on[rng.random(n) < 0.15] = np.nan
    on[0] = -0.0
    left, right = _split(ids, on, is_left, rng)
    left = left.set_column(1, "t", pa.array(np.asarray(left["t"]), mask=rng.random(left.num_rows) < 0.15))
    right = right.set_column(1, "t", pa.array(np.asarray(right["t"]), mask=rng.random(right.num_rows) < 0.15))
    for direction in DIRECTIONS:
        for exact in (True, False):
            _both(gpu, cpu, left, right, on="t", by="g", direction=direction, allow_exact_matches=exact)
    _both(gpu, cpu, left, right, on="t", by="g", direction="nearest", tolerance=0.5)


@pytest.mark.parametrize("typ", ["int8", "uint16", "int32", "uint64", "timestamp", "date32"])
def test_on_widths(gpu, cpu, typ):
    n = T + 300
    rng = np.random.default_rng(len(typ))
    if typ == "timestamp":
        col = lambda m: pa.array(rng.integers(10 ** 15, 10 ** 15 + 900, m), pa.timestamp("ns"))
    elif typ == "date32":
        col = lambda m: pa.array(rng.integers(19000, 19400, m).astype(np.int32), pa.date32())
    else:
        info = np.iinfo(typ)
        col = lambda m: pa.array(rng.integers(info.min, info.max, m, dtype=typ, endpoint=True))
    left = pa.table({"g": rng.integers(0, 5, n), "t": col(n)})
    right = pa.table({"g": rng.integers(0, 5, n // 2), "t": col(n // 2), "b": np.arange(n // 2)})
    _both(gpu, cpu, left, right, on="t", by="g", direction="backward", tolerance=20)
    _both(gpu, cpu, left, right, on="t", by="g", direction="nearest", allow_exact_matches=False)
    _both(gpu, cpu, left, right, on="t", by="g", direction="forward", allow_exact_matches=False, tolerance=(1 << 63) - 1)


def test_string_by_column(gpu, cpu):
    n = T + 77
    rng = np.random.default_rng(5)
    key = lambda m: pa.array([None if x == 0 else "k%d" % x for x in rng.integers(0, 9, m)])
    left = pa.table({"s": key(n), "i": rng.integers(0, 3, n), "t": rng.integers(0, 300, n)})
    right = pa.table({"s": key(n), "i": rng.integers(0, 3, n), "t": rng.integers(0, 300, n),
                      "txt": pa.array(["r%d" % i for i in range(n)])})
    for direction in DIRECTIONS:
        _both(gpu, cpu, left, right, on="t", by=["s", "i"], direction=direction)
        _both(gpu, cpu, left, right, on="t", by="s", direction=direction, allow_exact_matches=False, tolerance=7)


def test_sliced_columns_start_off_a_16_byte_boundary(gpu, cpu):
    n = T + 5
    rng = np.random.default_rng(6)
    l = pa.table({"g": rng.integers(0, 3, n + 3).astype(np.int32), "t": rng.integers(0, 500, n + 3)})
    r = pa.table({"g": rng.integers(0, 3, n + 3).astype(np.int32), "t": rng.integers(0, 500, n + 3),
                  "b": pa.array(rng.integers(-9, 9, n + 3), mask=rng.random(n + 3) < 0.2)})
    wl, wr = l.slice(3, n), r.slice(3, n)
    for direction in DIRECTIONS:
        exp = expected(wl, wr, on="t", by="g", direction=direction, tolerance=3)
        for ctx in (gpu, cpu):
            tables = (Table(l, ctx).slice(3, n), Table(r, ctx).slice(3, n))
            c = check_asof(ctx, wl, wr, exp=exp, tables=tables, on="t", by="g", direction=direction, tolerance=3)
            assert c["asof.scan"] == (2 if direction == "nearest" else 1), c


def _global():
    """unique right `on` values: no tie depends on the order the shuffled right rows arrive in"""
    nl, nr = 2 * T + 17, T + 300
    rng = np.random.default_rng(7)
    left = pa.table({"g": rng.integers(0, 25, nl), "t": rng.integers(0, nr, nl), "row": np.arange(nl)})
    right = pa.table({"g": rng.integers(0, 25, nr), "t": rng.permutation(nr),
                      "b": pa.array(rng.integers(-99, 99, nr), mask=rng.random(nr) < 0.1)})
    return left, right


DIST_KW = dict(on="t", by="g", direction="nearest", tolerance=60)


def _dist(ctx):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    left, right = _global()
    tl = Table(left.take(pa.array(np.arange(rank, left.num_rows, world))), ctx)
    tr = Table(right.take(pa.array(np.arange(rank, right.num_rows, world))), ctx)
    C.trace_enable(True)
    C.trace_reset()
    out = tl.distributed_asof_join(tr, **DIST_KW).to_arrow()
    return out, dict(C.trace_counters())


def test_distributed_asof_join_on_device():
    res = run_distributed(_dist, 2, device="cuda:0")
    left, right = _global()
    on = [set(r[0].column(0).to_pylist()) for r in res]  # every group on one rank
    assert on[0].isdisjoint(on[1])
    assert all(r[1].get("asof.scan", 0) == 2 for r in res), [r[1] for r in res]
    assert_asof(pa.concat_tables([r[0] for r in res]), left, right, row_id="row", **DIST_KW)
