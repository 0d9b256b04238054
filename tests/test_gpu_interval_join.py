"""Interval joins on the MI355X: the rank pass (k_interval_rank_tile / k_win_carry / k_interval_rank),
k_interval_counts and the tiled expansion k_interval_expand of kernels/interval.hip behind
ops/interval.cpp.  Every case runs on a GPU context and on a CPU context and both are held to the
engine-independent oracle (interval_utils), computed once; interval.tiles > 0 on the GPU shows that the
kernels ran (there is no other device path).

Shapes.  Rank pass: nr + 2 nl on wave, block and tile edges (W - 1 / W / W + 1 / 2W, W =
C.window_tile_rows()), a multi-block count (2 x 100 003 with about one match per interval), the two
lopsided pairs, and one case whose carry scan loops.  Expansion: pair totals 0, 1, T - 1, T, T + 1 and
3T + 17 (T = C.interval_tile_rows()); one left row that straddles tiles; more than 2T left rows without
output inside one tile (the span that cannot be staged in LDS), and the same with a filler each; empty
first and last rows; one pair per row; all pairs in the last row."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from cylon_amd._lib import C
from interval_utils import CLOSED, HOWS, assert_multiset, check_interval, counts_of, expected
from dist_utils import run_distributed

pytestmark = pytest.mark.gpu

T = C.interval_tile_rows()
W = C.window_tile_rows()
BIG = 100_003
KW = dict(lower="lo", upper="hi", on="t")


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _both(gpu, cpu, left, right, step=0, exp=None, **kw):
    if exp is None:
        exp = expected(left, right, **kw)  # once, for both contexts
    assert len(exp) <= 320_000
    cg = check_interval(gpu, left, right, step, exp=exp, **kw)
    cc = check_interval(cpu, left, right, step, exp=exp, **kw)
    names = ("interval.sort", "interval.rank_tiles", "interval.pairs", "interval.matched", "interval.tiles")
    assert [cg.get(k) for k in names] == [cc.get(k) for k in names], (cg, cc)
    if exp and left.num_rows and right.num_rows:
        assert cg["interval.tiles"] > 0, cg
    return cg


def _narrow(nl, nr, seed, groups=5):
    """unique right `on` values 0 .. nr - 1 in group on % groups; a left row of group g owns the rows of g
    among lower .. lower + groups - 1: one, where the interval does not run past nr - 1"""
    rng = np.random.default_rng(seed)
    t = rng.permutation(nr)
    lo = rng.integers(0, nr, nl)
    left = pa.table({"g": rng.integers(0, groups, nl).astype(np.int32), "lo": lo, "hi": lo + groups - 1,
                     "a": np.arange(nl)})
    right = pa.table({"g": (t % groups).astype(np.int32), "t": t,
                      "b": pa.array(rng.integers(-99, 99, nr), mask=rng.random(nr) < 0.1)})
    return left, right


# (nl, nr): nr + 2 nl = 3, 127, 320, 512, W - 1, W, W + 1, 2W
RANK_SIZES = [(1, 1), (31, 65), (100, 120), (128, 256), (500, W - 1 - 1000), (512, W - 1024), (1000, W + 1 - 2000),
              (W // 2, W)]


@pytest.mark.parametrize("nl,nr", RANK_SIZES)
def test_rank_pass_sizes(gpu, cpu, nl, nr):
    left, right = _narrow(nl, nr, nl + nr, groups=3)
    for closed in CLOSED:
        _both(gpu, cpu, left, right, by="g", closed=closed, **KW)
    _both(gpu, cpu, left, right, how="left", **KW)  # no `by`: about three matches each


@pytest.mark.parametrize("nl,nr", [(BIG, BIG), (1, BIG), (BIG, 1)])
def test_rank_pass_many_blocks(gpu, cpu, nl, nr):
    left, right = _narrow(nl, nr, 11 + nl % 7 + nr % 5)
    if nl == 1:  # the one left row owns its whole group
        left = pa.table({"g": pa.array([2], pa.int32()), "lo": [-1], "hi": [nr], "a": [0]})
    c = _both(gpu, cpu, left, right, by="g", **KW)
    if nl == nr:
        assert 0.9 * BIG < c["interval.matched"] <= BIG, c
    elif nl == 1:
        assert c["interval.matched"] == len(range(2, nr, 5)), c
    _both(gpu, cpu, left, right, by="g", closed="neither", how="left", **KW)


def test_rank_carry_scan_loops(gpu, cpu):
    """more tiles than one carry step covers: nr + 2 nl = 5W + 100 positions at 2 tiles per step"""
    assert C.window_carry_tiles() >= 2
    left, right = _narrow(2 * W, W + 100, 3, groups=2)
    assert -(-(right.num_rows + 2 * left.num_rows) // W) >= 5
    for closed in CLOSED:
        _both(gpu, cpu, left, right, step=2, by="g", closed=closed, **KW)
    # every right row before every U-copy and after every L-copy: the carries are the whole story
    left = pa.table({"lo": np.zeros(2 * W, np.int64), "hi": np.full(2 * W, 9)})
    right = pa.table({"t": np.arange(10) % 10, "b": np.arange(10)})
    c = _both(gpu, cpu, left, right, step=2, **KW)
    assert c["interval.matched"] == 20 * W, c


def _from_counts(counts, seed, decoys=True):
    """left row i owns exactly counts[i] right rows: its interval is [100 i, 100 i + 10] and its right
    rows take the values 100 i + k % 11 (ties); the right rows are shuffled.  decoys: right rows
    between the intervals and with a null or NaN `on`"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    nl = len(counts)
    owner = np.repeat(np.arange(nl), counts)
    k = np.arange(len(owner)) - np.repeat(np.cumsum(counts) - counts, counts)
    t = (100 * owner + k % 11).astype(np.float64)
    mask = np.zeros(len(t), bool)
    if decoys:
        t = np.concatenate([t, [-5.0, 50.0, np.nan, 100.0 * nl + 50, 0.0, np.nan]])
        mask = np.concatenate([mask, [False, False, False, False, True, False]])
    p = rng.permutation(len(t))
    left = pa.table({"lo": 100.0 * np.arange(nl), "hi": 100.0 * np.arange(nl) + 10, "a": np.arange(nl)})
    right = pa.table({"t": pa.array(t[p], mask=mask[p]), "b": np.arange(len(t))})
    return left, right


def _composition(total, nl, seed):
    """counts of nl rows that add up to total, about half of them 0"""
    rng = np.random.default_rng(seed)
    w = rng.random(nl) * (rng.random(nl) < 0.5)
    w[0] += 1e-9
    return rng.multinomial(total, w / w.sum())


@pytest.mark.parametrize("total", [0, 1, T - 1, T, T + 1, 3 * T + 17])
def test_expansion_pair_totals(gpu, cpu, total):
    counts = _composition(total, 500, total)
    left, right = _from_counts(counts, total + 1)
    exp = expected(left, right, **KW)
    assert len(exp) == total and counts_of(exp, 500) == counts.tolist()
    c = _both(gpu, cpu, left, right, exp=exp, **KW)
    assert c["interval.pairs"] == total and c["interval.tiles"] == -(-total // T), c
    _both(gpu, cpu, left, right, how="left", **KW)


LAYOUTS = {
    # one left row owning more than 2T pairs, between rows owning one pair each
    "one_row_straddles_tiles": [1] * 50 + [2 * T + 100] + [1] * 50,
    # more than 2T consecutive left rows without a match inside one tile: the span that cannot be staged
    "zeros_between_two_rows": [3] + [0] * (2 * T + 50) + [4],
    "zeros_between_two_tiles": [T - 5] + [0] * (2 * T + 50) + [T + 9],
    "first_and_last_rows_empty": [0, 5, 0, 7, 0],
    "one_pair_per_row": [1] * (T + 300),
    "all_pairs_in_the_last_row": [0] * 300 + [T + 50],
}


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_expansion_layouts(gpu, cpu, layout, how):
    counts = LAYOUTS[layout]
    left, right = _from_counts(counts, len(layout))
    exp = expected(left, right, how=how, **KW)
    fillers = sum(c == 0 for c in counts) if how == "left" else 0
    assert len(exp) == sum(counts) + fillers and sum(j is None for _, j in exp) == fillers
    c = _both(gpu, cpu, left, right, exp=exp, how=how, **KW)
    assert c["interval.matched"] == sum(counts), c


@pytest.mark.parametrize("closed", CLOSED)
def test_closed_across_tile_boundaries_with_ties(gpu, cpu, closed):
    rng = np.random.default_rng(3)
    nl, nr = T + 300, T
    lo = rng.integers(0, 400, nl)
    left = pa.table({"g": rng.integers(0, 3, nl), "lo": lo, "hi": lo + rng.integers(-1, 4, nl), "a": np.arange(nl)})
    right = pa.table({"g": rng.integers(0, 3, nr), "t": rng.integers(0, 400, nr),
                      "b": pa.array(rng.integers(-99, 99, nr), mask=rng.random(nr) < 0.1)})
    for how in HOWS:
        c = _both(gpu, cpu, left, right, by="g", closed=closed, how=how, **KW)
        assert c["interval.pairs"] > T, c


@pytest.mark.parametrize("typ", ["float32", "float64"])
def test_float_values_with_nan_and_nulls_at_group_ends(gpu, cpu, typ):
    """NaN and null values sort to the end of their group; a group holds 2100 positions of the merged
    order, so the groups straddle the tile edges of the rank pass"""
    rng = np.random.default_rng(4)
    nl, nr = W, W + 40

    def val(n, add=0.0):
        v = (np.arange(n) // 3 / 4 + add).astype(typ)
        v[rng.random(n) < 0.1] = np.nan
        return pa.array(v, mask=rng.random(n) < 0.1)

    lo = val(nl)
    lo = pa.array([-0.0] + lo.to_pylist()[1:], lo.type)
    left = pa.table({"g": np.arange(nl) // 700, "lo": lo, "hi": val(nl, 1.0), "a": np.arange(nl)})
    right = pa.table({"g": np.arange(nr) // 700, "t": val(nr), "b": np.arange(nr)})
    pl, pr = rng.permutation(nl), rng.permutation(nr)
    left, right = left.take(pa.array(pl)), right.take(pa.array(pr))
    for closed in CLOSED:
        c = _both(gpu, cpu, left, right, by="g", closed=closed, **KW)
        assert c["interval.matched"] > 2 * W, c
    _both(gpu, cpu, left, right, by="g", how="left", **KW)


@pytest.mark.parametrize("typ", ["int8", "uint16", "int32", "uint64", "timestamp", "date32"])
def test_value_widths(gpu, cpu, typ):
    nl, nr = 700, T + 300
    rng = np.random.default_rng(len(typ))
    if typ == "timestamp":
        col = lambda m: pa.array(rng.integers(10 ** 15, 10 ** 15 + 900, m), pa.timestamp("ns"))
    elif typ == "date32":
        col = lambda m: pa.array(rng.integers(19000, 19400, m).astype(np.int32), pa.date32())
    else:
        info = np.iinfo(typ)

        def col(m):
            v = rng.integers(info.min, info.max, m, dtype=typ, endpoint=True)
            v[:4] = [info.min, info.max, info.max, info.min]  # the extremes are ordinary values
            return pa.array(v)
    left = pa.table({"g": rng.integers(0, 5, nl), "lo": col(nl), "hi": col(nl)})
    right = pa.table({"g": rng.integers(0, 5, nr), "t": col(nr), "b": np.arange(nr)})
    c = _both(gpu, cpu, left, right, by="g", **KW)
    assert c["interval.matched"] > T, c
    _both(gpu, cpu, left, right, by="g", closed="neither", how="left", **KW)


def test_string_by_and_two_by_columns(gpu, cpu):
    n = T + 77
    rng = np.random.default_rng(5)
    key = lambda m: pa.array([None if x == 0 else "k%d" % x for x in rng.integers(0, 9, m)])
    lo = rng.integers(0, 300, n)
    left = pa.table({"s": key(n), "i": rng.integers(0, 3, n), "lo": lo, "hi": lo + rng.integers(0, 5, n)})
    right = pa.table({"s": key(n), "i": rng.integers(0, 3, n), "t": rng.integers(0, 300, n),
                      "txt": pa.array(["r%d" % i for i in range(n)])})
    for closed in ("both", "left"):
        _both(gpu, cpu, left, right, by=["s", "i"], closed=closed, **KW)
        _both(gpu, cpu, left, right, by="s", closed=closed, how="left", **KW)


def test_sliced_columns_start_off_a_16_byte_boundary(gpu, cpu):
    n = T + 5
    rng = np.random.default_rng(6)
    lo = rng.integers(0, 500, n + 3)
    l = pa.table({"g": rng.integers(0, 3, n + 3).astype(np.int32), "lo": lo, "hi": lo + rng.integers(0, 4, n + 3)})
    r = pa.table({"g": rng.integers(0, 3, n + 3).astype(np.int32), "t": rng.integers(0, 500, n + 3),
                  "b": pa.array(rng.integers(-9, 9, n + 3), mask=rng.random(n + 3) < 0.2)})
    wl, wr = l.slice(3, n), r.slice(3, n)
    for how in HOWS:
        exp = expected(wl, wr, by="g", how=how, **KW)
        for ctx in (gpu, cpu):
            tables = (Table(l, ctx).slice(3, n), Table(r, ctx).slice(3, n))
            c = check_interval(ctx, wl, wr, exp=exp, tables=tables, by="g", how=how, **KW)
            assert c["interval.tiles"] == -(-len(exp) // T), c


def _global():
    nl, nr = T + 17, T + 300
    rng = np.random.default_rng(7)
    lo = rng.integers(0, 400, nl)
    left = pa.table({"g": rng.integers(0, 25, nl), "lo": lo, "hi": lo + rng.integers(-1, 40, nl), "lrow": np.arange(nl)})
    right = pa.table({"g": rng.integers(0, 25, nr), "t": rng.integers(0, 400, nr), "rrow": np.arange(nr),
                      "b": pa.array(rng.integers(-99, 99, nr), mask=rng.random(nr) < 0.1)})
    return left, right


DIST_KW = dict(by="g", closed="left", how="left", **KW)


def _dist(ctx):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    left, right = _global()
    tl = Table(left.take(pa.array(np.arange(rank, left.num_rows, world))), ctx)
    tr = Table(right.take(pa.array(np.arange(rank, right.num_rows, world))), ctx)
    C.trace_enable(True)
    C.trace_reset()
    out = tl.distributed_interval_join(tr, **DIST_KW).to_arrow()
    return out, dict(C.trace_counters())


def test_distributed_interval_join_on_device():
    res = run_distributed(_dist, 2, device="cuda:0")
    left, right = _global()
    on = [set(r[0].column(0).to_pylist()) for r in res]  # every group on one rank
    assert on[0].isdisjoint(on[1])
    assert all(r[1].get("interval.tiles", 0) > 0 for r in res), [r[1] for r in res]
    exp = expected(left, right, **DIST_KW)
    assert sum(r[1]["interval.pairs"] for r in res) == len(exp) > T
    assert_multiset(pa.concat_tables([r[0] for r in res]), left, right, exp, "lrow", "rrow", **DIST_KW)
