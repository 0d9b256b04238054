"""Top-k row selection on the MI355X: the radix-select kernels of kernels/topk.hip (k_topk_scan /
k_topk_hist / k_topk_pick / k_topk_collect) behind ops/topk.cpp.  Every case is compared, WITHOUT
re-sorting and over every column, with the numpy oracle (topk_utils) and with the same call on a CPU
context; the trace counters prove that the select ran and the sort fallback did not.

Shapes: wave (63 / 64 / 65), block (255 / 257), tile (one 16-byte-load tile of int64 keys is 2048
rows: 4095 / 4097) and multi-block (100 003 rows: 48 full tiles and a tail over 49 blocks) edges; one
case has more tiles than the grid has blocks (2048), so that the grid-stride loop goes round."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import CylonContext, Table
from dist_utils import run_distributed
from topk_utils import D, assert_same, check_topk, clustered_int64, expected, max_passes

pytestmark = pytest.mark.gpu

BIG = 100_003


def _ctx(device, **cfg):
    c = CylonContext(config=None, distributed=False, device=device)
    c.add_config("topk_select_min_rows", "0")
    c.add_config("topk_rows_per_k", "1")  # any k < rows
    for k, v in cfg.items():
        c.add_config(k, str(v))
    return c


# a candidate limit of 64 rows, so that tables this small still run histogram passes
@pytest.fixture(scope="module")
def gsel():
    return _ctx("cuda:0", topk_candidates=64)


@pytest.fixture(scope="module")
def csel():
    return _ctx("cpu", topk_candidates=64)


@pytest.fixture(scope="module")
def gdefault():
    return _ctx("cuda:0")


def _both(g, c, t, by, asc, k, path="select"):
    """GPU and CPU contexts against the oracle; the two counter sets must agree on the pass structure"""
    cg = check_topk(g, t, by, asc, k, path=path)
    cc = check_topk(c, t, by, asc, k, path=path)
    if path == "select":
        assert cg["topk.passes"] == cc["topk.passes"] and cg["topk.key_reads"] == cc["topk.key_reads"], (cg, cc)
    return cg


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4095, 4097, BIG])
def test_tile_and_tail_edges(gsel, csel, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, endpoint=True)
    keys[rng.random(n) < 0.2] = 11  # ties
    t = pa.table({"k": keys, "row": np.arange(n), "f": rng.random(n)})
    for asc in (True, False):
        for k in sorted({1, 64, n - 1}):
            c = _both(gsel, csel, t, "k", asc, k, path="select" if 0 < k < n else None)
            assert n <= 64 or not 0 < k < n or c["topk.passes"] >= 1, c


def test_more_tiles_than_blocks(gsel, csel):
    n = 2048 * 2048 + 2 * 2048 + 77
    rng = np.random.default_rng(2)
    t = pa.table({"k": rng.integers(-(1 << 40), 1 << 40, n), "row": np.arange(n)})
    _both(gsel, csel, t, "k", False, 5000)


def test_sliced_column_starts_off_a_16_byte_boundary(gsel, csel):
    """a table slice's key column begins 8 bytes past a 16-byte boundary: the kernels' scalar head"""
    n = 4097 + 3
    rng = np.random.default_rng(3)
    t = pa.table({"k": rng.integers(-1000, 1000, n), "row": np.arange(n)})
    for ctx in (gsel, csel):
        got = Table(t, ctx).slice(3, 4097).topk(65, "k", False).to_arrow()
        assert_same(got, expected(t.slice(3, 4097), "k", False, 65))


@pytest.mark.parametrize("dt", ["int8", "int16", "float16", "float32"])
def test_narrow_key_types(gsel, csel, dt):
    n = 4097
    rng = np.random.default_rng(len(dt))
    dt = np.dtype(dt)
    if dt.kind == "f":
        keys = (rng.standard_normal(n) * 50).astype(dt)
        keys[rng.choice(n, 40, replace=False)] = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf], dt)[np.arange(40) % 5]
    else:
        keys = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
    t = pa.table({"k": pa.array(keys), "row": np.arange(n)})
    for asc in (True, False):
        for k in (1, 64, n - 1):
            _both(gsel, csel, t, "k", asc, k)


@pytest.mark.parametrize("shape", ["constant", "sorted", "two_digits", "random"])
def test_lds_histogram_paths(gsel, csel, shape):
    """constant / sorted keys: every wave's lanes share a digit (one LDS add per wave); keys alternating
    between two digits and random keys: per-lane LDS atomics"""
    n = BIG
    rng = np.random.default_rng(4)
    if shape == "constant":
        keys = np.full(n, -5, np.int64)
    elif shape == "sorted":
        keys = np.sort(rng.integers(0, 1 << 62, n))
    elif shape == "two_digits":
        keys = np.where(np.arange(n) % 2 == 0, 3, 1 << 61).astype(np.int64) + rng.integers(0, 2, n)
    else:
        keys = rng.integers(-(1 << 62), 1 << 62, n)
    t = pa.table({"k": keys, "row": np.arange(n)})
    for asc in (True, False):
        c = _both(gsel, csel, t, "k", asc, 1000)
        assert c["topk.passes"] >= 1, c


def test_multi_pass_refinement(gsel, csel):
    rng = np.random.default_rng(5)
    t = pa.table({"k": clustered_int64(rng, BIG), "row": np.arange(BIG), "f": rng.random(BIG)})
    for asc in (True, False):
        c = _both(gsel, csel, t, "k", asc, BIG // 2)
        assert c["topk.passes"] >= 3, c


def test_bits_exhausted_ties(gsel, csel):
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 5, BIG)
    t = pa.table({"k": keys, "row": np.arange(BIG)})
    assert max_passes(keys) == 1
    for asc in (True, False):
        c = _both(gsel, csel, t, "k", asc, 30_000)
        # one pass over the 3 image bits, then the 17 bits of the row number until <= 64 rows remain
        assert 2 <= c["topk.passes"] <= 1 + -(-17 // D), c


@pytest.mark.parametrize("asc", [True, False])
def test_nullable_float_key_with_nan_and_signed_zero(gsel, csel, asc):
    n = 4097
    rng = np.random.default_rng(7)
    keys = rng.standard_normal(n)
    keys[rng.choice(n, 300, replace=False)] = np.array([np.nan, -0.0, 0.0])[np.arange(300) % 3]
    mask = rng.random(n) < 0.3
    t = pa.table({"k": pa.array(keys, mask=mask), "row": np.arange(n)})
    nonnull = int((~mask).sum())
    _both(gsel, csel, t, "k", asc, 500)
    c = _both(gsel, csel, t, "k", asc, nonnull + 9)
    assert c.get("topk.null_fill") == 1, c


def test_payload_through_the_gather(gsel, csel, gdefault):
    n = 4097
    rng = np.random.default_rng(8)
    t = pa.table({"k": rng.integers(-99, 99, n).astype(np.int32),
                  "s": pa.array([None if i % 13 == 0 else "p%d" % i for i in range(n)]),
                  "ni": pa.array(rng.integers(0, 9, n), mask=rng.random(n) < 0.2),
                  "f": rng.random(n)})
    for asc in (True, False):
        _both(gsel, csel, t, "k", asc, 333)
        _both(gdefault, csel, t, "k", asc, 333, path=None)  # default limit: no pass, every row a candidate


def _dist(ctx, k):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    ctx.add_config("topk_select_min_rows", "0")
    ctx.add_config("topk_rows_per_k", "1")
    ctx.add_config("topk_candidates", "64")
    n = 20_000
    rng = np.random.default_rng(9)
    g = pa.table({"k": rng.integers(0, 7, n), "grow": np.arange(n), "f": rng.random(n)})
    local = g.take(pa.array(np.arange(rank, n, world)))
    return local, [Table(local, ctx).distributed_topk(k, "k", asc).to_arrow() for asc in (True, False)]


def test_distributed_topk_on_device():
    k = 100
    res = run_distributed(_dist, 2, k, device="cuda:0")
    cat = pa.concat_tables([r[0] for r in res])
    for i, asc in enumerate((True, False)):
        assert_same(res[0][1][i], expected(cat, "k", asc, k))
        assert res[1][1][i].num_rows == 0 and res[1][1][i].column_names == cat.column_names
