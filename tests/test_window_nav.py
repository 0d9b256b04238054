"""Navigation and distribution window functions (FIRST / LAST / NTH_VALUE, FFILL / BFILL, NTILE,
PERCENT_RANK, CUME_DIST) on the CPU context: the sequential twin kernels/cpu_window_nav.cpp behind
ops/window.cpp, against the engine-independent oracle (window_nav_utils), plus the error cases, the
counters and the Table / DataFrame / ops / C ABI / distributed surfaces."""
import ctypes
import os

import numpy as np
import pyarrow as pa
import pytest

import cylon_amd.ops as ops
from cylon_amd import CylonContext, CylonEnv, DataFrame, Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from window_nav_utils import assert_nav, check_nav, expected, run_nav

DATA = os.path.join(os.path.dirname(__file__), "data", "input")
N = 600


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def all_funcs(v="v", k=3, limit=2):
    return {"fv": ("first_value", v), "lv": ("last_value", v), "fvi": ("first_value", v, True),
            "lvi": ("last_value", v, True), "n1": ("nth_value", v, 1), "nk": ("nth_value", v, k), "ff": ("ffill", v),
            "bf": ("bfill", v), "ffl": ("ffill", v, limit), "bfl": ("bfill", v, limit), "nt": ("ntile", k),
            "pr": "percent_rank", "cd": "cume_dist"}


def _values(rng, n, kind, nulls):
    if kind == "float64":
        v = (rng.integers(-40, 40, n) / 4).astype(np.float64)
        v[rng.random(n) < 0.1] = np.nan
        v[rng.random(n) < 0.1] = -0.0
        arr = list(v)
    elif kind == "string":
        arr = ["s%d" % x for x in rng.integers(0, 30, n)]
    elif kind == "bool":
        arr = [bool(x) for x in rng.integers(0, 2, n)]
    else:
        arr = [int(x) for x in rng.integers(-1000, 1000, n)]
    typ = {"float64": pa.float64(), "string": pa.string(), "bool": pa.bool_(), "int32": pa.int32(),
           "int64": pa.int64()}[kind]
    if nulls:
        mask = rng.random(n) < nulls
        arr = [None if m else x for x, m in zip(arr, mask)]
    return pa.array(arr, typ)


def _table(rng, n, kind="int64", nulls=0.3, groups=9):
    return pa.table({"g": rng.integers(0, groups, n), "o": rng.integers(0, n // 3 + 1, n),
                     "o2": rng.integers(0, 3, n).astype(np.int32), "v": _values(rng, n, kind, nulls)})


@pytest.mark.parametrize("nulls", [0.0, 0.3], ids=["dense", "nulls"])
@pytest.mark.parametrize("kind", ["int32", "int64", "float64", "string", "bool"])
def test_every_function_and_type(cpu, kind, nulls):
    t = _table(np.random.default_rng(len(kind) + int(nulls * 10)), N, kind, nulls)
    c = check_nav(cpu, t, "g", "o", True, all_funcs())
    if nulls:  # one forward and one reversed fill scan for the six specs that need one
        assert c["window.nav.fill"] == 2 and c["window.nav.skipped"] == 0, c
    else:
        assert c["window.nav.fill"] == 0 and c["window.nav.skipped"] == 4, c
    assert c["window.nav.gather"] == (10 - c["window.nav.skipped"] if kind == "string" else 0), c


@pytest.mark.parametrize("layout", ["desc", "two_keys", "no_order", "no_partition", "neither"])
def test_orders_and_partitions(cpu, layout):
    t = _table(np.random.default_rng(5), N, "float64")
    part, order, asc = {"desc": ("g", "o", False), "two_keys": ("g", ["o2", "o"], [False, True]),
                        "no_order": ("g", None, True), "no_partition": (None, ["o2", "o"], True),
                        "neither": (None, None, True)}[layout]
    check_nav(cpu, t, part, order, asc, all_funcs())
    if layout == "no_order":  # all rows of a partition are peers
        got = Table(t, cpu).window(part, order, asc, {"pr": "percent_rank", "cd": "cume_dist"}).to_arrow()
        assert set(got["pr"].to_pylist()) == {0.0} and set(got["cd"].to_pylist()) == {1.0}


def test_all_null_and_one_row_partitions(cpu):
    t = pa.table({"g": [0, 0, 0, 1, 2, 2, 3], "o": [2, 1, 0, 0, 1, 0, 0],
                  "v": pa.array([None, None, None, 5.0, None, 7.0, None], pa.float64())})
    f = all_funcs(k=2, limit=1)
    check_nav(cpu, t, "g", "o", True, f)
    got = Table(t, cpu).window("g", "o", True, f).to_arrow()
    assert got["pr"].to_pylist()[3] == 0.0 and got["cd"].to_pylist()[3] == 1.0 and got["nt"].to_pylist()[3] == 1
    assert got["ff"].to_pylist()[:3] == [None] * 3 and got["lvi"].to_pylist()[:3] == [None] * 3
    assert got["ff"].to_pylist()[4:6] == [7.0, 7.0] and got["bf"].to_pylist()[4:6] == [None, 7.0]


def test_ntile_shapes(cpu):
    t = pa.table({"g": [0] * 7 + [1] * 3, "o": list(range(7)) + [2, 1, 0]})
    f = {"k3": ("ntile", 3), "k1": ("ntile", 1), "k7": ("ntile", 7), "k9": ("ntile", 9), "big": ("ntile", 1 << 62)}
    check_nav(cpu, t, "g", "o", True, f)
    got = Table(t, cpu).window("g", "o", True, f).to_arrow()
    assert got["k3"].to_pylist()[:7] == [1, 1, 1, 2, 2, 3, 3]  # s = 7, k = 3: buckets of 3, 2, 2
    assert got["k1"].to_pylist() == [1] * 10
    assert got["k7"].to_pylist()[:7] == got["k9"].to_pylist()[:7] == list(range(1, 8))  # k = s, k > s
    assert got["big"].to_pylist()[7:] == [3, 2, 1]


def test_fill_limits(cpu):
    # a gap of 4 nulls after a value, then a NaN (a value: it stops the fill and is copied), then nulls
    nan = float("nan")
    v = [1.0, None, None, None, None, 2.0, nan, None, None, -0.0, None]
    t = pa.table({"o": list(range(len(v))), "v": pa.array(v, pa.float64())})
    n = len(v)
    f = {"l%d" % k: ("ffill", "v", k) for k in (1, 3, 4, n, 10 ** 12)}
    f.update({"b%d" % k: ("bfill", "v", k) for k in (1, 3, 4, n)})
    check_nav(cpu, t, None, "o", True, f)
    got = Table(t, cpu).window(None, "o", True, f).to_arrow()
    assert got["l1"].to_pylist()[:6] == [1.0, 1.0, None, None, None, 2.0]
    assert got["l3"].to_pylist()[:6] == [1.0, 1.0, 1.0, 1.0, None, 2.0]  # the gap minus 1
    assert got["l4"].to_pylist()[:6] == [1.0] * 5 + [2.0]  # exactly the gap
    tail = got["l%d" % n].to_pylist()[6:]
    assert tail[0] != tail[0] and tail[1] != tail[1] and tail[2] != tail[2], tail  # NaN copied, 2.0 stopped
    assert str(tail[3]) == "-0.0" and str(tail[4]) == "-0.0", tail
    assert got["b3"].to_pylist()[:6] == [1.0, None, 2.0, 2.0, 2.0, 2.0]
    # descending order fills from the other side
    check_nav(cpu, t, None, "o", False, f)


def test_invalid_arguments(cpu):
    t = Table(pa.table({"g": [1, 1, 2], "o": [1, 2, 3], "v": pa.array([1, None, 3])}), cpu)
    for bad in (0, -1):
        with pytest.raises(Exception, match="nth_value"):
            t.window("g", "o", True, {"x": ("nth_value", "v", bad)})
        with pytest.raises(Exception, match="ntile"):
            t.window("g", "o", True, {"x": ("ntile", bad)})
    for fn in ("ffill", "bfill"):
        with pytest.raises(Exception, match="limit"):
            t.window("g", "o", True, {"x": (fn, "v", -1)})
    with pytest.raises(Exception, match="ignore_nulls"):
        t.window("g", "o", True, {"x": ("nth_value", "v", 1, True)})
    with pytest.raises(Exception, match="already exists"):
        t.window("g", "o", True, {"v": ("ffill", "v")})
    with pytest.raises(Exception, match="already exists"):
        t.window("g", "o", True, {None: "cume_dist", "cume_dist": "percent_rank"})
    with pytest.raises(KeyError):
        t.window("g", "o", True, {"x": ("ffill", "nope")})
    with pytest.raises(ValueError, match="expected"):
        t.window("g", "o", True, {"x": ("nth_value", "v")})
    with pytest.raises(ValueError, match="takes no argument"):
        t.window("g", "o", True, {"x": ("cume_dist", "v")})
    with pytest.raises(ValueError, match="limit must be greater than 0"):
        t.ffill(by="g", order_by="o", limit=0)
    nav = lambda funcs, cols, args, ign=(False,), lim=(0,): C.window_nav(  # noqa: E731
        t.native, [0], [1], [True], funcs, cols, args, ["x"], [0], [0], [0.0], [0.0], [False], [1], list(ign), list(lim))
    for col in (-1, 3):
        with pytest.raises(Exception, match="of column"):
            nav([22], [col], [0])
    with pytest.raises(Exception, match="window function"):
        nav([27], [2], [0])
    with pytest.raises(Exception, match="differ in length"):
        nav([22], [2], [0], ign=())
    # the older entry points still stop where they stopped
    with pytest.raises(Exception, match="window function"):
        C.window_range_frames(t.native, [0], [1], [True], [22], [2], [0], ["x"], [0], [0], [0.0], [0.0], [False], [1])
    with pytest.raises(Exception, match="window function"):
        C.window(t.native, [0], [1], [True], [19], [2], [0], ["x"])


def test_empty_table_and_default_names(cpu):
    e = pa.table({"g": pa.array([], pa.int64()), "o": pa.array([], pa.float64()), "v": pa.array([], pa.float32()),
                  "s": pa.array([], pa.string())})
    f = all_funcs()
    f["fs"] = ("ffill", "s")
    got = Table(e, cpu).window("g", "o", True, f).to_arrow()
    assert got.num_rows == 0 and got.column_names == e.column_names + list(f)
    want = [pa.float32()] * 10 + [pa.int64(), pa.float64(), pa.float64(), pa.string()]
    assert [got[c].type for c in f] == want
    t = pa.table({"g": [1, 1, 2], "v": pa.array([1, None, 3])})
    specs = [("first_value", "v"), ("last_value", "v"), ("nth_value", "v", 2), ("ffill", "v"), ("bfill", "v"),
             ("ntile", 2), "percent_rank", "cume_dist"]
    names = ["first_value_v", "last_value_v", "nth_value_v", "ffill_v", "bfill_v", "ntile", "percent_rank", "cume_dist"]
    for spec, name in zip(specs, names):
        got = Table(t, cpu).window("g", "v", True, {None: spec}).to_arrow()
        assert got.column_names == ["g", "v", name]
        assert_nav(got, t, "g", "v", True, {None: spec})


def test_mixed_calls_equal_the_separate_ones(cpu):
    t = _table(np.random.default_rng(8), N, "int64")
    old = {"cs": ("cumsum", "v"), "rs": ("rolling_sum", "v", 2, 1), "gs": ("range_sum", "v", 3, 0), "rk": "rank",
           "lg": ("lag", "v", 2)}
    new = all_funcs()
    tt = Table(t, cpu)
    both = tt.window("g", "o", True, {**old, **new}).to_arrow()
    assert both.select(t.column_names + list(old)).equals(tt.window("g", "o", True, old).to_arrow())
    assert both.select(t.column_names + list(new)).equals(tt.window("g", "o", True, new).to_arrow())
    assert_nav(both.select(t.column_names + list(new)), t, "g", "o", True, new)


def test_existing_specs_count_what_they_counted(cpu):
    """a call without a new spec reports no navigation counter and the scans it always ran"""
    t = _table(np.random.default_rng(9), N, "int64")
    f = {"cs": ("cumsum", "v"), "rs": ("rolling_sum", "v", 2, 1), "rk": "rank"}
    _, c = run_nav(cpu, t, "g", "o", True, f)
    assert c["window.scan"] == 4 and not any(k.startswith("window.nav") for k in c), c


def test_counters(cpu):
    t = _table(np.random.default_rng(10), N, "int64")
    c = check_nav(cpu, t, "g", "o", True, {"ff": ("ffill", "v"), "ff2": ("ffill", "v", 2), "lv": ("last_value", "v", True)})
    # the fill scan once, and the reversed rank scan for the tails LAST_VALUE reads
    assert c["window.nav.fill"] == 1 and c["window.scan"] == 2 and c["window.nav.gather"] == 0, c
    c = check_nav(cpu, t, "g", "o", True, {"ff": ("ffill", "v"), "bf": ("bfill", "v")})
    assert c["window.nav.fill"] == 2 and c["window.scan"] == 2, c
    d = pa.table({"g": t["g"], "o": t["o"], "v": pa.array(np.arange(N))})
    c = check_nav(cpu, d, "g", "o", True, {"ff": ("ffill", "v"), "bf": ("bfill", "v", 3), "lv": ("last_value", "v", True)})
    assert c["window.nav.fill"] == 0 and c["window.nav.skipped"] == 2 and c["window.scan"] == 1, c
    c = check_nav(cpu, t, "g", "o", True, {"nt": ("ntile", 4), "pr": "percent_rank", "cd": "cume_dist"})
    assert c["window.scan"] == 2 and c["window.nav.fill"] == 0, c  # one rank scan each way
    c = check_nav(cpu, t, "g", "o", True, {"fv": ("first_value", "v")})
    assert c["window.scan"] == 1, c


def test_table_frame_and_ops_surface(cpu):
    t = _table(np.random.default_rng(12), N, "float64")
    f = {"ff": ["ffill", "v", 2], "lv": ("last_value", "v", True), "cd": "cume_dist", "rn": "row_number"}
    nav = {k: s for k, s in f.items() if k != "rn"}
    tt = Table(t, cpu)
    keep = t.column_names + list(nav)
    assert_nav(tt.window("g", "o", True, f).to_arrow().select(keep), t, "g", "o", True, nav)
    assert_nav(ops.window(tt, "g", "o", True, f).to_arrow().select(keep), t, "g", "o", True, nav)
    assert_nav(ops.distributed_window(tt, "g", "o", True, f).to_arrow().select(keep), t, "g", "o", True, nav)
    assert_nav(DataFrame(t).window("g", "o", True, f).to_arrow().select(keep), t, "g", "o", True, nav)
    env = CylonEnv(distributed=False, device="cpu")
    assert_nav(DataFrame(t).window("g", "o", True, f, env=env).to_arrow().select(keep), t, "g", "o", True, nav)
    assert len(tt._window_nav_args("g", "o", True, f)) == 15
    # calls without a new spec go where they went
    assert len(tt._window_range_args("g", "o", True, {"r": ("range_sum", "v", 1, 0)})) == 13


@pytest.mark.parametrize("fn", ["ffill", "bfill"])
def test_dataframe_fill(cpu, fn):
    rng = np.random.default_rng(13)
    n = 200
    t = pa.table({"g": rng.integers(0, 5, n), "o": rng.permutation(n), "a": _values(rng, n, "float64", 0.4),
                  "s": _values(rng, n, "string", 0.4), "d": pa.array(np.arange(n))})
    df = DataFrame(t)
    got = getattr(df, fn)(by="g", order_by="o", limit=2).to_arrow()
    assert got.column_names == t.column_names
    exp = expected(t, "g", "o", True, {c: (fn, c, 2) for c in ("a", "s", "d")})
    want = pa.table({"g": t["g"], "o": t["o"], "a": pa.array(exp["a"], pa.float64()), "s": pa.array(exp["s"], pa.string()),
                     "d": t["d"]})
    assert_nav(got, want, None, None, True, {})
    # the named columns only; neither by nor order_by: input row order
    got = getattr(df, fn)(columns=["s"]).to_arrow()
    exp = expected(t, None, None, True, {"s": (fn, "s")})
    assert got.column_names == t.column_names and got["s"].to_pylist() == exp["s"]
    assert got["a"].null_count == t["a"].null_count
    # the Table underneath, positional columns
    got = getattr(Table(t, cpu), fn)(by=[0], order_by=[1], columns=[2]).to_arrow()
    assert got["a"].null_count == pa.array(expected(t, "g", "o", True, {"a": (fn, "a")})["a"]).null_count


def test_c_abi_window_nav(cpu):
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_init(b"cpu") == 0
    assert lib.cylon_read_csv(os.path.join(DATA, "csv1_0.csv").encode(), b"NAV_A") == 0
    whole = Table(context=cpu, _native=C.registry_get("NAV_A")).to_arrow()
    k, v = whole.column_names[0], whole.column_names[1]
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    names = (ctypes.c_char_p * 6)(b"ff", None, b"nth", b"nt", b"cd", b"lvi")
    rc = lib.cylon_window_nav(b"NAV_A", (i32 * 1)(0), 1, (i32 * 1)(1), (i32 * 1)(0), 1,
                              (i32 * 6)(22, 19, 21, 24, 26, 20), (i32 * 6)(1, 1, 1, -1, -1, 1),
                              (i64 * 6)(0, 0, 2, 3, 0, 0), None, None, None, None, None, None,
                              (i32 * 6)(0, 0, 0, 0, 0, 1), (i64 * 6)(1, 0, 0, 0, 0, 0), names, 6, 0, b"NAV_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=cpu, _native=C.registry_get("NAV_OUT")).to_arrow()
    f = {"ff": ("ffill", v, 1), "first_value_" + v: ("first_value", v), "nth": ("nth_value", v, 2), "nt": ("ntile", 3),
         "cd": "cume_dist", "lvi": ("last_value", v, True)}
    assert_nav(out, whole, k, v, False, f)
    # the two new arrays may be NULL, and the older functions pass through
    rc = lib.cylon_window_nav(b"NAV_A", (i32 * 1)(0), 1, (i32 * 1)(1), None, 1, (i32 * 2)(23, 0), (i32 * 2)(1, -1),
                              None, None, None, None, None, None, None, None, None, None, 2, 0, b"NAV_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=cpu, _native=C.registry_get("NAV_OUT")).to_arrow()
    assert out.column_names == whole.column_names + ["bfill_" + v, "row_number"]
    assert_nav(out.select(whole.column_names + ["bfill_" + v]), whole, k, v, True, {None: ("bfill", v)})
    for funcs, args, ign, lim, msg in (((i32 * 1)(27), None, None, None, b"window function"),
                                       ((i32 * 1)(21), (i64 * 1)(0), None, None, b"nth_value"),
                                       ((i32 * 1)(21), (i64 * 1)(1), (i32 * 1)(1), None, b"ignore_nulls"),
                                       ((i32 * 1)(22), None, None, (i64 * 1)(-2), b"limit")):
        assert lib.cylon_window_nav(b"NAV_A", (i32 * 1)(0), 1, (i32 * 1)(1), None, 1, funcs, (i32 * 1)(1), args, None,
                                    None, None, None, None, None, ign, lim, None, 1, 0, b"NAV_X") != 0
        assert msg in lib.cylon_last_error()
    assert lib.cylon_window_range_frames(b"NAV_A", None, 0, None, None, 0, (i32 * 1)(22), (i32 * 1)(1), None, None,
                                         None, None, None, None, None, None, 1, 0, b"NAV_X") != 0  # still stops at 18
    for t in (b"NAV_A", b"NAV_OUT"):
        assert lib.cylon_remove_table(t) == 0


def _global():
    n = 1500
    rng = np.random.default_rng(14)
    return pa.table({"g": rng.integers(0, 40, n), "o": rng.permutation(n),
                     "v": pa.array(rng.integers(-9, 9, n).astype(np.float64), mask=rng.random(n) < 0.4),
                     "s": _values(rng, n, "string", 0.4), "row": np.arange(n)})


DIST_FUNCS = {"ff": ("ffill", "v"), "ffs": ("ffill", "s", 1), "bf": ("bfill", "v", 2), "lv": ("last_value", "v", True),
              "nt": ("ntile", 4), "cd": "cume_dist", "pr": "percent_rank"}


def _dist(ctx):
    """rank r holds rows r, r + W, ... of the global table"""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    g = _global()
    tt = Table(g.take(pa.array(np.arange(rank, g.num_rows, world))), ctx)
    return tt.distributed_window("g", "o", True, DIST_FUNCS).to_arrow()


def test_distributed_window_with_ffill_two_ranks():
    res = run_distributed(_dist, 2)
    g = _global()
    on = [set(r["g"].to_pylist()) for r in res]  # every partition is on one rank
    assert on[0].isdisjoint(on[1]) and on[0] | on[1] == set(g["g"].to_pylist())
    # `o` is unique, so the window order does not depend on which rank held a row
    assert_nav(pa.concat_tables(res), g, "g", "o", True, DIST_FUNCS, row_id="row")
