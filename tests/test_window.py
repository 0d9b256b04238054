"""Window functions (ranking, running aggregates, lag / lead) on the CPU twin (kernels/cpu_window.cpp)
behind ops/window.cpp.  Every result is compared in input row order, null positions included, with an
oracle that does not use the engine (window_utils): float running sums against the exact prefix sum
under the gamma_m * A_m bound of docs/semantics.md, everything else with ==."""
import ctypes
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import cylon_amd.ops as ops
from cylon_amd import CylonContext, CylonEnv, DataFrame, Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from window_utils import assert_window, check_window, expected

DATA = os.path.join(os.path.dirname(__file__), "data", "input")
N = 700
RANKS = {"rn": "row_number", "rk": "rank", "dr": "dense_rank"}


def all_funcs(v, lag=2):
    return dict(RANKS, cnt=("cumcount", v), s=("cumsum", v), lo=("cummin", v), hi=("cummax", v),
                prev=("lag", v, lag), nxt=("lead", v, 1))


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _values(rng, dt, n):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return rng.integers(-1000, 1000, n).astype(dt) / dt.type(8)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v[:4] = [info.min, info.max, info.max, info.min]
    return v


@pytest.mark.parametrize("dt", ["int8", "int16", "int32", "int64", "uint32", "uint64", "float32", "float64"])
def test_every_function_on_every_value_type(cpu, dt):
    rng = np.random.default_rng(len(dt) + ord(dt[0]))
    t = pa.table({"g": rng.integers(0, 9, N), "o": rng.integers(0, 40, N), "v": _values(rng, dt, N)})
    c = check_window(cpu, t, "g", "o", True, all_funcs("v"))
    assert c["window.scan"] == 5, c  # one flags scan for the rankings and lag / lead, four value scans
    nv = pa.table({"g": t["g"], "o": t["o"], "v": pa.array(_values(rng, dt, N), mask=rng.random(N) < 0.3)})
    check_window(cpu, nv, "g", "o", False, all_funcs("v"))


def test_nullable_keys_nan_and_string_partitions(cpu):
    rng = np.random.default_rng(3)
    o = rng.integers(0, 6, N).astype(np.float64)
    o[rng.random(N) < 0.15] = np.nan
    o[rng.random(N) < 0.1] = -0.0
    v = rng.standard_normal(N)
    v[rng.random(N) < 0.1] = np.nan
    t = pa.table({"s": pa.array([None if x == 0 else "key-%d" % x for x in rng.integers(0, 7, N)]),
                  "g": pa.array(rng.integers(0, 3, N).astype(np.float64), mask=rng.random(N) < 0.2),
                  "o": pa.array(o, mask=rng.random(N) < 0.15),
                  "v": pa.array(v, mask=rng.random(N) < 0.2),
                  "i": rng.integers(-5, 5, N)})
    minmax = dict(RANKS, cnt=("cumcount", "v"), lo=("cummin", "v"), hi=("cummax", "v"), prev=("lag", "v", 1),
                  si=("cumsum", "i"), ps=("lead", "s", 2))
    for asc in (True, False):
        check_window(cpu, t, "s", "o", asc, minmax)           # string partition key with nulls
        check_window(cpu, t, ["s", "g"], ["o", "i"], [asc, not asc], minmax)  # two and two, mixed directions
        check_window(cpu, t, "g", "o", asc, minmax)           # nullable float partition key


def test_empty_partition_and_order_lists(cpu):
    rng = np.random.default_rng(4)
    t = pa.table({"g": rng.integers(0, 5, N), "o": rng.integers(0, 30, N), "v": rng.integers(-9, 9, N)})
    f = all_funcs("v")
    assert check_window(cpu, t, None, "o", False, f)["window.sort"] == 1   # one partition, ordered
    assert check_window(cpu, t, "g", None, True, f)["window.sort"] == 1    # partitions in input row order
    assert check_window(cpu, t, None, None, True, f)["window.sort"] == 0   # a plain running scan over the table
    got = Table(t, cpu).window(funcs={"s": ("cumsum", "v"), "rn": "row_number", "rk": "rank"}).to_arrow()
    assert got["s"].to_pylist() == list(np.cumsum(t["v"].to_numpy()))
    assert got["rn"].to_pylist() == list(range(1, N + 1)) and set(got["rk"].to_pylist()) == {1}


def test_peers_rank_dense_rank_row_number_differ(cpu):
    t = pa.table({"g": [1, 1, 1, 1, 1, 1, 2, 2], "o": [5, 5, 7, 7, 7, 9, 5, 5]})
    got = Table(t, cpu).window("g", "o", True, RANKS).to_arrow()
    assert got["rn"].to_pylist() == [1, 2, 3, 4, 5, 6, 1, 2]
    assert got["rk"].to_pylist() == [1, 1, 3, 3, 3, 6, 1, 1]
    assert got["dr"].to_pylist() == [1, 1, 2, 2, 2, 3, 1, 1]
    check_window(cpu, t, "g", "o", True, RANKS)
    check_window(cpu, t, "g", "o", False, RANKS)


def test_integer_cumsum_wraps(cpu):
    big = (1 << 62) + 5
    t = pa.table({"g": [0, 0, 0, 0, 1, 1], "v": pa.array([big, big, big, -big, big, 7], pa.int64()),
                  "u": pa.array([1 << 63, 1 << 63, 5, 1, (1 << 64) - 1, 1], pa.uint64())})
    got = Table(t, cpu).window("g", None, True, {"s": ("cumsum", "v"), "su": ("cumsum", "u")}).to_arrow()
    assert got["s"].to_pylist()[:4] == [big, 2 * big - (1 << 64), 3 * big - (1 << 64), 2 * big - (1 << 64)]
    assert got["su"].to_pylist() == [1 << 63, 0, 5, 6, (1 << 64) - 1, 0]
    check_window(cpu, t, "g", None, True, {"s": ("cumsum", "v"), "su": ("cumsum", "u")})


def exact_float_table(rng, n, groups):
    """integer-valued float64, every prefix (in any order) below 2^53: any summation order is exact"""
    return pa.table({"g": rng.integers(0, groups, n), "o": rng.permutation(n),
                     "v": rng.integers(0, 1 << 30, n).astype(np.float64)})


def cancellation_table(n_big, n_small):
    """a partition of values near 1e16 sorts immediately before a partition of values near 1: a running
    sum formed as a global prefix minus an offset would lose every digit of the second partition"""
    rng = np.random.default_rng(5)
    big = 1e16 * (1 + rng.random(n_big))
    small = 1 + rng.random(n_small)
    g = np.concatenate([np.zeros(n_big, np.int64), np.ones(n_small, np.int64)])
    p = rng.permutation(n_big + n_small)
    return pa.table({"g": g[p], "o": rng.permutation(n_big + n_small), "v": np.concatenate([big, small])[p]})


def test_float_cumsum_exact_and_under_cancellation(cpu):
    t = exact_float_table(np.random.default_rng(6), N, 4)
    got = Table(t, cpu).window("g", "o", True, {"s": ("cumsum", "v")}).to_arrow()
    want = expected(t, "g", "o", True, {"s": ("cumsum", "v")})["s"]
    assert got["s"].to_pylist() == [float(e[0]) for e in want]  # ==: every order is exact here
    c = cancellation_table(400, 300)
    check_window(cpu, c, "g", "o", True, {"s": ("cumsum", "v")})  # each row to the bound of its own partition


def test_lag_lead_offsets_on_a_string_column(cpu):
    rng = np.random.default_rng(7)
    n = 60
    t = pa.table({"g": np.repeat(np.arange(3), 20), "o": rng.permutation(n),
                  "s": pa.array([None if i % 7 == 0 else "s%02d" % i for i in range(n)])})
    for off in (0, 1, 19, 20, 21, 10 ** 15):
        check_window(cpu, t, "g", "o", True, {"a": ("lag", "s", off), "b": ("lead", "s", off)})
    got = Table(t, cpu).window("g", "o", True, {"a": ("lag", "s", 0), "z": ("lead", "s", 20)}).to_arrow()
    assert got["a"].to_pylist() == t["s"].to_pylist() and got["z"].null_count == n
    assert got.schema.field("a").type == pa.string() or got.schema.field("a").type == pa.large_string()


def test_errors(cpu):
    t = pa.table({"g": [1, 2], "s": ["a", "b"], "v": [1.0, 2.0]})
    tt = Table(t, cpu)
    for fn in ("cumsum", "cummin", "cummax"):
        with pytest.raises(Exception, match="numeric"):
            tt.window("g", None, True, {"x": (fn, "s")})
    with pytest.raises(Exception, match="offset"):
        tt.window("g", None, True, {"x": ("lag", "v", -1)})
    with pytest.raises(Exception, match="already exists"):
        tt.window("g", None, True, {"v": "row_number"})          # collides with an input column
    with pytest.raises(Exception, match="already exists"):
        C.window(tt.native, [0], [], [], [0, 1], [-1, -1], [0, 0], ["x", "x"])  # two outputs, one name
    with pytest.raises(ValueError):
        tt.window("g", None, True, {"x": "median"})
    with pytest.raises(ValueError):
        tt.window("g", None, True, {"x": ("median", "v")})
    with pytest.raises(KeyError):
        tt.window("g", None, True, {"x": ("cumsum", "missing")})
    with pytest.raises(KeyError):
        tt.window("missing", None, True, {"x": "rank"})
    with pytest.raises(Exception, match="window function"):
        C.window(tt.native, [0], [], [], [9], [-1], [0], ["x"])


def test_empty_table_empty_specs_and_default_names(cpu):
    t = pa.table({"g": pa.array([], pa.int32()), "txt": pa.array([], pa.string()), "v": pa.array([], pa.float32())})
    f = dict(all_funcs("v"), ps=("lag", "txt", 1))
    got = Table(t, cpu).window("g", "v", True, f).to_arrow()
    assert got.num_rows == 0 and got.column_names == t.column_names + list(f)
    assert [got.schema.field(n).type for n in ("rn", "rk", "dr", "cnt")] == [pa.int64()] * 4
    assert got.schema.field("s").type == pa.float64() and got.schema.field("ps").type == t.schema.field("txt").type
    assert got.schema.field("lo").type == pa.float32() and got.schema.field("prev").type == pa.float32()
    full = pa.table({"g": [1, 1, 2], "v": [1.5, 2.5, 4.0]})
    tt = Table(full, cpu)
    same = tt.window("g", "v", True, {}).to_arrow()
    assert same.equals(full)
    named = C.window(tt.native, [0], [1], [True], [0, 1, 2, 3, 4, 5, 6, 7, 8], [-1, -1, -1, 1, 1, 1, 1, 1, 1],
                     [0, 0, 0, 0, 0, 0, 0, 1, 1], [""] * 9)
    assert named.column_names()[2:] == ["row_number", "rank", "dense_rank", "cumcount_v", "cumsum_v", "cummin_v",
                                        "cummax_v", "lag_v", "lead_v"]


def test_table_frame_and_ops_surface(cpu):
    rng = np.random.default_rng(8)
    t = pa.table({"g": rng.integers(0, 6, N), "o": rng.integers(0, 50, N), "v": rng.integers(-99, 99, N)})
    f = {"rn": "row_number", "s": ("cumsum", "v"), "p": ("lag", "v", 2)}
    tt = Table(t, cpu)
    assert_window(tt.window("g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    assert_window(tt.window(partition_by=["g"], order_by=["o"], ascending=[False], funcs=f).to_arrow(), t, "g", "o",
                  False, f)
    assert_window(ops.window(tt, "g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    assert_window(ops.distributed_window(tt, "g", "o", True, f).to_arrow(), t, "g", "o", True, f)  # world 1
    assert_window(ops.distributed_window(tt, None, "o", True, f).to_arrow(), t, None, "o", True, f)  # ... no key needed
    assert_window(DataFrame(t).window("g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    env = CylonEnv(distributed=False, device="cpu")  # world 1: the local operator
    assert_window(DataFrame(t).window("g", "o", True, f, env=env).to_arrow(), t, "g", "o", True, f)
    assert C.window_tile_rows() > 0 and C.window_carry_tiles() > 0


def test_dataframe_window_matches_pandas():
    rng = np.random.default_rng(9)
    df = pd.DataFrame({"g": rng.integers(0, 8, N), "o": rng.integers(0, 25, N), "v": rng.integers(-50, 50, N),
                       "x": rng.integers(0, 1 << 20, N).astype(np.float64)})
    got = DataFrame(pa.Table.from_pandas(df, preserve_index=False)).window(
        "g", "o", True, {"rn": "row_number", "rk": "rank", "dr": "dense_rank", "s": ("cumsum", "v"),
                         "sx": ("cumsum", "x"), "lo": ("cummin", "v"), "hi": ("cummax", "v"),
                         "p": ("lag", "v", 1), "q": ("lead", "v", 2)}).to_arrow().to_pandas()
    by = df.sort_values(["g", "o"], kind="stable")
    grp = by.groupby("g")
    assert got["s"].equals(grp["v"].cumsum().sort_index())
    assert got["sx"].equals(grp["x"].cumsum().sort_index())
    assert got["lo"].equals(grp["v"].cummin().sort_index()) and got["hi"].equals(grp["v"].cummax().sort_index())
    assert got["rk"].equals(grp["o"].rank(method="min").sort_index().astype(np.int64))
    assert got["dr"].equals(grp["o"].rank(method="dense").sort_index().astype(np.int64))
    assert got["rn"].equals(grp["o"].rank(method="first").sort_index().astype(np.int64))
    assert got["rn"].equals((grp.cumcount() + 1).sort_index())
    for name, k in (("p", 1), ("q", -2)):
        want = grp["v"].shift(k).sort_index()
        assert got[name].isna().equals(want.isna()) and (got[name].dropna() == want.dropna()).all()


def test_c_abi_window(ctx):
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_capi_version() == 1
    assert lib.cylon_init(b"cpu") == 0
    assert lib.cylon_read_csv(os.path.join(DATA, "csv1_0.csv").encode(), b"WIN_A") == 0
    whole = Table(context=ctx, _native=C.registry_get("WIN_A")).to_arrow()
    k, v = whole.column_names[0], whole.column_names[1]
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    names = (ctypes.c_char_p * 3)(b"rn", None, b"prev")
    rc = lib.cylon_window(b"WIN_A", (i32 * 1)(0), 1, (i32 * 1)(1), (i32 * 1)(0), 1, (i32 * 3)(0, 4, 7),
                          (i32 * 3)(-1, 1, 1), (i64 * 3)(0, 0, 1), names, 3, 0, b"WIN_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=ctx, _native=C.registry_get("WIN_OUT")).to_arrow()
    f = {"rn": "row_number", "cumsum_" + v: ("cumsum", v), "prev": ("lag", v, 1)}
    assert_window(out, whole, k, v, False, f)
    assert lib.cylon_window(b"WIN_A", None, 0, None, None, 0, (i32 * 1)(2), None, None, None, 1, 1, b"WIN_OUT") == 0
    assert Table(context=ctx, _native=C.registry_get("WIN_OUT")).to_arrow().column_names[-1] == "dense_rank"
    assert lib.cylon_window(b"WIN_A", None, 0, None, None, 0, (i32 * 1)(42), None, None, None, 1, 0, b"WIN_X") != 0
    assert lib.cylon_window(b"WIN_A", None, 0, None, None, 0, (i32 * 1)(7), (i32 * 1)(1), (i64 * 1)(-3), None, 1, 0,
                            b"WIN_X") != 0
    rc = lib.cylon_window(b"WIN_missing", None, 0, None, None, 0, (i32 * 1)(0), None, None, None, 1, 0, b"WIN_X")
    assert rc != 0 and b"WIN_missing" in lib.cylon_last_error()
    for t in (b"WIN_A", b"WIN_OUT"):
        assert lib.cylon_remove_table(t) == 0


def test_cpp_example_prints_the_window_rows(tmp_path):
    """examples/cpp/relational_example.cpp: Window keeps every row of its input"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "cpp", "bin", "relational_example")
    if not os.path.exists(exe):
        pytest.fail("examples/cpp/bin/relational_example missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "cpu", os.path.join(DATA, "csv1_0.csv"), os.path.join(DATA, "csv2_0.csv"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(line.split() for line in r.stdout.splitlines())
    assert got["window"] == got["left"] and int(got["window"]) > 0, got


def _global():
    """unique order keys: the window order does not depend on the order the shuffled rows arrive in"""
    n = 1500
    rng = np.random.default_rng(10)
    return pa.table({"g": rng.integers(0, 40, n), "o": rng.permutation(n),
                     "v": pa.array(rng.integers(-9, 9, n).astype(np.float64), mask=rng.random(n) < 0.1),
                     "txt": pa.array(["s%d" % i for i in range(n)]), "row": np.arange(n)})


DIST_FUNCS = dict(all_funcs("v"), ps=("lag", "txt", 1))


def _dist(ctx, case):
    """rank r holds rows r, r + W, ... of the global table"""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    g = _global()
    tt = Table(g.take(pa.array(np.arange(rank, g.num_rows, world))), ctx)
    if case == "no_key":
        try:
            tt.distributed_window(None, "o", True, {"rn": "row_number"})
        except Exception as e:  # the same error on every rank, before any exchange
            return str(e)
        return "no error"
    return tt.distributed_window("g", "o", False, DIST_FUNCS).to_arrow()


def test_distributed_window_two_ranks():
    res = run_distributed(_dist, 2, "keyed")
    g = _global()
    on = [set(r["g"].to_pylist()) for r in res]  # every partition is on one rank
    assert on[0].isdisjoint(on[1]) and on[0] | on[1] == set(g["g"].to_pylist())
    assert_window(pa.concat_tables(res), g, "g", "o", False, DIST_FUNCS, row_id="row")


def test_distributed_window_needs_a_partition_column():
    res = run_distributed(_dist, 2, "no_key")
    assert all("partition column" in r for r in res), res
