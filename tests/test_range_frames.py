"""RANGE frames (RANGE BETWEEN a PRECEDING AND b FOLLOWING over the one order column's values) on the CPU
context: the sequential twin kernels/cpu_frame_range.cpp behind ops/window.cpp, against the
engine-independent oracle (range_frame_utils), plus the error cases and the Table / DataFrame / ops /
C ABI / distributed surfaces."""
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
from range_frame_utils import assert_range, check_range, expected
from rolling_utils import assert_rolling

DATA = os.path.join(os.path.dirname(__file__), "data", "input")
N = 700
INT_TYPES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"]


def five(v, p, f, minp=1):
    return {"c": ("range_count", v, p, f), "s": ("range_sum", v, p, f, minp), "m": ("range_mean", v, p, f, minp),
            "lo": ("range_min", v, p, f, minp), "hi": ("range_max", v, p, f, minp)}


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _values(rng, n, dt, nulls=0.25):
    dt = np.dtype(dt)
    if dt.kind == "f":
        v = (rng.integers(-4000, 4000, n) / 16).astype(dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(max(info.min, -1000), min(info.max, 1000), n).astype(dt)
    return pa.array(v, mask=rng.random(n) < nulls) if nulls else pa.array(v)


def _table(rng, n, groups, key_dt=np.int64, val_dt=np.int64, spread=None, key_nulls=0.0):
    """keys in [0, spread): ties when spread < n, gaps wider than a small offset when spread >> n"""
    key_dt = np.dtype(key_dt)
    spread = spread or n // 2 + 1
    if key_dt.kind == "f":
        o = (rng.integers(0, 4 * spread, n) / 4).astype(key_dt)
    else:
        o = rng.integers(0, min(spread, np.iinfo(key_dt).max), n).astype(key_dt)
    o = pa.array(o, mask=rng.random(n) < key_nulls) if key_nulls else pa.array(o)
    return pa.table({"g": rng.integers(0, groups, n), "o": o, "v": _values(rng, n, val_dt)})


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("frame", [(0, 0), (1, 0), (0, 1), (2, 3), (40, 0), (0, 64), (None, 0), (0, None),
                                   (None, None), (10 ** 15, 1)], ids=str)
def test_frames_against_the_oracle(cpu, frame, asc):
    rng = np.random.default_rng(1)
    for n, groups in ((1, 1), (65, 3), (N, 1), (N, 9), (N, N)):
        check_range(cpu, _table(rng, n, groups), "g", "o", asc, five("v", *frame))
    check_range(cpu, _table(rng, N, 4), None, "o", asc, five("v", *frame))  # no partition column
    check_range(cpu, _table(rng, N, 4, key_nulls=0.1), "g", "o", asc, five("v", *frame))  # null keys


@pytest.mark.parametrize("spread", [1, 5, 10 ** 6], ids=["all_equal", "ties", "gaps"])
def test_key_patterns(cpu, spread):
    """all keys equal: the frame is the partition; gaps wider than the offset: the frame is one row"""
    rng = np.random.default_rng(2)
    t = _table(rng, N, 5, spread=spread)
    c = check_range(cpu, t, "g", "o", True, five("v", 2, 1))
    assert c["window.range.bounds"] == 1, c
    got = Table(t, cpu).window("g", "o", True, {"n": ("range_count", "g", 2, 1), "all": ("cumcount", "g")}).to_arrow()
    sizes = pd.Series(t["g"].to_pylist()).value_counts()
    if spread == 1:
        assert got["n"].to_pylist() == [sizes[g] for g in t["g"].to_pylist()]
    if spread == 10 ** 6:
        assert np.mean(np.array(got["n"].to_pylist()) == 1) > 0.95


@pytest.mark.parametrize("dt", INT_TYPES + ["float32", "float64"])
def test_value_and_key_types(cpu, dt):
    rng = np.random.default_rng(3)
    check_range(cpu, _table(rng, N, 5, val_dt=dt), "g", "o", True, five("v", 3, 2))
    t = _table(rng, N, 5, key_dt=dt, spread=100)
    for asc in (True, False):
        check_range(cpu, t, "g", "o", asc, five("v", 3, 2))
        if np.dtype(dt).kind == "f":
            check_range(cpu, t, "g", "o", asc, five("v", 0.75, 2))
            check_range(cpu, t, "g", "o", asc, five("v", None, 0.5))


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_timestamp_keys_take_offsets_in_their_unit(cpu, unit):
    rng = np.random.default_rng(4)
    ts = pa.array(rng.integers(0, 3000, N), pa.timestamp(unit))
    t = pa.table({"g": rng.integers(0, 4, N), "o": ts, "v": _values(rng, N, np.float64)})
    for asc in (True, False):
        check_range(cpu, t, "g", "o", asc, five("v", 5, 0))
    for typ in (pa.date32(), pa.time32("s"), pa.duration("ms"), pa.date64()):
        base = rng.integers(0, 300, N)
        col = pa.array(base * (86_400_000 if typ == pa.date64() else 1), pa.int64()).cast(
            pa.int32() if typ.bit_width == 32 else pa.int64()).cast(typ)
        off = 5 * (86_400_000 if typ == pa.date64() else 1)
        check_range(cpu, t.set_column(1, "o", col), "g", "o", True, five("v", off, off))


@pytest.mark.parametrize("asc", [True, False])
def test_int64_and_uint64_keys_at_their_extremes(cpu, asc):
    """o - a and o + b are mathematical integers: the lowest int64 with a = 5 has nothing below it"""
    rng = np.random.default_rng(5)
    lo, hi = -2 ** 63, 2 ** 63 - 1
    k = np.array([lo, lo, lo + 1, lo + 5, lo + 6, -1, 0, 1, hi - 6, hi - 5, hi - 1, hi, hi] * 20, np.int64)
    t = pa.table({"g": rng.integers(0, 2, len(k)), "o": k, "v": _values(rng, len(k), np.int32)})
    for frame in ((5, 0), (0, 5), (5, 5), (hi - 1, hi - 1), (hi - 1, 0), (None, 2)):
        check_range(cpu, t, "g", "o", asc, five("v", *frame))
    got = Table(t, cpu).window(None, "o", True, {"n": ("range_count", "o", 5, 0)}).to_arrow()
    assert got["n"].to_pylist()[0] == 40  # the two lowest keys' rows: nothing wrapped round from the top
    top = 2 ** 64 - 1
    u = np.array([0, 1, 5, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 3, top - 5, top - 1, top, top] * 20, np.uint64)
    t = pa.table({"g": rng.integers(0, 2, len(u)), "o": u, "v": _values(rng, len(u), np.int32)})
    for frame in ((5, 0), (0, 5), (4, 3), (hi - 1, hi - 1), (2 ** 62, 2 ** 62)):
        check_range(cpu, t, "g", "o", asc, five("v", *frame))


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_special_float_keys(cpu, dt, asc):
    """+-inf rows get their peers, and a finite row's frame the +-inf rows on a side whose offset is +inf;
    -0.0 == +0.0; NaN and null keys frame their own peer groups; UNBOUNDED is positional"""
    rng = np.random.default_rng(6)
    inf, nan = np.inf, np.nan
    k = np.array([-inf, -inf, -2.5, -0.0, 0.0, 0.0, 1.0, 1.5, 3.0, inf, inf, inf, nan, nan, -0.0, 1e30, -1e30] * 12, dt)
    keys = pa.array(k, mask=rng.random(len(k)) < 0.15)
    t = pa.table({"g": rng.integers(0, 3, len(k)), "o": keys, "v": _values(rng, len(k), np.float64)})
    for frame in ((0, 0), (0.0, 0.0), (1.5, 1), (inf, 0.0), (0.0, inf), (inf, inf), (None, 0), (0, None), (None, None),
                  (None, inf), (1e308, 1e308), (2, None)):
        check_range(cpu, t, "g", "o", asc, five("v", *frame))
    one = pa.table({"o": pa.array([-inf, -0.0, 0.0, 2.0, inf, nan, nan, None, None, None], pa.from_numpy_dtype(dt)),
                    "v": [1] * 10})
    n = lambda p, f: Table(one, cpu).window(None, "o", True, {"n": ("range_count", "v", p, f)}).to_arrow()["n"].to_pylist()
    assert n(0, 0) == [1, 2, 2, 1, 1, 2, 2, 3, 3, 3]
    assert n(inf, 0.0) == [1, 3, 3, 4, 1, 2, 2, 3, 3, 3]   # -inf joins the finite rows; +inf keeps its peers
    assert n(0.0, inf) == [1, 4, 4, 2, 1, 2, 2, 3, 3, 3]   # ... and +inf does, but no NaN and no null
    assert n(0, None) == [10, 9, 9, 7, 6, 5, 5, 3, 3, 3]   # unbounded following holds the NaN and null rows
    assert n(None, 0) == [1, 3, 3, 4, 5, 7, 7, 10, 10, 10]  # unbounded preceding of a null: up to its last null


def test_min_periods_nulls_and_wrapping_integer_sums(cpu):
    rng = np.random.default_rng(7)
    t = _table(rng, N, 6, spread=60)
    for minp in (1, 3):
        for frame in ((1, 1), (None, None)):
            check_range(cpu, t, "g", "o", True, five("v", *frame, minp))
    allnull = t.set_column(2, "v", pa.array([None] * N, pa.int64()))
    got = Table(allnull, cpu).window("g", "o", True, five("v", 1, 1)).to_arrow()
    assert got["s"].null_count == N and got["c"].null_count == 0 and set(got["c"].to_pylist()) == {0}
    for dt in ("int64", "uint64"):
        info = np.iinfo(dt)
        big = pa.table({"g": rng.integers(0, 3, N), "o": rng.integers(0, 50, N),
                        "v": rng.integers(info.min, info.max, N, dtype=dt, endpoint=True)})
        f = five("v", 4, 4)
        del f["m"]
        check_range(cpu, big, "g", "o", True, f)


@pytest.mark.parametrize("frame", [(0, 0), (3, 0), (2, 5), (100, 40), (None, 0), (None, None)], ids=str)
def test_consecutive_keys_make_range_frames_rows_frames(cpu, frame):
    """a distinct consecutive integer key per partition: RANGE (a, b) is ROWS (a, b)"""
    rng = np.random.default_rng(8)
    g = rng.integers(0, 7, N)
    o = np.zeros(N, np.int64)
    for k in range(7):
        idx = np.flatnonzero(g == k)
        o[idx] = rng.permutation(len(idx)) + 1000 * k
    for dt in (np.int64, np.float64):
        t = pa.table({"g": g, "o": o, "v": _values(rng, N, dt)})
        for asc in (True, False):
            rng_f = five("v", *frame)
            roll_f = {k: ("rolling_" + s[0][6:],) + s[1:] for k, s in rng_f.items()}
            got = Table(t, cpu).window("g", "o", asc, rng_f).to_arrow()
            assert_rolling(got, t, "g", "o", asc, roll_f)  # the ROWS oracle
            rows = Table(t, cpu).window("g", "o", asc, roll_f).to_arrow()
            if dt is np.int64:
                for name in ("c", "s", "lo", "hi"):
                    assert got[name].equals(rows[name]), name


def test_matches_pandas_groupby_rolling_5s_closed_both():
    rng = np.random.default_rng(9)
    secs = rng.permutation(6 * N)[:N]  # unique timestamps
    df = pd.DataFrame({"g": rng.integers(0, 8, N), "o": pd.to_datetime(secs, unit="s"),
                       "v": rng.integers(-50, 50, N).astype(np.float64)})
    df.loc[rng.random(N) < 0.2, "v"] = np.nan  # integer-valued floats with nulls: sums are exact
    t = pa.Table.from_pandas(df, preserve_index=False)
    unit = 10 ** {"s": 0, "ms": 3, "us": 6, "ns": 9}[t["o"].type.unit]
    got = DataFrame(t).window("g", "o", True, five("v", 5 * unit, 0)).to_arrow().to_pandas()
    by = df.sort_values(["g", "o"], kind="stable")
    roll = by.set_index("o").groupby("g")["v"].rolling("5s", closed="both", min_periods=1)
    for name, want in (("s", roll.sum()), ("lo", roll.min()), ("hi", roll.max()), ("m", roll.mean()),
                       ("c", roll.count())):
        want = pd.Series(want.to_numpy(), index=by.index).sort_index()
        if name == "c":
            assert (got[name] == want.astype(np.int64)).all(), name
            continue
        live = got["c"] > 0
        assert got[name].isna().equals(~live), name
        if name == "m":
            assert np.allclose(got[name][live], want[live], rtol=1e-12, atol=1e-12), name
        else:
            assert (got[name][live] == want[live]).all(), name


def test_mixed_specs_equal_the_single_calls(cpu):
    rng = np.random.default_rng(10)
    t = _table(rng, N, 5, val_dt=np.float64)
    f = {"rn": "row_number", "r": ("range_sum", "v", 3, 0), "cs": ("cumsum", "v"), "roll": ("rolling_max", "v", 2, 2),
         "prev": ("lag", "v", 2), "m": ("range_mean", "v", 3, 0, 2), "k": ("range_min", "o", None, 1)}
    c = check_range(cpu, t, "g", "o", True, f)
    assert c["window.frame.range"] == 3 and c["window.range.bounds"] == 2 and c["window.frame.lds"] == 1, c
    whole = Table(t, cpu).window("g", "o", True, f).to_arrow()
    for name, spec in f.items():
        assert Table(t, cpu).window("g", "o", True, {name: spec}).to_arrow()[name].equals(whole[name]), name


def test_specs_that_share_a_frame_share_one_bounds_search(cpu):
    rng = np.random.default_rng(11)
    t = _table(rng, N, 5)
    c = check_range(cpu, t, "g", "o", True, five("v", 4, 2))
    assert c["window.range.bounds"] == 1 and c["window.frame.range"] == 5, c
    assert c["window.range.pyramids"] == 4, c  # count (the nulls), sum, min, max; the mean shares the sum's
    c = check_range(cpu, t, "g", "o", True, dict(five("v", 4, 2), x=("range_sum", "v", 4, 3)))
    assert c["window.range.bounds"] == 2 and c["window.range.pyramids"] == 4, c
    assert C.window_range_radix() == 8 and C.window_range_halo() >= 8


def test_errors(cpu):
    t = Table(pa.table({"g": [1, 1, 2], "v": [1, 2, 3], "s": ["a", "b", "c"], "f": [0.5, 1.5, 2.5],
                        "h": pa.array(np.array([1, 2, 3], np.float16)), "b": [True, False, True]}), cpu)
    ok = t.window("g", "v", True, {"x": ("range_sum", "v", 1, 0)}).to_arrow()["x"].to_pylist()
    assert ok == [1, 3, 3]
    with pytest.raises(Exception, match="preceding"):
        t.window("g", "v", True, {"x": ("range_sum", "v", -1, 0)})
    with pytest.raises(Exception, match="following"):
        t.window("g", "v", True, {"x": ("range_max", "v", 0, -2)})
    for frame in ((-0.5, 0.0), (0.0, -1.0), (float("nan"), 0.0), (1.0, float("nan"))):
        with pytest.raises(Exception, match="preceding"):
            t.window("g", "f", True, {"x": ("range_sum", "v", *frame)})
    with pytest.raises(Exception, match="float offset"):  # on an integer order column
        t.window("g", "v", True, {"x": ("range_sum", "v", 1.0, 0)})
    assert t.window("g", "f", True, {"x": ("range_sum", "v", 1, 0)}).row_count == 3  # an int on a float column
    with pytest.raises(Exception, match="min_periods"):
        t.window("g", "v", True, {"x": ("range_sum", "v", 1, 0, 0)})
    with pytest.raises(Exception, match="fixed-width numeric"):
        t.window("g", "v", True, {"x": ("range_sum", "s", 1, 0)})
    for fn in ("range_sum", "range_mean"):
        with pytest.raises(Exception, match="fixed-width numeric"):
            t.window("g", "v", True, {"x": (fn, "h", 1, 0)})
    assert t.window("g", "v", True, {"x": ("range_max", "h", 1, 0), "n": ("range_count", "s", 1, 0)}).row_count == 3
    got = t.window("g", "v", True, {"n": ("range_count", "s", 1, 0, -3)})  # RANGE_COUNT ignores min_periods
    assert got.to_arrow()["n"].to_pylist() == [1, 2, 1]
    # exactly one order column, of an accepted type
    with pytest.raises(Exception, match="exactly one order column"):
        t.window("g", None, True, {"x": ("range_sum", "v", 1, 0)})
    with pytest.raises(Exception, match="exactly one order column"):
        t.window("g", ["v", "f"], True, {"x": ("range_sum", "v", 1, 0)})
    for bad in ("s", "h", "b"):
        with pytest.raises(Exception, match="order column"):
            t.window("g", bad, True, {"x": ("range_sum", "v", 1, 0)})
    with pytest.raises(Exception, match="already exists"):
        t.window("g", "v", True, {"v": ("range_sum", "v", 1, 0)})
    with pytest.raises(Exception, match="already exists"):
        t.window("g", "v", True, {None: ("range_sum", "v", 1, 0), "range_sum_v": ("range_max", "v", 1, 0)})
    with pytest.raises(ValueError, match="preceding, following"):
        t.window("g", "v", True, {"x": ("range_sum", "v", 1)})
    for bad in (True, "5s", [1]):
        with pytest.raises(ValueError, match="offset"):
            t.window("g", "v", True, {"x": ("range_sum", "v", bad, 0)})
    with pytest.raises(ValueError, match="unknown window function"):
        t.window("g", "v", True, {"x": ("range_median", "v", 1, 0)})
    with pytest.raises(KeyError):
        t.window("g", "v", True, {"x": ("range_sum", "nope", 1, 0)})
    # the older entry points still stop where they stopped
    with pytest.raises(Exception, match="window function"):
        C.window_frames(t.native, [0], [1], [True], [15], [1], [0], ["x"], [1], [0], [1])
    with pytest.raises(Exception, match="window function"):
        C.window_range_frames(t.native, [0], [1], [True], [19], [1], [0], ["x"], [1], [0], [0.0], [0.0], [False], [1])
    with pytest.raises(Exception, match="differ in length"):
        C.window_range_frames(t.native, [0], [1], [True], [15], [1], [0], ["x"], [1], [0], [0.0], [], [False], [1])


def test_empty_table_and_default_names(cpu):
    e = pa.table({"g": pa.array([], pa.int64()), "o": pa.array([], pa.float64()), "v": pa.array([], pa.float32())})
    f = {"a": ("range_count", "v", 1, 1), "b": ("range_sum", "v", 1, 1), "c": ("range_mean", "v", 1, 1),
         "d": ("range_min", "v", 1, 1)}
    got = Table(e, cpu).window("g", "o", True, f).to_arrow()
    assert got.num_rows == 0 and got.column_names == ["g", "o", "v", "a", "b", "c", "d"]
    assert [got[c].type for c in "abcd"] == [pa.int64(), pa.float64(), pa.float64(), pa.float32()]
    t = pa.table({"g": [1, 1, 2], "v": [1, 2, 3]})
    for fn in ("range_count", "range_sum", "range_mean", "range_min", "range_max"):
        got = Table(t, cpu).window("g", "v", True, {None: (fn, "v", 1, 0)}).to_arrow()
        assert got.column_names == ["g", "v", fn + "_v"]
        assert_range(got, t, "g", "v", True, {None: (fn, "v", 1, 0)})


def test_table_frame_and_ops_surface(cpu):
    rng = np.random.default_rng(12)
    t = _table(rng, N, 6)
    f = {"rn": "row_number", "r": ("range_sum", "v", 3, 0), "m": ["range_mean", "v", None, None, 2]}
    tt = Table(t, cpu)
    assert_range(tt.window("g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    assert_range(tt.window(partition_by=["g"], order_by=["o"], ascending=[False], funcs=f).to_arrow(), t, "g", "o",
                 False, f)
    assert_range(ops.window(tt, "g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    assert_range(ops.distributed_window(tt, "g", "o", True, f).to_arrow(), t, "g", "o", True, f)  # world 1
    assert_range(DataFrame(t).window("g", "o", True, f).to_arrow(), t, "g", "o", True, f)
    env = CylonEnv(distributed=False, device="cpu")
    assert_range(DataFrame(t).window("g", "o", True, f, env=env).to_arrow(), t, "g", "o", True, f)
    assert len(tt._window_range_args("g", "o", True, f)) == 13
    # calls without a range spec go where they went
    assert len(tt._window_frame_args("g", "o", True, {"r": ("rolling_sum", "v", 1, 0)})) == 10


def test_c_abi_window_range_frames(ctx):
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_init(b"cpu") == 0
    assert lib.cylon_read_csv(os.path.join(DATA, "csv1_0.csv").encode(), b"RANGE_A") == 0
    whole = Table(context=ctx, _native=C.registry_get("RANGE_A")).to_arrow()
    k, v = whole.column_names[0], whole.column_names[1]
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    names = (ctypes.c_char_p * 4)(b"rn", None, b"top", b"roll")
    rc = lib.cylon_window_range_frames(b"RANGE_A", (i32 * 1)(0), 1, (i32 * 1)(1), (i32 * 1)(1), 1,
                                       (i32 * 4)(0, 15, 18, 10), (i32 * 4)(-1, 1, 1, 1), None,
                                       (i64 * 4)(0, 2, (1 << 63) - 1, 1), (i64 * 4)(0, 1, 0, 1), None, None, None,
                                       (i64 * 4)(1, 2, 1, 1), names, 4, 0, b"RANGE_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=ctx, _native=C.registry_get("RANGE_OUT")).to_arrow()
    f = {"rn": "row_number", "range_sum_" + v: ("range_sum", v, 2, 1, 2), "top": ("range_max", v, None, 0),
         "roll": ("rolling_sum", v, 1, 1)}
    assert_range(out, whole, k, v, True, f)
    if pa.types.is_floating(whole[v].type):  # float offsets beside the integer ones
        rc = lib.cylon_window_range_frames(b"RANGE_A", (i32 * 1)(0), 1, (i32 * 1)(1), None, 1, (i32 * 1)(15),
                                           (i32 * 1)(1), None, (i64 * 1)(0), (i64 * 1)((1 << 63) - 1), (f64 * 1)(0.5),
                                           (f64 * 1)(0.0), (i32 * 1)(1), None, None, 1, 0, b"RANGE_OUT")
        assert rc == 0, lib.cylon_last_error()
        out = Table(context=ctx, _native=C.registry_get("RANGE_OUT")).to_arrow()
        assert_range(out, whole, k, v, True, {None: ("range_sum", v, 0.5, None)})
    assert lib.cylon_window_range_frames(b"RANGE_A", None, 0, None, None, 0, (i32 * 1)(15), (i32 * 1)(1), None, None,
                                         None, None, None, None, None, None, 1, 0, b"RANGE_X") != 0
    assert b"exactly one order column" in lib.cylon_last_error()
    assert lib.cylon_window_range_frames(b"RANGE_A", None, 0, None, None, 0, (i32 * 1)(19), (i32 * 1)(1), None, None,
                                         None, None, None, None, None, None, 1, 0, b"RANGE_X") != 0
    assert b"window function" in lib.cylon_last_error()
    assert lib.cylon_window_frames(b"RANGE_A", None, 0, None, None, 0, (i32 * 1)(15), (i32 * 1)(1), None, None, None,
                                   None, None, 1, 0, b"RANGE_X") != 0  # the ROWS entry point still stops at 13
    for t in (b"RANGE_A", b"RANGE_OUT"):
        assert lib.cylon_remove_table(t) == 0


def _global():
    n = 1500
    rng = np.random.default_rng(13)
    return pa.table({"g": rng.integers(0, 40, n), "o": rng.integers(0, 200, n),
                     "v": pa.array(rng.integers(-9, 9, n).astype(np.float64), mask=rng.random(n) < 0.1),
                     "row": np.arange(n)})


DIST_FUNCS = dict(five("v", 3, 2, 2), rn="row_number", cs=("cumsum", "v"), tot=("range_sum", "v", None, None),
                  roll=("rolling_max", "v", 1, 1))


def _dist(ctx):
    """rank r holds rows r, r + W, ... of the global table"""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    g = _global()
    tt = Table(g.take(pa.array(np.arange(rank, g.num_rows, world))), ctx)
    return tt.distributed_window("g", "o", False, DIST_FUNCS).to_arrow()


def test_distributed_window_with_range_specs_two_ranks():
    res = run_distributed(_dist, 2)
    g = _global()
    on = [set(r["g"].to_pylist()) for r in res]  # every partition is on one rank
    assert on[0].isdisjoint(on[1]) and on[0] | on[1] == set(g["g"].to_pylist())
    # ties in `o` keep row order only inside a rank's input: the rank-free specs are compared
    f = {k: s for k, s in DIST_FUNCS.items() if k not in ("rn", "cs", "roll")}
    got = pa.concat_tables(res)
    keep = g.column_names + list(f)
    assert_range(got.select(keep), g, "g", "o", False, f, row_id="row")
