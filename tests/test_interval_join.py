"""Interval joins on the CPU twin (kernels/cpu_interval.cpp) behind ops/interval.cpp.  Every result --
C.interval_join_indices in the specified order, C.interval_join_counts and the table -- is compared with
an oracle that does not use the engine (interval_utils)."""
import ctypes
import os

import numpy as np
import pyarrow as pa
import pytest

import cylon_amd.ops as ops
from cylon_amd import CylonContext, CylonEnv, CylonError, DataFrame, Table
from cylon_amd._lib import C
from interval_utils import CLOSED, HOWS, assert_multiset, assert_table, check_interval, counts_of, expected
from dist_utils import run_distributed

DATA = os.path.join(os.path.dirname(__file__), "data", "input")
N = 400
INVALID = 4  # Code::Invalid
INF = float("inf")
NAN = float("nan")


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


def _pair(seed, nl=N, nr=N, groups=7, span=60):
    """unsorted, duplicate values on both sides and between them, groups 0 and 1 only left, the last two
    only right; about a tenth of the intervals have lower > upper"""
    rng = np.random.default_rng(seed)
    names = np.array(["k%d" % i for i in range(groups + 2)])
    lg, rg = rng.integers(0, groups, nl), rng.integers(2, groups + 2, nr)
    lo = rng.integers(0, span, nl)
    left = pa.table({"g": lg, "s": pa.array(names[lg % 3]), "lo": lo, "hi": lo + rng.integers(-1, 9, nl),
                     "a": np.arange(nl)})
    right = pa.table({"g": rg, "s": pa.array(names[rg % 3]), "t": rng.integers(0, span, nr),
                      "b": pa.array(rng.standard_normal(nr), mask=rng.random(nr) < 0.1),
                      "txt": pa.array(["r%d" % i for i in range(nr)])})
    return left, right


KW = dict(lower="lo", upper="hi", on="t")


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("closed", CLOSED)
def test_closed_how_and_groups(cpu, closed, how):
    left, right = _pair(1)
    for by in (None, "g", ["g", "s"]):
        exp = expected(left, right, by=by, closed=closed, how=how, **KW)
        c = check_interval(cpu, left, right, exp=exp, by=by, closed=closed, how=how, **KW)
        assert 0 < c["interval.matched"] <= c["interval.pairs"], c
        assert (c["interval.pairs"] > c["interval.matched"]) == (how == "left")
    assert 0 in counts_of(expected(left, right, by="g", closed=closed, **KW), N)  # groups 0 and 1 have no right rows


def test_closed_with_ties_on_both_bounds_and_between_the_sides(cpu):
    left = pa.table({"lo": [2, 2, 3, 5, 2], "hi": [4, 2, 2, 5, 9]})
    right = pa.table({"t": [4, 2, 3, 2, 4, 5, 1], "b": [0, 1, 2, 3, 4, 5, 6]})
    want = {
        "both": [(0, 1), (0, 3), (0, 2), (0, 0), (0, 4), (1, 1), (1, 3), (3, 5), (4, 1), (4, 3), (4, 2), (4, 0), (4, 4), (4, 5)],
        "left": [(0, 1), (0, 3), (0, 2), (4, 1), (4, 3), (4, 2), (4, 0), (4, 4), (4, 5)],
        "right": [(0, 2), (0, 0), (0, 4), (4, 2), (4, 0), (4, 4), (4, 5)],
        "neither": [(0, 2), (4, 2), (4, 0), (4, 4), (4, 5)],
    }
    for closed in CLOSED:
        assert expected(left, right, closed=closed, **KW) == want[closed]  # the oracle against a hand-made list
        check_interval(cpu, left, right, closed=closed, **KW)
        exp = expected(left, right, closed=closed, how="left", **KW)
        assert [p for p in exp if p[1] is not None] == want[closed]
        assert sorted({i for i, j in exp if j is None}) == sorted(set(range(5)) - {i for i, _ in want[closed]})
        check_interval(cpu, left, right, closed=closed, how="left", exp=exp, **KW)


def _values(rng, typ, n):
    if typ in ("float32", "float64"):
        return pa.array((rng.integers(-400, 400, n) / 8).astype(typ))
    if typ == "timestamp":
        return pa.array(rng.integers(10 ** 15, 10 ** 15 + 500, n), pa.timestamp("us"))
    if typ == "date32":
        return pa.array(rng.integers(19000, 19200, n).astype(np.int32), pa.date32())
    if typ == "duration":
        return pa.array(rng.integers(-250, 250, n), pa.duration("ms"))
    info = np.iinfo(typ)
    v = rng.integers(max(info.min, -100), min(info.max, 100), n).astype(typ)
    v[:4] = [info.min, info.max, info.max, info.min]
    return pa.array(v)


@pytest.mark.parametrize("typ", ["int8", "uint16", "int32", "uint64", "int64", "float32", "float64", "timestamp",
                                 "date32", "duration"])
def test_every_value_type(cpu, typ):
    rng = np.random.default_rng(len(typ) + ord(typ[0]))
    n = 200
    left = pa.table({"g": rng.integers(0, 3, n), "lo": _values(rng, typ, n), "hi": _values(rng, typ, n)})
    right = pa.table({"g": rng.integers(0, 3, n), "t": _values(rng, typ, n), "b": np.arange(n)})
    for closed in CLOSED:
        c = check_interval(cpu, left, right, by="g", closed=closed, **KW)
        assert c["interval.matched"] > 0, c
    check_interval(cpu, left, right, by="g", how="left", **KW)


@pytest.mark.parametrize("typ", ["int8", "uint64", "int64"])
def test_integer_extremes_are_ordinary_values(cpu, typ):
    info = np.iinfo(typ)
    t = getattr(pa, typ)()
    mid = (info.min + info.max) // 2
    left = pa.table({"lo": pa.array([info.min, info.min, mid, info.max, info.max], t),
                     "hi": pa.array([info.max, info.min, info.max, info.max, info.min], t)})
    right = pa.table({"t": pa.array([info.max, info.min, mid, info.min, info.max], t)})
    assert counts_of(expected(left, right, **KW), 5) == [5, 2, 3, 2, 0]
    assert counts_of(expected(left, right, closed="neither", **KW), 5) == [1, 0, 0, 0, 0]
    for closed in CLOSED:
        for how in HOWS:
            check_interval(cpu, left, right, closed=closed, how=how, **KW)


def test_infinities_and_signed_zero(cpu):
    left = pa.table({"lo": [-INF, 0.0, -0.0, -INF, INF, 1.0], "hi": [INF, INF, 0.0, -INF, INF, -INF]})
    right = pa.table({"t": [-0.0, INF, 0.0, -INF, 5.0, NAN, None], "b": np.arange(7)})
    # row 0 owns every usable right row, in `on` order then row order: -inf, -0.0, 0.0, 5.0, inf
    exp = expected(left, right, **KW)
    assert [j for i, j in exp if i == 0] == [3, 0, 2, 4, 1]
    assert [j for i, j in exp if i == 1] == [0, 2, 4, 1]  # +0.0 <= -0.0
    assert [j for i, j in exp if i == 2] == [0, 2] and [j for i, j in exp if i == 3] == [3]
    assert [j for i, j in exp if i == 4] == [1] and not [j for i, j in exp if i == 5]
    assert counts_of(expected(left, right, closed="neither", **KW), 6) == [3, 1, 0, 0, 0, 0]
    assert counts_of(expected(left, right, closed="left", **KW), 6) == [4, 3, 0, 0, 0, 0]
    for typ in (pa.float64(), pa.float32()):
        l = pa.table({"lo": left["lo"].cast(typ), "hi": left["hi"].cast(typ)})
        r = pa.table({"t": right["t"].cast(typ), "b": right["b"]})
        for closed in CLOSED:
            for how in HOWS:
                check_interval(cpu, l, r, closed=closed, how=how, **KW)


@pytest.mark.parametrize("typ", ["float32", "float64", "int32"])
def test_nulls_and_nan(cpu, typ):
    rng = np.random.default_rng(5)
    n = 300

    def val(width=0):
        v = ((rng.integers(-80, 80, n) + width) / 4).astype(typ)
        if typ != "int32":
            v[rng.random(n) < 0.1] = np.nan
        return pa.array(v, mask=rng.random(n) < 0.1)

    def key():
        k = rng.integers(0, 4, n).astype(np.float64)
        k[k == 3] = np.nan  # NaN keys match NaN keys
        return pa.array(k, mask=rng.random(n) < 0.15)  # null keys match null keys

    left = pa.table({"g": key(), "lo": val(), "hi": val(40), "a": np.arange(n)})
    right = pa.table({"g": key(), "t": val(), "b": pa.array(np.arange(n), mask=rng.random(n) < 0.2)})
    lg, ll, lh, rt = (c.to_pylist() for c in (left["g"], left["lo"], left["hi"], right["t"]))
    bad = lambda v: v is None or v != v
    for closed in CLOSED:
        for how in HOWS:
            exp = expected(left, right, by="g", closed=closed, how=how, **KW)
            assert any(j is not None and lg[i] is None for i, j in exp)  # null by = null by
            assert any(j is not None and lg[i] is not None and lg[i] != lg[i] for i, j in exp)
            assert all(j is None for i, j in exp if bad(ll[i]) or bad(lh[i]))  # SQL's unknown comparison
            assert all(not bad(rt[j]) for _, j in exp if j is not None)
            check_interval(cpu, left, right, by="g", closed=closed, how=how, exp=exp, **KW)
        check_interval(cpu, left, right, closed=closed, **KW)


def test_empty_inputs_and_prefixes(cpu):
    left, right = _pair(6, 50, 40)
    for l, r in ((left.slice(0, 0), right), (left, right.slice(0, 0)), (left.slice(0, 0), right.slice(0, 0))):
        for how in HOWS:
            c = check_interval(cpu, l, r, by=["g", "s"], how=how, **KW)
            assert "interval.sort" not in c, c
    got = Table(left, cpu).interval_join(Table(right.slice(0, 0), cpu), by="g", how="left", **KW).to_arrow()
    assert got.num_rows == 50 and all(got.column(c).null_count == 50 for c in range(5, 10))
    assert got.select(range(5)).equals(left)
    got = Table(left, cpu).interval_join(Table(right.slice(0, 0), cpu), by="g", **KW).to_arrow()
    assert got.num_rows == 0 and got.schema.types == left.schema.types + right.schema.types
    got = Table(left.slice(0, 0), cpu).interval_join(Table(right, cpu), by="g", how="left", **KW).to_arrow()
    assert got.num_rows == 0 and got.num_columns == 10
    kw = dict(lower="lo", upper=3, on=2, left_by=["g"], right_by=[0], left_prefix="l_", right_prefix="r_")
    got = Table(left, cpu).interval_join(Table(right, cpu), **kw).to_arrow()
    assert got.column_names == ["l_g", "l_s", "l_lo", "l_hi", "l_a", "r_g", "r_s", "r_t", "r_b", "r_txt"]
    assert_table(got, left, right, expected(left, right, **kw), **kw)
    check_interval(cpu, left, right, how="left", **kw)


def test_counts_alone(cpu):
    left, right = _pair(9, 300, 500)
    tl, tr = Table(left, cpu), Table(right, cpu)
    for closed in CLOSED:
        want = counts_of(expected(left, right, by="g", closed=closed, **KW), 300)
        assert tl.interval_join_counts(tr, by="g", closed=closed, **KW).tolist() == want
    assert tl.interval_join_counts(Table(right.slice(0, 0), cpu), **KW).tolist() == [0] * 300
    assert Table(left.slice(0, 0), cpu).interval_join_counts(tr, **KW).numel() == 0


def test_errors(cpu):
    left, right = _pair(7, 20, 20)
    tl, tr = Table(left, cpu), Table(right, cpu)

    def invalid(fn):
        with pytest.raises((ValueError, CylonError)) as e:
            fn()
        if isinstance(e.value, CylonError):
            assert e.value.args[1] == INVALID, e.value.args

    bad = {"bool": pa.array([True] * 20), "half": pa.array(np.zeros(20, np.float16)), "str": left["s"],
           "dec": pa.array([1] * 20, pa.decimal128(10, 2)), "list": pa.array([[1]] * 20, pa.list_(pa.int64()))}
    for name, col in bad.items():
        l = Table(pa.table({"lo": col, "hi": col, "t": col}), cpu)
        invalid(lambda: l.interval_join(l, **KW))
    f = Table(pa.table({"t": np.arange(20.0), "g": right["g"], "s": right["s"]}), cpu)
    invalid(lambda: tl.interval_join(f, **KW))                                   # int64 bounds against a float64 `on`
    m = Table(pa.table({"lo": np.arange(20), "hi": np.arange(20.0)}), cpu)
    invalid(lambda: m.interval_join(tr, **KW))                                   # `lower` and `upper` differ
    invalid(lambda: tl.interval_join(tr, left_by="g", right_by="s", **KW))       # `by` types differ
    invalid(lambda: tl.interval_join(tr, left_by=["g", "s"], right_by=["g"], **KW))
    invalid(lambda: C.interval_join(tl.native, tr.native, 2, 3, 2, [0, 1], [0]))
    invalid(lambda: tl.interval_join(tr, closed="open", **KW))
    invalid(lambda: tl.interval_join(tr, closed=4, **KW))
    invalid(lambda: tl.interval_join(tr, how="outer", **KW))
    invalid(lambda: tl.interval_join(tr, how=2, **KW))
    invalid(lambda: C.interval_join(tl.native, tr.native, 2, 3, 2, [], [], -1))
    invalid(lambda: C.interval_join(tl.native, tr.native, 2, 3, 2, [], [], 0, -1))
    invalid(lambda: tl.interval_join(tr, lower=5, upper=3, on=2))
    invalid(lambda: tl.interval_join(tr, lower=2, upper=-1, on=2))
    invalid(lambda: tl.interval_join(tr, lower=2, upper=3, on=9))
    invalid(lambda: tl.interval_join(tr, left_by=[9], right_by=[0], **KW))
    invalid(lambda: tl.interval_join(tr, left_by=[0], right_by=[5], **KW))
    invalid(lambda: tl.interval_join(tr, lower=None, upper="hi", on="t"))
    invalid(lambda: C.interval_join_indices(tl.native, tr.native, 9, 3, 2, [], []))
    invalid(lambda: C.interval_join_counts(tl.native, tr.native, 2, 3, 2, [], [], 7))
    with pytest.raises(ValueError):
        tl.interval_join(tr, closed="open", **KW)
    with pytest.raises(ValueError):
        tl.interval_join(tr, how="outer", **KW)
    with pytest.raises(KeyError):
        tl.interval_join(tr, lower="missing", upper="hi", on="t")
    with pytest.raises(KeyError):
        tl.interval_join(tr, lower="lo", upper="hi", on="missing")
    with pytest.raises(KeyError):
        tl.interval_join(tr, by="missing", **KW)
    # more than kMaxFusedCols - 1 = 15 `by` columns
    wide_l = Table(pa.table({"lo": [1], "hi": [2], **{"k%d" % i: [0] for i in range(16)}}), cpu)
    wide_r = Table(pa.table({"t": [1], **{"k%d" % i: [0] for i in range(16)}}), cpu)
    by = ["k%d" % i for i in range(16)]
    invalid(lambda: wide_l.interval_join(wide_r, by=by, **KW))
    assert wide_l.interval_join(wide_r, by=by[:15], **KW).to_arrow().num_rows == 1


def test_table_ops_and_frame_surfaces(cpu):
    left, right = _pair(8, 200, 200)
    kw = dict(by="g", closed="left", how="left", left_prefix="x_", right_prefix="y_", **KW)
    tl, tr = Table(left, cpu), Table(right, cpu)
    want = tl.interval_join(tr, **kw).to_arrow()
    assert_table(want, left, right, expected(left, right, **kw), **kw)
    okw = {k: v for k, v in kw.items() if k not in KW}
    assert ops.interval_join(tl, tr, "lo", "hi", "t", **okw).to_arrow().equals(want)
    assert ops.distributed_interval_join(tl, tr, "lo", "hi", "t", **okw).to_arrow().equals(want)  # world 1
    nb = dict(kw, by=None)
    assert tl.distributed_interval_join(tr, **nb).to_arrow().equals(tl.interval_join(tr, **nb).to_arrow())  # no key needed
    fkw = dict(by="g", closed="left", how="left", suffixes=("x_", "y_"), **KW)
    assert DataFrame(left).merge_interval(DataFrame(right), **fkw).to_arrow().equals(want)
    env = CylonEnv(distributed=False, device="cpu")
    assert DataFrame(left).merge_interval(DataFrame(right), env=env, **fkw).to_arrow().equals(want)
    got = DataFrame(left).merge_interval(DataFrame(right), "lo", "hi", "t", left_by="g", right_by="g").to_arrow()
    assert_table(got, left, right, expected(left, right, by="g", **KW), left_prefix="_x", right_prefix="_y")


def test_c_abi_interval_join(ctx):
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_init(b"cpu") == 0
    left, right = _pair(10, 120, 90)
    C.registry_put("IV_A", Table(left, ctx).native)
    C.registry_put("IV_B", Table(right, ctx).native)
    i32 = ctypes.c_int32
    rc = lib.cylon_interval_join(b"IV_A", b"IV_B", 2, 3, 2, None, None, 0, 3, 1, b"l_", b"r_", b"IV_OUT", 0)
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=ctx, _native=C.registry_get("IV_OUT")).to_arrow()
    kw = dict(closed="neither", how="left", left_prefix="l_", right_prefix="r_", **KW)
    assert_table(out, left, right, expected(left, right, **kw), **kw)
    # a `by` column, distributed at world 1
    rc = lib.cylon_interval_join(b"IV_A", b"IV_B", 2, 3, 2, (i32 * 1)(0), (i32 * 1)(0), 1, 0, 0, None, None, b"IV_OUT", 1)
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=ctx, _native=C.registry_get("IV_OUT")).to_arrow()
    assert_table(out, left, right, expected(left, right, by="g", **KW))
    rc = lib.cylon_interval_join(b"IV_missing", b"IV_B", 2, 3, 2, None, None, 0, 0, 0, None, None, b"IV_X", 0)
    assert rc != 0 and b"IV_missing" in lib.cylon_last_error()
    assert lib.cylon_interval_join(b"IV_A", b"IV_B", 2, 3, 2, None, None, 0, 7, 0, None, None, b"IV_X", 0) != 0
    assert b"closed" in lib.cylon_last_error()
    assert lib.cylon_interval_join(b"IV_A", b"IV_B", 2, 3, 2, None, None, 0, 0, 5, None, None, b"IV_X", 0) != 0
    assert b"how" in lib.cylon_last_error()
    for t in (b"IV_A", b"IV_B", b"IV_OUT"):
        assert lib.cylon_remove_table(t) == 0


def _global():
    rng = np.random.default_rng(12)
    nl, nr = 900, 1100
    lo = rng.integers(0, 200, nl)
    left = pa.table({"g": rng.integers(0, 40, nl), "lo": lo, "hi": lo + rng.integers(-2, 30, nl), "lrow": np.arange(nl)})
    right = pa.table({"g": rng.integers(5, 45, nr), "t": rng.integers(0, 200, nr), "rrow": np.arange(nr),
                      "b": pa.array(rng.standard_normal(nr), mask=rng.random(nr) < 0.1),
                      "txt": pa.array(["s%d" % i for i in range(nr)])})
    return left, right


DIST_KW = dict(by="g", closed="right", how="left", **KW)


def _dist(ctx, case):
    """rank r holds rows r, r + W, ... of both global tables"""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    left, right = _global()
    tl = Table(left.take(pa.array(np.arange(rank, left.num_rows, world))), ctx)
    tr = Table(right.take(pa.array(np.arange(rank, right.num_rows, world))), ctx)
    if case == "no_key":
        try:
            tl.distributed_interval_join(tr, **KW)
        except Exception as e:  # the same error on every rank, before any exchange
            return str(e)
        return "no error"
    return tl.distributed_interval_join(tr, **DIST_KW).to_arrow()


def test_distributed_interval_join_two_ranks():
    res = run_distributed(_dist, 2, "keyed")
    left, right = _global()
    on = [set(r.column(0).to_pylist()) for r in res]  # every group is on one rank
    assert on[0].isdisjoint(on[1]) and on[0] | on[1] == set(left["g"].to_pylist())
    exp = expected(left, right, **DIST_KW)
    assert any(j is None for _, j in exp) and sum(j is not None for _, j in exp) > 1000
    assert_multiset(pa.concat_tables(res), left, right, exp, "lrow", "rrow", **DIST_KW)


def test_distributed_interval_join_needs_a_by_column():
    res = run_distributed(_dist, 2, "no_key")
    assert all("`by` column" in r for r in res), res
