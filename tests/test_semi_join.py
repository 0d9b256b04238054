"""Left semi / anti joins on CPU contexts (ops/join_semi.cpp semi_join_local; kernels/cpu_semi.cpp is the
twin of kernels/semi_join.hip): every key kind, payload kind, degenerate input and public surface,
against a Python-set oracle that does not use the engine (semi_join_utils).  Local results are
compared WITHOUT sorting: they keep the left table's row order (docs/semantics.md)."""
import ctypes
import os

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import DataFrame, JoinConfig, Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from semi_join_utils import assert_same_rows, canon, expected, semi_mask

DATA = os.path.join(os.path.dirname(__file__), "data", "input")
N = 3000


def _payload(rng, n):
    return {"f": rng.random(n),
            "ni": pa.array(rng.integers(-9, 9, n), mask=rng.random(n) < 0.2),
            "s": pa.array([f"row{i}" if i % 7 else None for i in range(n)]),
            "l": pa.array([[int(i), int(i) + 1][: i % 3] for i in range(n)], pa.list_(pa.int64()))}


def _int_tables(dtype, lo, hi, seed=0, nl=N, nr=N - 500):
    rng = np.random.default_rng(seed)
    a = pa.table({"k": rng.integers(lo, hi, nl).astype(dtype), **_payload(rng, nl)})
    b = pa.table({"k": rng.integers(lo, 2 * hi - lo, nr).astype(dtype), "w": rng.random(nr)})
    return a, b


def _check(ctx, a, b, on, algorithm="hash", c=None):
    res = {}
    for how in ("semi", "anti"):
        C.trace_enable(True)
        C.trace_reset()
        got = Table(a, ctx).join(Table(b, ctx), how, algorithm, on=on, left_prefix="l_", right_prefix="r_")
        if c is not None:
            c[how] = dict(C.trace_counters())
        C.trace_enable(False)
        assert_same_rows(got.to_arrow(), expected(a, b, how, on, prefix="l_"))
        res[how] = got
    # the two outputs partition left
    assert res["semi"].row_count + res["anti"].row_count == a.num_rows
    return res


@pytest.mark.parametrize("dtype,lo,hi", [(np.int64, -(1 << 40), (1 << 40) + 1500), (np.int64, 0, 1500),
                                         (np.int32, -700, 800), (np.uint16, 0, 1500)])
@pytest.mark.parametrize("algorithm", ["hash", "sort"])
def test_int_keys_all_payload_kinds(ctx, dtype, lo, hi, algorithm):
    a, b = _int_tables(dtype, lo, hi)
    if hi - lo < 1 << 20:
        assert 0 < semi_mask(a, b, ["k"]).sum() < a.num_rows
    c = {}
    _check(ctx, a, b, ["k"], algorithm, c)
    assert "join.semi.general" not in c["semi"], c  # the CPU twin of the mark kernel ran
    assert c["semi"]["join.semi.matched"] == semi_mask(a, b, ["k"]).sum()
    # one non-null integer key: the set oracle agrees with numpy's
    assert np.array_equal(semi_mask(a, b, ["k"]), np.isin(a["k"].to_numpy(), b["k"].to_numpy()))


def test_nullable_int_key_null_matches_null(ctx):
    rng = np.random.default_rng(1)
    a, b = _int_tables(np.int64, 0, 1500, seed=1)
    a = a.set_column(0, "k", pa.array(a["k"].to_numpy(), mask=rng.random(a.num_rows) < 0.05))
    both = _check(ctx, a, b, ["k"])  # no null on the right: null keys are anti rows
    assert both["anti"].to_arrow()["l_k"].null_count == a["k"].null_count
    b = b.set_column(0, "k", pa.array(b["k"].to_numpy(), mask=np.arange(b.num_rows) == 17))
    both = _check(ctx, a, b, ["k"])  # one null on the right: every null key is a semi row
    assert both["semi"].to_arrow()["l_k"].null_count == a["k"].null_count > 0


def test_two_key_columns_with_nulls(ctx):
    rng = np.random.default_rng(2)

    def side(n, extra):
        return pa.table({"k": pa.array(rng.integers(0, 60, n), mask=rng.random(n) < 0.1),
                         "g": pa.array(rng.integers(0, 40, n).astype(np.int16), mask=rng.random(n) < 0.1), **extra})

    a, b = side(N, _payload(rng, N)), side(N // 2, {"w": rng.random(N // 2)})
    m = semi_mask(a, b, ["k", "g"])
    assert 0 < m.sum() < N
    nulls = np.array([x is None or y is None for x, y in zip(a["k"].to_pylist(), a["g"].to_pylist())])
    assert (m & nulls).any() and (~m & nulls).any()  # null-holding keys on both sides of the split
    _check(ctx, a, b, ["k", "g"])


def test_float64_key_inner_identity(ctx):
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.integers(0, 500, 50).astype(np.float64) / 4, [0.0, -0.0, np.nan, np.inf]])
    a = pa.table({"k": rng.choice(vals, N), "f": rng.random(N)})
    b = pa.table({"k": rng.choice(vals[::2], N // 2)})
    ta, tb = Table(a, ctx), Table(b, ctx)
    li, _ = C.join_indices(ta.native, tb.native, "inner", "hash", [0], [0])
    inner = np.zeros(N, bool)
    inner[li.numpy()] = True
    for how, m in (("semi", inner), ("anti", ~inner)):
        got = ta.join(tb, how, "hash", on=["k"]).to_arrow()
        assert got["f"].to_pylist() == a.filter(pa.array(m))["f"].to_pylist()


@pytest.mark.parametrize("kind", ["string", "fixed_binary"])
def test_var_and_fixed_bytes_keys(ctx, kind):
    rng = np.random.default_rng(4)

    def keys(n, hi):
        v = rng.integers(0, hi, n)
        if kind == "string":
            return pa.array([f"key-{x}" * (1 + x % 3) for x in v])
        return pa.array([int(x).to_bytes(6, "little") for x in v], pa.binary(6))

    a = pa.table({"k": keys(N, 900), **_payload(rng, N)})
    b = pa.table({"k": keys(N // 2, 1800)})
    assert 0 < semi_mask(a, b, ["k"]).sum() < N
    c = {}
    _check(ctx, a, b, ["k"], c=c)
    assert c["semi"].get("join.semi.general") == 1, c


def test_degenerate_inputs(ctx):
    a, b = _int_tables(np.int64, 0, 1500, seed=5)
    empty_a, empty_b = a.slice(0, 0), b.slice(0, 0)
    for x, y in ((empty_a, b), (a, empty_b), (empty_a, empty_b)):
        both = _check(ctx, x, y, ["k"])
        assert both["semi"].row_count == 0 and both["anti"].row_count == x.num_rows
    every = pa.table({"k": np.arange(0, 1500)})  # every left row matches
    assert _check(ctx, a, every, ["k"])["anti"].row_count == 0
    none = pa.table({"k": np.arange(5000, 5100)})  # no left row matches
    assert _check(ctx, a, none, ["k"])["semi"].row_count == 0


def test_identity_with_inner_join_indices(ctx):
    a, b = _int_tables(np.int32, -700, 800, seed=6)
    ta, tb = Table(a, ctx), Table(b, ctx)
    li, _ = C.join_indices(ta.native, tb.native, "inner", "hash", [0], [0])
    in_inner = np.unique(li.numpy())
    rows, partner = C.join_indices(ta.native, tb.native, "semi", "hash", [0], [0])
    assert np.array_equal(rows.numpy(), in_inner)  # ascending, each left row once
    assert partner.numpy().tolist() == [-1] * len(in_inner)
    rows, partner = C.join_indices(ta.native, tb.native, "anti", "sort", [0], [0])
    assert np.array_equal(rows.numpy(), np.setdiff1d(np.arange(a.num_rows), in_inner))
    assert (partner.numpy() == -1).all()


def test_every_surface(ctx, tmp_path):
    a, b = _int_tables(np.int64, 0, 1500, seed=7)
    ta, tb = Table(a, ctx), Table(b, ctx)
    exp = {how: expected(a, b, how, ["k"]) for how in ("semi", "anti")}
    for how, spellings in (("semi", ["semi", "left_semi", "leftsemi", "SEMI"]),
                           ("anti", ["anti", "left_anti", "leftanti", "Anti"])):
        for s in spellings:
            assert_same_rows(ta.join(tb, s, "hash", on=["k"]).to_arrow(), exp[how])
            assert_same_rows(ta.distributed_join(tb, s, "sort", on=["k"]).to_arrow(), exp[how])
        assert_same_rows(JoinConfig(how, "hash", 0, 0).apply(ta, tb).to_arrow(), exp[how])
    # differently named key columns, prefixes: left's columns only, the right prefix is ignored
    b2 = b.rename_columns(["rk", "w"])
    got = ta.join(Table(b2, ctx), "semi", "hash", left_on=["k"], right_on=["rk"], left_prefix="L.", right_prefix="R.")
    assert_same_rows(got.to_arrow(), expected(a, b2, "semi", ["k"], ["rk"], prefix="L."))
    assert got.to_arrow().schema.types == a.schema.types
    # DataFrame.merge
    da, db = DataFrame(a), DataFrame(b)
    m = da.merge(db, how="anti", on="k", suffixes=("", "_r"))
    assert_same_rows(m.to_arrow(), exp["anti"])
    m = da.merge(db, how="semi", algorithm="hash", on=["k"], suffixes=("x_", "y_"), sort=True)
    assert sorted(m.to_arrow()["x_f"].to_pylist()) == sorted(exp["semi"]["f"].to_pylist())
    assert m.to_arrow()["x_k"].to_pylist() == sorted(exp["semi"]["k"].to_pylist())
    # the string-id registry
    C.registry_put("semi_L", ta.native)
    C.registry_put("semi_R", tb.native)
    for how in ("semi", "left_anti"):
        code, msg = C.registry_join("semi_L", "semi_R", how, "hash", [0], [0], "semi_out", False)
        assert code == 0, msg
        out = Table(context=ctx, _native=C.registry_get("semi_out"))
        assert_same_rows(out.to_arrow(), exp["semi" if how == "semi" else "anti"])
    for t in ("semi_L", "semi_R", "semi_out"):
        C.registry_remove(t)
    # unknown types still raise
    with pytest.raises(KeyError):
        ta.join(tb, "semi_anti", "hash", on=["k"])
    with pytest.raises(Exception, match="unsupported join type"):
        C.join(ta.native, tb.native, "right_semi", "hash", [0], [0], "", "")
    with pytest.raises(KeyError):
        JoinConfig("right_anti")


def test_c_abi_join_types_4_and_5(ctx):
    import pandas as pd
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_init(b"cpu") == 0
    a_csv, b_csv = os.path.join(DATA, "csv1_0.csv"), os.path.join(DATA, "csv2_0.csv")
    assert lib.cylon_read_csv(a_csv.encode(), b"SA") == 0 and lib.cylon_read_csv(b_csv.encode(), b"SB") == 0
    pa_, pb = pd.read_csv(a_csv), pd.read_csv(b_csv)
    m = np.isin(pa_.iloc[:, 0].to_numpy(), pb.iloc[:, 0].to_numpy())
    assert 0 < m.sum() < len(m)
    for jt, want in ((4, int(m.sum())), (5, int((~m).sum()))):
        for alg in (0, 1):
            assert lib.cylon_join(b"SA", b"SB", jt, alg, 0, 0, b"SJ") == 0
            assert lib.cylon_row_count(b"SJ") == want
            assert lib.cylon_column_count(b"SJ") == pa_.shape[1]
        assert lib.cylon_distributed_join(b"SA", b"SB", jt, 1, 0, 0, b"SJ") == 0
        assert lib.cylon_row_count(b"SJ") == want
    for t in (b"SA", b"SB", b"SJ"):
        assert lib.cylon_remove_table(t) == 0


def _dist(ctx, how, n):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    rng = np.random.default_rng(100 + rank)
    a = pa.table({"k": rng.integers(0, 400, n), "g": pa.array(rng.integers(0, 3, n), mask=rng.random(n) < 0.1),
                  "s": pa.array([f"r{rank}-{i}" for i in range(n)]), "f": rng.random(n)})
    m = n // 2 + 10 * rank
    b = pa.table({"x": rng.random(m), "g": pa.array(rng.integers(0, 3, m), mask=rng.random(m) < 0.1),
                  "k": rng.integers(0, 800, m)})
    got = Table(a, ctx).distributed_join(Table(b, ctx), how, "hash", left_on=["k", "g"], right_on=["k", "g"],
                                         left_prefix="l_")
    assert world > 1
    return a, b, got.to_arrow()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("how", ["semi", "anti"])
def test_distributed_union_of_ranks_equals_oracle(world, how):
    res = run_distributed(_dist, world, how, 1500)
    a = pa.concat_tables([r[0] for r in res])
    b = pa.concat_tables([r[1] for r in res])
    got = pa.concat_tables([r[2] for r in res])
    exp = expected(a, b, how, ["k", "g"], prefix="l_")
    assert 0 < exp.num_rows < a.num_rows
    assert got.column_names == exp.column_names
    assert canon(got) == canon(exp)
