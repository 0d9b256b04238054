"""GPU tests for group-by, set operations, unique, aggregates and the RCCL
communicator (world size 1 on the single-GPU box; the 8-GPU path is exercised
by the driver's scaling bench)."""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

from cylon_amd import C, Table

pytestmark = pytest.mark.gpu


def _frame(n=200_000, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=n)
    v[rng.random(n) < 0.05] = np.nan
    return pd.DataFrame({"k": rng.integers(0, 5000, n), "s": [f"g{x}" for x in rng.integers(0, 40, n)], "v": v,
                         "i": rng.integers(-10**6, 10**6, n)})


def _sorted(df, keys):
    return df.sort_values(keys).reset_index(drop=True)


@pytest.mark.parametrize("keys", [["k"], ["s"], ["k", "s"]])
def test_groupby_gpu_vs_cpu(gpu_ctx, ctx, keys):
    df = _frame()
    ops = ["sum", "count", "min", "max", "mean", "var", "std", "nunique", "median"]
    g = Table.from_pandas(gpu_ctx, df).local_groupby(keys, {"v": ops, "i": ["sum", "min", "max"]}).to_pandas()
    c = Table.from_pandas(ctx, df).local_groupby(keys, {"v": ops, "i": ["sum", "min", "max"]}).to_pandas()
    g, c = _sorted(g, keys), _sorted(c, keys)
    assert list(g.columns) == list(c.columns)
    for col in g.columns:
        if g[col].dtype.kind == "f":
            np.testing.assert_allclose(g[col].to_numpy(), c[col].to_numpy(), rtol=1e-9, atol=1e-9, equal_nan=True)
        else:
            assert g[col].tolist() == c[col].tolist()


def test_groupby_small_group_count_lds_path(gpu_ctx):
    n = 1_000_000
    k = torch.randint(0, 7, (n,), device="cuda")
    v = torch.rand(n, device="cuda", dtype=torch.float64)
    t = Table.from_torch(gpu_ctx, {"k": k, "v": v})
    out = t.local_groupby("k", {"v": ["sum", "count", "min", "max"]}).sort("k").to_pandas()
    df = pd.DataFrame({"k": k.cpu().numpy(), "v": v.cpu().numpy()})
    exp = df.groupby("k")["v"].agg(["sum", "count", "min", "max"]).reset_index()
    np.testing.assert_allclose(out["sum_v"], exp["sum"], rtol=1e-9)
    assert out["count_v"].tolist() == exp["count"].tolist()
    assert np.array_equal(out["min_v"], exp["min"]) and np.array_equal(out["max_v"], exp["max"])


def test_set_ops_and_unique_gpu_vs_cpu(gpu_ctx, ctx):
    rng = np.random.default_rng(3)
    a = pa.table({"x": rng.integers(0, 300, 50_000), "s": [f"v{v}" for v in rng.integers(0, 9, 50_000)]})
    b = pa.table({"x": rng.integers(200, 500, 30_000), "s": [f"v{v}" for v in rng.integers(0, 9, 30_000)]})
    for op in ("union", "subtract", "intersect"):
        g = getattr(Table(a, gpu_ctx), op)(Table(b, gpu_ctx)).to_arrow()
        c = getattr(Table(a, ctx), op)(Table(b, ctx)).to_arrow()
        assert g.equals(c), op
    for keep in ("first", "last"):
        g = Table(a, gpu_ctx).unique(["x"], keep=keep).to_arrow()
        c = Table(a, ctx).unique(["x"], keep=keep).to_arrow()
        assert g.equals(c)


def test_scalar_aggregates_gpu(gpu_ctx):
    df = _frame(100_000, 9)
    t = Table.from_pandas(gpu_ctx, df)
    assert t.sum("i").to_pydict()["i"][0] == df["i"].sum()
    assert t.count("v").to_pydict()["v"][0] == df["v"].count()
    assert t.min("v").to_pydict()["v"][0] == df["v"].min()
    assert t.max("i").to_pydict()["i"][0] == df["i"].max()
    assert t.mean("v").to_pydict()["v"][0] == pytest.approx(df["v"].mean())
    assert t.std("v").to_pydict()["v"][0] == pytest.approx(df["v"].std())
    assert t.quantile("v", 0.5).to_pydict()["v"][0] == pytest.approx(df["v"].median())


def test_rccl_communicator_world1():
    """Exercises the ProcessGroup communicator on RCCL (backend nccl) on one GPU."""
    import torch.distributed as dist
    from cylon_amd import CylonContext, RCCLConfig
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    os.environ["RANK"] = "0"
    os.environ["WORLD_SIZE"] = "1"
    os.environ["LOCAL_RANK"] = "0"
    ctx = CylonContext(config=RCCLConfig(), distributed=True)
    try:
        assert ctx.get_world_size() == 1 and ctx.on_gpu
        x = torch.arange(10, device="cuda", dtype=torch.int64)
        assert torch.equal(ctx._ctx.alltoallv(x, [10]), x)
        y = torch.ones(4, device="cuda")
        assert torch.equal(ctx.allreduce(y.clone(), "sum"), y)
        assert torch.equal(ctx.allgather(x), x)
        ctx.barrier()
        t = Table(pa.table({"k": [1, 2, 3], "v": [1.0, 2.0, 3.0]}), ctx)
        j = t.distributed_join(t, "inner", "hash", on=[0], left_prefix="l_", right_prefix="r_")
        assert j.row_count == 3
        g = t.groupby("k", {"v": "sum"})
        assert g.row_count == 3
    finally:
        ctx.finalize()
        if dist.is_initialized():
            dist.destroy_process_group()


def test_device_memory_pool(gpu_ctx):
    pool = gpu_ctx.memory_pool()
    assert pool.backend_name() == "hip_caching_allocator" and pool.device().startswith("cuda")
    before = pool.bytes_allocated()
    x = pool.empty([1 << 20], "int64")
    assert x.is_cuda and pool.bytes_allocated() == before + 8 * (1 << 20)
    x.fill_(3)
    assert int(x.sum()) == 3 * (1 << 20)
    del x
    assert pool.bytes_allocated() == before


def test_native_index_lookup_on_gpu(gpu_ctx, ctx):
    import numpy as np
    from cylon_amd.indexing.index import IndexingSchema
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 500, 20000)
    res = []
    for cx in (gpu_ctx, ctx):
        t = Table(pa.table({"k": keys, "v": np.arange(20000)}), cx)
        t.set_index("k", IndexingSchema.HASH, drop=True)
        res.append(t.loc[[7, 3, 499, 1000], "v"].to_pandas()["v"].tolist())
    assert res[0] == res[1] and len(res[0]) == int(np.isin(keys, [7, 3, 499]).sum())


def _setop_frames(n1, n2, seed):
    rng = np.random.default_rng(seed)

    def mk(n, lo, hi):
        f = rng.choice(np.array([0.5, -0.0, 0.0, np.nan, 1.25]), n)
        valid = rng.random(n) > 0.1
        return pa.table({"x": rng.integers(lo, hi, n),
                         "f": pa.array(f, mask=~valid),
                         "s": [f"v{v}" for v in rng.integers(0, 4, n)],
                         "i": pa.array(rng.integers(0, 3, n).astype(np.int32))})
    return mk(n1, 0, 3000), mk(n2, 2000, 5000)


def _same_rows_in_order(g, c):
    """Tables equal row by row (NaN == NaN, bitwise -0.0 vs 0.0 distinguished)."""
    if g.schema != c.schema or g.num_rows != c.num_rows:
        return False
    for name in g.column_names:
        x, y = g.column(name).combine_chunks(), c.column(name).combine_chunks()
        if not x.is_null().equals(y.is_null()):
            return False
        xv, yv = x.fill_null(0) if x.null_count else x, y.fill_null(0) if y.null_count else y
        if pa.types.is_floating(x.type):
            a, b = np.asarray(xv), np.asarray(yv)
            if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                nan = np.isnan(a) & np.isnan(b)
                if not np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]):
                    return False
        elif not xv.equals(yv):
            return False
    return True


@pytest.mark.parametrize("strings", [False, True])
def test_radix_set_ops_match_cpu_exactly(gpu_ctx, ctx, monkeypatch, strings):
    """LDS radix distinct path (forced on small inputs): same rows in the same order as the CPU twin, with
    duplicates, nulls, NaN (== NaN), -0.0 (== 0.0), strings."""
    from cylon_amd._lib import C
    monkeypatch.setenv("CYLON_RADIX_SETOP_MIN_ROWS", "1")
    a, b = _setop_frames(60_000, 40_000, 5)
    if not strings:
        a, b = a.drop(["s"]), b.drop(["s"])
    C.trace_enable(True)
    C.trace_reset()
    for op in ("union", "subtract", "intersect"):
        g = getattr(Table(a, gpu_ctx), op)(Table(b, gpu_ctx)).to_arrow()
        c = getattr(Table(a, ctx), op)(Table(b, ctx)).to_arrow()
        assert g.num_rows == c.num_rows > 0, op
        assert _same_rows_in_order(g, c), op
    for keep in ("first", "last"):
        for cols in (["x"], ["f", "i"]):
            g = Table(a, gpu_ctx).unique(cols, keep=keep).to_arrow()
            c = Table(a, ctx).unique(cols, keep=keep).to_arrow()
            assert _same_rows_in_order(g, c), (keep, cols)
    counters = dict(C.trace_counters())
    C.trace_enable(False)
    assert counters.get("setop.radix.exceptions", 0) > 0 and "setop.radix.fallback" not in counters, counters


def test_radix_union_all_distinct_fast_path(gpu_ctx, monkeypatch):
    monkeypatch.setenv("CYLON_RADIX_SETOP_MIN_ROWS", "1")
    g = torch.Generator(device="cuda").manual_seed(1)
    n = 2_000_000
    L = Table.from_torch(gpu_ctx, {"k": torch.randint(0, 1 << 40, (n,), generator=g, device="cuda"),
                                   "v": torch.rand(n, generator=g, device="cuda", dtype=torch.float64)})
    R = Table.from_torch(gpu_ctx, {"k": torch.randint(0, 1 << 40, (n,), generator=g, device="cuda"),
                                   "v": torch.rand(n, generator=g, device="cuda", dtype=torch.float64)})
    u = L.union(R)
    assert u.row_count == 2 * n
    both = L.union(L)
    assert both.row_count == n
    assert torch.equal(both.to_torch()["k"], L.to_torch()["k"])
    assert L.intersect(L).row_count == n and L.subtract(L).row_count == 0


def test_native_parquet_to_and_from_hbm(gpu_ctx, tmp_path):
    import pyarrow.parquet as pq
    from cylon_amd.io import read_parquet, write_parquet
    at = pa.table({"k": [3, None, 1], "s": ["x", "yy", None], "f": [0.5, None, 2.0]})
    p = str(tmp_path / "g.parquet")
    pq.write_table(at, p)
    t = read_parquet(gpu_ctx, p)
    assert t.device.startswith("cuda") and t.to_arrow().equals(at)
    write_parquet(t.sort("k"), str(tmp_path / "o.parquet"))
    assert pq.read_table(str(tmp_path / "o.parquet")).column("k").to_pylist() == [1, 3, None]


def test_sorted_merge_join_matches_cpu(gpu_ctx, ctx, monkeypatch):
    """algorithm="sort" on the device: row-sorted tables + monotone merge (forced on small inputs);
    same rows as the CPU twin, output ordered by key."""
    from cylon_amd._lib import C
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1")
    monkeypatch.setenv("CYLON_RADIX_SORT_MIN_ROWS", "1")
    monkeypatch.setenv("CYLON_RANGE_JOIN", "0")
    rng = np.random.default_rng(12)
    a = pa.table({"k": rng.integers(-3000, 3000, 40_000), "x": rng.random(40_000),
                  "i": pa.array(rng.integers(0, 9, 40_000).astype(np.int32))})
    b = pa.table({"k": rng.integers(-3000, 3000, 25_000), "y": rng.random(25_000)})
    C.trace_enable(True)
    C.trace_reset()
    g = Table(a, gpu_ctx).join(Table(b, gpu_ctx), "inner", "sort", on=["k"], left_prefix="l_",
                               right_prefix="r_").to_pandas()
    assert C.trace_counters().get("join.sortmerge.rows_out", 0) == len(g)
    C.trace_enable(False)
    c = Table(a, ctx).join(Table(b, ctx), "inner", "sort", on=["k"], left_prefix="l_", right_prefix="r_").to_pandas()
    assert len(g) == len(c) > 0
    assert np.all(np.diff(g["l_k"].to_numpy()) >= 0)
    key = lambda df: sorted(map(tuple, df[sorted(df.columns)].to_numpy().tolist()))
    assert key(g) == key(c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["hot_key", "sparse_left", "dense_left", "disjoint"])
def test_sorted_merge_join_window_shapes(gpu_ctx, ctx, monkeypatch, shape):
    """The tiled merge count stages a right-key window per 2048-row left tile in LDS; windows larger than
    LDS (a hot key, a sparse left side over a dense right side) take the global-memory walk with galloping."""
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1")
    monkeypatch.setenv("CYLON_RADIX_SORT_MIN_ROWS", "1")
    rng = np.random.default_rng(5)
    if shape == "hot_key":
        lk = np.concatenate([rng.integers(0, 50_000, 30_000), np.full(40, 777)])
        rk = np.concatenate([rng.integers(0, 50_000, 30_000), np.full(9_000, 777)])
    elif shape == "sparse_left":
        lk, rk = rng.integers(0, 10**6, 3_000), rng.integers(0, 10**6, 300_000)
    elif shape == "dense_left":
        lk, rk = rng.integers(0, 10**6, 300_000), rng.integers(0, 10**6, 3_000)
    else:
        lk, rk = rng.integers(0, 10**5, 20_000), rng.integers(2 * 10**5, 3 * 10**5, 20_000)
    a = pa.table({"k": lk, "x": np.arange(len(lk), dtype=np.float64)})
    b = pa.table({"k": rk, "y": np.arange(len(rk), dtype=np.float64)})
    g = Table(a, gpu_ctx).join(Table(b, gpu_ctx), "inner", "sort", on=["k"]).to_pandas()
    c = Table(a, ctx).join(Table(b, ctx), "inner", "sort", on=["k"]).to_pandas()
    assert len(g) == len(c)
    key = lambda df: sorted(map(tuple, df[sorted(df.columns)].to_numpy().tolist()))
    assert key(g) == key(c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["signed_wide", "int32_nullable", "dups"])
def test_range_join_matches_cpu(gpu_ctx, ctx, monkeypatch, shape):
    """algorithm="sort" through the range join (order-preserving range partitions + per-partition LDS join by
    exact key offset): same rows as the CPU twin, ordered by key."""
    from cylon_amd._lib import C
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1")
    rng = np.random.default_rng(21)
    if shape == "signed_wide":
        base = -(2 ** 40)
        a = pa.table({"k": base + rng.integers(0, 100_000, 50_000), "x": rng.random(50_000)})
        b = pa.table({"k": base + rng.integers(0, 100_000, 30_000), "y": rng.random(30_000)})
    elif shape == "int32_nullable":
        ka = rng.integers(-20_000, 30_000, 40_000).astype(np.int32)
        kb = rng.integers(-20_000, 30_000, 35_000).astype(np.int32)
        xa = pa.array(rng.random(40_000), mask=rng.random(40_000) < 0.1)
        ib = pa.array(rng.integers(0, 100, 35_000).astype(np.int8), mask=rng.random(35_000) < 0.2)
        a = pa.table({"k": pa.array(ka), "x": xa})
        b = pa.table({"k": pa.array(kb), "i": ib, "z": rng.random(35_000)})
    else:
        a = pa.table({"k": rng.integers(0, 256, 20_000), "x": rng.random(20_000)})
        b = pa.table({"k": rng.integers(0, 256, 20_000), "y": rng.random(20_000)})
    C.trace_enable(True)
    C.trace_reset()
    g = Table(a, gpu_ctx).join(Table(b, gpu_ctx), "inner", "sort", on=["k"], left_prefix="l_",
                               right_prefix="r_").to_pandas()
    assert C.trace_counters().get("join.range.rows_out", -1) == len(g)
    C.trace_enable(False)
    c = Table(a, ctx).join(Table(b, ctx), "inner", "sort", on=["k"], left_prefix="l_", right_prefix="r_").to_pandas()
    assert len(g) == len(c) > 0
    assert np.all(np.diff(g["l_k"].to_numpy().astype(np.int64)) >= 0)
    key = lambda df: sorted(map(tuple, df[sorted(df.columns)].fillna(-1).to_numpy().tolist()))
    assert key(g) == key(c)


@pytest.mark.parametrize("schema", ["HASH", "BTREE"])
def test_persistent_index_on_device(schema):
    """Device-built persistent index (sorted images + device hash table) vs a numpy oracle."""
    import pyarrow as pa
    from cylon_amd.indexing import IndexingSchema, build_index
    rng = np.random.default_rng(8)
    n = 1_000_000
    vals = rng.integers(0, 200_000, n)
    idx = build_index(pa.array(vals), IndexingSchema[schema], "cuda:0")
    labels = rng.integers(0, 210_000, 500).tolist()
    got = idx.positions_of_list(labels).numpy()
    order = np.argsort(vals, kind="stable")
    sv = vals[order]
    exp = np.concatenate([order[np.searchsorted(sv, l, "left"):np.searchsorted(sv, l, "right")] for l in labels])
    assert np.array_equal(got, exp)
    assert idx.persistent_rows == n


def test_staged_ingest_roundtrip(gpu_ctx, monkeypatch):
    """From-Arrow ingest through the pinned staging ring (io/h2d.cpp) is exact: columns larger than
    one staging chunk (and not a multiple of it), a sliced nullable column, strings, and bool
    values unpacked on the device; the pageable path gives the same table."""
    from cylon_amd._lib import C
    n = 5_000_003  # 40 MB int64 column: two 32 MiB chunks, the second partial
    rng = np.random.default_rng(11)
    k = rng.integers(-2**62, 2**62, n)
    valid = rng.random(n) > 0.1
    tbl = pa.table({"k": pa.array(k), "nk": pa.array(k, mask=~valid),
                    "b": pa.array(rng.random(n) < 0.3), "f": pa.array(rng.random(n)),
                    "s": pa.array([f"x{i % 1000}" for i in range(n)])}).slice(7, n - 7)
    got = Table.from_arrow(gpu_ctx, tbl).to_arrow()
    for c in tbl.column_names:
        assert got.column(c).equals(tbl.column(c)), c
    monkeypatch.setenv("CYLON_STAGED_INGEST", "0")
    ref = Table.from_arrow(gpu_ctx, tbl).to_arrow()
    for c in tbl.column_names:
        assert got.column(c).equals(ref.column(c)), c
    # the raw binding: an odd byte count into a larger tensor
    src = np.arange(3 << 20, dtype=np.uint8)
    dst = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda:0")
    C.h2d_copy(src.ctypes.data, src.nbytes - 5, dst)
    assert torch.equal(dst[:src.nbytes - 5].cpu(), torch.from_numpy(src[:-5]))
    assert int(dst[src.nbytes - 5:].sum()) == 0


def test_persistent_string_hash_index_on_device():
    """Device-built string Hash index (hash runs + byte verification) vs a Python oracle."""
    from cylon_amd.indexing import IndexingSchema, build_index
    rng = np.random.default_rng(9)
    n = 400_000
    vals = [f"key-{int(x)}" for x in rng.integers(0, 50_000, n)]
    idx = build_index(pa.array(vals), IndexingSchema.HASH, "cuda:0")
    assert idx.persistent_rows == n
    labels = [vals[int(i)] for i in rng.integers(0, n, 200)] + ["absent-1", "key-"]
    got = idx.positions_of_list(labels).numpy()
    pos = {}
    for i, v in enumerate(vals):
        pos.setdefault(v, []).append(i)
    exp = np.array([p for l in labels for p in pos.get(l, [])], dtype=np.int64)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("n", [0, 1, 5000, 200_000])
def test_string_select_kernel_matches_cpu(gpu_ctx, ctx, n):
    """K15 select_var (kernels/select.hip: string where / fill_null) on the device against its CPU
    twin and Arrow: per-row other, broadcast scalar, null other; rows up to ~3 KB exercise the
    16-byte vector body with unaligned heads."""
    import pyarrow.compute as pc
    rng = np.random.default_rng(n + 1)
    lens = rng.integers(0, 3000, n) if n else np.zeros(0, np.int64)
    lens[::3] = rng.integers(0, 20, len(lens[::3]))
    a = pa.array([None if i % 9 == 0 else "x" * int(lens[i]) + str(i) for i in range(n)], pa.string())
    o = pa.array([None if i % 4 == 0 else "y%d" % i for i in range(n)], pa.string())
    cond = rng.random(n) < 0.4
    at = pa.table({"a": a, "o": o})
    res = []
    for cx in (gpu_ctx, ctx):
        t = Table(at, cx)
        cols = t.native.columns()
        c = torch.from_numpy(cond)
        outs = [C.select_var(cols[0], cols[1], c), C.select_var(cols[0], None, c)]
        fill = t.fillna("F").to_arrow().column("a").combine_chunks()
        res.append([t._wrap(C.Table(t.native.context(), [x])).to_arrow().column("a").combine_chunks() for x in outs]
                   + [fill])
    for g, h in zip(res[0], res[1]):
        assert g.equals(h)
    assert res[0][0].equals(pc.if_else(pa.array(cond, pa.bool_()), a, o))
    assert res[0][2].equals(pc.fill_null(a, "F"))


def test_string_number_casts_on_device(gpu_ctx):
    """K15 astype string <-> number on the device (kernels/strcast.hip) against Arrow's host casts."""
    import pyarrow.compute as pc
    rng = np.random.default_rng(4)
    n = 1_000_000
    ints = rng.integers(-10**12, 10**12, n)
    mask = rng.random(n) < 0.03
    s_int = pa.array([str(x) for x in ints], mask=mask)
    s_flt = pa.array([f"{x / 1000:.3f}" for x in ints], mask=mask)
    t = Table(pa.table({"i": s_int, "f": s_flt, "x": pa.array(ints, mask=mask)}), gpu_ctx)
    c = t.native.columns()
    from cylon_amd.data import compute as cp
    assert all(cp._device_cast(col, typ, True) is not None
               for col, typ in zip(c, (pa.int64(), pa.float64(), pa.string())))  # the device path runs
    out = t.astype({"i": pa.int64(), "f": pa.float64(), "x": pa.string()}).to_arrow()
    assert out.column("i").to_pylist() == pc.cast(s_int, pa.int64()).to_pylist()
    assert out.column("f").to_pylist() == pc.cast(s_flt, pa.float64()).to_pylist()
    bits = lambda a: pc.fill_null(a, 0.0).to_numpy().view(np.uint64)  # noqa: E731  (-0.0 is not 0.0)
    assert np.array_equal(bits(out.column("f").combine_chunks()), bits(pc.cast(s_flt, pa.float64())))
    assert out.column("x").to_pylist() == pc.cast(pa.array(ints, mask=mask), pa.string()).to_pylist()
