"""QUANTILE on every path against an independent type-2 oracle.

The aggregate has four implementations (the CPU twin cpu::group_quantile, the global-path kernel
k_quantile, and inside k_rg_quantile the single-key wave radix select, the mixed-key bitonic bucket
and the rank-counting loop for buckets over 128 rows).  Each is compared here with a plain-Python
statement of R's type-2 rule (docs/semantics.md, "QUANTILE"), never with another path.

Tolerance: exact equality of values and null masks (`==`, so -0.0 equals +0.0).  An order statistic
is a copy of an input value; the averaged case is one rounded add and an exact halving, the same
expression everywhere.  The data keeps NaN out and magnitudes where a + b cannot overflow.  The
fused aggregates run on integer-valued float64 data of small magnitude, whose sums are exact in any
order, so sum, mean, min, max and count are compared exactly as well."""
import functools
import math

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Code, CylonError, Table
from cylon_amd._lib import C

QS = (0.0, 1.0, 0.5, 0.25, 0.75, 0.1, 0.9, 1 / 3, 1 / 7, 6 / 7)
LADDER = range(1, 131)  # group sizes: the one-row group, both sides of the 64- and 128-row wave limits


# ---- the oracle (shares nothing with the project)
def oracle(values, q):
    """R type 2 over the non-null values, each converted to float64 first; None for no value."""
    x = sorted(float(v) for v in values if v is not None)
    n = len(x)
    if n == 0:
        return None
    np_ = n * q
    j = math.floor(np_)
    if j >= n:
        return x[n - 1]
    if np_ == j and j > 0:
        return 0.5 * (x[j - 1] + x[j])
    return x[j]


def test_oracle_matches_numpy_averaged_inverted_cdf():
    """numpy's 'averaged_inverted_cdf' is R type 2; it lerps between the two order statistics, so only
    integer-valued data is bit-comparable.  n = 1..200, every q of the set, q = 1 -> max included."""
    rng = np.random.default_rng(1)
    cases = 0
    for n in range(1, 201):
        x = rng.integers(-1000, 1000, n).astype(np.float64)
        for q in QS:
            assert oracle(x.tolist(), q) == float(np.quantile(x, q, method="averaged_inverted_cdf")), (n, q)
            cases += 1
    assert cases == 200 * len(QS)
    assert oracle([3.0, 1.0, 2.0], 1.0) == 3.0 and oracle([3.0, 1.0, 2.0], 0.0) == 1.0
    assert oracle([None, None], 0.5) is None and oracle([], 0.5) is None


# ---- the kernel's bucket function, mirrored (radix_groupby.hip k_rg_quantile, bucket_of)
def bucket_of(key):
    u = key & 0xFFFFFFFFFFFFFFFF
    f = (u ^ (u >> 32)) & 0xFFFFFFFF
    return ((f * 0x9E3779B1) & 0xFFFFFFFF) >> 21


def _bucket_sizes(keys):
    """bucket -> {key: rows} of a key column, assuming one partition."""
    out = {}
    for k in keys:
        d = out.setdefault(bucket_of(k), {})
        d[k] = d.get(k, 0) + 1
    return out


def _lone_bucket_keys(rng, count, taken=()):
    """`count` int64 keys (both signs, high half set), each alone in its bucket and off `taken`."""
    used, keys = set(taken), []
    while len(keys) < count:
        k = int(rng.integers(-(1 << 40), 1 << 40))
        if bucket_of(k) not in used:
            used.add(bucket_of(k))
            keys.append(k)
    return keys


# ---- data sets (built once, fixed seed, shuffled row order); a data set is (arrow table, key columns)
def _shuffled(rng, cols):
    n = len(next(iter(cols.values())))
    order = rng.permutation(n)
    out = {}
    for name, c in cols.items():
        if isinstance(c, tuple):  # (values, null mask)
            out[name] = pa.array(c[0][order], mask=c[1][order])
        else:
            out[name] = pa.array(c[order])
    return pa.table(out)


def _distinct(rng, n):
    return (rng.permutation(n) - n // 2) * (1.0 / 3.0)


_INT_RANGES = {"int8": (-128, 128), "int16": (-(1 << 15), 1 << 15), "int32": (-(1 << 31), 1 << 31),
               "int64": (-(1 << 62), 1 << 62), "uint8": (0, 256), "uint32": (0, 1 << 32)}
DTYPE_Q = {"float32": 1 / 3, "int8": 0.5, "int16": 0.25, "int32": 0.75, "int64": 0.9, "uint8": 0.1,
           "uint32": 6 / 7, "uint64": 1 / 7}


@functools.lru_cache(maxsize=None)
def ladder(variant):
    """One int64 key per group size 1..130, every key alone in its bucket (single-key wave select up
    to 128 rows, rank counting above).  variant: distinct | ties | nullable | two_keys | a dtype."""
    rng = np.random.default_rng(20)
    keys = _lone_bucket_keys(rng, len(LADDER))
    k = np.repeat(np.array(keys, dtype=np.int64), list(LADDER))
    n = len(k)
    mask = None
    if variant in ("distinct", "two_keys"):
        x = _distinct(rng, n)
    elif variant == "ties":  # integers in [-3, 3] as float64, half of the zeros negative
        x = rng.integers(-3, 4, n).astype(np.float64)
        x[(x == 0.0) & (rng.random(n) < 0.5)] = -0.0
        assert np.signbit(x[x == 0.0]).any() and not np.signbit(x[x == 0.0]).all()
    elif variant == "nullable":  # ~10 % nulls, three groups all null; integer-valued: exact sums
        x = rng.integers(-1000, 1001, n).astype(np.float64)
        mask = (rng.random(n) < 0.1) | np.isin(k, [keys[0], keys[64], keys[129]])
    elif variant == "float32":
        x = (rng.standard_normal(n) * 100.0).astype(np.float32)
        mask = rng.random(n) < 0.1
    elif variant == "uint64":  # above 2^63
        x = rng.integers(1 << 63, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
        mask = rng.random(n) < 0.1
    else:
        lo, hi = _INT_RANGES[variant]
        x = rng.integers(lo, hi, n, dtype=np.int64 if lo < 0 else np.uint64).astype(variant)
        mask = rng.random(n) < 0.1
    cols = {"k": k, "x": x if mask is None else (x, mask)}
    names = ["k"]
    if variant == "two_keys":  # int64 + int16: an exact composite key; the second field splits the groups
        cols = {"k": k, "g": rng.integers(-1, 2, n).astype(np.int16), "x": x}
        names = ["k", "g"]
    return _shuffled(rng, cols), tuple(names)


# (sizes of the keys sharing one bucket); the kinds by total: <= 64 one-slot wave, 65..128 two-slot
# wave, > 128 rank counting
_SMALL_SETS = ((30, 34), (5, 5), (1, 1, 1), (10, 10, 10, 10))
_MID_SETS = ((32, 33), (60, 40, 28), (50, 30, 20), (20, 20, 20, 20))
_BIG_SETS = ((150, 1, 1, 1), (70, 70), (100, 40, 10))
# (set, position by ascending key) of the colliding groups whose values are all null
_ALL_NULL = ((_SMALL_SETS[0], 0), (_MID_SETS[2], 2), (_BIG_SETS[2], 1))


@functools.lru_cache(maxsize=None)
def collisions():
    """<= 2000 rows, >= 100 groups: one partition, with sets of 2-4 keys sharing a bucket."""
    rng = np.random.default_rng(21)
    pool = {}
    for k in rng.integers(-(1 << 40), 1 << 40, 40_000).tolist():
        pool.setdefault(bucket_of(k), set()).add(k)
    buckets = iter(sorted(b for b, ks in pool.items() if len(ks) >= 4))
    sizes, all_null, force_null = {}, set(), set()
    for sets in (_SMALL_SETS, _MID_SETS, _BIG_SETS):
        for s in sets:
            ks = sorted(pool[next(buckets)])[:len(s)]
            sizes.update(zip(ks, s))
            if s[-1] > 1:
                force_null.add(ks[-1])  # the bucket's largest key gets null rows (the pad convention)
            for t, pos in _ALL_NULL:
                if t is s:
                    all_null.add(ks[pos])
    fillers = _lone_bucket_keys(rng, 70, taken={bucket_of(k) for k in sizes})
    sizes.update((key, 1 + i % 12) for i, key in enumerate(fillers))
    k = np.repeat(np.array(list(sizes), dtype=np.int64), list(sizes.values()))
    n = len(k)
    x = rng.integers(-20, 21, n).astype(np.float64)
    mask = (rng.random(n) < 0.15) | np.isin(k, list(all_null))
    for key in force_null:
        mask[np.flatnonzero(k == key)[0]] = True
    return _shuffled(rng, {"k": k, "x": (x, mask)}), ("k",)


@functools.lru_cache(maxsize=None)
def large_group(variant):
    """One group of 2500 rows (rank counting at scale) plus 500 one-row groups: one partition."""
    rng = np.random.default_rng(22)
    keys = rng.choice(np.arange(-5000, 5000), 501, replace=False).astype(np.int64) * 1_000_003
    k = np.concatenate([np.full(2500, keys[0]), keys[1:]])
    n = len(k)
    if variant == "distinct":
        return _shuffled(rng, {"k": k, "x": _distinct(rng, n)}), ("k",)
    x = rng.integers(-50, 51, n).astype(np.float64)  # ties, ~10 % nulls
    return _shuffled(rng, {"k": k, "x": (x, rng.random(n) < 0.1)}), ("k",)


@functools.lru_cache(maxsize=None)
def over_capacity():
    """One group of 5000 rows, above the radix kernel's 4096-row partition capacity, plus 1000 small groups."""
    rng = np.random.default_rng(23)
    keys = rng.choice(np.arange(-50_000, 50_000), 1001, replace=False).astype(np.int64) * 7919
    k = np.concatenate([np.full(5000, keys[0]), np.repeat(keys[1:], 1 + np.arange(1000) % 3)])
    n = len(k)
    x = np.round(rng.standard_normal(n) * 100.0, 1)
    return _shuffled(rng, {"k": k, "x": (x, rng.random(n) < 0.1)}), ("k",)


DATASETS = {**{f"ladder_{v}": functools.partial(ladder, v) for v in ("distinct", "ties", "nullable", "two_keys")},
            "collisions": collisions,
            "large_distinct": functools.partial(large_group, "distinct"),
            "large_ties_nullable": functools.partial(large_group, "ties_nullable"),
            "over_capacity": over_capacity}


@functools.lru_cache(maxsize=None)
def _groups(name):
    """group key (tuple) -> the group's values (None for null), from the arrow table itself."""
    if name in DATASETS:
        t, keys = DATASETS[name]()
    else:
        t, keys = ladder(name)
    out = {}
    for *kk, v in zip(*[t[c].to_pylist() for c in keys], t["x"].to_pylist()):
        out.setdefault(tuple(kk), []).append(v)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, q):
    return {k: oracle(v, q) for k, v in _groups(name).items()}


def _dataset(name):
    return DATASETS[name]() if name in DATASETS else ladder(name)


def _result(tbl, nkeys, col):
    """group key -> value of result column `col` (by position: two quantiles share a name)."""
    a = tbl.to_arrow()
    keys = list(zip(*[a.column(i).to_pylist() for i in range(nkeys)]))
    vals = a.column(col).to_pylist()
    assert len(set(keys)) == len(keys), "a group came out twice"
    return dict(zip(keys, vals))


def _assert_equal(got, exp, what):
    assert got.keys() == exp.keys(), f"{what}: groups differ"
    bad = [(k, got[k], exp[k]) for k in exp if (got[k] is None) != (exp[k] is None) or
           (exp[k] is not None and not got[k] == exp[k])]
    assert not bad, f"{what}: {len(bad)} of {len(exp)} groups differ, (key, got, oracle): {bad[:5]}"


def _check_groupby(T, name, keys, q, what, **kw):
    got = T.local_groupby(list(keys), {"x": [("quantile", q)]}, **kw)
    _assert_equal(_result(got, len(keys), len(keys)), expected(name, q), f"{what} {name} q={q!r}")


# ---- what the data sets must contain, by the mirror: fails loudly if the kernel's hash changes
def test_ladder_keys_have_their_own_buckets():
    t, _ = ladder("distinct")
    b = _bucket_sizes(t["k"].to_pylist())
    assert len(b) == len(LADDER) and all(len(d) == 1 for d in b.values())
    assert sorted(next(iter(d.values())) for d in b.values()) == list(LADDER)


def test_collisions_cover_every_bucket_kind():
    t, _ = collisions()
    assert t.num_rows <= 2000
    groups = _groups("collisions")
    assert len(groups) >= 100
    mixed = [d for d in _bucket_sizes(t["k"].to_pylist()).values() if len(d) > 1]
    assert all(2 <= len(d) <= 4 for d in mixed)
    totals = sorted(sum(d.values()) for d in mixed)
    assert len([s for s in totals if s <= 64]) >= 3 and 64 in totals
    assert len([s for s in totals if 65 <= s <= 128]) >= 3 and 65 in totals and 128 in totals
    assert len([s for s in totals if s > 128]) >= 3
    assert any(sorted(d.values()) == [1, 1, 1, 150] for d in mixed)
    nulls = {k[0]: sum(v is None for v in vs) for k, vs in groups.items()}
    # the largest key of a mixed bucket has null rows next to valid ones; a colliding group is all null
    for lo, hi in ((2, 64), (65, 128), (129, 4096)):
        kind = [d for d in mixed if lo <= sum(d.values()) <= hi]
        assert any(0 < nulls[max(d)] < d[max(d)] for d in kind), (lo, hi)
        assert any(nulls[k] == d[k] for d in kind for k in d), (lo, hi)


# ---- CPU context
_CPU_SETS = list(DATASETS) + list(DTYPE_Q)


@pytest.mark.parametrize("name", _CPU_SETS)
def test_cpu_hash_groupby_matches_oracle(ctx, name):
    t, keys = _dataset(name)
    T = Table(t, ctx)
    for q in ((DTYPE_Q[name],) if name in DTYPE_Q else QS):
        _check_groupby(T, name, keys, q, "cpu hash")


@pytest.mark.parametrize("name", ["ladder_distinct", "ladder_ties", "ladder_nullable", "ladder_two_keys",
                                  "collisions", "large_ties_nullable"])
def test_cpu_pipeline_groupby_matches_oracle(ctx, name):
    t, keys = _dataset(name)
    T = Table(t.sort_by([(c, "ascending") for c in keys]), ctx)
    for q in QS:
        _check_groupby(T, name, keys, q, "cpu pipeline", algorithm="pipeline")


def _scalar_columns():
    rng = np.random.default_rng(24)
    cols = {}
    for n in (1, 2, 7, 64, 65, 129, 1000):
        cols[f"distinct_{n}"] = pa.array(_distinct(rng, n))
    cols["ties_nullable"] = pa.array(rng.integers(-3, 4, 500).astype(np.float64), mask=rng.random(500) < 0.2)
    cols["int32_nullable"] = pa.array(rng.integers(-1000, 1000, 333).astype(np.int32), mask=rng.random(333) < 0.1)
    cols["all_null"] = pa.array([None] * 9, type=pa.float64())
    cols["empty"] = pa.array([], type=pa.float64())
    return cols


def _check_scalar(context):
    for name, col in _scalar_columns().items():
        T = Table(pa.table({"x": col}), context)
        for q in QS:
            out = T.quantile("x", q).to_arrow()
            assert out.num_rows == 1 and out.num_columns == 1
            got, exp = out.column(0).to_pylist()[0], oracle(col.to_pylist(), q)
            assert (got is None) == (exp is None) and (exp is None or got == exp), (name, q, got, exp)


def test_cpu_scalar_quantile_matches_oracle(ctx):
    _check_scalar(ctx)


@pytest.mark.parametrize("q", [-0.1, 1.5, float("nan")])
def test_bad_q_is_rejected(ctx, q):
    """q outside [0, 1] or NaN raises Code.Invalid at the ops-level entries, before any dispatch (the
    check is host code shared by both devices, so it is tested on the CPU context only)."""
    t = pa.table({"k": [1, 1, 2], "x": [1.0, 2.0, 3.0]})
    T = Table(t, ctx)
    calls = [lambda: T.local_groupby(["k"], {"x": [("quantile", q)]}),
             lambda: T.local_groupby(["k"], {"x": ["sum", ("quantile", q)]}, algorithm="pipeline"),
             lambda: T.groupby(["k"], {"x": [("quantile", q)]}),
             lambda: T.groupby(["k"], {"x": [("quantile", q)]}, algorithm="pipeline"),
             lambda: T.quantile("x", q)]
    for call in calls:
        with pytest.raises(CylonError) as e:
            call()
        assert e.value.args[1] == int(Code.Invalid), e.value.args
    # the bounds themselves are valid; q only matters for QUANTILE
    assert T.quantile("x", 0.0).to_arrow().column(0).to_pylist() == [1.0]
    assert T.quantile("x", 1.0).to_arrow().column(0).to_pylist() == [3.0]
    assert T.local_groupby(["k"], {"x": [("var", 0)]}).row_count == 2


# ---- GPU
def _traced(fn):
    C.trace_enable(True)
    C.trace_reset()
    try:
        return fn(), dict(C.trace_counters())
    finally:
        C.trace_enable(False)


def _gpu_groupby(T, keys, aggs, monkeypatch, radix):
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", "1" if radix else str(1 << 62))
    out, cnt = _traced(lambda: T.local_groupby(list(keys), aggs))
    if not radix:
        assert cnt.get("groupby.radix.quantile", 0) == 0, cnt
    return out, cnt


_GPU_SETS = [n for n in DATASETS if n != "over_capacity"] + list(DTYPE_Q)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _GPU_SETS + ["over_capacity"])
def test_gpu_global_path_matches_oracle(gpu_ctx, monkeypatch, name):
    """k_quantile (kernels/groupby.hip): values sorted by (group, value), one thread per group."""
    t, keys = _dataset(name)
    T = Table(t, gpu_ctx)
    for q in ((DTYPE_Q[name],) if name in DTYPE_Q else QS):
        got, _ = _gpu_groupby(T, keys, {"x": [("quantile", q)]}, monkeypatch, radix=False)
        _assert_equal(_result(got, len(keys), len(keys)), expected(name, q), f"gpu global {name} q={q!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _GPU_SETS)
def test_gpu_radix_path_matches_oracle(gpu_ctx, monkeypatch, name):
    """k_rg_quantile (kernels/radix_groupby.hip): the wave radix select (ladder groups up to 128
    rows), the bitonic mixed bucket (collisions) and rank counting (buckets over 128 rows)."""
    t, keys = _dataset(name)
    T = Table(t, gpu_ctx)
    for q in ((DTYPE_Q[name],) if name in DTYPE_Q else QS):
        got, cnt = _gpu_groupby(T, keys, {"x": [("quantile", q)]}, monkeypatch, radix=True)
        assert cnt.get("groupby.radix.quantile", 0) == 1, cnt
        assert cnt.get("groupby.radix.quantile_overflow_fallback", 0) == 0, cnt
        _assert_equal(_result(got, len(keys), len(keys)), expected(name, q), f"gpu radix {name} q={q!r}")


@pytest.mark.gpu
def test_gpu_radix_over_capacity_falls_back(gpu_ctx, monkeypatch):
    """A 5000-row group never fits a 4096-row partition: the radix path gives up (the fallback counter)
    and the global path answers, still equal to the oracle."""
    t, keys = over_capacity()
    T = Table(t, gpu_ctx)
    for q in QS:
        got, cnt = _gpu_groupby(T, keys, {"x": [("quantile", q)]}, monkeypatch, radix=True)
        assert cnt.get("groupby.radix.quantile_overflow_fallback", 0) == 1, cnt
        assert cnt.get("groupby.radix.quantile", 0) == 0, cnt
        _assert_equal(_result(got, 1, 1), expected("over_capacity", q), f"gpu over capacity q={q!r}")


@functools.lru_cache(maxsize=None)
def _expected_fused(name):
    """group -> (sum, min, max, count, mean) of integer-valued data: exact in any order."""
    out = {}
    for k, vs in _groups(name).items():
        x = [float(v) for v in vs if v is not None]
        assert all(v == int(v) and abs(v) <= 1000 for v in x)
        s = math.fsum(x)
        out[k] = (s, min(x), max(x), len(x), s / len(x)) if x else (0.0, None, None, 0, None)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ladder_nullable", "ladder_ties", "collisions", "large_ties_nullable"])
def test_gpu_radix_fused_matches_oracle(gpu_ctx, monkeypatch, name):
    """The quantile kernel also produces SUM / MIN / MAX / COUNT / MEAN of its own float64 column."""
    t, keys = _dataset(name)
    T = Table(t, gpu_ctx)
    fused = _expected_fused(name)
    for q in QS:
        aggs = {"x": [("quantile", q), "sum", "min", "max", "count", "mean"]}
        got, cnt = _gpu_groupby(T, keys, aggs, monkeypatch, radix=True)
        assert cnt.get("groupby.radix.quantile", 0) == 1, cnt
        assert cnt.get("groupby.radix.quantile_fused_aggs", 0) == 5, cnt
        assert cnt.get("groupby.radix.quantile_overflow_fallback", 0) == 0, cnt
        _assert_equal(_result(got, 1, 1), expected(name, q), f"gpu fused quantile {name} q={q!r}")
        for i, agg in enumerate(("sum", "min", "max", "count", "mean")):
            _assert_equal(_result(got, 1, 2 + i), {k: v[i] for k, v in fused.items()},
                          f"gpu fused {agg} {name} q={q!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ladder_nullable", "collisions"])
@pytest.mark.parametrize("radix", [True, False], ids=["radix", "global"])
def test_gpu_two_quantiles_in_one_call(gpu_ctx, monkeypatch, name, radix):
    t, keys = _dataset(name)
    T = Table(t, gpu_ctx)
    for qa, qb in ((0.0, 1.0), (0.25, 0.75), (1 / 3, 0.9), (6 / 7, 1 / 7), (0.5, 0.1)):
        got, cnt = _gpu_groupby(T, keys, {"x": [("quantile", qa), ("quantile", qb)]}, monkeypatch, radix)
        if radix:
            assert cnt.get("groupby.radix.quantile", 0) == 2, cnt
            assert cnt.get("groupby.radix.quantile_overflow_fallback", 0) == 0, cnt
        _assert_equal(_result(got, 1, 1), expected(name, qa), f"gpu two quantiles {name} first q={qa!r}")
        _assert_equal(_result(got, 1, 2), expected(name, qb), f"gpu two quantiles {name} second q={qb!r}")


@pytest.mark.gpu
def test_gpu_scalar_quantile_matches_oracle(gpu_ctx):
    _check_scalar(gpu_ctx)
