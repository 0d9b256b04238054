"""SUM / MEAN / VAR / STDDEV / COUNT on every path against an exact rational oracle.

Every path (CPU hash and pipeline group-by, the scalar aggregates, the GPU global-path kernels
k_agg_scalar / k_agg_lds / k_agg_global, the GPU radix path's RG_SUMF / RG_CNT / RG_M2 planes, the
GPU pipeline group-by, and the distributed two-phase group-by on gloo and RCCL) is compared, group by
group (looked up by the group's key), with exact arithmetic on the float64 images of the non-null
values -- never with another path of the project.

Oracle.  Per group, every non-null value is converted to float64 first; then, exactly (integers
over a common power-of-two denominator, the quotients as fractions.Fraction):

    n,  S = sum x,  mu = S / n,  M2 = sum (x - mu)^2 = sum (n x - S)^2 / n^2,  A = sum |x|.

Tolerances (derived, not measured).  u = 2^-53 is the unit roundoff of float64.

* SUM of a float column.  Any order of the n - 1 rounded additions (a loop, a wave tree, atomics in
  the order the hardware serves them, per-rank partials added later) gives
  |got - S| <= ((1 + u)^(n-1) - 1) * A <= n u A.
* MEAN = fl(fl(S) / n): |got - mu| <= (n-1) u A / n + u |fl(S)| / n  <= u A + u |mu|  (to first
  order; the second-order terms are below u^2 n A, far inside the slack of (n-1)/n vs 1).
* delta = 2 u A bounds the error of any float64 mean of the group: |m - mu| <= u A + u |mu| <= 2 u A.
* VAR over all rows of the group about a computed mean m (tight).  sum (x - m)^2 = M2 + n (m - mu)^2
  exactly (the cross term is 2 (mu - m) sum (x - mu) = 0), so the exact sum of squares about m is
  within n delta^2 of M2.  Each term fl(fl(x - m)^2) carries 3 roundings and the sum of n such
  non-negative terms n - 1 more: a factor (1 + u)^(n+2), bounded by (n + 4) u relative to the exact
  sum M2 + n delta^2.  Dividing by n - ddof and multiplying back costs 2 u M2:
      |got (n - ddof) - M2| <= (n + 4) u (M2 + n delta^2) + n delta^2 + 2 u M2.
* VAR from merged partial states (loose; the distributed path).  With parts i of n_i rows and
  means m_i, M2 = sum_i M2_i + sum_i n_i (mu_i - mu)^2.  Each M2_i obeys the tight bound for its
  rows; the computed d_i = m_i - m differs from mu_i - mu by at most 2 delta, so
  sum n_i d_i^2 is off by at most 2 * 2 delta sum n_i |mu_i - mu| / 2 + O(delta^2)
  <= 2 delta sqrt(n sum n_i (mu_i - mu)^2) <= 2 delta sqrt(n M2) (Cauchy-Schwarz), the O(delta^2)
  part being covered by the n delta^2 of the tight bound; the extra products and additions cost
  4 u M2.  Loose = tight + 2 delta sqrt(n M2) + 4 u M2.  When one pass covers all rows the cross
  term is exactly zero and the tight bound holds.
* VAR >= 0 always.
* STDDEV = fl(sqrt(var)): got^2 = var (1 + u)^2 plus the rounding of the square itself, so with
  v = M2 / (n - ddof) and tol_var = tol_M2 / (n - ddof):
      |got^2 - v| <= tol_var + 3 u (v + tol_var)      (no division by a zero variance).
* COUNT, the integer SUM (Python integers; int64 result) and every null mask are exact: n = 0 gives
  a null mean / var / std, count 0 and sum 0; n - ddof <= 0 gives a null var / std.  An integer sum
  beyond int64 wraps, which is outside the contract: it is compared only where the exact sum fits.

The self-tests at the top run no project code: they hold the oracle to math.fsum / statistics, and
show on every data set that a plain float64 two-pass M2 meets the tight bound, that a Chan merge of
three splits meets the loose bound, and that the textbook sum x^2 - (sum x)^2 / n violates the loose
bound on the `offset` and `const` data -- the data discriminate.

Every test prints its worst error / bound ratio per aggregate (`pytest -s` shows them)."""
import collections
import functools
import math
import statistics
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C

from oracle_utils import INT64_MIN, LADDER, deal_round_robin, spawn_once, traced, wide_keys

U = Fraction(1, 1 << 53)

CLASSES = ("offset", "offset6", "const", "mixed", "float32", "int64_big", "int8")
ONE_GROUP = (1, 65, 4097)

Stats = collections.namedtuple("Stats", "n S mu M2 A I")  # I: the exact sum of integer values


# ---- the oracle (shares nothing with the project)
def oracle(values):
    """Stats of the non-null values, each converted to float64 first; exact."""
    r = [float(v).as_integer_ratio() for v in values if v is not None]
    n = len(r)
    ints = sum(v for v in values if isinstance(v, int))  # (as Python integers: no rounding)
    if n == 0:
        return Stats(0, Fraction(0), None, None, Fraction(0), 0)
    D = max(d for _, d in r)  # denominators are powers of two: the largest is the common one
    X = [p * (D // d) for p, d in r]
    S = sum(X)
    return Stats(n, Fraction(S, D), Fraction(S, n * D), Fraction(sum((n * x - S) ** 2 for x in X), n * n * D * D),
                 Fraction(sum(abs(x) for x in X), D), ints)


def test_oracle_matches_fsum_and_statistics():
    rng = np.random.default_rng(1)
    for n in list(range(1, 40)) + [100, 1000]:
        x = rng.integers(-1000, 1000, n).tolist()
        st = oracle(x)
        assert st.n == n and st.S == math.fsum(x) and st.A == math.fsum(abs(v) for v in x)
        assert st.mu == Fraction(sum(x), n) == statistics.mean(Fraction(v) for v in x)
        assert st.M2 == sum((Fraction(v) - st.mu) ** 2 for v in x)
        assert st.M2 == statistics.pvariance([Fraction(v) for v in x]) * n
        if n > 1:
            assert st.M2 / (n - 1) == statistics.variance([Fraction(v) for v in x])
    # values are taken as float64: a float32 0.1 and an int above 2^53 as their float64 images
    assert oracle([np.float32(0.1)]).S == Fraction(float(np.float32(0.1)))
    assert oracle([(1 << 53) + 1]).S == 1 << 53 and oracle([(1 << 53) + 1, None, 2]).I == (1 << 53) + 3
    assert oracle([0.5, None, 0.25]) == Stats(2, Fraction(3, 4), Fraction(3, 8), Fraction(1, 32), Fraction(3, 4), 0)
    assert oracle([None, None]).n == 0 and oracle([]).n == 0


# ---- the tolerances
def _sqrt_up(f):
    """An upper bound of sqrt(f) (math.sqrt is correctly rounded; the float of f is within 2^-52)."""
    return Fraction(math.sqrt(float(f))) * (1 + Fraction(1, 1 << 40))


def tol_m2(st, loose):
    n, M2 = st.n, st.M2
    delta = 2 * U * st.A
    t = (n + 4) * U * (M2 + n * delta * delta) + n * delta * delta + 2 * U * M2
    if loose:
        t += 2 * delta * _sqrt_up(n * M2) + 4 * U * M2
    return t


def _ratio(err, tol):
    if err <= tol:
        return float(err / tol) if tol > 0 else 0.0
    return float(err / tol) if tol > 0 else math.inf


def judge(op, ddof, got, st, loose, integer):
    """(verdict, error / bound) of one result; verdict None = right, else what is wrong.
    A ratio of None: an exact comparison (or none: an integer sum beyond int64)."""
    n = st.n
    if op == "count":
        return (None if got == n else f"count {got} != {n}"), None
    if op == "sum" and integer:
        if not -(1 << 63) <= st.I < (1 << 63):
            return None, None
        return (None if got == st.I and isinstance(got, int) else f"sum {got!r} != {st.I}"), None
    if op == "sum":
        if got is None:
            return "sum is null", None
        err, tol = abs(Fraction(got) - st.S), n * U * st.A
        return (None if err <= tol else f"sum {got!r}"), _ratio(err, tol)
    if op == "mean":
        if n == 0 or got is None:
            return (None if (n == 0 and got is None) else f"mean {got!r} of {n} values"), None
        err, tol = abs(Fraction(got) - st.mu), U * st.A + U * abs(st.mu)
        return (None if err <= tol else f"mean {got!r}"), _ratio(err, tol)
    assert op in ("var", "std")
    if n - ddof <= 0 or got is None:
        return (None if (n - ddof <= 0 and got is None) else f"{op} {got!r} of {n} values, ddof {ddof}"), None
    if not got >= 0:
        return f"{op} {got!r} is negative or NaN", None
    t2 = tol_m2(st, loose)
    if op == "var":
        err, tol = abs(Fraction(got) * (n - ddof) - st.M2), t2
    else:
        v, tv = st.M2 / (n - ddof), t2 / (n - ddof)
        err, tol = abs(Fraction(got) ** 2 - v), tv + 3 * U * (v + tv)
    return (None if err <= tol else f"{op} {got!r} (exact M2 {float(st.M2)!r})"), _ratio(err, tol)


# ---- data: value classes
def _values(cls, rng, n):
    z = rng.standard_normal(n)
    if cls == "offset":
        return 1e9 + z
    if cls == "offset6":
        return 1e6 + z
    if cls == "const":
        return np.full(n, 0.1)
    if cls == "mixed":  # |x| in [1e-11, 1e9]: no subnormal, no overflow of a square
        z = np.where(np.abs(z) < 1e-3, np.copysign(1e-3, z), z)
        return z * 10.0 ** rng.integers(-8, 9, n)
    if cls == "float32":
        return (1e4 + z).astype(np.float32)
    if cls == "int64_big":  # [2^53, 2^61), every binade: float64 rounds them
        lo = np.int64(1) << rng.integers(53, 61, n)
        return lo + (rng.integers(0, 1 << 60, n) & (lo - 1))
    assert cls == "int8"
    return rng.integers(-128, 128, n).astype(np.int8)


def _second_class(cls):
    return "offset6" if cls == "mixed" else "mixed"


# ---- data: shapes (group sizes and keys)
def _shape_keys(shape, rng):
    """(key of each row, the key whose values are all null or None)"""
    if shape.startswith("one_group_"):
        return np.full(int(shape.rsplit("_", 1)[1]), 42, dtype=np.int64), None
    if shape == "hot":
        keys = wide_keys(rng, 501)
        return np.concatenate([np.full(5000, keys[0]), keys[1:]]).astype(np.int64), keys[7]
    if shape == "two_keys":  # a span of 42 bits: with the int16 field an exact composite key
        keys = (rng.choice(np.arange(-(1 << 20), 1 << 20), len(LADDER) + 1, replace=False) << 20).tolist()
        return np.repeat(np.array(keys, dtype=np.int64), list(LADDER) + [5]), keys[-1]
    assert shape in ("ladder", "many", "nullable_key")
    extra = 2100 if shape == "many" else 0
    keys = wide_keys(rng, len(LADDER) + 1 + extra)
    sizes = list(LADDER) + [5] + [1 + i % 6 for i in range(extra)]
    keys.append(INT64_MIN)  # the radix table's spare slot; the global path's sentinel slot
    sizes.append(100)
    return np.repeat(np.array(keys, dtype=np.int64), sizes), keys[len(LADDER)]


SHAPES = ("ladder", "many", "hot", "two_keys", "nullable_key") + tuple(f"one_group_{n}" for n in ONE_GROUP)


@functools.lru_cache(maxsize=None)
def dataset(shape, cls, nulls=True):
    """(arrow table with keys, x of class `cls` and y of a second class; key column names).
    Fixed seed, shuffled rows, ~10 % null values in x and in y, one group all null in x."""
    rng = np.random.default_rng([7, SHAPES.index(shape), CLASSES.index(cls), int(nulls)])
    k, null_key = _shape_keys(shape, rng)
    n = len(k)
    cols = {"k": k}
    names = ["k"]
    if shape == "two_keys":
        cols["g"] = rng.integers(-1, 2, n).astype(np.int16)
        names.append("g")
    for name, c in (("x", cls), ("y", _second_class(cls))):
        v = _values(c, rng, n)
        a = np.abs(v.astype(np.float64))  # no subnormal, no overflow (an integer 0 is neither)
        assert np.all(((a >= 1e-12) | (a == 0)) & (a <= 1e19))
        if not nulls:
            cols[name] = v
            continue
        mask = rng.random(n) < 0.1
        if name == "x" and null_key is not None:
            mask |= k == null_key
        cols[name] = (v, mask)
    if shape == "nullable_key":
        cols["k"] = (k, rng.random(n) < 0.08)
    order = rng.permutation(n)
    arrays = {name: pa.array(c[0][order], mask=c[1][order]) if isinstance(c, tuple) else pa.array(c[order])
              for name, c in cols.items()}
    return pa.table(arrays), tuple(names)


@functools.lru_cache(maxsize=None)
def _groups(shape, cls, nulls, col):
    t, keys = dataset(shape, cls, nulls)
    out = {}
    for *kk, v in zip(*[t[c].to_pylist() for c in keys], t[col].to_pylist()):
        out.setdefault(tuple(kk), []).append(v)
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, cls, nulls, col):
    """group key (tuple) -> Stats, from the arrow table itself"""
    return {k: oracle(v) for k, v in _groups(shape, cls, nulls, col).items()}


def _is_int(shape, cls, col):
    return pa.types.is_integer(dataset(shape, cls)[0][col].type)


GROUPED = [(s, c) for s in ("ladder", "many", "hot") for c in CLASSES] + [("two_keys", "offset"),
                                                                          ("nullable_key", "offset")]
SINGLE = [(f"one_group_{n}", c) for c in CLASSES for n in ONE_GROUP]
_ids = lambda cases: [f"{s}-{c}" for s, c in cases]


def test_datasets_hold_what_they_promise():
    for shape, cls in GROUPED + SINGLE:
        ex = expected(shape, cls, True, "x")
        t, keys = dataset(shape, cls)
        sizes = sorted(len(v) for v in _groups(shape, cls, True, "x").values())
        if shape in ("ladder", "many", "nullable_key"):
            assert (INT64_MIN,) in ex and 2 <= len(ex)
            assert any(k[0] is not None and k[0] > 1 << 32 for k in ex) and any(
                k[0] is not None and k[0] < -(1 << 32) for k in ex)
        if shape == "ladder":
            assert sizes == sorted(LADDER + (5, 100)) and len(ex) <= 2048
        if shape == "many":
            assert len(ex) > 2048 and t.num_rows < 11_000  # k_agg_global; > 1 radix partition
        if shape == "hot":
            assert sizes[-1] == 5000 and sizes[-2] == 1 and len(ex) == 501
        if shape == "nullable_key":
            assert (None,) in ex
        if shape == "two_keys":
            assert len(keys) == 2 and len(ex) > len(LADDER) + 1
        if not shape.startswith("one_group"):
            assert any(st.n == 0 for st in ex.values()), "a group without values"
            assert t["x"].null_count > 0 and t["y"].null_count > 0
        assert any(st.n >= 1 for st in ex.values())


# ---- self-test of the tolerances: plain numpy, no project code
def _two_pass(x):
    m = x.sum() / len(x)
    return float(((x - m) ** 2).sum())


def _chan3(x):
    n = mean = m2 = 0.0
    for part in np.array_split(x, 3):
        if len(part) == 0:
            continue
        pn, pm = float(len(part)), float(part.sum() / len(part))
        pm2 = float(((part - pm) ** 2).sum())
        d = pm - mean
        m2 += pm2 + d * d * n * pn / (n + pn)
        mean += d * pn / (n + pn)
        n += pn
    return m2


def _textbook(x):
    return float(np.dot(x, x) - x.sum() ** 2 / len(x))


@pytest.mark.parametrize("shape,cls", GROUPED + SINGLE, ids=_ids(GROUPED + SINGLE))
def test_tolerances_discriminate(shape, cls):
    rng = np.random.default_rng(3)
    ex = expected(shape, cls, True, "x")
    worst2 = worst3 = 0.0
    broke = 0
    for key, vals in _groups(shape, cls, True, "x").items():
        st = ex[key]
        if st.n == 0:
            continue
        x = rng.permutation(np.array([float(v) for v in vals if v is not None], dtype=np.float64))
        tight, loose = tol_m2(st, False), tol_m2(st, True)
        e2, e3 = abs(Fraction(_two_pass(x)) - st.M2), abs(Fraction(_chan3(x)) - st.M2)
        assert e2 <= tight, (key, st.n, float(e2), float(tight))
        assert e3 <= loose, (key, st.n, float(e3), float(loose))
        worst2, worst3 = max(worst2, _ratio(e2, tight)), max(worst3, _ratio(e3, loose))
        broke += abs(Fraction(_textbook(x)) - st.M2) > loose
    print(f"[moments] self-test {shape}/{cls}: two-pass/tight {worst2:.3g} chan/loose {worst3:.3g} "
          f"textbook breaks loose in {broke} of {len(ex)} groups")
    if cls in ("offset", "const") and not shape.startswith("one_group"):
        assert broke > 0, "the textbook formula passes: the data do not discriminate"


# ---- comparing a result table with the oracle
ALL_AGGS = {"x": [("var", 0), ("var", 1), ("var", 2), ("std", 0), ("std", 1), ("std", 2), "mean", "sum", "count"],
            "y": ["sum", "mean"]}
FAST_AGGS = {"x": ["sum", "mean", "count"], "y": ["mean", "sum"]}


def _specs(aggs):
    """result columns after the keys: (column, op, ddof)"""
    out = []
    for col, ops in aggs.items():
        for op in ops:
            out.append((col,) + (op if isinstance(op, tuple) else (op, 1)))
    return out


def _columns(tbl):
    a = tbl.to_arrow()
    return [a.column(i).to_pylist() for i in range(a.num_columns)]


def check(columns, aggs, shape, cls, what, loose=False, nulls=True):
    """Every group of every result column against the oracle; prints the worst error / bound."""
    nkeys = len(dataset(shape, cls, nulls)[1])
    specs = _specs(aggs)
    assert len(columns) == nkeys + len(specs), (len(columns), nkeys, specs)
    keys = list(zip(*columns[:nkeys]))
    assert len(set(keys)) == len(keys), f"{what}: a group came out twice"
    worst, bad = {}, []
    for j, (col, op, ddof) in enumerate(specs):
        exp = expected(shape, cls, nulls, col)
        assert set(keys) == exp.keys(), f"{what}: groups differ"
        for k, got in zip(keys, columns[nkeys + j]):
            verdict, ratio = judge(op, ddof, got, exp[k], loose, _is_int(shape, cls, col))
            if ratio is not None:
                worst[op] = max(worst.get(op, 0.0), ratio)
            if verdict is not None:
                bad.append((col, op, ddof, k, exp[k].n, verdict, ratio))
    print(f"[moments] {what} {shape}/{cls}: " + " ".join(f"{op} {r:.3g}" for op, r in sorted(worst.items())))
    assert not bad, f"{what} {shape}/{cls}: {len(bad)} results off, " \
                    f"(column, op, ddof, key, n, what, error / bound): {bad[:6]}"


# ---- CPU context
@pytest.mark.parametrize("shape,cls", GROUPED + SINGLE, ids=_ids(GROUPED + SINGLE))
def test_cpu_hash_groupby_matches_oracle(ctx, shape, cls):
    t, keys = dataset(shape, cls)
    check(_columns(Table(t, ctx).local_groupby(list(keys), ALL_AGGS)), ALL_AGGS, shape, cls, "cpu hash")


@pytest.mark.parametrize("shape,cls", GROUPED, ids=_ids(GROUPED))
def test_cpu_pipeline_groupby_matches_oracle(ctx, shape, cls):
    t, keys = dataset(shape, cls)
    T = Table(t.sort_by([(c, "ascending") for c in keys]), ctx)
    check(_columns(T.local_groupby(list(keys), ALL_AGGS, algorithm="pipeline")), ALL_AGGS, shape, cls, "cpu pipeline")


def _scalar_one(T, col, op, ddof):
    out = (getattr(T, op)(col, ddof=ddof) if op in ("var", "std") else getattr(T, op)(col)).to_arrow()
    assert out.num_rows == 1 and out.num_columns == 1
    return out.column(0).to_pylist()[0]


def _check_scalar(context, cls, what):
    worst, bad = {}, []
    cases = [(f"one_group_{n}", dataset(f"one_group_{n}", cls)[0], None) for n in ONE_GROUP]
    typ = cases[0][1]["x"].type
    cases.append(("empty", pa.table({"x": pa.array([], type=typ)}), oracle([])))
    cases.append(("all_null", pa.table({"x": pa.array([None] * 9, type=typ)}), oracle([None] * 9)))
    for shape, t, st in cases:
        T = Table(t, context)
        for col in ("x", "y") if st is None else ("x",):
            s = st or expected(shape, cls, True, col)[(42,)]
            integer = pa.types.is_integer(t[col].type)
            for _, op, ddof in _specs({col: ALL_AGGS["x"]}):
                verdict, ratio = judge(op, ddof, _scalar_one(T, col, op, ddof), s, False, integer)
                if ratio is not None:
                    worst[op] = max(worst.get(op, 0.0), ratio)
                if verdict is not None:
                    bad.append((shape, col, op, ddof, verdict, ratio))
    print(f"[moments] {what} one_group/{cls}: " + " ".join(f"{op} {r:.3g}" for op, r in sorted(worst.items())))
    assert not bad, f"{what} {cls}: (shape, column, op, ddof, what, error / bound): {bad[:6]}"


@pytest.mark.parametrize("cls", CLASSES)
def test_cpu_scalar_aggregates_match_oracle(ctx, cls):
    _check_scalar(ctx, cls, "cpu scalar")


# ---- distributed: the two-phase group-by with merged partial states (loose bound for VAR / STDDEV)
DIST_CASES = [(s, c, "generic") for s, c in GROUPED] + [("ladder", c, "fast") for c in CLASSES]


def _dist_worker(ctx, cases, chunks, forced):
    """Every case on this rank's share of the rows: row j of a group (in table order) lives on rank
    j mod world, so every group of at least 2 rows spans ranks.  generic: nullable columns and VAR
    (phase 1 builds the partial states itself); fast: SUM / MEAN / COUNT of non-null columns (phase 1
    is a local hash group-by)."""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    if forced:
        assert world == 1 and ctx.is_distributed()
        ctx.add_config("force_shuffle", "1")
        ctx.add_config("shuffle_self_rccl", "1")
    ctx.add_config("shuffle_chunks", str(chunks))
    out = {}
    C.trace_enable(True)
    C.trace_reset()
    for shape, cls, form in cases:
        t, keys = dataset(shape, cls, form == "generic")
        mine = deal_round_robin(zip(*[t[c].to_pylist() for c in keys]), rank, world)
        T = Table(t.take(pa.array(mine, type=pa.int64())), ctx)
        assert T.device == ctx.device
        out[(shape, cls, form)] = _columns(T.groupby(list(keys), ALL_AGGS if form == "generic" else FAST_AGGS))
    counters = dict(C.trace_counters())
    C.trace_enable(False)
    return out, counters


_spawned, _merged = {}, {}


def _dist_results(world, device, chunks, rccl_forced=False):
    """One spawn per configuration, ever (a failed spawn is remembered, not repeated);
    (case -> result columns concatenated over the ranks, counters of every rank)."""
    cfg = (world, device, chunks, rccl_forced)
    res = spawn_once(_spawned, _dist_worker, DIST_CASES, world, device, chunks, rccl_forced)
    if cfg not in _merged:
        merged = {}
        for case in DIST_CASES:
            parts = [r[0][case] for r in res]
            merged[case] = [sum((p[i] for p in parts), []) for i in range(len(parts[0]))]
        _merged[cfg] = (merged, [r[1] for r in res])
    return _merged[cfg]


def _check_dist(results, case, what):
    shape, cls, form = case
    check(results[0][case], ALL_AGGS if form == "generic" else FAST_AGGS, shape, cls, f"{what} {form}", loose=True,
          nulls=form == "generic")


_dist_ids = [f"{s}-{c}-{f}" for s, c, f in DIST_CASES]


@pytest.mark.parametrize("case", DIST_CASES, ids=_dist_ids)
@pytest.mark.parametrize("world,chunks", [(2, 1), (3, 3)], ids=["2ranks", "3ranks_chunked"])
def test_cpu_distributed_groupby_matches_oracle(world, chunks, case):
    _check_dist(_dist_results(world, "cpu", chunks), case, f"cpu {world} ranks")


# ---- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls", GROUPED + SINGLE, ids=_ids(GROUPED + SINGLE))
def test_gpu_global_path_matches_oracle(gpu_ctx, monkeypatch, shape, cls):
    """kernels/groupby.hip: k_agg_scalar (one group), k_agg_lds (<= 2048 groups; `hot`: one contended
    LDS slot), k_agg_global (`many`); the INT64_MIN key sits in group_insert's sentinel slot."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", str(1 << 62))
    t, keys = dataset(shape, cls)
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), ALL_AGGS))
    assert "groupby.radix.groups" not in cnt, cnt
    check(_columns(got), ALL_AGGS, shape, cls, "gpu global")


RADIX_AGGS = {
    3: {"x": [("var", 0), ("var", 1), ("var", 2)]},
    4: {"x": [("var", 0), ("var", 1), ("var", 2), "mean", "sum"], "y": ["sum"]},
    8: {"x": [("var", 0), ("var", 1), ("var", 2), ("std", 0), ("std", 1), ("std", 2)], "y": [("var", 1), "mean"]},
}


@pytest.mark.gpu
@pytest.mark.parametrize("planes", sorted(RADIX_AGGS))
@pytest.mark.parametrize("shape,cls", GROUPED + SINGLE, ids=_ids(GROUPED + SINGLE))
def test_gpu_radix_path_matches_oracle(gpu_ctx, monkeypatch, shape, cls, planes):
    """kernels/radix_groupby.hip k_rg_agg with 3, 4 and 8 accumulator planes: RG_SUMF / RG_CNT in the
    first pass, RG_M2 in the second in-block pass (the INT64_MIN key in the spare slot S); `many`
    spans several partitions."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", "1")
    t, keys = dataset(shape, cls)
    aggs = RADIX_AGGS[planes]
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), aggs))
    assert cnt.get("groupby.radix.groups") == len(expected(shape, cls, True, "x")), cnt
    assert cnt.get("groupby.radix.overflow_fallback", 0) == 0, cnt
    check(_columns(got), aggs, shape, cls, f"gpu radix {planes} planes")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls", GROUPED, ids=_ids(GROUPED))
def test_gpu_pipeline_groupby_matches_oracle(gpu_ctx, shape, cls):
    t, keys = dataset(shape, cls)
    T = Table(t.sort_by([(c, "ascending") for c in keys]), gpu_ctx)
    check(_columns(T.local_groupby(list(keys), ALL_AGGS, algorithm="pipeline")), ALL_AGGS, shape, cls, "gpu pipeline")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_gpu_scalar_aggregates_match_oracle(gpu_ctx, cls):
    _check_scalar(gpu_ctx, cls, "gpu scalar")


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIST_CASES, ids=_dist_ids)
def test_gpu_distributed_groupby_matches_oracle(case):
    """2 ranks share cuda:0, the collectives go over gloo: the device kernels of both phases."""
    _check_dist(_dist_results(2, "cuda:0", 2), case, "gpu 2 ranks")


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIST_CASES, ids=_dist_ids)
def test_gpu_forced_rccl_groupby_matches_oracle(case):
    """A world-1 RCCL context with force_shuffle: the partial rows go through the chunked RCCL
    exchange and the combine merges them chunk by chunk."""
    results = _dist_results(1, "cuda:0", 4, True)
    _check_dist(results, case, "gpu forced rccl")
    assert results[1][0].get("shuffle.chunks", 0) > 0, results[1][0]
