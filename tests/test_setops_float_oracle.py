"""Union / intersect / subtract / unique on tables with a float column (NaN of either sign and any
payload, -0.0, +0.0, nulls) on every path against an oracle on bit patterns.

The contract (docs/semantics.md, "Set operations" and "Float join keys").  Rows are distinct under
the identity tuple of their cells -- null is null, every NaN one value, -0.0 == +0.0 (the identity
function of test_join_float_oracle.py, written from the contract).  The output keeps the first
occurrence of each surviving row in input order (`unique(keep="last")`: the last occurrences, in
input order); the distributed forms return the same rows in an unspecified order.  Each output row
is, bit for bit, SOME input row of its identity: which of the equal bit patterns stands for the
group is unspecified, as for `Unique`.  There are no tolerances in this file.

Paths: the CPU context; 2 ranks over gloo; on the GPU the small path (GroupIds) and the LDS radix
path (kernels/radix_setops.hip, forced with CYLON_RADIX_SETOP_MIN_ROWS=1: taken, no fallback).
Every case first asserts that a bit-equality oracle gives another answer on its inputs."""
import functools

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Table

from oracle_utils import column_bits, fspecials, make_array, spawn_once, traced
from test_join_float_oracle import CLASSES, FLOAT_FIELDS, fbits, identity

OPS = ("union", "intersect", "subtract", "unique_first", "unique_last")
SIZES = {"cpu": (300, 200), "gpu": (3000, 2000)}
CASES = [(c, n) for c in CLASSES for n in (True, False)]
_ids = [f"{c}-{'nullable' if n else 'nonnull'}" for c, n in CASES]
_RIGHT_LACKS = ("pnan", "nsnan", "pzero")


# ---- the oracle
def oracle(op, lrows, rrows):
    """the identities of the output rows, in output order; lrows / rrows: one identity tuple per row"""
    first = lambda rows: list(dict.fromkeys(rows))
    if op == "unique_first":
        return first(lrows)
    if op == "unique_last":
        return first(lrows[::-1])[::-1]
    if op == "union":
        return first(lrows + rrows)
    inright = set(rrows)
    return [k for k in first(lrows) if (k in inright) == (op == "intersect")]


def test_oracle_hand_table():
    F = fspecials(8)
    ident = lambda rows: [(identity(b, 8), i) for b, i in rows]
    L = ident([(F["pnan"], 1), (F["nzero"], 1), (F["nnan"], 1), (F["pzero"], 2), (None, 1), (F["pzero"], 1), (F["pinf"], 1)])
    R = ident([(F["nsnan"], 1), (None, 1), (F["nzero"], 3), (None, 2)])
    nan, zero, inf = "nan", (0, 0), (0, F["pinf"])
    assert oracle("unique_first", L, R) == [(nan, 1), (zero, 1), (zero, 2), (None, 1), (inf, 1)]
    assert oracle("unique_last", L, R) == [(nan, 1), (zero, 2), (None, 1), (zero, 1), (inf, 1)]
    assert oracle("union", L, R) == [(nan, 1), (zero, 1), (zero, 2), (None, 1), (inf, 1), (zero, 3), (None, 2)]
    assert oracle("intersect", L, R) == [(nan, 1), (None, 1)]
    assert oracle("subtract", L, R) == [(zero, 1), (zero, 2), (inf, 1)]


# ---- data
@functools.lru_cache(maxsize=None)
def dataset(cls, nullable, size="cpu"):
    """(left, right): tables (x of the class, i int64 in 0..3) whose rows repeat within and across the sides"""
    typ = CLASSES[cls]
    w = typ.bit_width // 8
    e, m = FLOAT_FIELDS[w]
    rng = np.random.default_rng([29, list(CLASSES).index(cls), int(nullable), list(SIZES).index(size)])
    F = fspecials(w)
    pool = list(F.values()) + [fbits(1.0, w), fbits(-1.0, w)]
    while len(pool) < 54:
        b = int.from_bytes(rng.bytes(w), "little")
        if (b >> m) & ((1 << e) - 1) != (1 << e) - 1 and b not in pool:
            pool.append(b)
    lacks = [F[s] for s in _RIGHT_LACKS]
    lpool, rpool = pool[:44], [b for b in pool[:14] + pool[24:] if b not in lacks]  # ten values on one side only, each
    out = []
    # the head rows: every pattern a side may hold, with i = 0; and with i = 3, which no other row has, a
    # NaN and a zero whose bits differ between the sides
    lhead = [(b, 0) for b in pool[:14]] + [(F["pzero"], 3), (F["pnan"], 3)]
    rhead = [(b, 0) for b in pool[13::-1] if b not in lacks] + [(F["nzero"], 3), (F["nnan"], 3)]
    for n, side, head in ((SIZES[size][0], lpool, lhead), (SIZES[size][1], rpool, rhead)):
        x = [side[j] for j in rng.integers(0, len(side), n)]
        i = rng.integers(0, 3, n).tolist()
        x[:len(head)], i[:len(head)] = [b for b, _ in head], [v for _, v in head]
        if nullable:
            for j in np.flatnonzero(rng.random(n) < 0.08):
                if j >= len(head):
                    x[j] = None
        perm = rng.permutation(n)
        out.append(pa.table({"x": make_array([x[j] for j in perm], typ, nullable),
                             "i": pa.array([i[j] for j in perm], pa.int64())}))
    return tuple(out)


def _rows(t, ident):
    w = t["x"].type.bit_width // 8
    return list(zip([ident(b, w) for b in column_bits(t["x"])], t["i"].to_pylist()))


def _inputs(cls, nullable, size, op):
    L, R = dataset(cls, nullable, size)
    return (L, None) if op.startswith("unique") else (L, R)


@functools.lru_cache(maxsize=None)
def expected(cls, nullable, size, op):
    """(identities in output order, identity -> the input rows (bits of x, i) of it).  Asserts first that
    a bit-equality oracle answers differently, through NaNs of different bits and through the two zeros."""
    L, R = _inputs(cls, nullable, size, op)
    lrows, rrows = _rows(L, identity), (_rows(R, identity) if R is not None else [])
    raw = lambda b, w: b
    lraw, rraw = _rows(L, raw), (_rows(R, raw) if R is not None else [])
    want = oracle(op, lrows, rrows)
    members = {}
    for k, r in zip(lrows + rrows, lraw + rraw):
        members.setdefault(k, set()).add(r)
    w = L["x"].type.bit_width // 8
    F = fspecials(w)
    nan_bits = {k: {b for b, _ in v} for k, v in members.items() if k[0] == "nan"}
    assert any(len(v) > 1 for v in nan_bits.values()) and {(F["pzero"], 0), (F["nzero"], 0)} <= members[((0, 0), 0)]
    assert (L["x"].null_count > 0) == nullable and len(want) < L.num_rows / 2
    by_bits = oracle(op, lraw, rraw)
    decided = lambda rows, keep: [r for r in rows if keep(r[0])]
    isnan, iszero = (lambda b: b is not None and identity(b, w) == "nan"), (lambda b: b in (F["pzero"], F["nzero"]))
    for kind, keep_b, keep_k in (("NaN", isnan, lambda k: k == "nan"), ("zero", iszero, lambda k: k == (0, 0))):
        as_identities = [(identity(b, w), i) for b, i in decided(by_bits, keep_b)]
        assert as_identities != decided(want, keep_k), f"{op}: bit equality gives the same {kind} rows"
    return want, members


def check(res, cls, nullable, size, op, what, ordered=True):
    L, _ = dataset(cls, nullable, size)
    want, members = expected(cls, nullable, size, op)
    assert res.column_names == L.column_names and res.schema.types == L.schema.types, f"{what}: {res.schema}"
    w = L["x"].type.bit_width // 8
    got_raw = list(zip(column_bits(res["x"]), res["i"].to_pylist()))
    got = [(identity(b, w), i) for b, i in got_raw]
    key = lambda k: (k[0] is None, str(k[0]), k[1])
    if not ordered:
        order = sorted(range(len(got)), key=lambda j: key(got[j]))
        got, got_raw, want = [got[j] for j in order], [got_raw[j] for j in order], sorted(want, key=key)
    differ = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{what}: {len(got)} rows, oracle {len(want)}; first difference at row {differ}"
    bad = [(k, r) for k, r in zip(got, got_raw) if r not in members[k]]
    assert not bad, f"{what}: rows that are no input row of their identity: {bad[:6]}"


def _run(ctx, cls, nullable, size, op, distributed=False, tables=None):
    L, R = tables or _inputs(cls, nullable, size, op)
    TL = Table(L, ctx)
    if op.startswith("unique"):
        fn = TL.distributed_unique if distributed else TL.unique
        return traced(lambda: fn(["x", "i"], keep=op.split("_")[1]).to_arrow())
    fn = getattr(TL, ("distributed_" if distributed else "") + op)
    return traced(lambda: fn(Table(R, ctx)).to_arrow())


# ---- CPU context
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls,nullable", CASES, ids=_ids)
def test_cpu_set_operation_matches_oracle(ctx, cls, nullable, op):
    expected(cls, nullable, "cpu", op)
    got, _ = _run(ctx, cls, nullable, "cpu", op)
    check(got, cls, nullable, "cpu", op, f"cpu {op} {cls}")


def _deal(rows_l, rows_r, rank, world):
    """row j of an identity's rows (left's, then right's, in table order) lives on rank j mod world"""
    seen, mine = {}, ([], [])
    for side, rows in enumerate((rows_l, rows_r)):
        for i, k in enumerate(rows):
            j = seen.get(k, 0)
            seen[k] = j + 1
            if j % world == rank:
                mine[side].append(i)
    return mine


def _dist_worker(ctx, cases, chunks, forced):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    ctx.add_config("shuffle_chunks", str(chunks))
    out = {}
    for cls, nullable in cases:
        L, R = dataset(cls, nullable)
        lrows, rrows = _deal(_rows(L, identity), _rows(R, identity), rank, world)
        mine = (L.take(pa.array(lrows, type=pa.int64())), R.take(pa.array(rrows, type=pa.int64())))
        for op in OPS:
            out[(cls, nullable, op)] = _run(ctx, cls, nullable, "cpu", op, distributed=True, tables=mine)[0]
    return out


_spawned = {}


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls,nullable", CASES, ids=_ids)
def test_cpu_distributed_set_operation_matches_oracle(cls, nullable, op):
    """2 ranks over gloo, 2 chunks: the equal patterns of one row start on different ranks"""
    expected(cls, nullable, "cpu", op)
    res = spawn_once(_spawned, _dist_worker, CASES, 2, "cpu", 2)
    got = pa.concat_tables([r[(cls, nullable, op)] for r in res])
    check(got, cls, nullable, "cpu", op, f"cpu 2 ranks {op} {cls}", ordered=False)


# ---- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls,nullable", CASES, ids=_ids)
def test_gpu_small_path_matches_oracle(gpu_ctx, cls, nullable, op):
    """GroupIds on the device: the row hash and rows_equal of the join (hash_join.hip)"""
    expected(cls, nullable, "cpu", op)
    got, cnt = _run(gpu_ctx, cls, nullable, "cpu", op)
    assert not any(k.startswith("setop.radix") for k in cnt), cnt
    check(got, cls, nullable, "cpu", op, f"gpu small {op} {cls}")


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("cls,nullable", CASES, ids=_ids)
def test_gpu_radix_path_matches_oracle(gpu_ctx, monkeypatch, cls, nullable, op):
    """kernels/radix_setops.hip: its own value hash and equality of NaN, the zeros and float16"""
    monkeypatch.setenv("CYLON_RADIX_SETOP_MIN_ROWS", "1")
    expected(cls, nullable, "gpu", op)
    got, cnt = _run(gpu_ctx, cls, nullable, "gpu", op)
    assert cnt.get("setop.radix.exceptions", 0) > 0, cnt  # the radix path answered (and found duplicates)
    assert cnt.get("setop.radix.fallback", 0) == 0 and cnt.get("setop.radix.order_violation_fallback", 0) == 0, cnt
    check(got, cls, nullable, "gpu", op, f"gpu radix {op} {cls}")
