"""Joins on float keys (NaN of either sign and any payload, -0.0, +0.0, nulls) on every path against an
oracle on bit patterns.

Every path -- C.join_indices (join_impl: the exact single key, the row hash + rows_equal, the sort
algorithm), Table.join, the CPU twin of the semi / anti kernel, the semi / anti general path,
distributed_join over gloo at 2 and 4 ranks (the chunked exchange included), and on the GPU the
device join_impl path, the LDS radix hash join on the exact key image and on the verified hashed key,
the LDS key-set semi / anti kernel and 2 ranks on one device -- is compared with the oracle below;
never with another path of the project, and never with pandas or numpy.

The contract (docs/semantics.md, "Float join keys").  Two non-null key cells are equal iff their
order images are: -0.0 == +0.0, every NaN equals every NaN whatever its sign bit or payload; null
equals null; float32 never joins float64 (Code::TypeError).  A join computes nothing: every output
cell, key columns included, is a bit-for-bit copy of the cell of the input row it came from (the
left key column keeps the left row's -0.0 or NaN payload, the right one the right row's).  Semi /
anti are defined by the inner join's left row numbers.

Oracle.  Plain Python on the raw bits of the Arrow buffers: a cell's identity is None for null, one
token for any NaN, else (sign, magnitude) with the two zeros folded -- written from the contract,
sharing nothing with kernels/order_image.hpp.  Every table carries a unique int64 row-id column;
the expected result is the multiset of (left id, right id) pairs from a dict of identity tuples
(outer types add (id, None) / (None, id)), for semi / anti the left ids in left order.  Through the
ids every output cell is compared with its input cell's bits, null masks, names and types exactly.
There are no tolerances in this file.

Each case first asserts on its own inputs that a pass means something: the oracle's result differs
from a bit-equality join of the same inputs through a NaN pair of different bits and through a +-0
pair (the right side lacks some of the NaN patterns and one of the zeros, the left side holds all),
NaN-keyed left rows without any NaN on the right are anti rows (shape one_null_rwithout), null keys
sit on both sides of the semi / anti split, and at most 200 000 pairs are expected.

Class x path pairs that are not on the path named (the counters show where they went; they are not
counted as coverage of that path, and nothing forces them onto it):

    shapes one_null, ff_null (a nullable float key)    LDS radix join (radix_keys packs nullable keys only
                                                       as integer composites): device join_impl
    shape one, INNER, algorithm sort                   LDS radix join (a one-key inner sort join of float
                                                       keys is join_impl's sort join; never the sorted-merge
                                                       or range join, which are for integer keys)
    shapes one_null, fi, ff_null, one_null_rwithout    LDS key-set semi / anti kernel and its CPU twin (one
                                                       simple key or an integer composite): general path
    shape fi on 2 ranks with 2 chunks                  LDS radix join (a hashed key does not write into
                                                       the chunked join's sink): device join_impl

Every other shape (one non-null float key; one nullable float key; (float, int32); (float, float
nullable)) x float64 / float32 / float16 x six join types x hash / sort runs on every path listed."""
import collections
import functools
import os
import struct

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C

from oracle_utils import FLOAT_FIELDS, column_bits, fspecials, make_array, spawn_once, traced
from semi_join_utils import max_distinct_per_partition, semi_partition_bits

NAN = "nan"
_FLOAT_FMT = {2: "<e", 4: "<f", 8: "<d"}


# ---- the oracle (shares nothing with the project)
def identity(bits, w):
    """what a float key cell is for the join: None (null), NAN, or (sign, magnitude) with one zero"""
    if bits is None:
        return None
    e, m = FLOAT_FIELDS[w]
    assert 0 <= bits < 1 << 8 * w
    exponent, mantissa, negative = (bits >> m) & ((1 << e) - 1), bits & ((1 << m) - 1), bits >> (8 * w - 1)
    if exponent == (1 << e) - 1 and mantissa:
        return NAN
    magnitude = (exponent << m) | mantissa
    return (0, 0) if magnitude == 0 else (negative, magnitude)


def oracle_pairs(lkeys, rkeys, how):
    """(left row, right row) of every match, left-major; None for the absent side of an outer row.
    lkeys / rkeys: one identity tuple per row."""
    index = {}
    for j, k in enumerate(rkeys):
        index.setdefault(k, []).append(j)
    pairs = []
    for i, k in enumerate(lkeys):
        js = index.get(k, ())
        pairs += [(i, j) for j in js]
        if not js and how in ("left", "outer"):
            pairs.append((i, None))
    if how in ("right", "outer"):
        present = set(lkeys)
        pairs += [(None, j) for j, k in enumerate(rkeys) if k not in present]
    return pairs


def oracle_semi(lkeys, rkeys, how):
    present = set(rkeys)
    return [i for i, k in enumerate(lkeys) if (k in present) == (how == "semi")]


def fbits(x, w):
    return int.from_bytes(struct.pack(_FLOAT_FMT[w], x), "little")


def decode(bits, w):
    return struct.unpack(_FLOAT_FMT[w], bits.to_bytes(w, "little"))[0]


def test_oracle_hand_table():
    qnan, nqnan, snan, nzero = 0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 1 << 63
    F = fspecials(8)
    assert (F["pnan"], F["nnan"], F["psnan"], F["nzero"]) == (qnan, nqnan, snan, nzero)
    ident = lambda bits, w: [(identity(b, w),) for b in bits]
    left, right = ident([qnan, nqnan, snan, 0, nzero], 8), ident([nqnan, qnan, nzero], 8)
    eight = [(i, j) for i in (0, 1, 2) for j in (0, 1)] + [(3, 2), (4, 2)]
    assert oracle_pairs(left, right, "inner") == eight
    assert oracle_pairs(left, right, "outer") == eight  # every row of both sides has a partner
    assert oracle_semi(left, right, "semi") == [0, 1, 2, 3, 4] and oracle_semi(left, right, "anti") == []
    left, right = ident([0x7e00, 0xfe00, 0x7c01, 0, 0x8000], 2), ident([0xfe00, 0x8000], 2)
    assert oracle_pairs(left, right, "inner") == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)]
    assert oracle_semi(left, right, "semi") == [0, 1, 2, 3, 4] and oracle_semi(left, right, "anti") == []
    # the two-column form of the probe: (k, g) with one g throughout
    left2 = [k + (7,) for k in ident([qnan, nqnan, snan, 0, nzero], 8)]
    right2 = [k + (7,) for k in ident([nqnan, qnan, nzero], 8)]
    assert oracle_pairs(left2, right2, "inner") == eight and oracle_semi(left2, right2, "anti") == []
    # infinities, denormals and the largest numbers are themselves; NaN is not infinity; null is null
    left = ident([F["pinf"], F["ninf"], F["pden"], F["nden"], F["pmax"], None, F["nsnan"]], 8)
    right = ident([F["nden"], None, F["pinf"], F["nmax"], None], 8)
    assert oracle_pairs(left, right, "inner") == [(0, 2), (3, 0), (5, 1), (5, 4)]
    assert oracle_pairs(left, right, "left") == [(0, 2), (1, None), (2, None), (3, 0), (4, None), (5, 1), (5, 4), (6, None)]
    assert oracle_pairs(left, right, "right") == [(0, 2), (3, 0), (5, 1), (5, 4), (None, 3)]
    assert oracle_pairs(left, right, "outer") == oracle_pairs(left, right, "left") + [(None, 3)]
    assert oracle_semi(left, right, "semi") == [0, 3, 5] and oracle_semi(left, right, "anti") == [1, 2, 4, 6]
    # a null in one column of two: the tuple matches only a tuple with the null in the same place
    assert oracle_pairs([(NAN, None), (None, NAN), ((0, 0), None)], [(NAN, None), ((0, 0), 3)], "outer") == \
        [(0, 0), (1, None), (2, None), (None, 1)]
    assert identity(0x3c00, 2) == (0, 0x3c00) and identity(0xbc00, 2) == (1, 0x3c00) and identity(0x7c00, 2) == (0, 0x7c00)
    assert identity(0xffc00000, 4) == NAN and identity(0x7f800001, 4) == NAN and identity(0xff800000, 4) == (1, 0x7f800000)


def test_oracle_on_plain_data_is_a_join_on_python_floats():
    rng = np.random.default_rng(7)
    for w in (2, 4, 8):
        e, m = FLOAT_FIELDS[w]
        pool = []
        while len(pool) < 30:  # free of NaN and of both zeros (and there are no nulls)
            b = int.from_bytes(rng.bytes(w), "little")
            if (b >> m) & ((1 << e) - 1) != (1 << e) - 1 and b & ((1 << (8 * w - 1)) - 1):
                pool.append(b)
        pool += [fspecials(w)[s] for s in ("pinf", "ninf", "pden", "nden", "pmax", "nmax")]
        lb, rb = [pool[i] for i in rng.integers(0, 30, 80)], [pool[i] for i in rng.integers(6, 36, 60)]
        lf, rf = [decode(b, w) for b in lb], [decode(b, w) for b in rb]
        for how in ("inner", "left", "right", "outer"):
            want = [(i, j) for i, x in enumerate(lf) for j, y in enumerate(rf) if x == y]
            if how in ("left", "outer"):
                want += [(i, None) for i, x in enumerate(lf) if x not in rf]
            if how in ("right", "outer"):
                want += [(None, j) for j, y in enumerate(rf) if y not in lf]
            got = oracle_pairs([(identity(b, w),) for b in lb], [(identity(b, w),) for b in rb], how)
            assert sorted(got, key=_pair_key) == sorted(want, key=_pair_key) and len(want) > 60, (w, how)
        assert oracle_semi([(identity(b, w),) for b in lb], [(identity(b, w),) for b in rb], "semi") == \
            [i for i, x in enumerate(lf) if x in rf]


def _pair_key(p):
    return tuple((x is None, x or 0) for x in p)


# ---- data
CLASSES = {"float64": pa.float64(), "float32": pa.float32(), "float16": pa.float16()}
SHAPES = ("one", "one_null", "fi", "ff_null")
SEMI_SHAPES = SHAPES + ("one_null_rwithout",)
SIZES = {"cpu": (300, 200, 40), "gpu": (3000, 2000, 300), "dist": (10_000, 6_000, 600)}  # left, right rows, random keys
HOWS = ("inner", "left", "right", "outer", "semi", "anti")
ALGORITHMS = ("hash", "sort")
LID0, RID0 = 10_000, 50_000
# the NaN patterns and the zero that the right side of each class does not hold (the left holds all)
_RIGHT_LACKS = {"float64": ("pnan", "nsnan", "pzero"), "float32": ("nnan", "psnan", "nzero"),
                "float16": ("nnan", "nsnan", "pzero")}
_NANS = ("pnan", "nnan", "psnan", "nsnan")
_G = (-(1 << 31), 0, 7, (1 << 31) - 1)  # the int32 second key: the right side never holds the last value

Data = collections.namedtuple("Data", "left right keys w lid rid lraw rraw lbits rbits")


def _key_rows(t, keys, ident):
    cols = []
    for k in keys:
        c = t[k]
        if pa.types.is_floating(c.type):
            w = c.type.bit_width // 8
            cols.append([ident(b, w) for b in column_bits(c)])
        else:
            cols.append(c.to_pylist())
    return list(zip(*cols))


@functools.lru_cache(maxsize=None)
def dataset(shape, cls, size="cpu"):
    """Left (k[, g | h], id, p) and right (id, q[, g | h], k) tables; fixed seed.  k is drawn with
    replacement from the class's pool: the twelve special patterns, +-1.0 and random finite
    patterns, some of them on one side only."""
    typ = CLASSES[cls]
    w = typ.bit_width // 8
    e, m = FLOAT_FIELDS[w]
    rng = np.random.default_rng([23, SEMI_SHAPES.index(shape), list(CLASSES).index(cls), list(SIZES).index(size)])
    nl, nr, nrand = SIZES[size]
    F = fspecials(w)
    special = list(F.values()) + [fbits(1.0, w), fbits(-1.0, w)]
    rand = []
    while len(rand) < nrand:
        b = int.from_bytes(rng.bytes(w), "little")
        if (b >> m) & ((1 << e) - 1) != (1 << e) - 1 and b not in special and b not in rand:
            rand.append(b)
    nside = max(3, nrand // 8)
    lonly, ronly = rand[:nside], rand[nside:2 * nside]
    lacks = [F[s] for s in _RIGHT_LACKS[cls]] + ([F[s] for s in _NANS] if shape.endswith("rwithout") else [])
    lpool = [b for b in special + rand if b not in ronly]
    rpool = [b for b in special + rand if b not in lonly and b not in lacks]
    draw = lambda pool, n: [pool[i] for i in rng.integers(0, len(pool), n)]
    lk, rk = draw(lpool, nl), draw(rpool, nr)
    lhead, rhead = special, [b for b in reversed(special) if b not in lacks]
    lk[:len(lhead)], rk[:len(rhead)] = lhead, rhead  # every pattern a side may hold, it holds
    second_l = second_r = None
    if shape == "fi":
        second_l = ("g", [0] * len(lhead) + [_G[i] for i in rng.integers(0, 4, nl - len(lhead))], pa.int32(), False)
        second_r = ("g", [0] * len(rhead) + [_G[i] for i in rng.integers(0, 3, nr - len(rhead))], pa.int32(), False)
    if shape == "ff_null":
        hpool = [fbits(1.0, w), F["pzero"], F["nzero"], F["pnan"], F["nnan"], None, fbits(2.0, w)]  # 2.0: left only
        second_l = ("h", [hpool[0]] * len(lhead) + [hpool[i] for i in rng.integers(0, 7, nl - len(lhead))], typ, True)
        second_r = ("h", [hpool[0]] * len(rhead) + [hpool[i] for i in rng.integers(0, 6, nr - len(rhead))], typ, True)
    knull = shape.startswith("one_null")
    if knull:
        for i in np.flatnonzero(rng.random(nl) < 0.08):
            if i >= len(lhead):
                lk[i] = None
        if not shape.endswith("rwithout"):
            for j in np.flatnonzero(rng.random(nr) < 0.08):
                if j >= len(rhead):
                    rk[j] = None
    lperm, rperm = rng.permutation(nl), rng.permutation(nr)
    place = lambda rows, perm: [rows[i] for i in perm]
    pnull = rng.random(nl) < 0.15
    p = [None if pnull[i] else b for i, b in enumerate(draw(special + rand, nl))]
    lcols = {"k": make_array(place(lk, lperm), typ, knull)}
    rcols = {"id": pa.array(np.arange(RID0, RID0 + nr), pa.int64()), "q": make_array(draw(special + rand, nr), typ, False)}
    keys = ["k"]
    if second_l:
        name, rows, styp, snull = second_l
        as_bits = lambda vals: [None if v is None else v & ((1 << styp.bit_width) - 1) for v in vals]
        lcols[name] = make_array(as_bits(place(rows, lperm)), styp, snull)
        rcols[name] = make_array(as_bits(place(second_r[1], rperm)), styp, snull)
        keys.append(name)
    lcols["id"] = pa.array(np.arange(LID0, LID0 + nl), pa.int64())
    lcols["p"] = make_array(p, typ, True)
    rcols["k"] = make_array(place(rk, rperm), typ, knull)
    left, right = pa.table(lcols), pa.table(rcols)
    raw = lambda b, w_: b
    return Data(left, right, tuple(keys), w, _key_rows(left, keys, identity), _key_rows(right, keys, identity),
                _key_rows(left, keys, raw), _key_rows(right, keys, raw),
                {n: column_bits(left[n]) for n in left.column_names}, {n: column_bits(right[n]) for n in right.column_names})


@functools.lru_cache(maxsize=None)
def expected(shape, cls, size, how):
    ds = dataset(shape, cls, size)
    return oracle_semi(ds.lid, ds.rid, how) if how in ("semi", "anti") else oracle_pairs(ds.lid, ds.rid, how)


@functools.lru_cache(maxsize=None)
def conditions(shape, cls, size="cpu"):
    """What makes a pass of this data set mean something (asserted before every join of it)."""
    ds = dataset(shape, cls, size)
    F = fspecials(ds.w)
    lk, rk = ds.lbits["k"], ds.rbits["k"]
    nan = lambda b: b is not None and identity(b, ds.w) == NAN
    assert {F[s] for s in F} <= set(lk) and (ds.left["k"].null_count > 0) == shape.startswith("one_null")
    assert set(lk) - set(rk) - set(F.values()) - {None} and set(rk) - set(lk)  # values on one side only
    want, by_bits = expected(shape, cls, size, "inner"), oracle_pairs(ds.lraw, ds.rraw, "inner")
    assert len(expected(shape, cls, size, "outer")) <= 200_000
    assert len(collections.Counter(lk)) < len(lk) / 2 and len(collections.Counter(rk)) < len(rk) / 2  # keys repeat
    null_rows = [i for i, k in enumerate(ds.lid) if None in k]
    semi = set(expected(shape, cls, size, "semi"))
    if shape.endswith("rwithout"):  # NaN-keyed (and null-keyed) left rows whose right side has no NaN (no null)
        assert not any(nan(b) for b in rk) and ds.right["k"].null_count == 0
        nan_rows = [i for i, b in enumerate(lk) if nan(b)]
        assert len({lk[i] for i in nan_rows}) == 4 and not semi & set(nan_rows) and null_rows and not semi & set(null_rows)
        assert semi
        return
    extra = set(want) - set(by_bits)
    assert set(by_bits) <= set(want)
    assert any(nan(lk[i]) and nan(rk[j]) and lk[i] != rk[j] for i, j in extra), "no NaN pair of different bits"
    assert any({lk[i], rk[j]} == {F["pzero"], F["nzero"]} for i, j in extra), "no pair of the two zeros"
    by_bits_semi = set(oracle_semi(ds.lraw, ds.rraw, "semi"))
    assert any(nan(lk[i]) for i in semi - by_bits_semi) and any(lk[i] in (F["pzero"], F["nzero"]) for i in semi - by_bits_semi)
    assert 0 < len(semi) < ds.left.num_rows
    if shape == "one_null":
        assert null_rows and set(null_rows) <= semi  # (their anti side: shape one_null_rwithout)
    if shape == "ff_null":  # nulls on both sides of the semi / anti split
        assert semi & set(null_rows) and set(null_rows) - semi
    if shape == "fi":  # a NaN-keyed left row whose (NaN, g) has no partner
        assert any(nan(lk[i]) for i in set(range(len(lk))) - semi)


# ---- comparing a result with the oracle
def _hex(b):
    return b if b is None else hex(b)


def check_pairs(li, ri, shape, cls, size, how, what):
    """row-number tensors of C.join_indices (-1: the absent side)"""
    li, ri = li.cpu().tolist(), ri.cpu().tolist()
    want = expected(shape, cls, size, how)
    if how in ("semi", "anti"):
        assert li == want, f"{what}: {len(li)} rows, oracle {len(want)}: {sorted(set(li) ^ set(want))[:8]} differ"
        assert ri == [-1] * len(li)
        return
    got = [(None if i < 0 else i, None if j < 0 else j) for i, j in zip(li, ri)]
    _same_pairs(got, want, what)


def _same_pairs(got, want, what):
    g, w = collections.Counter(got), collections.Counter(want)
    assert g == w, f"{what}: {len(got)} pairs, oracle {len(want)}; missing {sorted((w - g).elements(), key=_pair_key)[:6]}, " \
                   f"not due {sorted((g - w).elements(), key=_pair_key)[:6]}"
    assert sorted(got, key=_pair_key) == sorted(want, key=_pair_key)


def check_table(res, shape, cls, size, how, what, ordered):
    """Names, types, the pairs (for semi / anti the left ids, in left order when `ordered`), and through
    the row ids every cell of every column against the bits of its input cell (None: null)."""
    ds = dataset(shape, cls, size)
    semi = how in ("semi", "anti")
    sides = [("l_", ds.left, ds.lbits, LID0)] + ([] if semi else [("r_", ds.right, ds.rbits, RID0)])
    assert res.column_names == [p + n for p, t, _, _ in sides for n in t.column_names], f"{what}: {res.column_names}"
    assert res.schema.types == [ty for _, t, _, _ in sides for ty in t.schema.types], f"{what}: {res.schema.types}"
    got = {n: column_bits(res[n]) for n in res.column_names}
    want = expected(shape, cls, size, how)
    rows = [[None if v is None else v - id0 for v in got[p + "id"]] for p, _, _, id0 in sides]
    if semi:
        wanted, came = (want, rows[0]) if ordered else (sorted(want), sorted(rows[0]))
        assert came == wanted, f"{what}: {len(came)} rows, oracle {len(want)}: {sorted(set(came) ^ set(want))[:8]} differ"
    else:
        _same_pairs(list(zip(*rows)), want, what)
    bad = []
    for (p, t, bits, _), side_rows in zip(sides, rows):
        for n in t.column_names:
            src, out = bits[n], got[p + n]
            bad += [(p + n, r, _hex(out[o]), _hex(None if r is None else src[r]))
                    for o, r in enumerate(side_rows) if out[o] != (None if r is None else src[r])][:4]
    assert not bad, f"{what}: cells that are no copy of their input cell (column, input row, got, input): {bad[:8]}"


_CASES = [(s, c) for s in SHAPES for c in CLASSES]
_SEMI_CASES = [(s, c) for s in SEMI_SHAPES for c in CLASSES]  # (one_null_rwithout: a semi / anti data set)
_case_ids = lambda cases: [f"{s}-{c}" for s, c in cases]
_ALL_HOWS = [pytest.param(s, c, h, id=f"{s}-{c}-{h}") for s, c in _SEMI_CASES for h in HOWS
             if h in ("semi", "anti") or not s.endswith("rwithout")]
_KW = dict(left_prefix="l_", right_prefix="r_")


def _join(ctx, shape, cls, size, how, algorithm):
    ds = dataset(shape, cls, size)
    L, R = Table(ds.left, ctx), Table(ds.right, ctx)
    got, cnt = traced(lambda: L.join(R, how, algorithm, left_on=list(ds.keys), right_on=list(ds.keys), **_KW))
    return got.to_arrow(), cnt


def test_float32_key_against_float64_key_is_a_type_error(ctx):
    a, b = dataset("one", "float32"), dataset("one", "float64")
    for how in HOWS:
        with pytest.raises(Exception, match="join key types differ"):
            Table(a.left, ctx).join(Table(b.right, ctx), how, "hash", left_on=["k"], right_on=["k"])


# ---- CPU context
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape,cls,how", _ALL_HOWS)
def test_cpu_join_indices_match_oracle(ctx, shape, cls, how, algorithm):
    """join_impl: the exact key image (shape one), the row hash + rows_equal (the others), hash and sort"""
    conditions(shape, cls)
    ds = dataset(shape, cls)
    L, R = Table(ds.left, ctx), Table(ds.right, ctx)
    lc, rc = [ds.left.column_names.index(k) for k in ds.keys], [ds.right.column_names.index(k) for k in ds.keys]
    li, ri = C.join_indices(L.native, R.native, how, algorithm, lc, rc)
    check_pairs(li, ri, shape, cls, "cpu", how, f"cpu join_indices {how}/{algorithm} {shape}/{cls}")


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("how", HOWS[:4])
@pytest.mark.parametrize("shape,cls", _CASES, ids=_case_ids(_CASES))
def test_cpu_table_join_matches_oracle(ctx, shape, cls, how, algorithm):
    conditions(shape, cls)
    got, _ = _join(ctx, shape, cls, "cpu", how, algorithm)
    check_table(got, shape, cls, "cpu", how, f"cpu join {how}/{algorithm} {shape}/{cls}", ordered=False)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("how", ("semi", "anti"))
@pytest.mark.parametrize("cls", CLASSES)
def test_cpu_semi_anti_twin_kernel_matches_oracle(ctx, cls, how, algorithm):
    """kernels/cpu_semi.cpp on the exact image of one simple key"""
    conditions("one", cls)
    got, cnt = _join(ctx, "one", cls, "cpu", how, algorithm)
    assert "join.semi.general" not in cnt and cnt.get("join.semi.matched") == len(expected("one", cls, "cpu", "semi")), cnt
    check_table(got, "one", cls, "cpu", how, f"cpu twin {how}/{algorithm} {cls}", ordered=True)


_GENERAL = [c for c in _SEMI_CASES if c[0] != "one"]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("how", ("semi", "anti"))
@pytest.mark.parametrize("shape,cls", _GENERAL, ids=_case_ids(_GENERAL))
def test_cpu_semi_anti_general_path_matches_oracle(ctx, shape, cls, how, algorithm):
    """Unique(Project(right, keys)) + the inner join: the two must agree on what a key is"""
    conditions(shape, cls)
    got, cnt = _join(ctx, shape, cls, "cpu", how, algorithm)
    assert cnt.get("join.semi.general") == 1, cnt
    check_table(got, shape, cls, "cpu", how, f"cpu general {how}/{algorithm} {shape}/{cls}", ordered=True)


# ---- distributed: rows dealt so that the rows of one key -- its NaN patterns, its two zeros -- start on
# different ranks
def _deal(ds, rank, world):
    """Row numbers of this rank's share of (left, right): row j of a key's rows (left's, then right's,
    in table order) lives on rank j mod world."""
    seen, mine = {}, ([], [])
    for side, keys in enumerate((ds.lid, ds.rid)):
        for i, k in enumerate(keys):
            j = seen.get(k, 0)
            seen[k] = j + 1
            if j % world == rank:
                mine[side].append(i)
    return mine


def _dist_worker(ctx, cases, chunks, forced):
    rank, world = ctx.get_rank(), ctx.get_world_size()
    ctx.add_config("shuffle_chunks", str(chunks))
    if ctx.on_gpu:
        os.environ["CYLON_RADIX_JOIN_MIN_ROWS"] = "1024"
    out = {}
    for shape, cls, size, hows, algorithms in cases:
        ds = dataset(shape, cls, size)
        lrows, rrows = _deal(ds, rank, world)
        L = Table(ds.left.take(pa.array(lrows, type=pa.int64())), ctx)
        R = Table(ds.right.take(pa.array(rrows, type=pa.int64())), ctx)
        assert L.device == ctx.device
        for how in hows:
            for algorithm in algorithms:
                got, cnt = traced(lambda: L.distributed_join(R, how, algorithm, left_on=list(ds.keys),
                                                             right_on=list(ds.keys), **_KW))
                out[(shape, cls, how, algorithm)] = (got.to_arrow(), cnt)
    return out


DIST_CPU = [(s, c, "cpu", HOWS if not s.endswith("rwithout") else HOWS[4:], ALGORITHMS) for s, c in _SEMI_CASES]
DIST_GPU = [(s, c, "dist", HOWS, ("hash",)) for s in ("one", "fi") for c in CLASSES]
_spawned = {}


def _dist(cases, world, device, chunks):
    return spawn_once(_spawned, _dist_worker, cases, world, device, chunks)


def _dist_params(cases):
    return [pytest.param(s, c, h, a, id=f"{s}-{c}-{h}-{a}") for s, c, _, hows, algs in cases for h in hows for a in algs]


def test_dealing_splits_the_patterns_of_a_key():
    for world in (2, 4):
        for shape, cls in _CASES:
            ds = dataset(shape, cls)
            F = fspecials(ds.w)
            where = {}  # bit pattern of k -> ranks that start with a row of it
            for rank in range(world):
                lrows, rrows = _deal(ds, rank, world)
                for b in [ds.lbits["k"][i] for i in lrows] + [ds.rbits["k"][j] for j in rrows]:
                    where.setdefault(b, set()).add(rank)
            apart = lambda a, b: any(x != y for x in where[F[a]] for y in where[F[b]])
            assert all(apart(a, b) for a in _NANS for b in _NANS if a != b) and apart("pzero", "nzero"), (world, shape, cls)
            assert set.union(*[where[F[s]] for s in _NANS]) == set(range(world)) == where[F["pzero"]] | where[F["nzero"]]


@pytest.mark.parametrize("world,chunks", [(2, 1), (4, 3)], ids=["2ranks", "4ranks_chunked"])
@pytest.mark.parametrize("shape,cls,how,algorithm", _dist_params(DIST_CPU))
def test_cpu_distributed_join_matches_oracle(world, chunks, shape, cls, how, algorithm):
    conditions(shape, cls)
    res = _dist(DIST_CPU, world, "cpu", chunks)
    got = pa.concat_tables([r[(shape, cls, how, algorithm)][0] for r in res])
    check_table(got, shape, cls, "cpu", how, f"cpu {world} ranks {how}/{algorithm} {shape}/{cls}", ordered=False)


# ---- GPU
def _radix_declines(shape, how, algorithm):
    """local joins that the LDS radix hash join does not take (module docstring)"""
    return shape in ("one_null", "ff_null") or (shape == "one" and how == "inner" and algorithm == "sort")


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape,cls,how", _ALL_HOWS)
def test_gpu_join_impl_path_matches_oracle(gpu_ctx, monkeypatch, shape, cls, how, algorithm):
    """the device join_impl: k_key64 / k_row_hash64 / k_rows_equal, the global-table hash join and the
    sort join; semi / anti on the general path"""
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", str(1 << 62))
    conditions(shape, cls)
    got, cnt = _join(gpu_ctx, shape, cls, "cpu", how, algorithm)
    assert "join.radix.rows_out" not in cnt and "join.semi.radix" not in cnt, cnt
    if how in ("semi", "anti"):
        assert cnt.get("join.semi.general") == 1, cnt
    check_table(got, shape, cls, "cpu", how, f"gpu join_impl {how}/{algorithm} {shape}/{cls}", ordered=True)


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("how", HOWS[:4])
@pytest.mark.parametrize("shape,cls", _CASES, ids=_case_ids(_CASES))
def test_gpu_radix_join_matches_oracle(gpu_ctx, monkeypatch, shape, cls, how, algorithm):
    """kernels/radix_join.hip behind radix_join_any: one float key is the exact key image, (float, int32)
    the hashed key whose matches are verified on the output.  A float key never takes the sorted-merge
    or the range join."""
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1024")
    conditions(shape, cls, "gpu")
    got, cnt = _join(gpu_ctx, shape, cls, "gpu", how, algorithm)
    print(shape, cls, how, algorithm, cnt)
    assert "join.sortmerge.rows_out" not in cnt and "join.range.rows_out" not in cnt, cnt
    if _radix_declines(shape, how, algorithm):
        assert "join.radix.rows_out" not in cnt, cnt
    else:
        assert cnt.get("join.radix.rows_out") == len(expected(shape, cls, "gpu", how)), cnt
        assert ("join.radix.hashed_key" in cnt) == (shape == "fi"), cnt
        assert cnt.get("join.radix.overflow_fallback", 0) == 0 and "join.radix.hash_collision_fallback" not in cnt, cnt
    check_table(got, shape, cls, "gpu", how, f"gpu radix {how}/{algorithm} {shape}/{cls}", ordered=False)


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("how", ("semi", "anti"))
@pytest.mark.parametrize("shape,cls", _SEMI_CASES, ids=_case_ids(_SEMI_CASES))
def test_gpu_semi_anti_matches_oracle(gpu_ctx, monkeypatch, shape, cls, how, algorithm):
    """kernels/semi_join.hip k_sj_build / k_sj_probe on the exact image of one float key: both zeros are
    the image 0, the LDS set's empty-slot value, and sit on both sides.  The other shapes take the
    general path on the device."""
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1024")
    conditions(shape, cls, "gpu")
    ds = dataset(shape, cls, "gpu")
    if shape == "one":
        F = fspecials(ds.w)
        assert {F["pzero"], F["nzero"]} <= set(ds.lbits["k"]) and {F["pzero"], F["nzero"]} & set(ds.rbits["k"])
        bits = semi_partition_bits(ds.right.num_rows)
        assert max_distinct_per_partition(np.array(ds.rbits["k"], np.uint64).view(np.int64), bits) <= 4096  # kSJCap
    got, cnt = _join(gpu_ctx, shape, cls, "gpu", how, algorithm)
    print(shape, cls, how, algorithm, cnt)
    if shape == "one":
        assert cnt.get("join.semi.radix") == 1 and cnt.get("join.semi.overflow_fallback", 0) == 0, cnt
        assert "join.semi.general" not in cnt and cnt.get("join.semi.matched") == len(expected(shape, cls, "gpu", "semi")), cnt
    else:
        assert "join.semi.radix" not in cnt and cnt.get("join.semi.general") == 1, cnt
    check_table(got, shape, cls, "gpu", how, f"gpu semi kernel {how}/{algorithm} {shape}/{cls}", ordered=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls,how,algorithm", _dist_params(DIST_GPU))
def test_gpu_two_ranks_match_oracle(shape, cls, how, algorithm):
    """2 ranks share cuda:0, the collectives go over gloo, 2 chunks: the radix join writes the shuffled
    chunks of the exact float key into its sink; the key-set kernel marks the semi / anti rows."""
    conditions(shape, cls, "dist")
    res = _dist(DIST_GPU, 2, "cuda:0", 2)
    got = pa.concat_tables([r[(shape, cls, how, algorithm)][0] for r in res])
    for r in res:
        cnt = r[(shape, cls, how, algorithm)][1]
        print(shape, cls, how, algorithm, cnt)
        assert cnt.get("shuffle.chunks", 0) > 0, cnt
        if shape == "one":
            assert cnt.get("join.semi.radix" if how in ("semi", "anti") else "join.radix.rows_out", 0) > 0, cnt
            assert "join.semi.general" not in cnt and cnt.get("join.radix.overflow_fallback", 0) == 0, cnt
        else:
            assert "join.radix.rows_out" not in cnt and "join.semi.radix" not in cnt, cnt
    check_table(got, shape, cls, "dist", how, f"gpu 2 ranks {how}/{algorithm} {shape}/{cls}", ordered=False)
