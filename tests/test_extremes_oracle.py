"""MIN / MAX / NUNIQUE (and COUNT beside them) on every path against an exact oracle on bit patterns.

Every path -- CPU hash and pipeline group-by, the scalar aggregates, `unique`, the distributed
group-by and scalar aggregates, the GPU global-path kernels k_agg_scalar / k_agg_lds / k_agg_global,
the GPU radix path's RG_MIN / RG_MAX planes, the composed radix NUNIQUE, the quantile kernel's fused
MIN / MAX, the GPU pipeline group-by, 2 ranks on one device and the forced RCCL exchange -- is
compared, group by group (looked up by the group's key), with the oracle below; never with another
path of the project, and never with numpy's or pandas' min / max / unique, whose NaN rules differ.

The contract (docs/semantics.md, "MIN / MAX / NUNIQUE").  Nulls are skipped.  Values compare by
their order image: integers in their own order; floats in numeric order with -0.0 == +0.0 and every
NaN -- whatever its sign bit or payload -- one value above +inf.  MIN / MAX give back a value of the
column's type: -0.0 as +0.0, any NaN as the positive quiet NaN; null when there is no non-null value.
NUNIQUE is the number of distinct images (int64; 0, never null, without values).  Float group keys
and `unique` use the same equality.

Oracle.  Plain Python integers on the raw bits of the Arrow buffers (int.from_bytes); its image
function is written from the contract above (sign-magnitude arithmetic, not bit flips) and shares
nothing with kernels/order_image.hpp.  Results are compared bit for bit (a -0.0 where +0.0 is due
fails, so does a NaN other than the quiet one), null masks exactly, result types exactly.  There
are no tolerances in this file.

Class x path pairs that are not on the path named (the counters show the fallback; they are not
counted as coverage of that path, and nothing forces them onto it):

    shape fkey64_null (a nullable float key)   GPU radix planes, composed radix NUNIQUE
    shape nullable_key (a nullable int key)    composed radix NUNIQUE
    every class but float64                    the quantile kernel's fused MIN / MAX

Every other class (float64/32/16, int64, uint64, int8, uint16, int32, bool; nullable and not) runs
on every path listed."""
import collections
import functools
import struct

import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C

from oracle_utils import FLOAT_FIELDS as _FLOAT_FIELDS
from oracle_utils import width_kind as _wk
from oracle_utils import (INT64_MIN, LADDER, column_bits, deal_round_robin, fspecials, make_array, spawn_once, traced,
                          wide_keys)

Expect = collections.namedtuple("Expect", "min max nunique count")  # min / max: bits, or None for null

_FLOAT_FMT = {2: "<e", 4: "<f", 8: "<d"}


# ---- the oracle (shares nothing with the project)
def is_nan(bits, w):
    e, m = _FLOAT_FIELDS[w]
    return (bits >> m) & ((1 << e) - 1) == (1 << e) - 1 and bits & ((1 << m) - 1) != 0


def given_back(bits, w, kind):
    """the bits MIN / MAX return for a value: -0.0 as +0.0, any NaN as the positive quiet NaN"""
    if kind != "f":
        return bits
    e, m = _FLOAT_FIELDS[w]
    if is_nan(bits, w):
        return (((1 << e) - 1) << m) | (1 << (m - 1))
    return 0 if bits == 1 << (8 * w - 1) else bits


def image(bits, w, kind):
    """A non-negative integer whose order and equality are the contract's order and equality."""
    nb = 8 * w
    top = 1 << (nb - 1)
    assert 0 <= bits < 1 << nb
    if kind == "u":
        return bits
    if kind == "i":  # the two's complement value, shifted to start at 0
        return (bits - (1 << nb) if bits & top else bits) + top
    if is_nan(bits, w):
        return (1 << nb) - 1  # above +inf (whose image is top + the exponent field)
    magnitude = bits & (top - 1)
    return top - 1 - magnitude if bits & top and magnitude else top + magnitude


def oracle(values, w, kind):
    """values: bit patterns, None for null"""
    seen = {}
    count = 0
    for b in values:
        if b is not None:
            count += 1
            seen.setdefault(image(b, w, kind), given_back(b, w, kind))
    if not seen:
        return Expect(None, None, 0, 0)
    return Expect(seen[min(seen)], seen[max(seen)], len(seen), count)


def decode(bits, w, kind):
    if kind == "f":
        return struct.unpack(_FLOAT_FMT[w], bits.to_bytes(w, "little"))[0]
    return int.from_bytes(bits.to_bytes(w, "little"), "little", signed=kind == "i")


def fbits(x, w):
    return int.from_bytes(struct.pack(_FLOAT_FMT[w], x), "little")


def test_oracle_on_nan_free_data_is_python_min_max_set():
    rng = np.random.default_rng(5)
    for w, kind in [(2, "f"), (4, "f"), (8, "f"), (1, "i"), (2, "u"), (4, "i"), (8, "i"), (8, "u"), (1, "u")]:
        for n in (1, 2, 7, 200):
            bits = [int.from_bytes(rng.bytes(w), "little") for _ in range(n)]
            if kind == "f":
                sp = fspecials(w)
                bits = [b for b in bits if not is_nan(b, w)] + [sp[s] for s in ("pzero", "nzero", "pinf", "ninf", "pden",
                                                                               "nden", "pmax", "nmax")][:n + 1]
            vals = [decode(b, w, kind) for b in bits]
            exp = oracle(bits + [None], w, kind)
            assert decode(exp.min, w, kind) == min(vals) and decode(exp.max, w, kind) == max(vals), (w, kind, n)
            assert exp.nunique == len(set(vals)) and exp.count == len(vals)  # (a set folds -0.0 into 0.0)
            assert exp.min in [given_back(b, w, kind) for b in bits]


def test_oracle_hand_table():
    F = fspecials(8)
    one, two = fbits(1.0, 8), fbits(2.0, 8)
    qnan = 0x7ff8000000000000
    assert F["nnan"] == 0xfff8000000000000 and F["pnan"] == qnan and F["psnan"] == 0x7ff0000000000001
    table = [
        ([one, two, F["pnan"]], Expect(one, qnan, 3, 3)),
        ([one, two, F["nnan"]], Expect(one, qnan, 3, 3)),                 # the sign bit of a NaN means nothing
        ([F["nsnan"], one], Expect(one, qnan, 2, 2)),                     # nor does its payload
        ([F["nnan"], F["pnan"], F["psnan"], F["nsnan"]], Expect(qnan, qnan, 1, 4)),  # MIN is NaN only here
        ([F["pinf"], F["nnan"]], Expect(F["pinf"], qnan, 2, 2)),          # NaN is above +inf
        ([F["nzero"], F["pzero"], F["nzero"]], Expect(0, 0, 1, 3)),       # -0.0 == +0.0, given back as +0.0
        ([F["nzero"], one], Expect(0, one, 2, 2)),
        ([F["nden"], F["pden"], 0], Expect(F["nden"], F["pden"], 3, 3)),  # denormals are not zero
        ([F["ninf"], F["nmax"], F["pmax"], F["pinf"]], Expect(F["ninf"], F["pinf"], 4, 4)),
        ([None, None], Expect(None, None, 0, 0)),
        ([], Expect(None, None, 0, 0)),
        ([None, F["nzero"], None], Expect(0, 0, 1, 1)),
    ]
    for vals, exp in table:
        assert oracle(vals, 8, "f") == exp, [hex(v) if v is not None else v for v in vals]
    assert oracle([0x8000, 0x7e00, 0xfe01], 2, "f") == Expect(0, 0x7e00, 2, 3)
    assert oracle([0xffc00000, 0x3f800000], 4, "f") == Expect(0x3f800000, 0x7fc00000, 2, 2)
    i64 = lambda v: v & (1 << 64) - 1
    assert oracle([i64(-1), 0, i64(INT64_MIN), (1 << 63) - 1], 8, "i") == Expect(1 << 63, (1 << 63) - 1, 4, 4)
    assert oracle([1 << 63, (1 << 63) - 1, 0, (1 << 64) - 1], 8, "u") == Expect(0, (1 << 64) - 1, 4, 4)
    assert oracle([0x80, 0x7f, 0xff], 1, "i") == Expect(0x80, 0x7f, 3, 3) and oracle([1, 0, 1], 1, "u") == Expect(0, 1, 2, 3)


# ---- arrow columns <-> bit patterns
def _ident(col):
    """what makes two key rows one group: the image of a float key, the value of any other; None = null"""
    if pa.types.is_floating(col.type):
        w = col.type.bit_width // 8
        return [None if b is None else ("f", image(b, w, "f")) for b in column_bits(col)]
    return col.to_pylist()


# ---- data: value classes
CLASSES = {"float64": pa.float64(), "float32": pa.float32(), "float16": pa.float16(), "int64": pa.int64(),
           "uint64": pa.uint64(), "int8": pa.int8(), "uint16": pa.uint16(), "int32": pa.int32(), "bool": pa.bool_(),
           "float64_nonan": pa.float64()}  # (the last: for the quantile kernel, whose order of NaN is unspecified)
FLOATS = ("float64", "float32", "float16")
INTS = ("int64", "uint64", "int8", "uint16", "int32")


def _limits(w, kind):
    return (1 << (8 * w - 1), (1 << (8 * w - 1)) - 1) if kind == "i" else (0, (1 << 8 * w) - 1)


def _pools(cls):
    """(special bit patterns, ordinary bit patterns) of a class"""
    typ = CLASSES[cls]
    w, kind = _wk(typ)
    mask = (1 << 8 * w) - 1
    if cls == "bool":
        return [0, 1], [0, 1]
    if kind == "f":
        sp = fspecials(w)
        if cls == "float64_nonan":
            sp = {k: v for k, v in sp.items() if "nan" not in k}
        return list(sp.values()), [fbits(k / 4.0, w) for k in range(-40, 41)]
    if cls == "uint64":
        return [0, (1 << 63) - 1, 1 << 63, mask], list(range(1, 500)) + [(1 << 63) + i for i in range(1, 500)]
    if cls == "int8":
        return [0x80, 0x7f], list(range(256))
    lo, hi = _limits(w, kind)
    sp = [lo, hi, 0] + ([mask] if kind == "i" else [1 << (8 * w - 1)])  # -1 for the signed classes
    return sp, [v & mask for v in range(-300, 301)] if kind == "i" else list(range(1, 600))


def compositions(cls):
    """(tag, rows in row order) of the groups every data set of the class holds"""
    typ = CLASSES[cls]
    w, kind = _wk(typ)
    if cls == "bool":
        return [("only_min", [0]), ("only_max", [1]), ("mixed", [1, 0, 1]), ("all_null", [None] * 5),
                ("lone", [None, 1, None, None])]
    if kind != "f":
        lo, hi = _limits(w, kind)
        mid = [v & ((1 << 8 * w) - 1) for v in (3, 5, 7)]
        return [("only_min", [lo]), ("only_max", [hi]), ("only_min_thrice", [lo, None, lo, lo]), ("single", [mid[0]]),
                ("all_null", [None] * 5), ("min_first_max_last", [lo, mid[0], mid[1], hi]),
                ("max_first_min_last", [hi, mid[2], lo]), ("lone", [None, mid[1], None, None]),
                ("lone_min", [None, None, lo]), ("lone_max", [hi, None, None])]
    F = fspecials(w)
    o = lambda x: fbits(x, w)
    out = [("zeros_neg_first", [F["nzero"], F["pzero"], F["nzero"]]), ("negzero_pos", [o(2.0), F["nzero"], o(0.25)]),
           ("single", [o(7.25)]), ("single_negzero", [F["nzero"]]), ("all_null", [None] * 5),
           ("min_first_max_last", [o(-9.0), o(1.0), o(2.0), o(8.5)]), ("max_first_min_last", [o(9.5), o(1.0), o(-8.0)]),
           ("edges", [F["ninf"], F["nden"], F["pden"], F["nmax"], F["pmax"], F["pinf"]]),
           ("lone", [None, o(4.0), None, None]), ("lone_negzero", [F["nzero"], None, None]),
           ("dens", [F["pden"], F["nden"], F["pzero"]])]
    if cls != "float64_nonan":
        out += [("nans_both", [F["pnan"], F["nnan"], F["nsnan"], F["psnan"]]), ("nums_nnan", [F["nnan"], o(1.5), o(2.5)]),
                ("nums_pnan", [o(1.5), F["pnan"], o(-2.5)]), ("nums_nsnan", [o(3.0), F["nsnan"]]),
                ("nums_psnan", [F["psnan"], o(3.0), o(-1.0)]), ("inf_nan", [F["pinf"], F["nnan"]]),
                ("lone_nnan", [None, None, F["nnan"]]), ("single_nnan", [F["nnan"]])]
    return out


def _draw(rng, cls, n, nulls, rate):
    """n rows: a special with probability `rate`, else an ordinary value; ~10 % nulls"""
    special, ordinary = _pools(cls)
    pick = rng.random(n) < rate
    si, oi = rng.integers(0, len(special), n), rng.integers(0, len(ordinary), n)
    null = rng.random(n) < (0.1 if nulls else 0.0)
    return [None if null[i] else (special[si[i]] if pick[i] else ordinary[oi[i]]) for i in range(n)]


# ---- data: shapes
SHAPES = ("ladder", "many", "hot", "two_keys", "nullable_key", "one_group", "fkey64", "fkey32", "fkey64_null", "qfused")
_RATES = (0.0, 0.03, 0.3)
_I64 = (1 << 64) - 1


def _filler_sizes(shape):
    if shape == "many":
        return list(LADDER) + [1 + i % 6 for i in range(2100)] + [100]
    if shape == "hot":
        return [5000] + [1] * 500
    if shape == "qfused":  # one- and two-slot wave buckets (<= 64, <= 128 rows), rank counting (> 128), shared buckets
        return list(LADDER) + [100, 128, 129, 150] + [1 + i % 6 for i in range(1800)]
    if shape == "one_group":
        return [1500]
    return list(LADDER) + [100]


def _float_key_rows(w, rng):
    """key bit patterns per group: NaNs of both signs and payloads are one key, so are the zeros"""
    F = fspecials(w)
    groups = [[F[s] for s in ("nnan", "pnan", "psnan", "nsnan", "nnan", "psnan", "pnan", "nsnan", "nnan")],
              [F["nzero"], F["pzero"]] * 3, [F["pinf"]] * 4, [F["ninf"]] * 3, [F["pden"]] * 2, [F["nden"]] * 2,
              [F["pmax"]], [F["nmax"]]]
    sizes = (1, 2, 3, 63, 64, 65)
    groups += [[fbits(v / 8.0, w)] * sizes[i % len(sizes)] for i, v in enumerate(range(-24, 25)) if v != 0]
    return groups


@functools.lru_cache(maxsize=None)
def dataset(shape, cls, nulls=True):
    """(arrow table with the key column(s), x of class `cls` and an int64 y; key column names).
    Fixed seed; the rows of the groups are interleaved at random, each group's own rows in the order
    written; ~10 % nulls in x and in y when `nulls`, else none."""
    rng = np.random.default_rng([11, SHAPES.index(shape), list(CLASSES).index(cls), int(nulls)])
    typ = CLASSES[cls]
    names = ["k"]
    if shape.startswith("fkey"):
        kw = 4 if shape == "fkey32" else 8
        ktyp = pa.float32() if kw == 4 else pa.float64()
        krows = _float_key_rows(kw, rng)
        if shape == "fkey64_null":
            krows.append([None] * 7)
        xrows = [_draw(rng, cls, len(g), nulls, _RATES[i % 3]) for i, g in enumerate(krows)]
    else:
        ktyp = pa.int64()
        xrows = []
        if shape != "one_group":
            for _, rows in compositions(cls):
                rows = rows if nulls else [r for r in rows if r is not None]
                if rows:
                    xrows.append(rows)
        xrows += [_draw(rng, cls, n, nulls, _RATES[i % 3]) for i, n in enumerate(_filler_sizes(shape))]
        G = len(xrows)
        if shape == "two_keys":
            keys = (rng.choice(np.arange(-(1 << 20), 1 << 20), G, replace=False) << 20).tolist()
        else:
            keys = wide_keys(rng, G)
        if shape in ("ladder", "many", "nullable_key", "qfused"):
            keys[-1] = INT64_MIN  # the radix table's spare slot; the global path's sentinel slot
        if shape == "nullable_key":
            keys[len(keys) - 5] = None  # the filler group of 255 rows ...
            keys[2] = None              # ... and a composition: one group under the null key
        krows = [[None if k is None else k & _I64] * len(x) for k, x in zip(keys, xrows)]
    sizes = [len(x) for x in xrows]
    n = sum(sizes)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(labels)
    slots = np.argsort(labels, kind="stable")  # the table positions of group 0's rows, group 1's rows, ...

    def place(rows_by_group):
        out = [None] * n
        for pos, v in zip(slots.tolist(), (v for rows in rows_by_group for v in rows)):
            out[pos] = v
        return out

    key_nullable = shape in ("nullable_key", "fkey64_null")
    cols = {"k": make_array(place(krows), ktyp, key_nullable)}
    if shape == "two_keys":
        cols["g"] = make_array(place([[(i % 3 - 1) & 0xffff] * s for i, s in enumerate(sizes)]), pa.int16(), False)
        names.append("g")
    cols["x"] = make_array(place(xrows), typ, nulls)
    ynull = rng.random(n) < (0.1 if nulls else 0.0)
    yv = rng.integers(-100, 101, n)
    cols["y"] = make_array([None if ynull[i] else int(yv[i]) & _I64 for i in range(n)], pa.int64(), nulls)
    return pa.table(cols), tuple(names)


@functools.lru_cache(maxsize=None)
def _groups(shape, cls, nulls, col):
    """group identity (tuple) -> the bit patterns of its rows of `col` in row order, from the arrow table itself"""
    t, keys = dataset(shape, cls, nulls)
    out = {}
    for *kk, b in zip(*[_ident(t[k]) for k in keys], column_bits(t[col])):
        out.setdefault(tuple(kk), []).append(b)
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, cls, nulls, col):
    w, kind = _wk(dataset(shape, cls, nulls)[0][col].type)
    return {k: oracle(v, w, kind) for k, v in _groups(shape, cls, nulls, col).items()}


_MAIN = tuple(c for c in CLASSES if c != "float64_nonan")
GROUPED = ([("ladder", c, True) for c in _MAIN] + [("ladder", c, False) for c in FLOATS + INTS] +
           [("many", c, True) for c in ("float64", "float32", "int64", "uint64")] + [("many", "float64", False)] +
           [("hot", c, True) for c in ("float64", "int64", "uint64")] +
           [("one_group", c, True) for c in ("float64", "float16", "int64", "uint64")] +
           [("two_keys", "float64", True), ("nullable_key", "float64", True), ("nullable_key", "int64", True),
            ("fkey64", "float64", True), ("fkey32", "int64", True), ("fkey64_null", "float32", True)])
QFUSED = [("qfused", "float64_nonan", True), ("qfused", "float64_nonan", False)]
_ids = lambda cases: [f"{s}-{c}-{'nullable' if n else 'nonnull'}" for s, c, n in cases]


def test_datasets_hold_what_they_promise():
    for shape, cls, nulls in GROUPED + QFUSED:
        t, keys = dataset(shape, cls, nulls)
        groups = _groups(shape, cls, nulls, "x")
        w, kind = _wk(t["x"].type)
        assert t.num_rows < 11_500 and (t["x"].null_count > 0) == nulls and (t["y"].null_count > 0) == nulls
        sizes = sorted(len(v) for v in groups.values())
        if shape in ("ladder", "many", "nullable_key", "qfused"):
            assert (INT64_MIN,) in groups
            assert any(k[0] is not None and k[0] > 1 << 32 for k in groups) and any(
                k[0] is not None and k[0] < -(1 << 32) for k in groups)
            assert shape == "nullable_key" or set(LADDER) <= set(sizes)
        if shape == "ladder":
            assert 2 < len(groups) <= 2048  # k_agg_lds
        if shape in ("many", "qfused"):
            assert len(groups) > (2048 if shape == "many" else 1500)  # k_agg_global; several radix partitions
        if shape == "hot":
            assert sizes[-1] == 5000 and sizes[-2] <= 6
        if shape == "one_group":
            assert len(groups) == 1
        if shape in ("nullable_key", "fkey64_null"):
            assert (None,) in groups and t["k"].null_count > 0
        if shape == "two_keys":
            assert len(keys) == 2 and len({k[1] for k in groups}) == 3
        if shape.startswith("fkey"):
            kb = {b for b in column_bits(t["k"]) if b is not None}
            F = fspecials(t["k"].type.bit_width // 8)
            assert set(F.values()) <= kb and len(groups) < len(kb) + (shape == "fkey64_null")
            continue
        if shape == "one_group":
            continue
        # the group compositions, found by what they hold (not by their tags)
        vals = [[b for b in g if b is not None] for g in groups.values()]
        have = lambda pred: any(pred(v) for v in vals)
        img = lambda v: [image(b, w, kind) for b in v]
        assert have(lambda v: len(v) == 1)
        assert not nulls or any(len(g) > 1 and all(b is None for b in g) for g in groups.values())
        assert not nulls or any(len(g) > 2 and sum(b is not None for b in g) == 1 for g in groups.values())
        if cls == "bool":
            assert have(lambda v: set(v) == {0}) and have(lambda v: set(v) == {1}) and have(lambda v: set(v) == {0, 1})
            continue
        assert have(lambda v: len(v) >= 3 and img(v)[0] == min(img(v)) < min(img(v)[1:]) and img(v)[-1] == max(img(v)))
        assert have(lambda v: len(v) >= 3 and img(v)[0] == max(img(v)) and img(v)[-1] == min(img(v)) < min(img(v)[:-1]))
        if kind != "f":
            lo, hi = _limits(w, kind)
            assert have(lambda v: set(v) == {lo}) and have(lambda v: set(v) == {hi})
            continue
        F = fspecials(w)
        assert have(lambda v: len(v) > 1 and set(v) <= {F["nzero"], F["pzero"]} and v[0] == F["nzero"])
        assert have(lambda v: F["nzero"] in v and len(v) > 1 and all(b == F["nzero"] or decode(b, w, "f") > 0 for b in v))
        assert have(lambda v: {F["nden"], F["pden"], F["ninf"], F["pinf"], F["nmax"], F["pmax"]} <= set(v))
        nan = lambda b: is_nan(b, w)
        neg = lambda b: bool(b >> (8 * w - 1))
        if cls == "float64_nonan":
            assert not any(nan(b) for v in vals for b in v)
            continue
        assert have(lambda v: all(nan(b) for b in v) and {neg(b) for b in v} == {True, False})
        assert have(lambda v: any(nan(b) for b in v) and not all(nan(b) for b in v) and all(neg(b) for b in v if nan(b)))
        assert have(lambda v: any(nan(b) for b in v) and not all(nan(b) for b in v) and not any(neg(b) for b in v if nan(b)))
        assert have(lambda v: any(nan(b) and b not in (F["pnan"], F["nnan"]) for b in v) and not all(nan(b) for b in v))
        assert have(lambda v: F["pinf"] in v and any(nan(b) for b in v) and len(v) == 2)
        assert F["nnan"] in column_bits(t["x"]) and F["nsnan"] in column_bits(t["x"])  # arrow kept the bits


# ---- comparing a result table with the oracle
AGGS = {"x": ["min", "max", "nunique", "count"], "y": ["max", "min", "nunique"]}
MM_AGGS = {"x": ["min", "max", "count"], "y": ["min", "max"]}  # decomposable: the two-phase distributed form


def _specs(aggs):
    return [(col, op if isinstance(op, str) else op[0]) for col, ops in aggs.items() for op in ops]


def _hex(b):
    return b if b is None else hex(b)


def check(res, aggs, shape, cls, nulls, what):
    """Every group of every result column of the arrow table `res`, bit for bit; the key and result types."""
    t, keys = dataset(shape, cls, nulls)
    nk, specs = len(keys), _specs(aggs)
    assert res.num_columns == nk + len(specs), (res.schema, specs)
    for i, k in enumerate(keys):
        assert res.column(i).type == t[k].type, f"{what}: key {k} came out as {res.column(i).type}"
    got_keys = list(zip(*[_ident(res.column(i)) for i in range(nk)]))
    assert len(set(got_keys)) == len(got_keys), f"{what} {shape}/{cls}: a group came out twice"
    bad = []
    for j, (col, op) in enumerate(specs):
        if op in ("sum", "quantile"):
            continue  # (rides along to fill accumulator planes; checked by the moments / quantile suites)
        exp = expected(shape, cls, nulls, col)
        assert set(got_keys) == exp.keys(), f"{what} {shape}/{cls}: groups differ: " \
            f"{len(got_keys)} came out, {len(exp)} expected, e.g. {list(set(got_keys) ^ exp.keys())[:4]}"
        c = res.column(nk + j)
        want_type = t[col].type if op in ("min", "max") else pa.int64()
        assert c.type == want_type, f"{what}: {op}({col}) came out as {c.type}, not {want_type}"
        for k, b in zip(got_keys, column_bits(c)):
            want = getattr(exp[k], op)
            if b != want:
                bad.append((col, op, k, _hex(b), _hex(want), [_hex(v) for v in _groups(shape, cls, nulls, col)[k][:6]]))
    assert not bad, f"{what} {shape}/{cls}: {len(bad)} results off, " \
                    f"(column, op, group, got, oracle, the group's first rows): {bad[:6]}"


# ---- CPU context
@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_cpu_hash_groupby_matches_oracle(ctx, shape, cls, nulls):
    t, keys = dataset(shape, cls, nulls)
    got, cnt = traced(lambda: Table(t, ctx).local_groupby(list(keys), AGGS))
    assert "groupby.radix.groups" not in cnt, cnt
    check(got.to_arrow(), AGGS, shape, cls, nulls, "cpu hash")


@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_cpu_pipeline_groupby_matches_oracle(ctx, shape, cls, nulls):
    t, keys = dataset(shape, cls, nulls)
    T = Table(t.sort_by([(c, "ascending") for c in keys]), ctx)
    check(T.local_groupby(list(keys), AGGS, algorithm="pipeline").to_arrow(), AGGS, shape, cls, nulls, "cpu pipeline")


SCALAR_OPS = ("min", "max", "nunique", "count")
SCALAR = [(c, True) for c in _MAIN] + [(c, False) for c in FLOATS + INTS]
_sids = [f"{c}-{'nullable' if n else 'nonnull'}" for c, n in SCALAR]


@functools.lru_cache(maxsize=None)
def scalar_tables(cls, nulls):
    """(name, rows) of one-column tables: every composition, two fillers, an empty and an all-null table"""
    rng = np.random.default_rng([13, list(CLASSES).index(cls), int(nulls)])
    out = []
    for tag, rows in compositions(cls):
        rows = rows if nulls else [r for r in rows if r is not None]
        if rows:
            out.append((tag, rows))
    out += [("fill_65", _draw(rng, cls, 65, nulls, 0.03)), ("fill_1000", _draw(rng, cls, 1000, nulls, 0.3)),
            ("fill_4097_plain", _draw(rng, cls, 4097, nulls, 0.0)), ("empty", [])]
    return out


def _scalar_results(context, cls, nulls, rank=0, world=1):
    """name -> op -> (type, bits) of this rank's share (row i on rank i mod world) of every scalar table"""
    out = {}
    for name, rows in scalar_tables(cls, nulls):
        T = Table(pa.table({"x": make_array(rows[rank::world], CLASSES[cls], nulls)}), context)
        out[name] = {}
        for op in SCALAR_OPS:
            r = getattr(T, op)("x").to_arrow()
            assert r.num_rows == 1 and r.num_columns == 1, (name, op, r)
            out[name][op] = (r.column(0).type, column_bits(r.column(0))[0])
    return out


def _check_scalar(results, cls, nulls, what):
    typ = CLASSES[cls]
    w, kind = _wk(typ)
    bad = []
    for name, rows in scalar_tables(cls, nulls):
        exp = oracle(rows, w, kind)
        for op in SCALAR_OPS:
            got_type, b = results[name][op]
            want_type = typ if op in ("min", "max") else pa.int64()
            if got_type != want_type or b != getattr(exp, op):
                bad.append((name, op, str(got_type), _hex(b), _hex(getattr(exp, op))))
    assert not bad, f"{what} {cls}: (table, op, type, got, oracle): {bad[:8]}"


@pytest.mark.parametrize("cls,nulls", SCALAR, ids=_sids)
def test_cpu_scalar_aggregates_match_oracle(ctx, cls, nulls):
    _check_scalar(_scalar_results(ctx, cls, nulls), cls, nulls, "cpu scalar")


UNIQUE = [(c, n) for c in FLOATS for n in (True, False)]


def _check_unique(res, cls, nulls, what):
    """`unique` of the ladder data set's x: one row per image (and one null row), each an input value"""
    w = CLASSES[cls].bit_width // 8
    rows = column_bits(dataset("ladder", cls, nulls)[0]["x"])
    by_image = {}
    for b in rows:
        by_image.setdefault(None if b is None else image(b, w, "f"), set()).add(b)
    assert res.column(0).type == CLASSES[cls]
    got = column_bits(res.column(0))
    got_images = [None if b is None else image(b, w, "f") for b in got]
    assert len(set(got_images)) == len(got_images), f"{what} {cls}: a value came out twice: " \
        f"{[_hex(b) for b, i in zip(got, got_images) if got_images.count(i) > 1][:6]}"
    assert set(got_images) == by_image.keys(), f"{what} {cls}: {len(got)} rows, {len(by_image)} distinct values"
    assert all(b in by_image[i] for b, i in zip(got, got_images)), f"{what} {cls}: a row that is no input value"


@pytest.mark.parametrize("cls,nulls", UNIQUE, ids=[f"{c}-{'nullable' if n else 'nonnull'}" for c, n in UNIQUE])
def test_cpu_unique_of_a_float_column(ctx, cls, nulls):
    T = Table(dataset("ladder", cls, nulls)[0].select(["x"]), ctx)
    _check_unique(T.unique(["x"]).to_arrow(), cls, nulls, "cpu unique")


# ---- distributed: rows dealt round-robin, so a group's NaN, its -0.0 or its only non-null value sit
# alone on some rank, and some rank holds only nulls (or no row) of a group
DIST_CASES = ([("ladder", c, True) for c in _MAIN] + [("ladder", c, False) for c in FLOATS + INTS] +
              [("many", "float64", True), ("two_keys", "float64", True), ("nullable_key", "float64", True),
               ("nullable_key", "int64", True), ("fkey64", "float64", True), ("fkey32", "int64", True),
               ("fkey64_null", "float32", True)])


def _dist_worker(ctx, cases, chunks, forced):
    """Per case the group-by with NUNIQUE (raw rows are shuffled, one aggregation) and without (the
    two-phase form: partial MIN / MAX / COUNT states per rank, combined after the shuffle; nullable
    columns take the generic phase 1, non-null ones the local hash group-by); the scalar aggregates
    and distributed_unique on this rank's share."""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    if forced:
        assert world == 1 and ctx.is_distributed()
        ctx.add_config("force_shuffle", "1")
        ctx.add_config("shuffle_self_rccl", "1")
    ctx.add_config("shuffle_chunks", str(chunks))
    out = {}
    C.trace_enable(True)
    C.trace_reset()
    for shape, cls, nulls in cases:
        t, keys = dataset(shape, cls, nulls)
        mine = deal_round_robin(zip(*[_ident(t[k]) for k in keys]), rank, world)
        T = Table(t.take(pa.array(mine, type=pa.int64())), ctx)
        assert T.device == ctx.device
        for name, aggs in (("all", AGGS), ("minmax", MM_AGGS)):
            out[("groupby", name, shape, cls, nulls)] = T.groupby(list(keys), aggs).to_arrow()
    for cls, nulls in SCALAR:
        out[("scalar", cls, nulls)] = _scalar_results(ctx, cls, nulls, rank, world)
    for cls, nulls in UNIQUE:
        x = dataset("ladder", cls, nulls)[0].select(["x"])
        T = Table(x.take(pa.array(list(range(rank, x.num_rows, world)), type=pa.int64())), ctx)
        out[("unique", cls, nulls)] = T.distributed_unique(["x"]).to_arrow()
    counters = dict(C.trace_counters())
    C.trace_enable(False)
    return out, counters


_spawned = {}


def _dist(world, device, chunks, rccl_forced=False):
    return spawn_once(_spawned, _dist_worker, DIST_CASES, world, device, chunks, rccl_forced)


def _check_dist_groupby(res, case, what):
    for name, aggs in (("all", AGGS), ("minmax", MM_AGGS)):
        merged = pa.concat_tables([r[0][("groupby", name) + case] for r in res])
        check(merged, aggs, *case, f"{what} {name}")


def _check_dist_scalar(res, cls, nulls, what):
    for rank, r in enumerate(res):
        _check_scalar(r[0][("scalar", cls, nulls)], cls, nulls, f"{what} rank {rank}")


def _check_dist_unique(res, cls, nulls, what):
    _check_unique(pa.concat_tables([r[0][("unique", cls, nulls)] for r in res]), cls, nulls, what)


_WORLDS = pytest.mark.parametrize("world,chunks", [(2, 1), (3, 3)], ids=["2ranks", "3ranks_chunked"])


@pytest.mark.parametrize("case", DIST_CASES, ids=_ids(DIST_CASES))
@_WORLDS
def test_cpu_distributed_groupby_matches_oracle(world, chunks, case):
    _check_dist_groupby(_dist(world, "cpu", chunks), case, f"cpu {world} ranks")


@pytest.mark.parametrize("cls,nulls", SCALAR, ids=_sids)
@_WORLDS
def test_cpu_distributed_scalar_aggregates_match_oracle(world, chunks, cls, nulls):
    _check_dist_scalar(_dist(world, "cpu", chunks), cls, nulls, f"cpu {world} ranks scalar")


@pytest.mark.parametrize("cls,nulls", UNIQUE, ids=[f"{c}-{'nullable' if n else 'nonnull'}" for c, n in UNIQUE])
@_WORLDS
def test_cpu_distributed_unique_of_a_float_column(world, chunks, cls, nulls):
    _check_dist_unique(_dist(world, "cpu", chunks), cls, nulls, f"cpu {world} ranks unique")


# ---- GPU
def _radix_declines(shape):
    return shape == "fkey64_null"  # a nullable float key: the sort-based group ids of the global path


def _composed_declines(shape):
    return shape in ("fkey64_null", "nullable_key")  # the composed NUNIQUE joins on the keys: non-null keys only


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_gpu_global_path_matches_oracle(gpu_ctx, monkeypatch, shape, cls, nulls):
    """kernels/groupby.hip: k_agg_scalar (`one_group`), k_agg_lds (<= 2048 groups; `hot`: one contended
    LDS slot), k_agg_global (`many`); the INT64_MIN key sits in group_insert's sentinel slot; float keys
    are grouped by their image."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", str(1 << 62))
    t, keys = dataset(shape, cls, nulls)
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), AGGS))
    assert "groupby.radix.groups" not in cnt and "groupby.radix.nunique_columns" not in cnt, cnt
    check(got.to_arrow(), AGGS, shape, cls, nulls, "gpu global")


# accumulator planes of a nullable x and y (a non-null column needs no count plane beside MIN / MAX)
RADIX_AGGS = {
    2: {"x": ["min"]},                                                    # MIN, CNT
    4: {"x": ["min", "max"], "y": ["sum"]},                               # MIN, CNT, MAX | SUMI
    8: {"x": ["min", "max", "count"], "y": ["sum", "count", "min", "max"]},  # MIN, CNT, MAX | SUMI, CNT, MIN, MAX
}


@pytest.mark.gpu
@pytest.mark.parametrize("planes", sorted(RADIX_AGGS))
@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_gpu_radix_path_matches_oracle(gpu_ctx, monkeypatch, shape, cls, nulls, planes):
    """kernels/radix_groupby.hip k_rg_agg: RG_MIN / RG_MAX planes beside RG_SUMI / RG_CNT in the 2-, 4-
    and 8-plane tables (the INT64_MIN key in the spare slot S); `many` spans several partitions."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", "1")
    t, keys = dataset(shape, cls, nulls)
    aggs = RADIX_AGGS[planes]
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), aggs))
    if _radix_declines(shape):
        assert "groupby.radix.groups" not in cnt, cnt
    else:
        assert cnt.get("groupby.radix.groups") == len(expected(shape, cls, nulls, "x")), cnt
        assert cnt.get("groupby.radix.overflow_fallback", 0) == 0, cnt
    check(got.to_arrow(), aggs, shape, cls, nulls, f"gpu radix {planes} planes")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_gpu_radix_composed_nunique_matches_oracle(gpu_ctx, monkeypatch, shape, cls, nulls):
    """NUNIQUE composed from radix group-bys (ops/groupby.cpp radix_groupby_composed): the distinct
    (key, value) pairs counted per key, joined to the MIN / MAX / COUNT of a radix group-by."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", "1")
    t, keys = dataset(shape, cls, nulls)
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), AGGS))
    if _composed_declines(shape):
        assert "groupby.radix.nunique_columns" not in cnt, cnt
    else:
        assert cnt.get("groupby.radix.nunique_columns") == 2, cnt
    check(got.to_arrow(), AGGS, shape, cls, nulls, "gpu radix composed nunique")


QF_AGGS = {"x": [("quantile", 0.5), "min", "max", "count"]}


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls,nulls", QFUSED, ids=_ids(QFUSED))
def test_gpu_quantile_fused_min_max_match_oracle(gpu_ctx, monkeypatch, shape, cls, nulls):
    """k_rg_quantile<FUSE>: MIN / MAX / COUNT of the quantile's own float64 column from the wave select
    (buckets of one key, <= 64 and <= 128 rows), the sorted mixed buckets and the rank-counting rows of
    buckets over 128 rows.  No NaN (QUANTILE of NaN is unspecified); +-inf, +-0, denormals."""
    monkeypatch.setenv("CYLON_RADIX_GROUPBY_MIN_ROWS", "1")
    t, keys = dataset(shape, cls, nulls)
    T = Table(t, gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), QF_AGGS))
    assert cnt.get("groupby.radix.quantile") == 1 and cnt.get("groupby.radix.quantile_fused_aggs") == 3, cnt
    assert cnt.get("groupby.radix.quantile_overflow_fallback", 0) == 0, cnt
    check(got.to_arrow(), QF_AGGS, shape, cls, nulls, "gpu fused quantile")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls,nulls", GROUPED, ids=_ids(GROUPED))
def test_gpu_pipeline_groupby_matches_oracle(gpu_ctx, shape, cls, nulls):
    t, keys = dataset(shape, cls, nulls)
    T = Table(t.sort_by([(c, "ascending") for c in keys]), gpu_ctx)
    got, cnt = traced(lambda: T.local_groupby(list(keys), AGGS, algorithm="pipeline"))
    assert "groupby.radix.groups" not in cnt, cnt
    check(got.to_arrow(), AGGS, shape, cls, nulls, "gpu pipeline")


@pytest.mark.gpu
@pytest.mark.parametrize("cls,nulls", SCALAR, ids=_sids)
def test_gpu_scalar_aggregates_match_oracle(gpu_ctx, cls, nulls):
    _check_scalar(_scalar_results(gpu_ctx, cls, nulls), cls, nulls, "gpu scalar")


@pytest.mark.gpu
@pytest.mark.parametrize("cls,nulls", UNIQUE, ids=[f"{c}-{'nullable' if n else 'nonnull'}" for c, n in UNIQUE])
def test_gpu_unique_of_a_float_column(gpu_ctx, cls, nulls):
    T = Table(dataset("ladder", cls, nulls)[0].select(["x"]), gpu_ctx)
    _check_unique(T.unique(["x"]).to_arrow(), cls, nulls, "gpu unique")


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIST_CASES, ids=_ids(DIST_CASES))
def test_gpu_distributed_groupby_matches_oracle(case):
    """2 ranks share cuda:0, the collectives go over gloo: the device kernels of both phases."""
    _check_dist_groupby(_dist(2, "cuda:0", 2), case, "gpu 2 ranks")


@pytest.mark.gpu
@pytest.mark.parametrize("cls,nulls", SCALAR, ids=_sids)
def test_gpu_distributed_scalar_aggregates_match_oracle(cls, nulls):
    res = _dist(2, "cuda:0", 2)
    _check_dist_scalar(res, cls, nulls, "gpu 2 ranks scalar")
    if (cls, nulls) in UNIQUE:
        _check_dist_unique(res, cls, nulls, "gpu 2 ranks unique")


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIST_CASES, ids=_ids(DIST_CASES))
def test_gpu_forced_rccl_groupby_matches_oracle(case):
    """A world-1 RCCL context with force_shuffle: the partial rows (and the raw rows of the NUNIQUE
    form) go through the chunked RCCL exchange."""
    res = _dist(1, "cuda:0", 4, True)
    _check_dist_groupby(res, case, "gpu forced rccl")
    assert res[0][1].get("shuffle.chunks", 0) > 0, res[0][1]
