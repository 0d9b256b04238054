"""String <-> number casts (Table.astype; kernels/strcast.hip, kernels/strparse.hpp, the CPU twins and
ops/plumbing.cpp) on every path against an exact oracle.

The contract (docs/semantics.md, "String <-> number casts").  string -> float accepts
`[+-] digits [. digits] [(e|E) [+-] digits]` with at least one mantissa digit and nothing else, and
gives the correctly rounded (nearest, ties to even) binary64 / binary32 of the decimal, bit for bit,
whether the column is parsed on the device or by the host parser.  string -> integer accepts an
optional '-' (signed targets only; never '+') and decimal digits, and rejects values outside the
target's range.  A string that does not parse raises pa.ArrowInvalid unless its row is null.
integer -> string is Python's str().

Oracle.  tests/strcast_utils.py: exact fractions and integers, written from that text.  Expected
values come from it alone, except for the inf / nan spellings and hex literals, where Arrow's host
parser is the definition.  Every comparison is on the raw bits of the Arrow buffers, null masks and
result types exactly; there are no tolerances in this file.  A second test per corpus holds Arrow's
own cast to the same oracle, so "same as Arrow" is checked, not assumed.  Each test runs on the CPU
engine and on the GPU engine; the two are never compared with each other."""
import functools
import random
import struct
from fractions import Fraction

import pyarrow as pa
import pyarrow.compute as pc
import pytest

from cylon_amd import Table
from cylon_amd._lib import C
from cylon_amd.data import arrow_bridge as ab

from strcast_utils import (F32, F64, HOST, REJECT, SPECIAL, float_bits, int_range, int_to_str, layouts, one_chunk,
                           parse_decimal, parse_int, round_binary, string_array, string_cells, validity, value_bits)

FMT = {pa.float64(): F64, pa.float32(): F32}
INT_TYPES = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32()]
SIZES = [0, 1, 255, 256, 257]
BIG = 524_288 + 257  # one full grid of 2048 blocks x 256 threads and a ragged tail


@pytest.fixture(params=[pytest.param("ctx", id="cpu"), pytest.param("gpu_ctx", id="gpu", marks=pytest.mark.gpu)])
def cx(request):
    return request.getfixturevalue(request.param)


def astype(cx, arr, typ):
    return one_chunk(Table(pa.table({"s": arr}), cx).astype({"s": typ}).to_arrow().column(0))


def device_cast(cx, arr, typ):
    """the native cast alone: a column, or None when the column needs the host parser"""
    col = Table(pa.table({"s": arr}), cx).native.columns()[0]
    return C.cast_string_to_number(col, ab.to_cylon_type(typ))


# ---- corpora (lists of byte strings, deterministic)
def shift(m, e):
    """the integer m times 10^e (e <= 0) printed with -e fractional digits"""
    s = str(m).rjust(1 - e, "0")
    return (s[:e] + "." + s[e:]) if e else s


def fast_path(b):
    """The contract's device rows: at most 19 significant digits, mantissa <= 2^53, and a power of
    ten within +-22 once the fractional digits are counted in.  Everything else that parses goes to
    the host parser."""
    if b[:1] in (b"+", b"-"):
        b = b[1:]
    low = b.lower()
    mant, _, ex = low.partition(b"e")
    ip, _, fp = mant.partition(b".")
    digits = (ip + fp).lstrip(b"0")
    return len(digits) <= 19 and int(digits or b"0") <= 2 ** 53 and abs(int(ex or b"0") - len(fp)) <= 22


@functools.lru_cache(maxsize=None)
def f64_clinger():
    rows = []
    mants = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 1234567890123456789, (2 ** 53 + 1) * 1000, 12345678901234567890,
             (2 ** 53 + 1) * 10000, 7, 123]
    for m in mants:
        for e in (-23, -22, 22, 23):
            rows.append("%de%d" % (m, e))                                    # by the suffix
            rows.append(shift(m, e) if e < 0 else str(m) + "0" * e + ".0")   # by the digits
            rows.append("%sE%+d" % (shift(m, -5), e + 5))                    # by both
            rows.append("%se%d" % (shift(m, -30), e + 30))
    rows += ["1" + "0" * 25, "1.5" + "0" * 30, "0" * 40 + "123.5", "0." + "0" * 40 + "7", "0" * 40 + "." + "0" * 40,
             "1e0000000005", "1e99999999999999999999", "1e-99999999999999999999", "0e99999999999", "0e-99999999999",
             "-0e5", "0", "-0", "+0.0", "-0.0e-5", "-.0", "0.", "1e22", "1e23", "1e-22", "1e-23",
             "9007199254740993", "9007199254740992e22", "9007199254740993e22", "8.5e-22", "1.7976931348623157e308",
             "1.7976931348623159e308", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
             "2.2250738585072011e-308", "2.2250738585072014e-308", "0.1", "0.3", ".5", "5.", "+1e3", "1E-3"]
    rows += ["-" + r for r in rows if r[0] not in "+-"]
    return tuple(r.encode() for r in rows)


@functools.lru_cache(maxsize=None)
def f64_division():
    """{form: rows}: m < 2^53 with k = 1..22 fractional digits (the division), the same with a
    suffix e-k, and e+k for the multiplication"""
    rng = random.Random(1559917)
    pairs = []
    for _ in range(20000):
        bits = rng.randint(1, 53)
        pairs.append((rng.randrange(1 << (bits - 1), 1 << bits), rng.randint(1, 22)))
    return {"digits": tuple(shift(m, -k).encode() for m, k in pairs),
            "e-k": tuple(b"%de-%d" % p for p in pairs),
            "e+k": tuple(b"%de+%d" % p for p in pairs)}


# rounded twice (string -> binary64 -> binary32) these gave 0x3fc7ab60 for 0x3fc7ab5f and ..7a for ..7b
F32_NAMED = (b"1.559917390346527", b"1.394149124622345")


@functools.lru_cache(maxsize=None)
def f32_midpoints():
    """(device rows, extra rows).  Device rows: for 2000 binary32 midpoints in each of three
    binades the two decimals next to the midpoint (never on it) at the longest length whose integer
    mantissa stays below 2^53.  Extra rows: exact ties, the range edges, named regressions."""
    rng = random.Random(3274)
    rows = []
    ties = []
    for binade in (-10, 0, 20):
        for i in range(2000):
            mid = Fraction(2 * ((1 << 23) + rng.randrange(1 << 23)) + 1, 2) * Fraction(2) ** (binade - 23)
            p = 0
            while mid * 10 ** (p + 1) + 1 < 2 ** 53:
                p += 1
            x = mid * 10 ** p
            below, above = -(-x.numerator // x.denominator) - 1, x.numerator // x.denominator + 1
            assert Fraction(below, 10 ** p) < mid < Fraction(above, 10 ** p) and above < 2 ** 53 and p <= 22
            rows += [shift(below, -p), shift(above, -p)]
            if binade == 20 and i < 50:  # four fractional bits: the tie itself is a short decimal
                ties.append(shift(int(mid * 10 ** 4), -4))
    top = 2 ** 128 - 2 ** 103  # half an ulp above the largest binary32: the tie that rounds to inf
    extra = ties + ["16777217", "16777219", "1.000000059604644775390625", "1.000000178813934326171875",
                    "3.4028235e38", "3.5e38", "1e-46", str(top), str(top - 1), "1e39", "1.4e-45", "7e-46", "7.1e-46",
                    "1.17549435e-38", "1.1754942e-38", "1e-22", "9007199254740992e22"]
    extra += ["-" + r for r in extra]
    return tuple(r.encode() for r in rows) + F32_NAMED, tuple(r.encode() for r in extra)


PLAIN_SEED = 20


@functools.lru_cache(maxsize=None)
def plain():
    """20,000 values of at most 7 significant digits in mixed notation.  A draw whose binary64 is
    exactly a binary32 midpoint (71e8 = 27734375 * 2^8 is one: 25 significant bits) is drawn again:
    no seed avoids them all, and such a row sends a float32 column to the host parser."""
    rng = random.Random(PLAIN_SEED)
    rows = []
    while len(rows) < 20000:
        m = rng.randrange(10 ** rng.randint(1, 7))
        form = rng.randrange(6)
        if form == 0:
            s = str(m)
        elif form == 1:
            s = shift(m, -rng.randint(1, 9))
        elif form == 2:
            s = "%d%s%d" % (m, rng.choice("eE"), rng.randint(-15, 15))
        elif form == 3:
            s = "%s%s%+d" % (shift(m, -rng.randint(1, 7)), rng.choice("eE"), rng.randint(-12, 12))
        elif form == 4:
            s = shift(m, -rng.randint(1, 7)).lstrip("0")  # ".5"
            s = s if s != "." else ".0"
        else:
            s = str(m) + "."                              # "5."
        s = rng.choice(["", "", "-", "+"]) + s
        if float_bits(s.encode(), F64) & 0x1fffffff != 0x10000000:
            rows.append(s)
    return tuple(r.encode() for r in rows)


FLOAT_REJECTS = [b"", b".", b"+", b"-", b"-.", b"e5", b".e5", b"1e", b"1e+", b"1e-", b"1.5x", b" 1", b"1 ", b"1 .5",
                 b"1_0", b"1..2", b"1.2.3", b"--1", b"+-1", b"1e5.0", b"1e5e5", b"1e 5", b"0x10", b"1,5", b"1d5",
                 b"1\x00", b"\x001", b"1\x805", b"\xd9\xa1", b"in", b"infx", b"nanx", b"1f", b"1.5\n"]
FLOAT_SPECIALS = [b"inf", b"-inf", b"Infinity", b"-INFINITY", b"nan", b"NaN", b"-nan"]


def int_corpus(typ):
    """(valid rows, host-parser rows, rejected rows) of string -> typ, classified by the oracle"""
    lo, hi = int_range(typ)
    signed = lo < 0
    rows = [str(v).encode() for v in (lo - 1, lo, lo + 1, -1, 0, 1, hi - 1, hi, hi + 1)]
    rows += [b"-0", b"-00", b"007", b"0" * 25 + b"7", b"-" + b"0" * 25 + b"8", b"0" * 25 + str(hi).encode(),
             b"-" + b"0" * 25 + str(-lo).encode(), b"0" * 25,
             b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809",
             b"18446744073709551616", b"99999999999999999999", b"-99999999999999999999",
             b"-", b"--1", b"-+1", b"+1", b"+0", b"1-", b"", b" 1", b"1 ", b"1_0", b"1.0", b"1e2", b"1\n",
             b"1\x002", b"\x00", b"1\x80", b"\xff", b"\xd9\xa1", b"12a", b"a",
             b"0x", b"0X1f", b"-0x1", b"0xFF", b"0x7f", b"0xg", b"00x1"]
    kinds = [parse_int(r, lo, hi, signed) for r in rows]
    pick = lambda want: tuple(r for r, k in zip(rows, kinds) if want(k))  # noqa: E731
    return pick(lambda k: isinstance(k, int)), pick(lambda k: k == HOST), pick(lambda k: k == REJECT)


def cycle(rows, n):
    return tuple(rows[i % len(rows)] for i in range(n))


# ---- the comparisons
def expected_float_bits(rows, typ):
    exp = [float_bits(r, FMT[typ]) for r in rows]
    assert REJECT not in exp
    for i, e in enumerate(exp):
        if e == SPECIAL:  # Arrow's host parser defines these
            exp[i] = value_bits(pc.cast(pa.array([rows[i]], pa.binary()).cast(pa.string()), typ))[0]
    return exp


def check_values(got, typ, exp, live, what):
    assert got.type == typ, what
    assert len(got) == len(exp), what
    assert validity(got) == live, what
    bits = value_bits(got)
    bad = [(i, hex(bits[i]), hex(exp[i])) for i in range(len(exp)) if live[i] and bits[i] != exp[i]]
    assert not bad, (what, len(bad), "row, got, want", bad[:8])


def check_float_column(cx, rows, typ, what):
    exp = expected_float_bits(rows, typ)
    for name, arr, live in layouts(rows):
        check_values(astype(cx, arr, typ), typ, exp, live, (what, name))


def int_bits(v, typ):
    return v & ((1 << typ.bit_width) - 1)


def check_int_column(cx, rows, typ, what):
    lo, hi = int_range(typ)
    exp = [int_bits(parse_int(r, lo, hi, lo < 0), typ) for r in rows]
    for name, arr, live in layouts(rows):
        check_values(astype(cx, arr, typ), typ, exp, live, (what, name))


# ---- the oracle itself (CPU only; nothing of the project runs here)
def test_oracle_binary64_equals_python_float():
    """CPython's float() is correctly rounded: it checks the oracle, not the project."""
    rows = f64_clinger() + plain() + sum(f64_division().values(), ())
    for r in rows:
        assert float_bits(r, F64) == struct.unpack("<Q", struct.pack("<d", float(r)))[0], r


def test_oracle_binary32_known_values():
    known = {b"1.559917390346527": 0x3fc7ab5f, b"16777217": 0x4b800000, b"16777219": 0x4b800002,
             b"1.000000059604644775390625": 0x3f800000, b"1.000000178813934326171875": 0x3f800002,
             b"3.4028235e38": 0x7f7fffff, b"3.5e38": 0x7f800000, b"1e-46": 0, b"-1e-46": 0x80000000,
             b"1.4e-45": 1, b"7e-46": 0, b"7.1e-46": 1, b"1.17549435e-38": 0x00800000, b"0.1": 0x3dcccccd,
             str(2 ** 128 - 2 ** 103).encode(): 0x7f800000, str(2 ** 128 - 2 ** 103 - 1).encode(): 0x7f7fffff}
    for r, bits in known.items():
        assert float_bits(r, F32) == bits, r
    # every binary32 pattern that is exactly a decimal of the corpus maps back to itself
    for bits in (1, 0x007fffff, 0x00800000, 0x3f800001, 0x7f7fffff, 0x4b800001):
        v = Fraction(struct.unpack("<f", struct.pack("<I", bits))[0])
        assert round_binary(v, 0, *F32) == bits and round_binary(v, 1, *F32) == bits | 0x80000000


def test_oracle_classifies_the_corpora():
    for rows in (f64_clinger(), plain(), f32_midpoints()[0], f32_midpoints()[1]) + tuple(f64_division().values()):
        assert all(isinstance(parse_decimal(r), tuple) for r in rows)
    assert all(parse_decimal(r) == REJECT for r in FLOAT_REJECTS)
    assert all(parse_decimal(r) == SPECIAL for r in FLOAT_SPECIALS)
    for typ in INT_TYPES:
        valid, host, reject = int_corpus(typ)
        assert len(valid) >= 8 and len(host) >= 5 and len(reject) >= 25
        assert (b"-0" in reject and b"-0x1" in reject) == pa.types.is_unsigned_integer(typ)


def test_plain_f32_column_has_no_midpoint_doubles():
    """No row of the plain corpus, rounded to binary64, is exactly a binary32 midpoint (low 29
    mantissa bits 0x10000000): only such rows need the host parser for float32, so this column
    stays on the device path (test_path_taken)."""
    assert not [r for r in plain() if float_bits(r, F64) & 0x1fffffff == 0x10000000]
    # and the device rows of the midpoint corpus are the opposite case: nearly all of them are
    mids = [r for r in f32_midpoints()[0] if float_bits(r, F64) & 0x1fffffff == 0x10000000]
    assert len(mids) > 500


# ---- Arrow against the oracle (CPU only)
@pytest.mark.parametrize("typ", [pa.float64(), pa.float32()], ids=str)
def test_arrow_float_cast_matches_oracle(typ):
    corpora = [f64_clinger(), plain(), f32_midpoints()[0], f32_midpoints()[1]] + list(f64_division().values())
    for rows in corpora:
        exp = [float_bits(r, FMT[typ]) for r in rows]
        assert value_bits(pc.cast(string_array(rows), typ)) == exp
        assert value_bits(pc.cast(string_array(rows, pa.binary()), typ)) == exp
    for r in FLOAT_REJECTS:
        with pytest.raises(pa.ArrowInvalid):
            pc.cast(string_array([b"1", r]), typ)
    got = pc.cast(string_array(FLOAT_SPECIALS), typ).to_pylist()
    assert [str(g) for g in got] == ["inf", "-inf", "inf", "-inf", "nan", "nan", "nan"]


@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_arrow_int_cast_matches_oracle(typ):
    lo, hi = int_range(typ)
    valid, host, reject = int_corpus(typ)
    exp = [int_bits(parse_int(r, lo, hi, lo < 0), typ) for r in valid]
    assert value_bits(pc.cast(string_array(valid), typ)) == exp
    assert value_bits(pc.cast(string_array(valid, pa.binary()), typ)) == exp
    for r in reject:
        with pytest.raises(pa.ArrowInvalid):
            pc.cast(string_array([b"1", r]), typ)


@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_arrow_int_to_string_matches_oracle(typ):
    vals, nulls = int_values(typ, 257)
    arr = int_array(vals, typ, nulls)
    assert string_cells(pc.cast(arr, pa.string())) == expected_strings(vals, nulls)


# ---- string -> float
def test_f64_clinger_boundary(cx):
    rows = f64_clinger()
    check_float_column(cx, rows, pa.float64(), "whole corpus (host parser)")
    fast = tuple(r for r in rows if fast_path(r))
    assert 50 < len(fast) < len(rows) - 50
    check_float_column(cx, fast, pa.float64(), "fast-path rows")
    for r in rows:  # every row as a column of its own: no row borrows another row's path
        check_values(astype(cx, string_array([r]), pa.float64()), pa.float64(), [float_bits(r, F64)], [True], r)


@pytest.mark.parametrize("form", ["digits", "e-k", "e+k"])
def test_f64_division(cx, form):
    check_float_column(cx, f64_division()[form], pa.float64(), form)


@pytest.mark.parametrize("typ", [pa.float64(), pa.float32()], ids=str)
def test_float_plain(cx, typ):
    check_float_column(cx, plain(), typ, "plain")


@pytest.mark.parametrize("part", ["device", "extra", "all"])
def test_f32_midpoints(cx, part):
    """Fails on the parent commit for part "device": 458 of the 12,002 rows were rounded twice
    (string -> binary64 -> binary32), e.g. "1.559917390346527" gave 0x3fc7ab60 for 0x3fc7ab5f."""
    dev, extra = f32_midpoints()
    check_float_column(cx, {"device": dev, "extra": extra, "all": dev + extra}[part], pa.float32(), part)


def test_f32_division_corpus(cx):
    """the f64 division rows into float32: random rows, here for the fast-path range (1e-22 .. 9e37
    lies inside binary32's normal range, so neither subnormals nor overflow arise on the device)"""
    for form, rows in f64_division().items():
        check_float_column(cx, rows[:4000], pa.float32(), form)


def test_float_specials(cx):
    for typ in (pa.float64(), pa.float32()):
        check_float_column(cx, tuple(FLOAT_SPECIALS) + plain()[:50], typ, "specials")


@pytest.mark.parametrize("n", SIZES)
def test_float_row_counts(cx, n):
    for typ in (pa.float64(), pa.float32()):
        check_float_column(cx, plain()[:n], typ, n)


def test_float_big_column(cx):
    """one full grid and a ragged tail: the grid-stride loop runs twice"""
    rows = cycle(plain()[:4099], BIG)
    arr = string_array(rows, nulls=frozenset(range(5, BIG, 1001)))
    live = [i % 1001 != 5 for i in range(BIG)]
    check_values(astype(cx, arr, pa.float64()), pa.float64(), expected_float_bits(rows, pa.float64()), live, "big")


# ---- string -> integer
@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_int_valid_rows(cx, typ):
    valid, _, _ = int_corpus(typ)
    check_int_column(cx, valid, typ, "valid")
    for n in SIZES:
        check_int_column(cx, cycle(valid, n), typ, n)


@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_int_hex_rows_follow_arrow(cx, typ):
    valid, host, _ = int_corpus(typ)
    for r in host:
        arr = string_array(valid[:5] + (r,))
        assert device_cast(cx, arr, typ) is None, r
        try:
            want = pc.cast(arr, typ)
        except pa.ArrowInvalid:
            with pytest.raises(pa.ArrowInvalid):
                astype(cx, arr, typ)
        else:
            got = astype(cx, arr, typ)
            assert got.type == typ and validity(got) == [True] * 6 and value_bits(got) == value_bits(want), r


# ---- rejects
def check_rejects(cx, rejects, valid, typ):
    base = cycle(valid, 1000)
    for r in rejects:
        for pos in (0, 300, 999):
            rows = base[:pos] + (r,) + base[pos + 1:]
            with pytest.raises(pa.ArrowInvalid):
                astype(cx, string_array(rows), typ)
                pytest.fail("%r accepted as %s at row %d" % (r, typ, pos))
    # the same bytes under a null are never read
    for r in rejects:
        for pos in (0, 300, 999):
            arr = string_array(base[:pos] + (r,) + base[pos + 1:], nulls=frozenset([pos]), keep=True)
            got = astype(cx, arr, typ)
            assert got.type == typ and validity(got) == [i != pos for i in range(1000)], (r, pos)


@pytest.mark.parametrize("typ", [pa.float64(), pa.float32()], ids=str)
def test_float_rejects(cx, typ):
    check_rejects(cx, FLOAT_REJECTS, plain()[:1000], typ)


@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_int_rejects(cx, typ):
    """Fails on the parent commit for uint8 / uint16 / uint32: "-0" and "-00" (and "-000...08"
    only by its range) parsed as 0 where Arrow says "Failed to parse string: '-0'"."""
    valid, _, reject = int_corpus(typ)
    check_rejects(cx, reject, valid, typ)


# ---- paths
def host_rows(typ):
    return (b"1e23",) if typ == pa.float64() else (b"1e23", b"inf")


def device_float_columns():
    dev, _ = f32_midpoints()
    cols = [("plain", plain(), pa.float64()), ("plain", plain(), pa.float32()), ("midpoints", dev, pa.float32()),
            ("clinger", tuple(r for r in f64_clinger() if fast_path(r)), pa.float64())]
    for form, rows in f64_division().items():
        cols += [(form, rows, pa.float64()), (form, rows[:4000], pa.float32())]
    return cols


def test_float_path_independence(cx):
    """A row's bits do not depend on which parser its column went to.  Fails on the parent commit
    for float32 (midpoints: 458 rows differ; the double-rounded device result against Arrow's)."""
    for what, rows, typ in device_float_columns():
        alone = astype(cx, string_array(rows), typ)
        extra = host_rows(typ)
        assert device_cast(cx, string_array(rows + extra), typ) is None
        mixed = astype(cx, string_array(rows + extra), typ)
        a, m = value_bits(alone), value_bits(mixed)
        bad = [(i, rows[i], hex(a[i]), hex(m[i])) for i in range(len(rows)) if a[i] != m[i]]
        assert not bad, (what, str(typ), len(bad), "row, string, alone, beside a host row", bad[:8])
        assert m[len(rows):] == expected_float_bits(extra, typ)


def test_path_taken(cx):
    """The device parser, not the host's, converts the columns it is meant to convert -- a condition
    on the path, not a measurement -- and hands the others over."""
    for form, rows in f64_division().items():
        assert device_cast(cx, string_array(rows), pa.float64()) is not None, form
    for typ in (pa.float64(), pa.float32()):
        assert device_cast(cx, string_array(plain()), typ) is not None, typ
        assert device_cast(cx, string_array(plain(), nulls=frozenset(range(3, 20000, 7))), typ) is not None, typ
    for typ in INT_TYPES:
        assert device_cast(cx, string_array(int_corpus(typ)[0]), typ) is not None, typ
    some = plain()[:300]
    for typ in (pa.float64(), pa.float32()):
        for r in (b"inf", b"nan", b"-Infinity", b"12345678901234567890", b"1e23", b"1e-23", b"1.5e24",
                  b"0." + b"0" * 22 + b"1", b"9007199254740993"):
            assert device_cast(cx, string_array(some + (r,)), typ) is None, (typ, r)
        # ... but not for bytes under a null
        assert device_cast(cx, string_array(some + (b"inf",), nulls=frozenset([300]), keep=True), typ) is not None
    # a double that is exactly a binary32 midpoint goes to the host for float32 only
    assert device_cast(cx, string_array(some + (b"16777217",)), pa.float32()) is None
    assert device_cast(cx, string_array(some + (b"16777217",)), pa.float64()) is not None


# ---- integer -> string
def int_values(typ, n):
    """(values, null rows): +-10^k and +-(10^k - 1) for every k the type holds, the extrema and 0,
    cycled to n rows; the first and the last row are null (over the extrema as their values)"""
    lo, hi = int_range(typ)
    base = [0, lo, hi]
    k = 0
    while 10 ** k <= hi:
        base += [10 ** k, 10 ** k - 1] + ([-10 ** k, -(10 ** k - 1)] if lo < 0 else [])
        k += 1
    assert all(lo <= v <= hi for v in base)
    vals = [base[(i + 1) % len(base)] for i in range(n)]
    return vals, frozenset([0, n - 1]) if n else frozenset()


def int_array(vals, typ, nulls):
    n = len(vals)
    w = typ.bit_width // 8
    data = b"".join(int_bits(v, typ).to_bytes(w, "little") for v in vals)
    bm = bytearray((n + 7) // 8)
    for i in range(n):
        if i not in nulls:
            bm[i >> 3] |= 1 << (i & 7)
    return pa.Array.from_buffers(typ, n, [pa.py_buffer(bytes(bm)), pa.py_buffer(data)], null_count=len(nulls))


def expected_strings(vals, nulls):
    cells = [b"" if i in nulls else int_to_str(v) for i, v in enumerate(vals)]
    offs = [0]
    for c in cells:
        offs.append(offs[-1] + len(c))
    return offs, b"".join(cells)


def check_int_to_string(cx, typ, n):
    vals, nulls = int_values(typ, n)
    arr = int_array(vals, typ, nulls)
    got = astype(cx, arr, pa.string())
    assert got.type == pa.string()
    assert validity(got) == [i not in nulls for i in range(n)]
    assert string_cells(got) == expected_strings(vals, nulls)
    if n > 4:  # a slice with a non-zero offset of the same array
        got = astype(cx, arr.slice(2, n - 2), pa.string())
        assert validity(got) == [True] * (n - 3) + [False]
        assert string_cells(got) == expected_strings(vals[2:], frozenset([n - 3]))


@pytest.mark.parametrize("typ", INT_TYPES, ids=str)
def test_int_to_string(cx, typ):
    for n in SIZES + [2, 77]:
        check_int_to_string(cx, typ, n)


def test_int_to_string_big_column(cx):
    check_int_to_string(cx, pa.int32(), BIG)
