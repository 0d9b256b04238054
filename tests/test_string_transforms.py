"""String transforms on a CPU context (docs/semantics.md "String transforms"): slice, strip, case, concat
and replace of string / binary columns against the pure-Python oracle of strxform_utils.py, which is
itself held to pyarrow.compute on valid UTF-8; the Python surface (`.str`, `+`, the Arrow engine, the
Unicode fallback of upper / lower) and the argument errors.  All comparisons are exact.
"""
import operator

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import strpred_utils as U
import strxform_utils as X
from cylon_amd import DataFrame, Table
from cylon_amd._lib import C
from cylon_amd.data import compute

TEXT = ["", "a", "ab", "abc", "abcab", "  ab  ", "\tab\n", "ab ab", "abab", "aab", "ba", "AbC", "xABab", " ", "\n\v\f\r",
        "é", "日本", "日本語", "aé日𝄞", "𝄞", "éa", "abé", "éab", " é ", "ab" * 40, "c" * 70 + "ab", "aaaa", "bab", None]


def rows_of(values):
    return [U.as_bytes(v) for v in values]


def rand_rows(rng, n, lo=0, hi=12, null_every=0, alphabet=b"abc"):
    lens = rng.integers(lo, hi + 1, n)
    rows = [bytes(rng.choice(list(alphabet), int(k)).astype(np.uint8)) for k in lens]
    if null_every:
        for i in range(null_every // 2, n, null_every):
            rows[i] = None
    return rows


@pytest.fixture(scope="module")
def text(ctx):
    arr = pa.array(TEXT, pa.string())
    return Table(pa.table({"s": arr}), ctx), rows_of(TEXT), arr


def test_oracle_against_arrow(text):
    """The oracle itself, on valid UTF-8, against the Arrow kernels the semantics name."""
    _, rows, arr = text
    barr = arr.cast(pa.binary())
    for start, stop in X.SLICES + [(1, 4), (-2, -1), (3, None)]:
        assert X.o_slice(rows, start, stop) == rows_of(pc.utf8_slice_codeunits(arr, start=start or 0, stop=stop).to_pylist())
        assert X.o_slice(rows, start, stop, utf8=False) == pc.binary_slice(barr, start=start or 0, stop=stop).to_pylist()
    for how, fn in (("strip", pc.utf8_trim), ("lstrip", pc.utf8_ltrim), ("rstrip", pc.utf8_rtrim)):
        for cs in ("ab", " ", "a\n"):
            assert X.o_strip(rows, how, cs.encode()) == rows_of(fn(arr, characters=cs).to_pylist())
    assert X.o_strip(rows, "strip") == rows_of(pc.ascii_trim_whitespace(arr).to_pylist())
    assert X.o_strip(rows, "lstrip") == rows_of(pc.ascii_ltrim_whitespace(arr).to_pylist())
    assert X.o_strip(rows, "rstrip") == rows_of(pc.ascii_rtrim_whitespace(arr).to_pylist())
    assert X.o_case(rows, True) == rows_of(pc.ascii_upper(arr).to_pylist())
    assert X.o_case(rows, False) == rows_of(pc.ascii_lower(arr).to_pylist())
    other = TEXT[1:] + TEXT[:1]
    other[4] = None
    assert X.o_concat(rows, rows_of(other), b"-") == rows_of(
        pc.binary_join_element_wise(arr, pa.array(other, pa.string()), "-").to_pylist())
    assert X.o_concat(rows, b"x") == rows_of(pc.binary_join_element_wise(arr, "x", "").to_pylist())
    for pat, repl in (("ab", ""), ("ab", "x"), ("ab", "abcabc"), ("a", "aaaa"), ("aa", "a"), ("é", "e")):
        for count in (-1, 1, 2):
            assert X.o_replace(rows, pat.encode(), repl.encode(), count) == rows_of(
                pc.replace_substring(arr, pattern=pat, replacement=repl,
                                     max_replacements=None if count < 0 else count).to_pylist())


@pytest.mark.parametrize("binary", [False, True])
def test_battery_text(ctx, binary):
    rows = rows_of(TEXT)
    other = rows[3:] + rows[:3]
    other[7] = None
    X.battery(ctx, rows, other=other, binary=binary)
    X.battery(ctx, rows, other=other, binary=binary, pat=b"a", replacements=[b"aaaa", b""],
              slices=[(1, 4), (-2, -1), (3, None), (0, 0), (None, None)], funcs=("slice", "replace"))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(200 + n)
    X.battery(ctx, rand_rows(rng, n, null_every=7), other=rand_rows(rng, n, null_every=5))
    X.battery(ctx, rand_rows(rng, n), other=rand_rows(rng, n, 0, 3))  # no validity arrays


def test_utf8_units_and_malformed(ctx):
    """A slice boundary inside every character position of 1- to 4-byte characters; malformed cells
    follow the operational rule (a unit = one byte and the continuation bytes after it)."""
    cell = "aé日𝄞b".encode()
    rows = [cell, cell[::-1], b"\x80\x80\x80", b"a\xe6", b"\xe6\x97", b"\x80a\x80", "日本語".encode(), b"", None,
            " é ".encode(), " ab ".encode(), "abéab".encode()]
    slices = [(i, j) for i in range(-6, 7) for j in (None, -5, -1, 0, 2, 4, 6)]
    X.battery(ctx, rows, slices=slices, garbage=cell)
    X.battery(ctx, rows, slices=slices, garbage=cell, binary=True)


def test_nulls_and_validity(ctx):
    rows = [b" ab ", None, b"AB", b"", None, b"abab"] * 3
    other = [b"x", b"y", None, b"", None, b"ab"] * 3
    X.battery(ctx, rows, other=other)
    col = U.build_column(ctx, rows, garbage=X.GARBAGE)
    # a null scalar: every row is null, and a validity array comes out
    null = U.build_column(ctx, [None], garbage=b"zz")
    assert X.read(C.string_concat(col, null), True) == [None] * len(rows)
    assert X.read(C.string_concat(null, col, b"-"), True) == [None] * len(rows)
    dense = U.build_column(ctx, [b"a", b"b"])
    assert X.read(C.string_concat(dense, null), True) == [None, None]
    # no validity array in, none out; a valid scalar with a validity array gives one
    assert X.read(C.string_concat(dense, dense), False) == [b"aa", b"bb"]
    one = U.build_column(ctx, [b"q"], force_validity=True)
    assert X.read(C.string_concat(dense, one), True) == [b"aq", b"bq"]
    assert X.read(C.string_concat(one, one), True) == [b"qq"]
    # the non-ASCII flag: set by one byte in the last row, clear when that byte sits under a null row
    rows = [b"ab", b"CD", b"e\xc3\xa9"]
    for force in (False, True):
        res, flag = C.string_case(U.build_column(ctx, rows, force_validity=force), True)
        assert flag and X.read(res, force) == [b"AB", b"CD", b"E\xc3\xa9"]
    res, flag = C.string_case(U.build_column(ctx, rows[:2] + [None], garbage=b"e\xc3\xa9"), True)
    assert not flag and X.read(res, True) == [b"AB", b"CD", None]


def test_layouts(ctx):
    """Zero rows, a slice of a longer table whose neighbours would match, offsets[0] != 0, and the
    output of one transform fed into another and into the predicates."""
    empty = U.build_column(ctx, [])
    for got in (C.string_slice(empty, 0, 3), C.string_strip(empty), C.string_case(empty, True)[0],
                C.string_concat(empty, U.build_column(ctx, [b"x"])), C.string_replace(empty, b"a", b"b")):
        assert X.read(got, False, 0) == []
    rng = np.random.default_rng(4)
    rows = rand_rows(rng, 300, 0, 9, null_every=6, alphabet=b"ab AB")
    t = U.sliced(ctx, rows, 77, 377, pad=b" abAB ", garbage=X.GARBAGE, lead=3)
    X.battery(ctx, rows, col=t.native.column(0), other=rand_rows(rng, 300, 0, 4, null_every=11))
    # a column whose offsets do not begin at 0 (built by hand: the engine's own slices rebase them)
    full = U.build_column(ctx, [b" abAB "] * 5 + rows, garbage=X.GARBAGE, lead=1)
    part = C.Column("s", full.type, len(rows), full.data, full.offsets[5:].clone(), full.validity[5:].clone())
    X.battery(ctx, rows, col=part)
    dense = [r or b"" for r in rows]
    full = U.build_column(ctx, [b" abAB "] * 5 + dense, lead=1)
    X.battery(ctx, dense, col=C.Column("s", full.type, len(rows), full.data, full.offsets[5:].clone(), None))
    # chained
    col = U.build_column(ctx, rows, garbage=X.GARBAGE)
    step = C.string_replace(C.string_strip(C.string_case(col, False)[0]), b"a", b"bb")
    want = X.o_replace(X.o_strip(X.o_case(rows, False), "strip"), b"a", b"bb")
    assert X.read(step, True) == want
    assert U.col_result(C.string_match(step, U.KIND["contains"], b"bbb"))[0] == U.o_match(want, "contains", b"bbb")
    assert U.col_result(C.string_length(step, 1))[0] == U.o_length(want, "chars")


def test_argument_errors(ctx):
    s = U.build_column(ctx, [b"a", b"b"])
    b = U.build_column(ctx, [b"a", b"b"], binary=True)
    num = Table(pa.table({"x": [1, 2]}), ctx).native.column(0)
    limit = C.string_max_pattern_bytes

    def code_of(fn):
        with pytest.raises(C.CylonError) as e:
            fn()
        return e.value.args[1]
    type_error = code_of(lambda: C.string_match(num, 0, b"a"))
    for fn in (lambda: C.string_slice(num, 0, 1), lambda: C.string_strip(num), lambda: C.string_case(num, True),
               lambda: C.string_concat(num, s), lambda: C.string_concat(s, num), lambda: C.string_concat(s, b),
               lambda: C.string_replace(num, b"a", b"b")):
        assert code_of(fn) == type_error
    invalid = code_of(lambda: C.string_compare(s, U.build_column(ctx, [b"a"] * 3), 0))
    assert invalid != type_error
    assert code_of(lambda: C.string_replace(s, b"", b"x")) == invalid  # the empty pattern
    assert code_of(lambda: C.string_replace(s, b"a" * (limit + 1), b"x")) == invalid
    assert code_of(lambda: C.string_replace(s, b"a", b"x" * (limit + 1))) == invalid
    assert code_of(lambda: C.string_concat(s, s, b"-" * (limit + 1))) == invalid
    assert code_of(lambda: C.string_concat(s, U.build_column(ctx, [b"a"] * 3))) == invalid  # lengths
    assert code_of(lambda: C.string_strip(s, 3, "é".encode())) == invalid  # a non-ASCII set on a STRING column
    assert code_of(lambda: C.string_strip(s, 0)) == invalid
    # the limits themselves are accepted; a non-ASCII set on a BINARY column too
    assert X.read(C.string_replace(s, b"a" * limit, b"x" * limit)) == [b"a", b"b"]
    assert X.read(C.string_concat(s, s, b"-" * limit))[0] == b"a" + b"-" * limit + b"a"
    assert X.read(C.string_strip(U.build_column(ctx, [b"\xffa\xff"], binary=True), 3, b"\xff")) == [b"a"]
    assert X.read(C.string_replace(s, b"a", b"x", 0)) == [b"a", b"b"]  # max_replacements == 0 copies


def test_str_accessor_and_add(ctx):
    vals = [" Oslo ", "Ber-gen", None, "Ålesund", "", "os-lo-"]
    rows = rows_of(vals)
    for wrap in (lambda x: x, DataFrame):
        t = wrap(Table(pa.table({"city": vals, "n": [1, 2, 3, 4, 5, 6]}), ctx))
        table = (lambda r: r.to_table()) if wrap is DataFrame else (lambda r: r)
        s = t["city"].str
        assert isinstance(s.strip(), type(t))
        assert X.result(table(s.slice(0, 3))) == X.o_slice(rows, 0, 3)
        assert X.result(table(s.slice(stop=-1))) == X.o_slice(rows, None, -1)
        assert X.result(table(s[1:4])) == X.o_slice(rows, 1, 4)
        assert X.result(table(s[-3:])) == X.o_slice(rows, -3, None)
        assert X.result(table(s.strip())) == X.o_strip(rows, "strip")
        assert X.result(table(s.lstrip())) == X.o_strip(rows, "lstrip")
        assert X.result(table(s.rstrip("-o"))) == X.o_strip(rows, "rstrip", b"-o")
        assert X.result(table(s.replace("-", ""))) == X.o_replace(rows, b"-", b"")
        assert X.result(table(s.replace("-", "+", n=1))) == X.o_replace(rows, b"-", b"+", 1)
        assert X.result(table(s.replace("-", "+", regex=False))) == X.o_replace(rows, b"-", b"+")
        assert X.result(table(s.cat("!"))) == X.o_concat(rows, b"!")
        assert X.result(table(s.cat("!", sep="_"))) == X.o_concat(rows, b"!", b"_")
        assert X.result(table(s.cat(t["city"], sep="/"))) == X.o_concat(rows, rows, b"/")
        assert X.result(table(t["city"] + "x")) == X.o_concat(rows, b"x")
        assert X.result(table(t["city"] + "_" + t["city"])) == X.o_concat(X.o_concat(rows, b"_"), rows)
        assert table(s.upper()).to_pydict()["city"] == [None if v is None else v.upper() for v in vals]
        assert table(s.lower()).to_pydict()["city"] == [None if v is None else v.lower() for v in vals]
        with pytest.raises(NotImplementedError):
            s.replace("-", "", regex=True)
        with pytest.raises(NotImplementedError):
            s[::2]
        with pytest.raises(TypeError):
            t["n"].str.strip()
        with pytest.raises(TypeError):
            t["n"].str.upper()
    t = Table(pa.table({"city": vals}), ctx)
    with pytest.raises(C.CylonError):
        t.str.replace("", "x")
    with pytest.raises(TypeError):
        compute.str_concat(t, 5)
    assert (t + "x").column_names == ["city"] and (t + "x").native.column(0).type.type == C.Type.STRING
    # numbers still add as numbers
    assert (Table(pa.table({"n": [1, 2]}), ctx) + 1).to_pydict() == {"n": [2, 3]}


def test_unicode_case_fallback(ctx, monkeypatch):
    """upper / lower: all-ASCII data stays on the engine; a non-ASCII byte sends a STRING column to
    Arrow's utf8_upper / utf8_lower unless ascii_only; a BINARY column always maps ASCII only."""
    called = []
    real = compute._arrow_col
    monkeypatch.setattr(compute, "_arrow_col", lambda c: (called.append(1), real(c))[1])
    plain = Table(pa.table({"s": ["abC", None, "x y"]}), ctx)
    assert compute.str_upper(plain).to_pydict() == {"s": ["ABC", None, "X Y"]}
    assert compute.str_lower(plain).to_pydict() == {"s": ["abc", None, "x y"]}
    assert not called
    vals = ["é", "Straße", None, "abc", "ÉCOLE"]
    t = Table(pa.table({"s": vals}), ctx)
    got = compute.str_upper(t).to_pydict()["s"]
    assert got == pc.utf8_upper(pa.array(vals)).to_pylist() and got[0] == "É" and got[4] == "ÉCOLE"
    assert compute.str_lower(t).to_pydict() == {"s": ["é", "straße", None, "abc", "école"]}
    assert len(called) == 2
    assert compute.str_upper(t, ascii_only=True).to_pydict() == {"s": ["é", "STRAßE", None, "ABC", "ÉCOLE"]}
    assert len(called) == 2
    tb = Table(pa.table({"s": pa.array([b"\xc3\xa9a", None], pa.binary())}), ctx)
    assert X.result(compute.str_upper(tb)) == [b"\xc3\xa9A", None]
    assert len(called) == 2


def test_arrow_engine_and_routing(ctx, text, monkeypatch):
    """compute_engine="arrow" gives equal values through Arrow's host kernels; a non-ASCII strip set and
    an over-long literal go there too; nothing else does."""
    t, rows, arr = text
    tb = U.build_table(ctx, rows, binary=True)
    called = []
    real = compute._arrow_col
    monkeypatch.setattr(compute, "_arrow_col", lambda c: (called.append(1), real(c))[1])
    o = Table(pa.table({"o": pa.array(TEXT[2:] + TEXT[:2], pa.string())}), ctx)
    calls = [lambda x, **k: compute.str_slice(x, 1, -1, **k), lambda x, **k: compute.str_slice(x, -4, None, **k),
             lambda x, **k: compute.str_strip(x, **k), lambda x, **k: compute.str_lstrip(x, "ab", **k),
             lambda x, **k: compute.str_rstrip(x, " b", **k), lambda x, **k: compute.str_upper(x, **k),
             lambda x, **k: compute.str_lower(x, ascii_only=True, **k), lambda x, **k: compute.str_concat(x, "zz", **k),
             lambda x, **k: compute.str_concat(x, "zz", sep="-", **k), lambda x, **k: compute.str_concat(x, None, **k),
             lambda x, **k: compute.str_replace(x, "ab", "xyz", **k), lambda x, **k: compute.str_replace(x, "a", "", 1, **k)]
    for x in (t, tb):
        for fn in calls:
            n = len(called)
            dev = X.result(fn(x))
            unicode_case = fn is calls[5] and x is t  # the Unicode fallback of upper
            assert len(called) == n + (1 if unicode_case else 0)
            assert X.result(fn(x, engine="arrow")) == dev
            assert len(called) > n
    assert X.result(compute.str_concat(t, o, engine="arrow")) == X.result(compute.str_concat(t, o)) == \
        X.o_concat(rows, rows[2:] + rows[:2])
    # what the device path refuses
    n = len(called)
    uni = Table(pa.table({"s": ["ééabé", "é", None, "abc"]}), ctx)
    assert uni.str.strip("é").to_pydict() == {"s": ["ab", "", None, "abc"]}
    assert len(called) == n + 1
    long = "ab" * (C.string_max_pattern_bytes // 2 + 1)
    big = Table(pa.table({"s": [long + "c", "x", None]}), ctx)
    assert X.result(compute.str_replace(big, long, "y")) == [b"yc", b"x", None]
    assert X.result(compute.str_replace(big, "x", long)) == [long.encode() + b"c", long.encode(), None]
    assert X.result(compute.str_concat(big, "q", sep=long)) == X.o_concat(rows_of([long + "c", "x", None]), b"q", long.encode())
    assert len(called) == n + 5  # strip 1, replace 1 + 1, concat 2 (both operands)
    # a column past 2 GiB reaches Arrow with 64-bit offsets: the join's three arguments get one type
    c = t.native.column(0)
    for ta, tb in ((pa.large_string(), pa.string()), (pa.string(), pa.large_string()), (pa.large_string(),) * 2):
        got = compute._arrow_concat(c, pa.array(["a", None], ta), pa.array(["b", "c"], tb), b"-")
        assert got.to_pylist() == ["a-b", None]
    # the engine of the context's config
    n = len(called)
    assert compute.binary_op(t, "x", operator.add).native.column(0).type.type == C.Type.STRING
    assert len(called) == n


def test_sweep_against_oracle(ctx):
    rng = np.random.default_rng(17)
    rows = rand_rows(rng, 2000, 0, 40, null_every=13, alphabet=b"abcAB \t")
    other = rand_rows(rng, 2000, 0, 40, null_every=17)
    X.battery(ctx, rows, other=other)
