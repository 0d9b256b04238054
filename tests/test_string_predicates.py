"""String predicates on a CPU context (docs/semantics.md "String predicates"): comparison, starts_with
/ ends_with / contains, LIKE and length of string / binary columns against the pure-Python oracle of
strpred_utils.py, which is itself held to pyarrow.compute on valid UTF-8.  All comparisons are exact.
"""
import operator

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import strpred_utils as U
from cylon_amd import DataFrame, Table
from cylon_amd._lib import C
from cylon_amd.data import compute

TEXT = ["", "a", "ab", "abc", "abcab", "b", "bc", "cab", "a%b", "a_b", "a\\b", "axb", "axxbyc", "abc\n", "\n",
        "é", "日本", "日本語", "aé日𝄞", "𝄞", "éa", "xaé", "%", "_", "ab" * 40, "c" * 70 + "ab", None]
PATTERNS = ["", "a", "ab", "bc", "abc", "c", "é", "日", "本", "𝄞", "ab" * 41, "\n", "%", "_"]
LIKES = ["", "%", "%%", "_", "__", "___", "_%_", "a%b%c", "%__", "a%", "%b", "%ab%", "a_c", "a\\%b", "a\\_b",
         "a\\\\b", "%\\%%", "%é", "é%", "_本", "日%", "%\n", "_%", "%_", "a%%b", "%a%b%", "__%__", "%c%ab"]


def rows_of(values):
    return [U.as_bytes(v) for v in values]


def arrow_list(arr):
    return arr.to_pylist()


@pytest.fixture(scope="module")
def text(ctx):
    return Table(pa.table({"s": pa.array(TEXT, pa.string())}), ctx), rows_of(TEXT), pa.array(TEXT, pa.string())


@pytest.mark.parametrize("op", list(U.CMP_OPS))
def test_compare_scalar_and_column(ctx, text, op):
    t, rows, arr = text
    fn = {"eq": pc.equal, "ne": pc.not_equal, "lt": pc.less, "le": pc.less_equal, "gt": pc.greater,
          "ge": pc.greater_equal}[op]
    for s in ["", "ab", "abc", "abd", "é", "日本", "ab" * 40, "zz"]:
        want = U.o_compare(rows, s.encode(), op)
        assert want == arrow_list(fn(arr, s))  # the oracle against Arrow
        assert U.result(U.CMP_OPS[op](t, s)) == want
    other = TEXT[1:] + TEXT[:1]
    other[5] = None
    orows = rows_of(other)
    want = U.o_compare(rows, orows, op)
    assert want == arrow_list(fn(arr, pa.array(other, pa.string())))
    got = U.CMP_OPS[op](t, Table(pa.table({"o": pa.array(other, pa.string())}), ctx))
    assert U.result(got) == want
    assert got.column_names == ["s"] and got.native.column(0).type.type == C.Type.BOOL


def test_compare_prefix_equal_null_and_binary(ctx):
    """A proper prefix is smaller, equal cells, a null on either side, a null scalar, and unsigned byte
    order on a binary column with 0xff bytes."""
    a = [b"ab", b"abc", b"abc", None, b"x", b"\xff", b"\x7f\xff", b""]
    b = [b"abc", b"ab", b"abc", b"q", None, b"\x7f", b"\xff", b""]
    for binary in (False, True):
        ca, cb = U.build_column(ctx, a, binary=binary), U.build_column(ctx, b, binary=binary, name="o")
        for op, code in U.CMP_CODE.items():
            vals, has_valid = U.col_result(C.string_compare(ca, cb, code))
            assert vals == U.o_compare(a, b, op) and has_valid
            one = U.build_column(ctx, [b"abc"], binary=binary)
            assert U.col_result(C.string_compare(ca, one, code))[0] == U.o_compare(a, b"abc", op)
            null = U.build_column(ctx, [None], binary=binary, garbage=b"abc")
            assert U.col_result(C.string_compare(ca, null, code)) == ([None] * len(a), True)
    typ = pa.binary()
    arr = pa.array(a, typ)
    assert U.o_compare(a, b, "lt") == pc.less(arr, pa.array(b, typ)).to_pylist()
    # no validity array in, none out
    dense = U.build_column(ctx, [b"a", b"b"])
    assert U.col_result(C.string_compare(dense, dense, 0)) == ([True, True], False)
    assert U.col_result(C.string_compare(U.build_column(ctx, [b"a"], force_validity=True), dense.slice(0, 1), 0)) == \
        ([True], True)


@pytest.mark.parametrize("kind,fn", [("starts_with", pc.starts_with), ("ends_with", pc.ends_with),
                                     ("contains", pc.match_substring)])
def test_literal_predicates(ctx, text, kind, fn):
    t, rows, arr = text
    call = {"starts_with": compute.str_starts_with, "ends_with": compute.str_ends_with,
            "contains": compute.str_contains}[kind]
    for p in PATTERNS:
        want = U.o_match(rows, kind, p.encode())
        assert want == arrow_list(fn(arr, p)), p
        assert U.result(call(t, p)) == want, p
    # the empty pattern matches every non-null row, the empty row included; a longer pattern never
    assert U.result(call(t, "")) == [None if r is None else True for r in rows]
    assert U.result(call(t, "q" * 200)) == [None if r is None else False for r in rows]


def test_match_stays_inside_the_row(ctx):
    rows = [b"ab", b"cd"]
    t = U.build_table(ctx, rows)
    assert U.result(t.str.contains("bc")) == [False, False]
    assert U.result(t.str.startswith("abc")) == [False, False]
    assert U.result(t.str.endswith("bcd")) == [False, False]
    assert U.result(t.str.like("%bc%")) == [False, False]
    assert U.result(t.str.like("ab_")) == [False, False]


@pytest.mark.parametrize("pattern", LIKES)
def test_like(ctx, text, pattern):
    t, rows, arr = text
    want = U.o_match(rows, "like", pattern.encode())
    assert want == arrow_list(pc.match_like(arr, pattern))
    assert U.result(compute.str_like(t, pattern)) == want
    # the general matcher on the same pattern: '_%' in front keeps it off the classified kernels
    if not pattern.startswith("_"):
        want2 = U.o_match(rows, "like", b"%" + pattern.encode() + b"_%_")
        assert U.result(compute.str_like(t, "%" + pattern + "_%_")) == want2


def test_like_facts(ctx):
    """The pyarrow facts the semantics quote."""
    vals = ["é", "日本", "", "a%b", "axb", "a", "\n"]
    arr = pa.array(vals)
    t = Table(pa.table({"s": arr}), ctx)
    for pattern, want in [("_", [True, False, False, False, False, True, True]),
                          ("__", [False, True, False, False, False, False, False]),
                          ("", [False, False, True, False, False, False, False]),
                          ("a\\%b", [False, False, False, True, False, False, False])]:
        assert pc.match_like(arr, pattern).to_pylist() == want
        assert U.result(t.str.like(pattern)) == want


def test_like_escapes_oracle_only(ctx):
    """An escape before an ordinary character makes it literal; another escape character."""
    rows = rows_of(["ab", "a\\b", "a%b", "axb", "a!b", "a_b", None])
    t = U.build_table(ctx, rows)
    for pattern, esc in [("a\\b", "\\"), ("\\a\\b", "\\"), ("a!%b", "!"), ("a!!b", "!"), ("a!_b", "!"),
                         ("a\\%b", "!"), ("a!xb", "!")]:
        want = U.o_match(rows, "like", pattern.encode(), esc.encode())
        assert U.result(t.str.like(pattern, escape=esc)) == want, (pattern, esc)
    assert U.result(t.str.like("a!%b", escape="!")) == [False, False, True, False, False, False, None]


def test_malformed_utf8_oracle_only(ctx):
    """Malformed UTF-8 follows the operational rule (a unit = one byte and the continuation bytes
    after it); Arrow is not the yardstick."""
    rows = [b"\x80", b"a\x80", b"a\x80b", b"\xe6\x97", b"\xe6\x97\xa5\xe6", b"\xff\xfe", b"\x80\x80a", b"ab", None]
    t = U.build_table(ctx, rows)
    for pattern in ["_", "__", "a%", "%b", "a_", "_b", "%a%", "a%b", "_%_", "%_", "%"]:
        want = U.o_match(rows, "like", pattern.encode())
        assert U.result(t.str.like(pattern)) == want, pattern
    assert U.result(t.str.len()) == U.o_length(rows, "chars")
    assert U.result(t.str.len_bytes()) == U.o_length(rows, "bytes")
    assert U.result(t.str.contains(b"\x80")) == U.o_match(rows, "contains", b"\x80")
    # binary: a unit is a byte
    tb = U.build_table(ctx, rows, binary=True)
    for pattern in [b"_", b"__", b"\xff_", b"%\x80", b"_%_"]:
        assert U.result(compute.str_like(tb, pattern)) == U.o_match(rows, "like", pattern, utf8=False), pattern
    assert U.result(compute.str_starts_with(tb, b"\xff")) == U.o_match(rows, "starts_with", b"\xff")
    assert U.result(compute.str_length(tb, "bytes")) == U.o_length(rows, "bytes")


def test_oracle_like_forms_agree():
    rows = rows_of([x for x in TEXT if x is not None])
    for pattern in LIKES:
        toks = U.like_tokens(pattern.encode(), b"\\", True)
        for r in rows:
            us = U.units(r, True)
            assert U.like_recursive(tuple(us), tuple(toks)) == U.like_positions(us, toks)


def test_length(ctx, text):
    t, rows, arr = text
    assert U.o_length(rows, "chars") == pc.utf8_length(arr).to_pylist()
    assert U.o_length(rows, "bytes") == pc.binary_length(arr).to_pylist()
    got = compute.str_length(t)
    assert U.result(got) == U.o_length(rows, "chars") and got.native.column(0).type.type == C.Type.INT64
    assert U.result(compute.str_length(t, "bytes")) == U.o_length(rows, "bytes")


def test_layouts_nulls_and_empty(ctx):
    """Zero rows, a slice at an odd row, a zero-copy column that ends at its last byte, and null rows
    whose underlying bytes would match."""
    empty = U.build_table(ctx, [])
    for got in (empty == "a", empty.str.contains("a"), empty.str.like("a%_"), empty.str.len(), empty.str.len_bytes()):
        assert got.row_count == 0 and U.result(got) == []
    rows = [b"xab", None, b"ab", b"", None, b"b"] * 3
    for make in (lambda: U.build_table(ctx, rows, garbage=b"abab", lead=3),
                 lambda: U.sliced(ctx, rows, 3, 3 + len(rows), garbage=b"abab", lead=1)):
        t = make()
        assert U.result(t.str.contains("ab")) == U.o_match(rows, "contains", b"ab")
        assert U.result(t.str.like("%a_")) == U.o_match(rows, "like", b"%a_")
        assert U.result(t.str.like("_%b")) == U.o_match(rows, "like", b"_%b")
        assert U.result(t == "ab") == U.o_compare(rows, b"ab", "eq")
        assert U.result(t.str.len()) == U.o_length(rows, "chars")
        assert U.col_result(t.str.endswith("b").native.column(0))[1]


def test_argument_errors(ctx):
    s = U.build_column(ctx, [b"a", b"b"])
    b = U.build_column(ctx, [b"a", b"b"], binary=True)
    num = Table(pa.table({"x": [1, 2]}), ctx).native.column(0)

    def code_of(fn):
        with pytest.raises(C.CylonError) as e:
            fn()
        return e.value.args[1]
    type_error = code_of(lambda: C.string_compare(num, s, 0))
    assert code_of(lambda: C.string_match(num, 0, b"a")) == type_error
    assert code_of(lambda: C.string_length(num, 0)) == type_error
    assert code_of(lambda: C.string_compare(s, b, 0)) == type_error  # STRING with BINARY
    assert code_of(lambda: C.string_compare(s, num, 0)) == type_error
    assert code_of(lambda: C.string_length(b, 1)) == type_error  # code points of a binary column
    invalid = code_of(lambda: C.string_compare(s, U.build_column(ctx, [b"a"] * 3), 0))  # length
    assert invalid != type_error
    assert code_of(lambda: C.string_match(s, 3, b"ab\\")) == invalid  # trailing lone escape
    assert code_of(lambda: C.string_match(s, 3, b"\\\\\\")) == invalid
    assert code_of(lambda: C.string_match(s, 2, b"a" * (C.string_max_pattern_bytes + 1))) == invalid
    assert code_of(lambda: C.string_match(s, 9, b"a")) == invalid
    assert code_of(lambda: C.string_compare(s, s, 6)) == invalid
    assert code_of(lambda: C.string_length(s, 2)) == invalid
    C.string_match(s, 2, b"a" * C.string_max_pattern_bytes)  # the limit itself is accepted
    t = Table(pa.table({"s": ["a"], "x": [1]}), ctx)
    for fn in (lambda: compute.str_contains(t, "a"), lambda: compute.str_length(t), lambda: t.str.like("a")):
        with pytest.raises(TypeError):
            fn()
    with pytest.raises(TypeError):
        compute.str_length(Table(pa.table({"s": pa.array([b"a"], pa.binary())}), ctx), "chars")
    with pytest.raises(C.CylonError):
        t["s"].str.like("a\\")


def test_str_accessor(ctx):
    vals = ["Oslo", "Bergen", None, "Ålesund", "", "Os"]
    rows = rows_of(vals)
    for wrap in (lambda x: x, DataFrame):
        t = wrap(Table(pa.table({"city": vals, "n": [1, 2, 3, 4, 5, 6]}), ctx))
        s = t["city"].str
        table = (lambda r: r.to_table()) if wrap is DataFrame else (lambda r: r)
        assert isinstance(s.startswith("Os"), type(t))
        assert U.result(table(s.startswith("Os"))) == U.o_match(rows, "starts_with", b"Os")
        assert U.result(table(s.endswith("en"))) == U.o_match(rows, "ends_with", b"en")
        assert U.result(table(s.contains("s"))) == U.o_match(rows, "contains", b"s")
        assert U.result(table(s.contains("s", regex=False))) == U.o_match(rows, "contains", b"s")
        assert U.result(table(s.like("_s%"))) == U.o_match(rows, "like", b"_s%")
        assert U.result(table(s.like("O!%", escape="!"))) == [False] * 2 + [None] + [False] * 3
        assert U.result(table(s.len())) == U.o_length(rows, "chars")
        assert U.result(table(s.len_bytes())) == U.o_length(rows, "bytes")
        with pytest.raises(NotImplementedError):
            s.contains("s", regex=True)
        # a null counts as false in the filter
        assert table(t[t["city"].str.like("%s%")]).to_pydict() == {"city": ["Oslo", "Ålesund", "Os"], "n": [1, 4, 6]}
        assert table(t[t["city"] == "Oslo"]).to_pydict() == {"city": ["Oslo"], "n": [1]}


def test_arrow_fallbacks_same_values(ctx, text, monkeypatch):
    """The Arrow engine and an over-long pattern take Arrow's host kernels, with the same values."""
    t, rows, arr = text
    long = "ab" * (C.string_max_pattern_bytes // 2 + 1)
    big = Table(pa.table({"s": pa.array(TEXT + [long, "x" + long + "y"], pa.string())}), ctx)
    brows = rows_of(TEXT + [long, "x" + long + "y"])
    called = []
    real = compute._arrow_col
    monkeypatch.setattr(compute, "_arrow_col", lambda c: (called.append(1), real(c))[1])
    for kind, fn in [("starts_with", compute.str_starts_with), ("ends_with", compute.str_ends_with),
                     ("contains", compute.str_contains), ("like", compute.str_like)]:
        n = len(called)
        assert U.result(fn(big, long)) == U.o_match(brows, kind, long.encode())
        assert len(called) == n + 1
    assert U.result(compute.str_like(big, "%" + long + "_")) == U.o_match(brows, "like", b"%" + long.encode() + b"_")
    n = len(called)
    for p in ["ab", "%"]:
        assert U.result(compute.str_contains(t, p, engine="arrow")) == U.result(compute.str_contains(t, p))
        assert U.result(compute.str_starts_with(t, p, engine="arrow")) == U.result(compute.str_starts_with(t, p))
        assert U.result(compute.str_ends_with(t, p, engine="arrow")) == U.result(compute.str_ends_with(t, p))
    for p in ["a%b%c", "a\\%b", "_%_", "a!%b"]:
        esc = "!" if "!" in p else "\\"
        assert U.result(compute.str_like(t, p, esc, engine="arrow")) == U.result(compute.str_like(t, p, esc))
    for unit in ("chars", "bytes"):
        got = compute.str_length(t, unit, engine="arrow")
        assert U.result(got) == U.result(compute.str_length(t, unit))
        assert got.native.column(0).type.type == C.Type.INT64
    assert len(called) > n
    with pytest.raises(C.CylonError):
        compute.str_like(t, "ab\\", engine="arrow")
    # comparisons: the device engine does not touch Arrow, the Arrow engine does, same values
    n = len(called)
    dev = compute.binary_op(t, "abc", operator.lt)
    assert len(called) == n
    assert U.result(compute.binary_op(t, "abc", operator.lt, engine="arrow")) == U.result(dev)
    assert len(called) == n + 1


def test_arrow_fallback_binary_bytes_patterns(ctx):
    """A bytes pattern that is no UTF-8 on a BINARY column takes the Arrow fallback (the Arrow engine, or a
    pattern over the limit) as it takes the device path, with the same values."""
    rows = [b"\xffa", b"a\xff", b"\x80\xff\x80", b"a%\xff", b"", None, b"a"]
    t = U.build_table(ctx, rows, binary=True)
    for kind, fn in [("starts_with", compute.str_starts_with), ("ends_with", compute.str_ends_with),
                     ("contains", compute.str_contains)]:
        for p in (b"\xff", b"\x80\xff", b"a"):
            want = U.o_match(rows, kind, p)
            assert U.result(fn(t, p, engine="arrow")) == want
            assert U.result(fn(t, p)) == want
    for p, esc in [(b"\xff%", "\\"), (b"%\xff", "\\"), (b"_\xff_", "\\"), (b"a\\%\xff", "\\"), (b"a!%\xff", "!"),
                   (b"%\xff%", "\\")]:
        want = U.o_match(rows, "like", p, esc.encode(), utf8=False)
        assert U.result(compute.str_like(t, p, esc, engine="arrow")) == want, p
        assert U.result(compute.str_like(t, p, esc)) == want, p
    long = b"\xff" * (C.string_max_pattern_bytes + 1)
    big = U.build_table(ctx, rows + [long, b"a" + long], binary=True)
    brows = rows + [long, b"a" + long]
    assert U.result(compute.str_contains(big, long)) == U.o_match(brows, "contains", long)
    assert U.result(compute.str_like(big, b"_" + long)) == U.o_match(brows, "like", b"_" + long, utf8=False)
