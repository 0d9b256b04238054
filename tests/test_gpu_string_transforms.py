"""String transforms on the device (kernels/strxform.hip) against the pure-Python oracle of
strxform_utils.py: block edges, the boundaries between the LDS-staged path and the long-row path on the
input and on the output side, every destination alignment of a block's flush, nulls on block edges, long
rows, UTF-8, the column layouts the engine produces, a random sweep (also against the CPU context) and
the routing of the Table operators.  All comparisons are exact.

A write block owns 256 rows (128 for concat, whose input tiles are T / 2); T = C.string_tile_bytes().
"""
import numpy as np
import pyarrow as pa
import pytest

import strpred_utils as U
import strxform_utils as X
from cylon_amd import Table
from cylon_amd._lib import C
from cylon_amd.data import compute

pytestmark = pytest.mark.gpu

GARBAGE = X.GARBAGE


def rand_rows(rng, n, lo=0, hi=40, null_every=0, alphabet=b"abc"):
    lens = rng.integers(lo, hi + 1, n)
    rows = [bytes(rng.choice(list(alphabet), int(k)).astype(np.uint8)) for k in lens]
    if null_every:
        for i in range(null_every // 2, n, null_every):
            rows[i] = None
    return rows


def boundary_rows(rng, span, n_first=256, tail_rows=100, alphabet=b"abc "):
    """n_first rows whose bytes add up to exactly `span`, then short rows (a staged block follows)."""
    base = span // n_first
    lens = [base] * n_first
    lens[n_first // 2] += span - base * n_first
    rows = [bytes(rng.choice(list(alphabet), k).astype(np.uint8)) for k in lens]
    assert sum(len(r) for r in rows) == span
    return rows + rand_rows(rng, tail_rows, 0, 20, alphabet=alphabet)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_row_counts(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    X.battery(gpu_ctx, rand_rows(rng, n, 0, 12, null_every=7), other=rand_rows(rng, n, 0, 12, null_every=5))
    X.battery(gpu_ctx, rand_rows(rng, n, 0, 12), other=rand_rows(rng, n, 0, 3))  # no validity arrays


@pytest.mark.parametrize("delta", [0, 1, -1])
def test_input_span_boundary(gpu_ctx, delta):
    """256 rows of exactly T bytes are staged, of T + 1 take the long-row path; a staged block follows in
    the same launch.  For concat (128-row blocks, T / 2 per input) the same at T / 2, on either operand."""
    T = C.string_tile_bytes()
    rng = np.random.default_rng(7 + delta)
    rows = boundary_rows(rng, T + delta)
    X.battery(gpu_ctx, rows, other=rand_rows(rng, len(rows), 0, 3))
    nrows = list(rows)  # nulls on the boundary: the staged copy goes row by row
    nrows[0] = nrows[255] = nrows[256] = None
    lens = [len(r) for r in rows]
    col = U.build_column(gpu_ctx, nrows, garbage=lambda i: b" abAB"[:lens[i]].ljust(lens[i], b"a"), lead=1)
    X.battery(gpu_ctx, nrows, col=col, slices=[(1, -1)], replacements=[b"x"])
    half = boundary_rows(rng, T // 2 + delta, n_first=128)
    short = rand_rows(rng, len(half), 0, 3)
    X.battery(gpu_ctx, half, other=short, funcs=("concat",))
    X.battery(gpu_ctx, short, other=half, funcs=("concat",))


def test_output_span_boundary(gpu_ctx):
    """The input inside the tile, the output on either side of T: 256 rows of 60 bytes (15 360 B) with
    scalars of 3, 4 and 5 bytes give 16 128, 16 384 and 16 640 B; 128 such rows with scalars of 67, 68 and
    69 bytes give T - 128, T and T + 128 B in one concat block.  A replace that expands rows past T, and one
    that shrinks a T + 1 input below T."""
    T = C.string_tile_bytes()
    rng = np.random.default_rng(11)
    rows = [bytes(rng.choice(list(b"abc"), 60).astype(np.uint8)) for _ in range(256)] + rand_rows(rng, 100, 0, 20)
    col = U.build_column(gpu_ctx, rows, lead=5)
    for k in (3, 4, 5, 67, 68, 69):
        s = bytes(rng.choice(list(b"xyz"), k).astype(np.uint8))
        one = U.build_column(gpu_ctx, [s], lead=k)
        assert X.read(C.string_concat(col, one), False) == X.o_concat(rows, s), k
        assert X.read(C.string_concat(one, col), False) == X.o_concat(s, rows), k
        assert X.read(C.string_concat(col, col, s[:9]), False) == X.o_concat(rows, rows, s[:9]), k
    # 256 rows of 24 bytes: how many a's a block holds decides on which side of T its output lies
    for na in (10, 13, 14, 24):  # 6144 + 256 * 3 * na = 13 824, 16 128, 16 896, 24 576
        grow = [(b"a" * na + b"b" * (24 - na)) for _ in range(256)] + rand_rows(rng, 100, 0, 20)
        gcol = U.build_column(gpu_ctx, grow, lead=2)
        assert X.read(C.string_replace(gcol, b"a", b"aaaa"), False) == X.o_replace(grow, b"a", b"aaaa"), na
        assert X.read(C.string_replace(gcol, b"a", b"aaaa", 1), False) == X.o_replace(grow, b"a", b"aaaa", 1), na
    shrink = boundary_rows(rng, T + 1, alphabet=b"ab")
    scol = U.build_column(gpu_ctx, shrink, lead=7)
    for pat, repl in ((b"a", b""), (b"ab", b"a"), (b"b", b"bb")):
        assert X.read(C.string_replace(scol, pat, repl), False) == X.o_replace(shrink, pat, repl), (pat, repl)
    assert X.read(C.string_slice(scol, 1, None), False) == X.o_slice(shrink, 1, None)
    assert X.read(C.string_strip(scol, 3, b"a"), False) == X.o_strip(shrink, "strip", b"a")


def test_destination_alignment(gpu_ctx):
    """A first row of 0 ... 15 bytes in front of a fixed 300-row body moves the output start of every
    later block through all residues modulo 16; then 257 rows whose second block's output is 1 ... 15
    bytes: a head only, no vector group."""
    rng = np.random.default_rng(21)
    body = rand_rows(rng, 300, 3, 12, alphabet=b"abAB ")
    other = rand_rows(rng, 301, 0, 5)
    for k in range(16):
        rows = [b"abABabABabABabA"[:k]] + body
        X.battery(gpu_ctx, rows, other=other, slices=[(0, None), (1, -1)], replacements=[b"x", b"abc"],
                  funcs=("slice", "case", "concat", "replace"))
        nrows = list(rows)
        nrows[5] = None  # with a validity array upper / lower take the staged path
        X.battery(gpu_ctx, nrows, slices=[(0, 9)], funcs=("slice", "case", "strip"))
    first = rand_rows(rng, 256, 0, 9, alphabet=b"abAB ")
    for k in (1, 2, 7, 15):
        rows = first + [b"bABabABabABabAB"[:k]]
        X.battery(gpu_ctx, rows, other=[b""] * 257, slices=[(0, None)], replacements=[b"ab"])
        X.battery(gpu_ctx, rows[:3] + [None] + rows[4:], slices=[(0, None)], funcs=("slice", "case"))


def test_nulls_on_block_edges(gpu_ctx):
    rng = np.random.default_rng(31)
    rows = rand_rows(rng, 600, 0, 12, alphabet=b"abAB ")
    other = rand_rows(rng, 600, 0, 12)
    for i in (0, 127, 128, 255, 256, 511, 599):
        rows[i] = None
    for i in (1, 127, 129, 254, 256, 300):
        other[i] = None
    X.battery(gpu_ctx, rows, other=other)
    col = U.build_column(gpu_ctx, rows, garbage=GARBAGE)
    null = U.build_column(gpu_ctx, [None], garbage=b"zz")
    assert X.read(C.string_concat(col, null), True) == [None] * 600
    assert X.read(C.string_concat(null, col, b"-"), True) == [None] * 600
    dense = U.build_column(gpu_ctx, [b"a", b"b"])
    assert X.read(C.string_concat(dense, null), True) == [None, None]
    assert X.read(C.string_concat(dense, U.build_column(gpu_ctx, [b"q"], force_validity=True)), True) == [b"aq", b"bq"]
    assert X.read(C.string_concat(dense, dense), False) == [b"aa", b"bb"]


def test_long_rows(gpu_ctx):
    """One row of 40 000 bytes and one of 100 000 among short ones, for every function: matches that
    begin at lane 62, 63 and 0 of a 64-position step and overlap across steps, whitespace runs longer than
    a step at either end, a row of the strip set only."""
    rng = np.random.default_rng(41)

    def long_row(n):
        r = bytearray(rng.choice(list(b"xyzAB"), n).astype(np.uint8))
        for pos in (62, 63, 64, 64 * 17 + 63, 64 * 300 + 62, 64 * 500, n - 2):
            r[pos:pos + 2] = b"ab"
        r[1000:1006] = b"ababab"
        r[2047:2050] = b"aab"
        return b" \t" * 40 + bytes(r) + b" " * 130

    rows = [b" ab ", long_row(40000), b"", b"xaby", long_row(100000), None, b" " * 300, b"ab" * 5000, b"a" * 70]
    other = [b"q", b"r" * 20000, b"", None, b"ab", b"x", long_row(20000), b"z", b"y" * 90]
    X.battery(gpu_ctx, rows, other=other, garbage=b" ab" * 30, slices=X.SLICES + [(81, -131), (20000, 20010)])
    X.battery(gpu_ctx, rows, binary=True, garbage=b" ab" * 30, funcs=("slice", "strip"), slices=[(-50000, -3), (7, 39999)])


def test_utf8(gpu_ctx):
    """1- to 4-byte characters with a slice boundary at every character position, cells of continuation
    bytes only, a stray lead byte at the end of a cell, strip beside non-ASCII neighbours -- staged, and
    the same in rows longer than the tile."""
    T = C.string_tile_bytes()
    cell = "aé日𝄞b".encode()
    rows = [cell, cell[::-1], b"\x80\x80\x80", b"a\xe6", b"\xe6\x97", b"\x80a\x80", "日本語".encode(), b"", None,
            " é ".encode(), " ab ".encode(), "abéab".encode()]
    slices = [(i, j) for i in range(-6, 7) for j in (None, -5, -1, 0, 2, 4, 6)]
    X.battery(gpu_ctx, rows, slices=slices, garbage=cell)
    big = [cell * (3 * T // len(cell)) + b"z", b"\xc3\xa9" * T, cell, b"", None, b"\x80" * (T + 70), "日本".encode(),
           b" " + "é日".encode() * T + b"\xe6"]
    n_units = 5 * (3 * T // len(cell))
    slices = [(0, 3), (2, None), (-3, None), (None, -1), (5, 2), (-100, 100), (n_units - 1, n_units + 1),
              (63, 65), (64, 128), (-n_units - 1, 1), (1, 2)]
    X.battery(gpu_ctx, big, slices=slices, garbage=cell, funcs=("slice", "strip", "case"))
    # the non-ASCII flag: set by exactly one byte in the last row; clear when that byte sits under a null
    plain = [b"ab"] * 700
    for force in (False, True):
        res, flag = C.string_case(U.build_column(gpu_ctx, plain + [b"e\xc3"], force_validity=force, lead=3), True)
        assert flag and X.read(res, force) == [b"AB"] * 700 + [b"E\xc3"]
        res, flag = C.string_case(U.build_column(gpu_ctx, plain, force_validity=force), False)
        assert not flag
    res, flag = C.string_case(U.build_column(gpu_ctx, plain + [None], garbage=b"e\xc3\xa9"), True)
    assert not flag and X.read(res, True) == [b"AB"] * 700 + [None]


def test_sliced_and_engine_made_columns(gpu_ctx):
    """A Table.slice of a longer table whose neighbours hold matching bytes, a column whose offsets do
    not begin at 0, the output of a transform fed into another transform, into string_match, and into
    join and group-by keys."""
    rng = np.random.default_rng(51)
    rows = rand_rows(rng, 700, 0, 9, null_every=6, alphabet=b"ab AB")
    t = U.sliced(gpu_ctx, rows, 77, 777, pad=b" abAB ", garbage=GARBAGE, lead=3)
    X.battery(gpu_ctx, rows, col=t.native.column(0), other=rand_rows(rng, 700, 0, 4, null_every=11))
    full = U.build_column(gpu_ctx, [b" abAB "] * 5 + rows, garbage=GARBAGE, lead=1)
    part = C.Column("s", full.type, len(rows), full.data, full.offsets[5:].clone(), full.validity[5:].clone())
    X.battery(gpu_ctx, rows, col=part)
    dense = [r or b"" for r in rows]
    full = U.build_column(gpu_ctx, [b" abAB "] * 5 + dense, lead=1)
    X.battery(gpu_ctx, dense, col=C.Column("s", full.type, len(rows), full.data, full.offsets[5:].clone(), None))
    # chained, and into the predicates
    col = U.build_column(gpu_ctx, rows, garbage=GARBAGE)
    step = C.string_replace(C.string_strip(C.string_case(col, False)[0]), b"a", b"bb")
    want = X.o_replace(X.o_strip(X.o_case(rows, False), "strip"), b"a", b"bb")
    assert X.read(step, True) == want
    assert U.col_result(C.string_match(step, U.KIND["contains"], b"bbb"))[0] == U.o_match(want, "contains", b"bbb")
    assert U.col_result(C.string_length(step, 1))[0] == U.o_length(want, "chars")
    # normalised keys: " Ab", "ab ", "AB" all become "ab"
    raw = [(b" ", b"")[i % 2] + k + (b"", b"  ")[i % 3 == 0]
           for i, k in enumerate(rng.choice([b"ab", b"Ab", b"AB", b"ba", b"bA", b"abc", b"B"], 500))]
    keys = X.o_strip(X.o_case(raw, False), "strip")
    kcol = C.string_strip(C.string_case(U.build_column(gpu_ctx, raw, name="k"), False)[0])
    vals = Table(pa.table({"v": np.arange(500)}), gpu_ctx).native.column(0)
    kt = U.table_of(gpu_ctx, [kcol, vals])
    sums = {}
    for k, v in zip(keys, range(500)):
        sums[k.decode()] = sums.get(k.decode(), 0) + v
    g = kt.groupby("k", {"v": "sum"}).to_pydict()
    assert dict(zip(g["k"], [int(x) for x in g[[c for c in g if c != "k"][0]]])) == sums
    right = Table(pa.table({"k": ["ab", "ba", "zz"], "w": [10, 20, 30]}), gpu_ctx)
    j = kt.join(right, "inner", "hash", on=["k"], left_prefix="l_", right_prefix="r_").to_pydict()
    want_w = {"ab": 10, "ba": 20}
    assert sorted(zip(j["l_v"], j["r_w"])) == sorted((v, want_w[k.decode()]) for v, k in enumerate(keys)
                                                      if k.decode() in want_w)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sweep(ctx, gpu_ctx, seed):
    """GPU against the oracle, and GPU against the CPU context."""
    rng = np.random.default_rng(seed)
    rows = rand_rows(rng, 2000, 0, 40, null_every=13, alphabet=b"abcAB \t")
    other = rand_rows(rng, 2000, 0, 40, null_every=17)
    X.battery(gpu_ctx, rows, other=other)
    g, c = U.build_column(gpu_ctx, rows, garbage=GARBAGE, lead=3), U.build_column(ctx, rows, garbage=GARBAGE, lead=3)
    go, co = U.build_column(gpu_ctx, other, lead=2), U.build_column(ctx, other, lead=2)
    for fn in (lambda a, b: C.string_slice(a, 2, -2), lambda a, b: C.string_strip(a, 1, b"ab "),
               lambda a, b: C.string_case(a, True)[0], lambda a, b: C.string_concat(a, b, b"/"),
               lambda a, b: C.string_replace(a, b"ab", b"ba", 2)):
        assert X.read(fn(g, go)) == X.read(fn(c, co))
    assert C.string_case(g, True)[1] == C.string_case(c, True)[1]


def test_routing_stays_on_device(gpu_ctx, monkeypatch):
    """t.str.* and t + "x" on a device table never copy the column to the host, unless the engine is
    "arrow"."""
    rng = np.random.default_rng(3)
    rows, other = rand_rows(rng, 1000, 0, 8, null_every=9, alphabet=b"abAB "), rand_rows(rng, 1000, 0, 8)
    t, o = U.build_table(gpu_ctx, rows, garbage=GARBAGE), U.build_table(gpu_ctx, other)
    real = compute._arrow_col
    calls = []

    def no_host(col):
        raise AssertionError("the column went to the host")
    monkeypatch.setattr(compute, "_arrow_col", no_host)
    assert X.result(t.str.slice(1, 3)) == X.o_slice(rows, 1, 3)
    assert X.result(t.str[-2:]) == X.o_slice(rows, -2, None)
    assert X.result(t.str.strip()) == X.o_strip(rows, "strip")
    assert X.result(t.str.lstrip("a")) == X.o_strip(rows, "lstrip", b"a")
    assert X.result(t.str.rstrip("b ")) == X.o_strip(rows, "rstrip", b"b ")
    assert X.result(t.str.upper()) == X.o_case(rows, True)
    assert X.result(t.str.lower()) == X.o_case(rows, False)
    assert X.result(t.str.replace("ab", "-")) == X.o_replace(rows, b"ab", b"-")
    assert X.result(t.str.cat("x", sep="_")) == X.o_concat(rows, b"x", b"_")
    assert X.result(t.str.cat(o)) == X.o_concat(rows, other)
    assert X.result(t + "x") == X.o_concat(rows, b"x")
    assert X.result(t + o) == X.o_concat(rows, other)
    for res in (t.str.strip(), t.str.upper(), t + "x", t.str.replace("a", "b"), t.str[1:], t.str.cat(o)):
        col = res.native.column(0)
        assert res.device == t.device and col.data.is_cuda and col.offsets.is_cuda
    monkeypatch.setattr(compute, "_arrow_col", lambda c: (calls.append(1), real(c))[1])
    got = compute.str_strip(t, engine="arrow")
    assert calls and X.result(got) == X.o_strip(rows, "strip") and got.native.column(0).data.is_cuda
    n = len(calls)
    uni = U.build_table(gpu_ctx, ["é".encode(), b"ab", None])  # the Unicode fallback of upper / lower
    assert X.result(uni.str.upper()) == ["É".encode(), b"AB", None] and len(calls) == n + 1
