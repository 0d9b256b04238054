"""String predicates on the device (kernels/strmatch.hip) against the pure-Python oracle of
strpred_utils.py: block edges, the boundary between the LDS-staged path and the long-row path, long
rows, the column layouts the engine produces, a random sweep (also against the CPU context) and the
routing of the Table operators.  All comparisons are exact.
"""
import operator

import numpy as np
import pytest

import strpred_utils as U
from cylon_amd._lib import C
from cylon_amd.data import compute

pytestmark = pytest.mark.gpu

GARBAGE = b"abcabca"  # under every null row: it would match most patterns below
NEEDLES = [b"", b"a", b"ab", b"bca", b"cc"]
LIKES = [b"a%", b"%ab", b"%ab%", b"abc", b"", b"%", b"%ab%c", b"_b%", b"%a_", b"a%b%c", b"__", b"%_c_%"]


def rand_rows(rng, n, lo=0, hi=40, null_every=0, alphabet=b"abc"):
    lens = rng.integers(lo, hi + 1, n)
    rows = [bytes(rng.choice(list(alphabet), int(k)).astype(np.uint8)) for k in lens]
    if null_every:
        for i in range(null_every // 2, n, null_every):
            rows[i] = None
    return rows


def battery(ctx, rows, col=None, other=None, ocol=None, binary=False, likes=LIKES, needles=NEEDLES):
    """Every function on one column against the oracle."""
    if col is None:
        col = U.build_column(ctx, rows, binary=binary, garbage=GARBAGE, lead=5)
    utf8 = not binary
    nullable = col.validity is not None
    scalar = U.build_column(ctx, [b"ab"], binary=binary)
    if other is not None and ocol is None:
        ocol = U.build_column(ctx, other, binary=binary, garbage=GARBAGE, lead=9, name="o")
    for op, code in U.CMP_CODE.items():
        got = C.string_compare(col, scalar, code)
        assert U.col_result(got) == (U.o_compare(rows, b"ab", op), nullable), ("scalar", op)
        if other is not None:
            got = C.string_compare(col, ocol, code)
            assert U.col_result(got) == (U.o_compare(rows, other, op), nullable or ocol.validity is not None), op
    for kind in ("starts_with", "ends_with", "contains"):
        for p in needles:
            got = C.string_match(col, U.KIND[kind], p)
            assert U.col_result(got) == (U.o_match(rows, kind, p), nullable), (kind, p)
    for p in likes:
        got = C.string_match(col, U.KIND["like"], p)
        assert U.col_result(got) == (U.o_match(rows, "like", p, utf8=utf8), nullable), ("like", p)
    assert U.col_result(C.string_length(col, 0)) == (U.o_length(rows, "bytes"), nullable)
    if utf8:
        assert U.col_result(C.string_length(col, 1)) == (U.o_length(rows, "chars"), nullable)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_row_counts(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    battery(gpu_ctx, rand_rows(rng, n, 0, 12, null_every=7), other=rand_rows(rng, n, 0, 12, null_every=5))
    battery(gpu_ctx, rand_rows(rng, n, 0, 12), other=rand_rows(rng, n, 0, 3))  # no validity arrays


def boundary_rows(rng, span, n_first=256, tail_rows=100):
    """n_first rows whose bytes add up to exactly `span`, then short rows (a staged block follows)."""
    base = span // n_first
    lens = [base] * n_first
    lens[n_first // 2] += span - base * n_first
    rows = [bytes(rng.choice(list(b"abc"), k).astype(np.uint8)) for k in lens]
    assert sum(len(r) for r in rows) == span
    return rows + rand_rows(rng, tail_rows, 0, 20)


@pytest.mark.parametrize("delta", [0, 1, -1])
def test_path_boundary(gpu_ctx, delta):
    """A 256-row block of exactly T bytes is staged, of T + 1 takes the long-row path; a staged block
    follows in the same launch.  For the column comparison the second column's span decides."""
    T = C.string_tile_bytes()
    rng = np.random.default_rng(7 + delta)
    rows = boundary_rows(rng, T + delta)
    short = [r[:int(k)] for r, k in zip(rows, rng.integers(0, 30, len(rows)))]  # prefixes: span far below T
    short[3], short[300] = rows[3], rows[300]  # and equal cells
    battery(gpu_ctx, rows, other=short, likes=[b"%ab%c", b"_b%", b"a%b%c", b"%cab"], needles=[b"ab", b"bca"])
    battery(gpu_ctx, short, other=rows, likes=[b"%ab%c"], needles=[b"ab"])
    # nulls on the boundary: the staged copy goes row by row
    nrows = list(rows)
    nrows[0] = nrows[255] = nrows[256] = None
    lens = [len(r) for r in rows]
    col = U.build_column(gpu_ctx, nrows, garbage=lambda i: b"a" * lens[i], lead=1)
    battery(gpu_ctx, nrows, col=col, other=short, likes=[b"%ab%c", b"a%"], needles=[b"ab", b"a"])


def test_long_rows(gpu_ctx):
    """Rows of 3 T bytes among short ones: needles of 1, 3 and 65 bytes that begin at lane 62, 63 and 0
    of a 64-position step, a needle that is the row's last bytes, and one that would match only by
    reading into the next row."""
    T = C.string_tile_bytes()
    needles = [b"1", b"234", b"5" + b"6" * 63 + b"7"]
    rows = [b"x", b"", b"xx1"]
    for nd in needles:
        for pos in (64 * 300 + 62, 64 * 17 + 63, 64 * 500):
            r = bytearray(b"x" * (3 * T))
            r[pos:pos + len(nd)] = nd
            rows += [bytes(r), b"x" * 7]
        rows += [b"x" * (3 * T - len(nd)) + nd, b"xyz"]  # the row's last bytes
        rows += [b"x" * (3 * T) + nd[:-1] if len(nd) > 1 else b"x" * (3 * T), nd[-1:] + b"x"]  # across two rows
    rows += [None, b"x" * 100]
    col = U.build_column(gpu_ctx, rows, garbage=b"x" * 70 + b"1234", lead=3)
    for nd in needles:
        for kind in ("contains", "ends_with", "starts_with"):
            got = U.col_result(C.string_match(col, U.KIND[kind], nd))[0]
            assert got == U.o_match(rows, kind, nd), (kind, nd[:3])
    for p in (b"x%234%x_", b"%7", b"%1", b"_%1x%", b"x%", b"%4"):
        assert U.col_result(C.string_match(col, U.KIND["like"], p))[0] == U.o_match(rows, "like", p), p
    assert U.col_result(C.string_length(col, 0))[0] == U.o_length(rows, "bytes")
    assert U.col_result(C.string_length(col, 1))[0] == U.o_length(rows, "chars")
    # column against column: equal long rows, a proper prefix, one differing byte at lane 62 / 63 / 0
    other = list(rows)
    for i, r in enumerate(rows):
        if r is None or len(r) < T:
            continue
        q = bytearray(r)
        if i % 4 == 0:
            q[64 * 200 + (62, 63, 64)[i % 3]] ^= 1
        elif i % 4 == 1:
            q = q[:len(q) - 1 - i]
        elif i % 4 == 2:
            q[-1] ^= 3
        other[i] = bytes(q)
    other[2] = None
    ocol = U.build_column(gpu_ctx, other, garbage=b"x", lead=6)
    for op, code in U.CMP_CODE.items():
        assert U.col_result(C.string_compare(col, ocol, code))[0] == U.o_compare(rows, other, op), op
        assert U.col_result(C.string_compare(ocol, col, code))[0] == U.o_compare(other, rows, op), op
    # a scalar longer than the pattern buffer is compared from global memory
    big = U.build_column(gpu_ctx, [rows[3]])
    assert U.col_result(C.string_compare(col, big, 0))[0] == U.o_compare(rows, rows[3], "eq")
    assert U.col_result(C.string_compare(col, big, 2))[0] == U.o_compare(rows, rows[3], "lt")


def test_long_utf8_rows(gpu_ctx):
    T = C.string_tile_bytes()
    cell = "aé日𝄞".encode()
    rows = [cell * (3 * T // len(cell)) + b"z", b"\xc3\xa9" * T, cell, b"", None, "日本".encode()]
    col = U.build_column(gpu_ctx, rows, garbage=cell, lead=1)
    assert U.col_result(C.string_length(col, 1))[0] == U.o_length(rows, "chars")
    for p in ("%𝄞z".encode(), "_é%".encode(), "%日_a%z".encode(), b"__"):
        assert U.col_result(C.string_match(col, U.KIND["like"], p))[0] == U.o_match(rows, "like", p), p


def test_layouts(gpu_ctx):
    """A table sliced at an odd row, a zero-copy column that ends at its last byte, nulls over matching
    garbage, empty rows, 1-4-byte code points, a binary column with 0xff bytes."""
    rng = np.random.default_rng(5)
    rows = rand_rows(rng, 700, 0, 9, null_every=6)
    for i in range(3, 700, 10):
        rows[i] = b""
    other = rand_rows(rng, 700, 0, 9, null_every=11)
    t = U.sliced(gpu_ctx, rows, 77, 777, pad=b"abcabc", garbage=GARBAGE, lead=3)
    battery(gpu_ctx, rows, col=t.native.column(0), other=other)
    battery(gpu_ctx, rows, col=U.build_column(gpu_ctx, rows, garbage=GARBAGE, lead=0), other=other)
    battery(gpu_ctx, [b"", b"", None, b""], other=[b"", None, b"", b"a"])
    units = ["a", "é", "日", "𝄞", "b", "本"]
    text = [None if i % 9 == 4 else "".join(rng.choice(units, int(rng.integers(0, 7)))).encode() for i in range(600)]
    likes = [x.encode() for x in ("_", "__", "%é", "é%", "_本%", "%日_", "a_b", "%𝄞%a", "___%")]
    battery(gpu_ctx, text, other=text[1:] + text[:1], likes=likes, needles=["é".encode(), "日本".encode(), b"\x97"])
    raw = rand_rows(rng, 600, 0, 6, null_every=8, alphabet=b"a\xff\x80\x00")
    battery(gpu_ctx, raw, other=raw[2:] + raw[:2], binary=True, likes=[b"_", b"\xff%", b"%\x80_", b"a_%\xff"],
            needles=[b"\xff", b"\x80a", b"\x00"])


@pytest.fixture(scope="module")
def sweep(ctx, gpu_ctx):
    rng = np.random.default_rng(16)
    n = 20011
    rows = rand_rows(rng, n, 0, 40, null_every=13)
    other = [r if r is not None and i % 3 == 0 else o
             for i, (r, o) in enumerate(zip(rows, rand_rows(rng, n, 0, 40, null_every=17)))]
    cols = {}
    for name, c in (("gpu", gpu_ctx), ("cpu", ctx)):
        cols[name] = (U.build_column(c, rows, garbage=GARBAGE, lead=3),
                      U.build_column(c, other, garbage=GARBAGE, lead=2, name="o"),
                      U.build_column(c, [b"abcab"]))
    return rows, other, cols


def sweep_check(sweep, fn, want):
    rows, other, cols = sweep
    got = U.col_result(fn(*cols["gpu"]))
    assert got == (want, True)
    assert U.col_result(fn(*cols["cpu"])) == got


@pytest.mark.parametrize("op", list(U.CMP_CODE))
def test_sweep_compare(sweep, op):
    rows, other, _ = sweep
    code = U.CMP_CODE[op]
    sweep_check(sweep, lambda a, b, s: C.string_compare(a, s, code), U.o_compare(rows, b"abcab", op))
    sweep_check(sweep, lambda a, b, s: C.string_compare(a, b, code), U.o_compare(rows, other, op))


@pytest.mark.parametrize("kind,p", [("starts_with", b"ab"), ("ends_with", b"ca"), ("contains", b"abc"),
                                    ("contains", b"a"), ("like", b"%ab%cb"), ("like", b"a_%b"), ("like", b"%c_a%"),
                                    ("like", b"ab%"), ("like", b"%bb"), ("like", b"%cab%")])
def test_sweep_match(sweep, kind, p):
    sweep_check(sweep, lambda a, b, s: C.string_match(a, U.KIND[kind], p), U.o_match(sweep[0], kind, p))


@pytest.mark.parametrize("unit", ["bytes", "chars"])
def test_sweep_length(sweep, unit):
    sweep_check(sweep, lambda a, b, s: C.string_length(a, {"bytes": 0, "chars": 1}[unit]), U.o_length(sweep[0], unit))


def test_routing_stays_on_device(gpu_ctx, monkeypatch):
    """t == "abc", t < other and t.str.* on a device table never copy the column to the host."""
    rng = np.random.default_rng(3)
    rows, other = rand_rows(rng, 1000, 0, 8, null_every=9), rand_rows(rng, 1000, 0, 8)
    t, o = U.build_table(gpu_ctx, rows, garbage=GARBAGE), U.build_table(gpu_ctx, other)

    def no_host(col):
        raise AssertionError("the column went to the host")
    monkeypatch.setattr(compute, "_arrow_col", no_host)
    assert U.result(t == "abc") == U.o_compare(rows, b"abc", "eq")
    assert U.result(t < o) == U.o_compare(rows, other, "lt")
    assert U.result(t >= b"b") == U.o_compare(rows, b"b", "ge")
    assert U.result(t != o) == U.o_compare(rows, other, "ne")
    assert U.result(t.str.contains("b")) == U.o_match(rows, "contains", b"b")
    assert U.result(t.str.startswith("ab")) == U.o_match(rows, "starts_with", b"ab")
    assert U.result(t.str.endswith("c")) == U.o_match(rows, "ends_with", b"c")
    assert U.result(t.str.like("a%_c")) == U.o_match(rows, "like", b"a%_c")
    assert U.result(t.str.len()) == U.o_length(rows, "chars")
    assert U.result(t.str.len_bytes()) == U.o_length(rows, "bytes")
    res = t.str.contains("b")
    assert res.device == t.device and res.native.column(0).data.is_cuda
    kept = t[t.str.like("%b%")]
    assert kept.row_count == sum(1 for r in rows if r is not None and b"b" in r)
    assert compute.binary_op(t, "abc", operator.eq).native.column(0).data.is_cuda


def test_mixed_devices(ctx, gpu_ctx):
    """Columns on different devices: the native entry point refuses them (Invalid, the column and the
    scalar form, either way round); the Table operators keep Arrow's host kernels for such a pair, as
    before the device kernels, and put the result on the left table's device."""
    rng = np.random.default_rng(8)
    rows, other = rand_rows(rng, 300, 0, 6, null_every=7), rand_rows(rng, 300, 0, 6, null_every=5)
    g, c = U.build_column(gpu_ctx, rows), U.build_column(ctx, other)
    one_g, one_c = U.build_column(gpu_ctx, [b"ab"]), U.build_column(ctx, [b"ab"])
    with pytest.raises(C.CylonError) as e:
        C.string_compare(g, U.build_column(gpu_ctx, [b"a", b"b"]), 0)  # a length error: Code::Invalid
    invalid = e.value.args[1]
    for a, b in [(g, c), (c, g), (g, one_c), (c, one_g)]:
        with pytest.raises(C.CylonError) as e:
            C.string_compare(a, b, 0)
        assert e.value.args[1] == invalid and "different devices" in e.value.args[0]
    tg, tc = U.table_of(gpu_ctx, [g]), U.table_of(ctx, [c])
    got = tg < tc
    assert U.result(got) == U.o_compare(rows, other, "lt") and got.native.column(0).data.is_cuda
    got = tc == tg
    assert U.result(got) == U.o_compare(other, rows, "eq") and not got.native.column(0).data.is_cuda
    assert U.result(tg != tc) == U.o_compare(rows, other, "ne")
