"""Oracle, reader and the shared battery of the string transform tests (docs/semantics.md "String
transforms").

The oracle works on Python `bytes` objects -- slicing a list of units, bytes.strip / lstrip / rstrip, a
256-entry case table, `+` and bytes.replace -- and shares no code with the engine.  A row is `bytes` or
None (null).  The reader turns a result column into such a list and asserts the output layout on every
call.
"""
import strpred_utils as U
from cylon_amd._lib import C

SIDE = {"strip": 3, "lstrip": 1, "rstrip": 2}
WHITESPACE = b" \t\n\v\f\r"
GARBAGE = b" abAB ab\t"  # under every null row: it would match, strip and change case

UPPER = bytes(b - 32 if ord("a") <= b <= ord("z") else b for b in range(256))
LOWER = bytes(b + 32 if ord("A") <= b <= ord("Z") else b for b in range(256))

SLICES = [(0, 3), (2, None), (-3, None), (None, -1), (1, 1), (5, 2), (-100, 100)]
STRIP_SETS = [None, b"ab"]
REPLACEMENTS = [b"", b"x", b"ab", b"abcabc"]


# ------------------------------------------------------------------ oracle
def o_slice(rows, start, stop, utf8=True):
    return U.o_map(rows, lambda r: b"".join(U.units(r, utf8)[start:stop]))


def o_strip(rows, how, chars=None):
    cs = WHITESPACE if chars is None else chars
    return U.o_map(rows, lambda r: getattr(r, how)(cs))


def o_case(rows, upper):
    return U.o_map(rows, lambda r: r.translate(UPPER if upper else LOWER))


def o_concat(a, b, sep=b""):
    """a, b: a list of rows, or a bytes / None scalar"""
    n = len(a) if isinstance(a, list) else len(b)
    la = a if isinstance(a, list) else [a] * n
    lb = b if isinstance(b, list) else [b] * n
    return [None if x is None or y is None else x + sep + y for x, y in zip(la, lb)]


def o_replace(rows, pat, repl, count=-1):
    return U.o_map(rows, lambda r: r.replace(pat, repl, count))


def o_non_ascii(rows):
    return any(r is not None and any(b >= 0x80 for b in r) for r in rows)


# ------------------------------------------------------------------ reader
def read(col, nullable=None, n=None):
    """The cells of a string / binary result column as a list of bytes | None; asserts the layout:
    offsets[0] == 0, offsets non-decreasing, exactly offsets[n] data bytes, null rows of length 0,
    and a validity array present iff `nullable` (when given)."""
    offs = col.offsets.cpu().tolist()
    data = bytes(col.data.cpu().numpy().tobytes())
    assert col.type.type in (C.Type.STRING, C.Type.BINARY)
    assert len(offs) == col.length + 1 and offs[0] == 0
    if n is not None:
        assert col.length == n
    assert all(offs[i] <= offs[i + 1] for i in range(col.length)), "offsets decrease"
    assert col.data.numel() == offs[-1], (col.data.numel(), offs[-1])
    valid = None if col.validity is None else col.validity.cpu().tolist()
    if nullable is not None:
        assert (valid is not None) == nullable, "validity array"
    out = []
    for i in range(col.length):
        if valid is not None and not valid[i]:
            assert offs[i + 1] == offs[i], f"null row {i} has length {offs[i + 1] - offs[i]}"
            out.append(None)
        else:
            out.append(data[offs[i]:offs[i + 1]])
    return out


def result(table, i=0, nullable=None):
    return read(table.native.column(i), nullable)


# ------------------------------------------------------------------ battery
def battery(ctx, rows, col=None, other=None, ocol=None, binary=False, slices=SLICES, replacements=REPLACEMENTS,
            garbage=GARBAGE, pat=b"ab", funcs=("slice", "strip", "case", "concat", "replace")):
    """Every transform on one column against the oracle.  other: the rows of a second column for the
    column (+) column concat."""
    if col is None:
        col = U.build_column(ctx, rows, binary=binary, garbage=garbage, lead=5)
    utf8 = not binary
    nullable = col.validity is not None
    n = len(rows)
    if "slice" in funcs:
        for start, stop in slices:
            got = read(C.string_slice(col, start or 0, stop), nullable, n)
            assert got == o_slice(rows, start, stop, utf8), ("slice", start, stop)
    if "strip" in funcs:
        for how, side in SIDE.items():
            for cs in STRIP_SETS:
                got = read(C.string_strip(col, side, cs), nullable, n)
                assert got == o_strip(rows, how, cs), (how, cs)
    if "case" in funcs:
        for upper in (True, False):
            res, flag = C.string_case(col, upper)
            assert read(res, nullable, n) == o_case(rows, upper), ("case", upper)
            assert flag == o_non_ascii(rows), ("non-ASCII flag", upper)
    if "concat" in funcs:
        one = U.build_column(ctx, [b"<->"], binary=binary, lead=3)
        assert read(C.string_concat(col, one), nullable, n) == o_concat(rows, b"<->"), "col + scalar"
        assert read(C.string_concat(one, col), nullable, n) == o_concat(b"<->", rows), "scalar + col"
        assert read(C.string_concat(col, one, b"--"), nullable, n) == o_concat(rows, b"<->", b"--"), "sep"
        if other is not None:
            if ocol is None:
                ocol = U.build_column(ctx, other, binary=binary, garbage=garbage, lead=9, name="o")
            both = nullable or ocol.validity is not None
            assert read(C.string_concat(col, ocol), both, n) == o_concat(rows, other), "col + col"
            assert read(C.string_concat(ocol, col, b"--"), both, n) == o_concat(other, rows, b"--"), "col + sep + col"
    if "replace" in funcs:
        for repl in replacements:
            for count in (-1, 1):
                got = read(C.string_replace(col, pat, repl, count), nullable, n)
                assert got == o_replace(rows, pat, repl, count), ("replace", repl, count)
