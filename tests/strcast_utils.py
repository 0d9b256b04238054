"""Oracle and column helpers for tests/test_strcast_oracle.py (string <-> number casts).

The oracle is written from docs/semantics.md, "String <-> number casts", in plain Python on exact
integers and fractions.  It shares nothing with kernels/strparse.hpp and takes no expected value
from a float parser of Arrow, numpy or Python."""
import functools
import struct
from fractions import Fraction

import pyarrow as pa

REJECT = "reject"    # the cast must raise
SPECIAL = "special"  # an inf / nan spelling: the host parser's (Arrow's) result is the expectation
HOST = "host"        # a hex integer literal: Arrow's result, or Arrow's error, is the expectation

F64 = (11, 52)
F32 = (8, 23)
_DIGITS = frozenset(b"0123456789")
_SPECIALS = (b"inf", b"infinity", b"nan")


def _all_digits(b):
    return all(c in _DIGITS for c in b)


def parse_decimal(b):
    """[+-] digits [. digits] [(e|E) [+-] digits] with at least one mantissa digit, and nothing
    else: (sign, Fraction) with sign 1 for '-', REJECT, or SPECIAL for an inf / nan spelling."""
    sign = 0
    if b[:1] in (b"+", b"-"):
        sign = 1 if b[:1] == b"-" else 0
        b = b[1:]
    if b.lower() in _SPECIALS:
        return SPECIAL
    e = 0
    for i, c in enumerate(b):
        if c in b"eE":
            ex = b[i + 1:]
            b = b[:i]
            esign = -1 if ex[:1] == b"-" else 1
            if ex[:1] in (b"+", b"-"):
                ex = ex[1:]
            if not ex or not _all_digits(ex):
                return REJECT
            e = esign * int(ex)
            break
    ip, dot, fp = b.partition(b".")
    if not _all_digits(ip) or not _all_digits(fp) or not (ip or fp):
        return REJECT
    m = int(ip + fp)
    if m == 0:  # before the power of ten: e may have twenty digits
        return sign, Fraction(0)
    e -= len(fp)
    # anything this far outside binary64 rounds like its clamp (to inf, or to zero), at any width
    e = max(min(e, 400), -1200 - len(ip + fp))
    return sign, (Fraction(m * 10 ** e) if e >= 0 else Fraction(m, 10 ** -e))


def round_binary(frac, sign, ebits, mbits):
    """Bits of the IEEE 754 binary format with `ebits` exponent and `mbits` stored mantissa bits
    nearest to (-1)^sign * frac, ties to even: overflow to inf, subnormals, signed zero."""
    top = sign << (ebits + mbits)
    if frac == 0:
        return top
    assert frac > 0
    bias = (1 << (ebits - 1)) - 1
    emin = 1 - bias
    n, d = frac.numerator, frac.denominator
    e = n.bit_length() - d.bit_length()  # 2^(e-1) < frac < 2^(e+1)
    if (n << -e if e < 0 else n) < (d << e if e > 0 else d):
        e -= 1  # now 2^e <= frac < 2^(e+1)
    e = max(e, emin)
    sh = e - mbits  # the weight of the last kept bit
    if sh >= 0:
        d <<= sh
    else:
        n <<= -sh
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    # q carries the hidden bit (none for a subnormal), so a carry out of the mantissa walks into
    # the exponent field by itself
    bits = ((e - emin) << mbits) + q
    return top | min(bits, ((1 << ebits) - 1) << mbits)


@functools.lru_cache(maxsize=None)
def float_bits(b, fmt):
    """expected bits of the string -> float cast of `b`, or REJECT / SPECIAL"""
    p = parse_decimal(b)
    return p if isinstance(p, str) else round_binary(p[1], p[0], *fmt)


def parse_int(b, lo, hi, signed):
    """Optional '-' (signed targets only, never '+'), one or more decimal digits, leading zeros
    allowed, the value within [lo, hi]: the int, REJECT, or HOST for a hex literal."""
    if b[:1] == b"-":
        if not signed:
            return REJECT
        neg, b = True, b[1:]
    else:
        neg = False
    if b[:2] in (b"0x", b"0X"):
        return HOST
    if not b or not _all_digits(b):
        return REJECT
    v = -int(b) if neg else int(b)
    return v if lo <= v <= hi else REJECT


def int_to_str(v):
    return str(v).encode()


def int_range(typ):
    bits = typ.bit_width
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if pa.types.is_signed_integer(typ) else (0, (1 << bits) - 1)


# ---- raw Arrow buffers
def validity(arr):
    """the null mask as a list of bools, read from the validity bitmap"""
    buf = arr.buffers()[0]
    if buf is None:
        assert arr.null_count == 0
        return [True] * len(arr)
    raw = buf.to_pybytes()
    o = arr.offset
    return [bool(raw[(o + i) >> 3] >> ((o + i) & 7) & 1) for i in range(len(arr))]


_UFMT = {1: "B", 2: "H", 4: "I", 8: "Q"}


def value_bits(arr):
    """the cells of a fixed-width array as unsigned integers (null cells: whatever is there)"""
    w = arr.type.bit_width // 8
    n = len(arr)
    if n == 0:
        return []
    raw = arr.buffers()[1].to_pybytes()
    return list(struct.unpack_from("<%d%s" % (n, _UFMT[w]), raw, arr.offset * w))


def string_cells(arr):
    """(lengths, bytes) of a string array from its offsets and data buffers, relative to the first
    row, so that an array with a non-zero offset compares equal to one without"""
    n = len(arr)
    w, f = (8, "q") if pa.types.is_large_string(arr.type) else (4, "i")
    offs = struct.unpack_from("<%d%s" % (n + 1, f), arr.buffers()[1].to_pybytes(), arr.offset * w) if arr.buffers()[1] \
        else (0,) * (n + 1)
    data = arr.buffers()[2].to_pybytes() if arr.buffers()[2] is not None else b""
    return [o - offs[0] for o in offs], data[offs[0]:offs[n]]


def one_chunk(col):
    return col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col


# ---- columns
GARBAGE = b"\x00z 1e+"  # under a null, or outside a slice: must never be parsed


def string_array(rows, typ=None, nulls=None, keep=False):
    """A string / binary array over `rows` (bytes); rows whose index is in `nulls` are null, with
    GARBAGE as their bytes, or with keep their own (pa.array would leave them empty)."""
    typ = typ or pa.string()
    nulls = nulls or ()
    cells = [GARBAGE if i in nulls and not keep else r for i, r in enumerate(rows)]
    offs = [0]
    for c in cells:
        offs.append(offs[-1] + len(c))
    bufs = [None, pa.py_buffer(struct.pack("<%di" % len(offs), *offs)), pa.py_buffer(b"".join(cells))]
    if nulls:
        bm = bytearray((len(rows) + 7) // 8)
        for i in range(len(rows)):
            if i not in nulls:
                bm[i >> 3] |= 1 << (i & 7)
        bufs[0] = pa.py_buffer(bytes(bm))
    return pa.Array.from_buffers(typ, len(rows), bufs, null_count=len(set(nulls)))


def layouts(rows):
    """[(name, array, live)]: the column as it is, nullable (every 7th row null over garbage bytes),
    as a slice with a non-zero offset of a longer array, and as pa.binary(); live[i] tells whether
    row i holds rows[i] (else it is null)."""
    n = len(rows)
    every7 = frozenset(range(3, n, 7))
    pad = [GARBAGE, b"junk", b""]
    return [
        ("plain", string_array(rows), [True] * n),
        ("nullable", string_array(rows, nulls=every7), [i not in every7 for i in range(n)]),
        ("slice", string_array(pad + list(rows) + pad).slice(len(pad), n), [True] * n),
        ("binary", string_array(rows, pa.binary()), [True] * n),
    ]
