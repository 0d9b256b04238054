"""Elementwise compute on device columns (K15; reference: python/pycylon/data/compute.pyx:43-813).

The reference evaluates these operators in Python/Cython over pyarrow.compute or
numpy on the host.  Here fixed-width columns stay on the table's device and the
operators run as device tensor expressions (ROCm kernels on MI355X), with the
validity byte-mask propagated explicitly.  String / binary columns stay on the
device too: where / fill_null (kernels/select.hip), the string <-> number casts
(kernels/strcast.hip), the string predicates (kernels/strmatch.hip) --
comparisons of a string column with a str / bytes scalar or with a string column
of the same kind, str_starts_with / str_ends_with / str_contains / str_like and
str_length -- and the string transforms (kernels/strxform.hip), which produce a
string column from a string column: str_slice, str_strip / str_lstrip /
str_rstrip, str_upper / str_lower, str_concat (also `t + "x"` and `a + b` of
string columns) and str_replace.  What does not fit those kernels (operands of
different kinds, a pattern or literal over C.string_max_pattern_bytes, a
non-ASCII strip set, Unicode case mapping of non-ASCII text, other arithmetic
on strings) is evaluated by Arrow compute on the host, as in the reference,
with the same values.

Engine selection keeps the reference's `compute_engine` config key: "arrow"
forces the host Arrow path, anything else uses the device path.
"""
import operator
from typing import Any, Callable, List, Optional

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import torch

from .._lib import C
from . import arrow_bridge as ab

T = C.Type

_CMP = {operator.eq: "equal", operator.ne: "not_equal", operator.lt: "less", operator.gt: "greater",
        operator.le: "less_equal", operator.ge: "greater_equal"}
_ARITH = {operator.add: "add", operator.sub: "subtract", operator.mul: "multiply", operator.truediv: "divide"}


def is_var(col) -> bool:
    return col.offsets is not None


def col_values(col) -> torch.Tensor:
    """Typed value tensor of a fixed-width column (bool as torch.bool)."""
    t = col.data
    if col.type.type == T.BOOL:
        return t.to(torch.bool)
    return t


def col_valid(col) -> Optional[torch.Tensor]:
    v = col.validity
    return None if v is None else v.to(torch.bool)


def make_col(name: str, values: torch.Tensor, valid: Optional[torch.Tensor] = None, like=None):
    vt = None if valid is None else valid.to(torch.uint8).contiguous()
    if (like is not None and not is_var(like) and like.type.type != T.BOOL and values.dtype != torch.bool
            and ab.torch_dtype(like.type) == values.dtype):
        data = values.contiguous()
        return C.Column(name, like.type, data.numel(), data, None, vt)
    return ab.column_from_tensor(name, values, vt)


def _and_valid(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return a & b


def _arrow_col(col) -> pa.Array:
    return ab.column_to_arrow(col)


def _from_arrow(name, arr, device):
    return ab.column_from_arrow(name, arr, device)


def _scalar_for(col, value):
    if isinstance(value, (bool, int, float, np.number)):
        return value
    raise TypeError(f"unsupported scalar {value!r} for column {col.name}")


def binary_op(table, other, op: Callable, engine: str = "device"):
    """Elementwise op between a table and a scalar or an equally shaped table."""
    from .table import Table
    cols = table.native.columns()
    dev = table.device
    other_cols = other.native.columns() if isinstance(other, Table) else None
    if other_cols is not None and len(other_cols) != len(cols):
        raise ValueError("tables must have the same number of columns")
    out = []
    for i, c in enumerate(cols):
        oc = other_cols[i] if other_cols is not None else None
        if engine != "arrow":
            res = _string_compare(c, oc, other, op, dev)
            if res is None and op is operator.add:
                res = _string_add(c, oc, other, dev)
            if res is not None:
                out.append(res)
                continue
        use_arrow = engine == "arrow" or is_var(c) or (oc is not None and is_var(oc)) or isinstance(other, str)
        if use_arrow:
            fn = _CMP.get(op) or _ARITH.get(op) or {operator.and_: "and_kleene", operator.or_: "or_kleene"}.get(op)
            rhs = _arrow_col(oc) if oc is not None else other
            res = getattr(pc, fn)(_arrow_col(c), rhs)
            out.append(_from_arrow(c.name, res, dev))
            continue
        a = col_values(c)
        va = col_valid(c)
        if oc is not None:
            b = col_values(oc)
            vb = col_valid(oc)
        else:
            b = _scalar_for(c, other)
            vb = None
        if op is operator.truediv:
            res = a.to(torch.float64) / (b.to(torch.float64) if torch.is_tensor(b) else float(b))
        else:
            res = op(a, b)
        out.append(make_col(c.name, res, _and_valid(va, vb), like=c if res.dtype == a.dtype else None))
    return table._wrap(C.Table(table.native.context(), out))


def unary_op(table, fn: Callable, name: str = "", engine: str = "device"):
    cols = table.native.columns()
    out = []
    for c in cols:
        if is_var(c) or engine == "arrow":
            res = getattr(pc, {"neg": "negate", "invert": "invert"}[name])(_arrow_col(c))
            out.append(_from_arrow(c.name, res, table.device))
            continue
        v = col_values(c)
        out.append(make_col(c.name, fn(v), col_valid(c), like=c))
    return table._wrap(C.Table(table.native.context(), out))


def is_null(table, invert: bool = False):
    out = []
    for c in table.native.columns():
        n = c.length
        v = col_valid(c)
        isn = torch.zeros(n, dtype=torch.bool, device=c.data.device) if v is None else ~v
        if not is_var(c) and c.type.type in (T.FLOAT, T.DOUBLE, T.HALF_FLOAT):
            isn = isn | torch.isnan(c.data)
        out.append(make_col(c.name, ~isn if invert else isn))
    return table._wrap(C.Table(table.native.context(), out))


def _var_scalar(c, value, device):
    """One-row device column of c's type holding value (None if value does not convert)."""
    try:
        arr = pa.array([value], type=ab.to_arrow_type(c.type))
    except (pa.ArrowInvalid, pa.ArrowTypeError, TypeError, ValueError):
        return None
    return ab.column_from_arrow(c.name, arr, device)


def _select_var(c, other, cond, device):
    """K15 device select of a string / binary column (kernels/select.hip): cond ? c : other, where
    other is None (null), a scalar (broadcast) or a column of c's type; None when other does not
    fit (the caller then uses Arrow's host kernels)."""
    if other is None:
        b = None
    elif isinstance(other, C.Column):
        if not is_var(other) or other.type.type != c.type.type or other.length not in (1, c.length):
            return None
        b = other
    else:
        b = _var_scalar(c, other, device)
        if b is None:
            return None
    return C.select_var(c, b, cond.to(torch.uint8))


def is_text(col) -> bool:
    return col.type.type in (T.STRING, T.BINARY)


# the numbers of kernels/strmatch_common.hpp (StrCmpOp, StrMatchKind, StrLenUnit)
_STR_CMP = {operator.eq: 0, operator.ne: 1, operator.lt: 2, operator.le: 3, operator.gt: 4, operator.ge: 5}
_STR_KIND = {"starts_with": 0, "ends_with": 1, "contains": 2, "like": 3}
_STR_UNIT = {"bytes": 0, "chars": 1}


def _string_compare(c, oc, other, op, device):
    """K15 device comparison of a string / binary column (kernels/strmatch.hip) with the column oc
    of the same kind and length, or with the str / bytes scalar `other`; None when the operands do
    not fit (the caller then uses Arrow's host kernels)."""
    code = _STR_CMP.get(op)
    if code is None or not is_text(c):
        return None
    if oc is not None:
        if not is_text(oc) or oc.type.type != c.type.type or oc.length != c.length or \
                oc.data.device != c.data.device:
            return None
        b = oc
    elif isinstance(other, (str, bytes)):
        b = _var_scalar(c, other, device)
        if b is None:
            return None
    else:
        return None
    return C.string_compare(c, b, code)


def _pattern_bytes(pattern) -> bytes:
    if isinstance(pattern, str):
        return pattern.encode("utf-8")
    if isinstance(pattern, (bytes, bytearray)):
        return bytes(pattern)
    raise TypeError(f"a string pattern must be str or bytes, not {type(pattern).__name__}")


def _engine_of(table, engine):
    return engine or table.context.get_config("compute_engine", "device") or "device"


def _text_columns(table, what):
    cols = table.native.columns()
    for c in cols:
        if not is_text(c):
            raise TypeError(f"{what}: column {c.name} ({c.type}) is not a string / binary column")
    return cols


def _arrow_like_pattern(pattern: bytes, escape: bytes) -> bytes:
    """The LIKE pattern (bytes) rewritten for Arrow's match_like, whose escape character is the
    backslash: an escaped %, _ or backslash stays escaped, any other escaped byte is literal."""
    out, i = [], 0
    while i < len(pattern):
        ch = pattern[i:i + 1]
        if ch == escape:
            i += 1
            if i >= len(pattern):
                raise C.CylonError("like: the pattern ends in a lone escape character")
            ch = pattern[i:i + 1]
            out.append(b"\\" + ch if ch in (b"%", b"_", b"\\") else ch)
        else:
            out.append(b"\\\\" if ch == b"\\" else ch)
        i += 1
    return b"".join(out)


def _str_match(table, kind, pattern, engine=None, escape="\\"):
    cols = _text_columns(table, "str_" + kind)
    pat = _pattern_bytes(pattern)
    esc = _pattern_bytes(escape)
    if len(esc) != 1:
        raise ValueError("the escape must be one single-byte character")
    out = []
    if _engine_of(table, engine) == "arrow" or len(pat) > C.string_max_pattern_bytes:
        for c in cols:
            arr = _arrow_col(c)
            if kind == "like":
                res = pc.match_like(arr, _arrow_like_pattern(pat, esc))
            else:
                fn = {"starts_with": pc.starts_with, "ends_with": pc.ends_with, "contains": pc.match_substring}[kind]
                res = fn(arr, pat)
            out.append(_from_arrow(c.name, res, table.device))
    else:
        out = [C.string_match(c, _STR_KIND[kind], pat, esc) for c in cols]
    return table._wrap(C.Table(table.native.context(), out))


def str_starts_with(table, pattern, engine=None):
    """BOOL per cell: the cell begins with the literal pattern (Arrow's starts_with); null for a
    null cell.  Every column of the table must be string / binary."""
    return _str_match(table, "starts_with", pattern, engine)


def str_ends_with(table, pattern, engine=None):
    """BOOL per cell: the cell ends with the literal pattern (Arrow's ends_with)."""
    return _str_match(table, "ends_with", pattern, engine)


def str_contains(table, pattern, engine=None):
    """BOOL per cell: the literal pattern occurs in the cell (Arrow's match_substring; no regular
    expressions)."""
    return _str_match(table, "contains", pattern, engine)


def str_like(table, pattern, escape="\\", engine=None):
    """BOOL per cell: SQL LIKE anchored at both ends (Arrow's match_like): % any run, _ one code
    point (one byte of a binary column), the escape makes the next character literal."""
    return _str_match(table, "like", pattern, engine, escape)


def str_length(table, unit="chars", engine=None):
    """INT64 per cell: its length in code points (unit "chars", string columns only; Arrow's
    utf8_length) or in bytes (unit "bytes"; Arrow's binary_length)."""
    if unit not in _STR_UNIT:
        raise ValueError(f"unit must be 'chars' or 'bytes', not {unit!r}")
    cols = _text_columns(table, "str_length")
    for c in cols:
        if unit == "chars" and c.type.type != T.STRING:
            raise TypeError(f"str_length: the binary column {c.name} has no code points")
    if _engine_of(table, engine) == "arrow":
        fn = pc.utf8_length if unit == "chars" else pc.binary_length
        out = [_from_arrow(c.name, pc.cast(fn(_arrow_col(c)), pa.int64()), table.device) for c in cols]
    else:
        out = [C.string_length(c, _STR_UNIT[unit]) for c in cols]
    return table._wrap(C.Table(table.native.context(), out))


# ---------------------------------------------------------------- string transforms (kernels/strxform.hip)
_STRIP_SIDE = {"left": 1, "right": 2, "both": 3}
_ASCII_WHITESPACE = b" \t\n\v\f\r"


def _is_string(col) -> bool:
    return col.type.type == T.STRING


def _literal(c, value) -> Any:
    """A literal as Arrow takes it beside the column c: str for a STRING column, bytes for BINARY."""
    return value.decode("utf-8") if _is_string(c) else value


def _host_bytes_map(arr, fn):
    """fn over the cells (bytes) of a host binary array: what Arrow has no binary kernel for."""
    return pa.array([None if v is None else fn(v) for v in arr.to_pylist()], type=arr.type)


def _map_text(table, what, device_fn, arrow_fn, use_arrow):
    """One transform over every (string / binary) column of the table: device_fn(col) -> Column on
    the column's device, or arrow_fn(col, arrow array) -> arrow array on the host."""
    cols = _text_columns(table, what)
    if use_arrow:
        out = [_from_arrow(c.name, arrow_fn(c, _arrow_col(c)), table.device) for c in cols]
    else:
        out = [device_fn(c) for c in cols]
    return table._wrap(C.Table(table.native.context(), out))


def _slice_index(v, what):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"str_slice: {what} must be an integer or None, not {type(v).__name__}")
    return int(v)


def str_slice(table, start=None, stop=None, engine=None):
    """Every cell's units[start:stop] as Python slices it (step 1): code points of a string column
    (Arrow's utf8_slice_codeunits), bytes of a binary one (binary_slice).  A negative index counts
    from the end of the cell; both ends are clamped."""
    b, e = _slice_index(start, "start") or 0, _slice_index(stop, "stop")

    def arrow(c, arr):
        fn = pc.utf8_slice_codeunits if _is_string(c) else pc.binary_slice
        return fn(arr, start=b, stop=e)
    return _map_text(table, "str_slice", lambda c: C.string_slice(c, b, e), arrow, _engine_of(table, engine) == "arrow")


def _str_strip(table, side, chars, engine):
    what = {"both": "str_strip", "left": "str_lstrip", "right": "str_rstrip"}[side]
    cols = _text_columns(table, what)
    cs = None if chars is None else _pattern_bytes(chars)
    ascii_set = cs is None or all(b < 0x80 for b in cs)
    suffix = {"both": "trim", "left": "ltrim", "right": "rtrim"}[side]

    def arrow(c, arr):
        if not _is_string(c):  # Arrow trims text only: a binary column's cells are stripped one by one
            how = {"both": "strip", "left": "lstrip", "right": "rstrip"}[side]
            return _host_bytes_map(arr, lambda v: getattr(v, how)(_ASCII_WHITESPACE if cs is None else cs))
        if cs is None:
            return getattr(pc, "ascii_" + suffix + "_whitespace")(arr)
        return getattr(pc, "utf8_" + suffix)(arr, characters=cs.decode("utf-8"))
    use_arrow = _engine_of(table, engine) == "arrow" or (not ascii_set and any(_is_string(c) for c in cols))
    return _map_text(table, what, lambda c: C.string_strip(c, _STRIP_SIDE[side], cs), arrow, use_arrow)


def str_strip(table, chars=None, engine=None):
    """Remove the leading and trailing characters of the set `chars` from every cell; without
    `chars`, ASCII whitespace (space, \\t \\n \\v \\f \\r: Arrow's ascii_trim_whitespace -- Unicode
    whitespace stays, unlike pandas).  With `chars`: Arrow's utf8_trim / ascii_trim.  A set with a
    non-ASCII character on a string column is stripped by Arrow's host kernel."""
    return _str_strip(table, "both", chars, engine)


def str_lstrip(table, chars=None, engine=None):
    return _str_strip(table, "left", chars, engine)


def str_rstrip(table, chars=None, engine=None):
    return _str_strip(table, "right", chars, engine)


def _str_case(table, upper, ascii_only, engine):
    what = "str_upper" if upper else "str_lower"
    cols = _text_columns(table, what)
    arrow_engine = _engine_of(table, engine) == "arrow"
    out = []
    for c in cols:
        unicode_map = not ascii_only and _is_string(c)
        if arrow_engine:
            if unicode_map:
                fn = pc.utf8_upper if upper else pc.utf8_lower
            elif _is_string(c):
                fn = pc.ascii_upper if upper else pc.ascii_lower
            else:  # bytes.upper / lower map ASCII letters only
                def fn(arr):
                    return _host_bytes_map(arr, bytes.upper if upper else bytes.lower)
            out.append(_from_arrow(c.name, fn(_arrow_col(c)), table.device))
            continue
        res, non_ascii = C.string_case(c, upper)
        if unicode_map and non_ascii:
            # a non-ASCII byte in a live row: Unicode case mapping is Arrow's, on the host
            res = _from_arrow(c.name, (pc.utf8_upper if upper else pc.utf8_lower)(_arrow_col(c)), table.device)
        out.append(res)
    return table._wrap(C.Table(table.native.context(), out))


def str_upper(table, ascii_only=False, engine=None):
    """Upper case.  The device maps ASCII letters (Arrow's ascii_upper) and reports whether any live
    cell holds a non-ASCII byte; a string column that does, with ascii_only=False, is mapped by
    Arrow's utf8_upper on the host instead, so the answer is Unicode-correct either way and
    all-ASCII data never leaves the device.  A binary column always maps ASCII letters only."""
    return _str_case(table, True, ascii_only, engine)


def str_lower(table, ascii_only=False, engine=None):
    """Lower case; see str_upper."""
    return _str_case(table, False, ascii_only, engine)


def _concat_operand(c, other, device):
    """The other side of a concat with column c: a Column of c's kind, or None when it does not fit."""
    if isinstance(other, C.Column):
        return other if is_text(other) and other.type.type == c.type.type else None
    if isinstance(other, (str, bytes, bytearray)) or other is None:
        if isinstance(other, str) and not _is_string(c):
            other = other.encode("utf-8")
        return _var_scalar(c, bytes(other) if isinstance(other, bytearray) else other, device)
    return None


def _arrow_concat(c, a_arr, b_arr, sep):
    # a column past 2 GiB comes to the host with 64-bit offsets: the three arguments share one type
    large = any(pa.types.is_large_string(x.type) or pa.types.is_large_binary(x.type) for x in (a_arr, b_arr))
    if _is_string(c):
        typ = pa.large_string() if large else pa.string()
    else:
        typ = pa.large_binary() if large else pa.binary()
    return pc.binary_join_element_wise(a_arr.cast(typ), b_arr.cast(typ), pa.scalar(_literal(c, sep), type=typ))


def str_concat(table, other, sep="", engine=None):
    """a[i] + sep + other[i] for every column of the table (Arrow's binary_join_element_wise: null
    where either side is null).  other: a str / bytes scalar (None: a null, every row is null), or
    a table of as many string columns of the same kind, each of the table's length or one row."""
    from .table import Table
    cols = _text_columns(table, "str_concat")
    sp = _pattern_bytes(sep)
    if isinstance(other, Table):
        ocols = _text_columns(other, "str_concat")
        if len(ocols) != len(cols):
            raise ValueError("str_concat: tables must have the same number of columns")
    else:
        ocols = [other] * len(cols)
    use_arrow = _engine_of(table, engine) == "arrow" or len(sp) > C.string_max_pattern_bytes
    out = []
    for c, o in zip(cols, ocols):
        b = _concat_operand(c, o, c.data.device)
        if b is None:
            raise TypeError(f"str_concat: cannot concatenate column {c.name} ({c.type}) with {type(o).__name__}"
                            if not isinstance(o, C.Column) else
                            f"str_concat: column {o.name} ({o.type}) has not the type of {c.name} ({c.type})")
        if use_arrow or b.data.device != c.data.device:
            a_arr, b_arr = _arrow_col(c), _arrow_col(b)
            if c.length == 1 and b.length != 1:
                a_arr = a_arr[0]
            elif b.length == 1 and c.length != 1:
                b_arr = b_arr[0]
            out.append(_from_arrow(c.name, _arrow_concat(c, a_arr, b_arr, sp), table.device))
        else:
            out.append(C.string_concat(c, b, sp))
    return table._wrap(C.Table(table.native.context(), out))


def _string_add(c, oc, other, device):
    """`+` of a string / binary column with a str / bytes scalar or a column of the same kind
    (kernels/strxform.hip concat); None when the operands do not fit."""
    if not is_text(c):
        return None
    if oc is not None:
        if not is_text(oc) or oc.type.type != c.type.type or oc.length != c.length or \
                oc.data.device != c.data.device:
            return None
        b = oc
    elif isinstance(other, (str, bytes)):
        b = _concat_operand(c, other, device)
        if b is None:
            return None
    else:
        return None
    return C.string_concat(c, b, b"")


def str_replace(table, pat, repl, n=-1, engine=None):
    """Replace the leftmost non-overlapping occurrences of the literal `pat` by `repl`, at most n per
    cell (n < 0: all), byte-wise: Python's bytes.replace, Arrow's replace_substring.  No regular
    expressions; an empty pattern is an error."""
    p, r = _pattern_bytes(pat), _pattern_bytes(repl)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError("str_replace: n must be an integer")
    n = -1 if n < 0 else int(n)
    if not p:
        raise C.CylonError("string replace: the pattern is empty")
    limit = C.string_max_pattern_bytes

    def arrow(c, arr):
        return pc.replace_substring(arr, pattern=_literal(c, p), replacement=_literal(c, r),
                                    max_replacements=None if n < 0 else n)
    use_arrow = _engine_of(table, engine) == "arrow" or len(p) > limit or len(r) > limit
    return _map_text(table, "str_replace", lambda c: C.string_replace(c, p, r, n), arrow, use_arrow)


class StringMethods:
    """The `.str` accessor of a Table / DataFrame whose columns are all string / binary: each method
    returns a table of the same shape -- BOOL or INT64 columns from the predicates, so
    `t[t["name"].str.like("A%")]` filters through __getitem__, where a null counts as false; string /
    binary columns from the transforms (slice, strip, upper / lower, cat, replace)."""

    def __init__(self, table, wrap=None):
        self._table = table
        self._wrap = wrap or (lambda t: t)

    def startswith(self, pat):
        return self._wrap(str_starts_with(self._table, pat))

    def endswith(self, pat):
        return self._wrap(str_ends_with(self._table, pat))

    def contains(self, pat, regex=False):
        """Literal substring test.  pandas' default is regex=True; here the default is the literal
        match, and regex=True raises NotImplementedError (regular expressions are not supported)."""
        if regex:
            raise NotImplementedError("str.contains(regex=True): regular expressions are not supported")
        return self._wrap(str_contains(self._table, pat))

    def like(self, pattern, escape="\\"):
        return self._wrap(str_like(self._table, pattern, escape))

    def len(self):
        """Length in code points."""
        return self._wrap(str_length(self._table, "chars"))

    def len_bytes(self):
        return self._wrap(str_length(self._table, "bytes"))

    def slice(self, start=None, stop=None):
        """Code points [start:stop] of every cell (bytes of a binary column); step 1 only."""
        return self._wrap(str_slice(self._table, start, stop))

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("str[...] takes a slice")
        if key.step not in (None, 1):
            raise NotImplementedError("str[...]: a slice step other than 1 is not supported")
        return self.slice(key.start, key.stop)

    def strip(self, chars=None):
        """Strip ASCII whitespace (chars=None; Unicode whitespace stays, unlike pandas) or the
        characters of `chars` from both ends."""
        return self._wrap(str_strip(self._table, chars))

    def lstrip(self, chars=None):
        return self._wrap(str_lstrip(self._table, chars))

    def rstrip(self, chars=None):
        return self._wrap(str_rstrip(self._table, chars))

    def upper(self):
        return self._wrap(str_upper(self._table))

    def lower(self):
        return self._wrap(str_lower(self._table))

    def cat(self, other, sep=""):
        """cell + sep + other: other a str / bytes scalar or a table / frame of string columns."""
        other = getattr(other, "_table", other)  # a DataFrame's table
        return self._wrap(str_concat(self._table, other, sep))

    def replace(self, pat, repl, n=-1, regex=False):
        """Literal replacement.  pandas' default was regex=True for long; here the default is the
        literal, and regex=True raises NotImplementedError."""
        if regex:
            raise NotImplementedError("str.replace(regex=True): regular expressions are not supported")
        return self._wrap(str_replace(self._table, pat, repl, n))


def fill_null(table, value):
    out = []
    for c in table.native.columns():
        if c.validity is None and (is_var(c) or c.type.type not in (T.FLOAT, T.DOUBLE)):
            out.append(c)
            continue
        if is_var(c):
            res = _select_var(c, value, c.validity, table.device) if value is not None else c
            out.append(res if res is not None else _from_arrow(c.name, pc.fill_null(_arrow_col(c), value),
                                                               table.device))
            continue
        v = col_values(c)
        mask = col_valid(c)
        fill = torch.full_like(v, value)
        isn = (~mask if mask is not None else torch.zeros_like(v, dtype=torch.bool))
        if v.is_floating_point():
            isn = isn | torch.isnan(v)
        out.append(make_col(c.name, torch.where(isn, fill, v), None, like=c))
    return table._wrap(C.Table(table.native.context(), out))


def where(table, condition, other=None):
    """Keep values where condition (bool table, same shape, or one column) holds, else other/null."""
    from .table import Table
    ccols = condition.native.columns()
    out = []
    for i, c in enumerate(table.native.columns()):
        cond = ccols[i] if len(ccols) > 1 else ccols[0]
        cv = col_values(cond)
        cvv = col_valid(cond)
        if cvv is not None:
            cv = cv & cvv
        if is_var(c):
            rhs = other.native.column(i) if isinstance(other, Table) else other
            res = _select_var(c, rhs, cv, table.device)
            if res is None:  # other of another type: Arrow's host if_else (casts / raises like pandas)
                rhs = other.to_arrow().column(i) if isinstance(other, Table) else other
                res = _from_arrow(c.name, pc.if_else(pa.array(cv.cpu().numpy()), _arrow_col(c), rhs), table.device)
            out.append(res)
            continue
        v = col_values(c)
        valid = col_valid(c)
        if other is None:
            nv = cv if valid is None else (valid & cv)
            out.append(make_col(c.name, v, nv, like=c))
        else:
            ov = col_values(other.native.column(i)) if isinstance(other, Table) else torch.full_like(v, other)
            out.append(make_col(c.name, torch.where(cv, v, ov), valid, like=c))
    return table._wrap(C.Table(table.native.context(), out))


def is_in(table, values, skip_null: bool = True):
    """Membership test per column; values: list/set (all columns), dict (per column name) or Table."""
    from .table import Table
    out = []
    for i, c in enumerate(table.native.columns()):
        if isinstance(values, dict):
            vals = values.get(c.name, [])
        elif isinstance(values, Table):
            vals = values.to_arrow().column(i).to_pylist()
        else:
            vals = list(values)
        if is_var(c):
            vals = [v for v in vals if isinstance(v, (str, bytes))]
        else:
            vals = [v for v in vals if not isinstance(v, (str, bytes))]
        if is_var(c):  # device hash join of the column against the distinct value set
            n = c.length
            res = torch.zeros(n, dtype=torch.bool, device=c.data.device)
            if vals and n:
                vs = pa.array(vals, type=ab.to_arrow_type(c.type)).unique()
                vt = C.Table(table.native.context(), [ab.column_from_arrow("v", vs, table.device)])
                lt = C.Table(table.native.context(), [c])
                li, _ = C.join_indices(lt, vt, "inner", "hash", [0], [0])
                res[li.to(res.device)] = True
            valid = col_valid(c)
            if valid is not None:
                res = res & valid
            out.append(make_col(c.name, res))
            continue
        v = col_values(c)
        vs = torch.tensor([x for x in vals if x is not None], dtype=v.dtype, device=v.device) if vals else \
            torch.empty(0, dtype=v.dtype, device=v.device)
        res = torch.isin(v, vs)
        valid = col_valid(c)
        if valid is not None:
            res = res & valid
        out.append(make_col(c.name, res))
    return table._wrap(C.Table(table.native.context(), out))


def _device_cast(c, target: pa.DataType, safe: bool):
    """Numeric -> numeric casts on the column's device (torch), with Arrow's safe-cast checks:
    float -> int must be integral and in range, int -> narrower int must be in range, int -> float
    must lie within the float's exact integer range (2^53 / 2^24).  uint64 sources go to Arrow."""
    src = ab.to_arrow_type(c.type)
    num = lambda t: pa.types.is_integer(t) or pa.types.is_floating(t)  # noqa: E731
    try:
        # K15 string <-> number casts on the device (kernels/strcast.hip); None: the host parser
        if is_var(c):
            # uint64 targets: the device parser reads int64, Arrow's host cast takes the full range
            if pa.types.is_string(src) and num(target) and target not in (pa.float16(), pa.uint64()):
                return C.cast_string_to_number(c, ab.to_cylon_type(target))
            return None
        if pa.types.is_string(target) and pa.types.is_integer(src) and src != pa.uint64() and c.type.type != T.BOOL:
            return C.cast_integer_to_string(c, ab.to_cylon_type(target))
    except C.CylonError as e:
        raise pa.ArrowInvalid(str(e)) from None
    if c.type.type == T.BOOL:
        return None
    if not (num(src) and num(target)) or target == pa.float16() or src == pa.float16():
        return None
    if src == pa.uint64():  # torch has no full uint64 min/max/compare support: Arrow's host kernels
        return None
    ct = ab.to_cylon_type(target)
    tdt = ab.torch_dtype(ct)
    v = c.data
    valid = col_valid(c)
    if safe and pa.types.is_integer(target):
        live = v if valid is None else v[valid]
        if live.numel():
            info = np.iinfo(target.to_pandas_dtype())
            if pa.types.is_floating(src):
                if not bool(torch.all(torch.isfinite(live)) and torch.all(live == torch.trunc(live))):
                    raise pa.ArrowInvalid(f"column {c.name}: float values would be truncated")
                lo, hi = float(live.min()), float(live.max())
            else:
                lo, hi = int(live.min()), int(live.max())
            if lo < info.min or hi > info.max:
                raise pa.ArrowInvalid(f"column {c.name}: integer value out of range for {target}")
    if safe and pa.types.is_floating(target) and pa.types.is_integer(src):
        # Arrow's safe int -> float cast refuses integers beyond the float's exact range
        live = v if valid is None else v[valid]
        lim = 2 ** 53 if target == pa.float64() else 2 ** 24
        if live.numel() and (int(live.min()) < -lim or int(live.max()) > lim):
            raise pa.ArrowInvalid(f"column {c.name}: integer value not in range: {-lim} to {lim}")
    out = v.to(tdt)
    return C.Column(c.name, ct, c.length, out.contiguous(), None,
                    None if c.validity is None else c.validity.contiguous())


def cast(table, dtype, safe: bool = True):
    """astype: dtype may be a single type or {column: type}.  Numeric -> numeric, string -> number
    and integer -> string casts run on the table's device; everything else (float -> string,
    dates, hex / special-value strings) goes through Arrow's cast kernels on the host."""
    from ..types import to_arrow
    cols = table.native.columns()
    targets = [dtype.get(c.name) if isinstance(dtype, dict) else dtype for c in cols]
    dev = [None if t is None else _device_cast(c, to_arrow(t), safe) for c, t in zip(cols, targets)]
    if all(t is None or d is not None for t, d in zip(targets, dev)):
        out = [c if d is None else d for c, d in zip(cols, dev)]
        return table._wrap(C.Table(table.native.context(), out))
    at = table.to_arrow()
    arrays, names = [], []
    for name, col in zip(at.column_names, at.columns):
        t = dtype.get(name) if isinstance(dtype, dict) else dtype
        arrays.append(col if t is None else pc.cast(col, to_arrow(t), safe=safe))
        names.append(name)
    from .table import Table
    return Table(pa.Table.from_arrays(arrays, names=names), table.context)


def apply_map(table, func: Callable):
    at = table.to_arrow()
    arrays = [pa.array([func(x) for x in col.to_pylist()]) for col in at.columns]
    from .table import Table
    return Table(pa.Table.from_arrays(arrays, names=at.column_names), table.context)


def unique_values(table, column=0) -> List[Any]:
    return table.to_arrow().column(column).unique().to_pylist()


def nunique(table, column=0) -> int:
    return len(unique_values(table, column))


# ---------------------------------------------------------------------------
# Reference entry points (python/pycylon/data/compute.pyx), mapped onto the
# device engine above.  Same names and argument order as pycylon.
# ---------------------------------------------------------------------------
def comparison_compute_op_iter(array, other, op):
    """compute.pyx:78 — elementwise comparison of a 1-D array with a scalar."""
    return np.asarray([op(x, other) for x in np.asarray(array)], dtype=bool)


def comparison_compute_np_op(array, other, op):
    """compute.pyx:108 — vectorised comparison of a numpy array with a scalar."""
    return op(np.asarray(array), other)


def table_compare_ar_op(table, other, op):
    """compute.pyx:127 — comparison through the Arrow (host) engine."""
    return binary_op(table, other, op, engine="arrow")


def table_compare_np_op(table, other, op):
    """compute.pyx:164 — the reference's numpy engine; here the device engine."""
    return binary_op(table, other, op, engine="device")


def table_compare_op(table, other, op, engine="arrow"):
    """compute.pyx:198."""
    return binary_op(table, other, op, engine=engine)


def invert(table):
    """compute.pyx:226 — logical not of bool columns (other types raise, as in the reference)."""
    for c in table.native.columns():
        if c.type.type != T.BOOL:
            raise ValueError(f"Invert only support for bool types, but found {c.type}")
    return unary_op(table, torch.logical_not, "invert")


def neg(table):
    """compute.pyx:246 — negation of numeric columns."""
    return unary_op(table, torch.neg, "neg")


def division_op(table, op, value):
    """compute.pyx:267 — table / scalar (op: operator.truediv or operator.floordiv)."""
    return binary_op(table, value, op)


def math_op(table, op, value, engine="device"):
    """compute.pyx:441 — table (+ - * /) scalar or table."""
    return binary_op(table, value, op, engine="arrow" if engine == "arrow" else "device")


def math_op_numpy(table, op, value):
    """compute.pyx:299."""
    return math_op(table, op, value, "numpy")


def math_op_arrow(table, op, value):
    """compute.pyx:347."""
    return math_op(table, op, value, "arrow")


def math_op_c_numpy(table, op, value):
    """compute.pyx:373."""
    return math_op(table, op, value, "numpy")


def unique(table):
    """compute.pyx:454 — per column, the number of distinct values (a one-row table)."""
    from .table import Table
    return Table.from_pydict(table.context, {name: [nunique(table, i)] for i, name in enumerate(table.column_names)})


def compare_array_like_values(l_org_ar, l_cmp_ar, skip_null=True):
    """compute.pyx:509 — membership of each value of l_org_ar in l_cmp_ar (pyarrow arrays)."""
    return pc.is_in(l_org_ar, options=pc.SetLookupOptions(value_set=pa.array(l_cmp_ar), skip_nulls=skip_null))


def drop_na(table, how: str, axis=0):
    """compute.pyx:714."""
    return table.dropna(axis=axis, how=how)


def infer_map(table, func):
    """compute.pyx:792 — func applied to every column as a numpy array; one output column each."""
    from .table import Table
    arrays = [pa.array(np.asarray(func(col.to_numpy(zero_copy_only=False))))
              for col in table.to_arrow().combine_chunks().itercolumns()]
    return Table.from_arrow(table.context, pa.Table.from_arrays(arrays, names=table.column_names))
