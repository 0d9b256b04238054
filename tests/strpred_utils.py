"""Oracle and column builders for the string predicate tests (docs/semantics.md "String predicates").

The oracle works on Python `bytes` objects with startswith / endswith / slicing / comparison of
bytes and a LIKE on lists of units; it shares no code with the engine.  A row is `bytes` or None
(null); a result is a list of bool / int / None.
"""
import functools
import operator

import torch

from cylon_amd import Table
from cylon_amd._lib import C

CMP_OPS = {"eq": operator.eq, "ne": operator.ne, "lt": operator.lt, "le": operator.le, "gt": operator.gt,
           "ge": operator.ge}
CMP_CODE = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5}
KIND = {"starts_with": 0, "ends_with": 1, "contains": 2, "like": 3}


def as_bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else (None if x is None else bytes(x))


# ------------------------------------------------------------------ oracle
@functools.lru_cache(maxsize=256)
def units(b: bytes, utf8: bool):
    """The units of a cell: single bytes (binary), or one byte with the continuation bytes after it."""
    if not utf8:
        return tuple(b[i:i + 1] for i in range(len(b)))
    out = []
    for i in range(len(b)):
        if out and 0x80 <= b[i] <= 0xBF:
            out[-1] += b[i:i + 1]
        else:
            out.append(b[i:i + 1])
    return tuple(out)


def like_tokens(pattern: bytes, escape: bytes, utf8: bool):
    """[("lit", unit) | ("one",) | ("any",)]; ValueError for a trailing lone escape."""
    toks, run, i = [], b"", 0

    def flush():
        nonlocal run
        toks.extend(("lit", u) for u in units(run, utf8))
        run = b""
    while i < len(pattern):
        ch = pattern[i:i + 1]
        if ch == escape:
            if i + 1 >= len(pattern):
                raise ValueError("trailing escape")
            run += pattern[i + 1:i + 2]
            i += 2
            continue
        if ch in (b"%", b"_"):
            flush()
            toks.append(("any",) if ch == b"%" else ("one",))
        else:
            run += ch
        i += 1
    flush()
    return toks


def like_recursive(us, toks):
    """The textbook recursive LIKE over a list of units (short cells only: it recurses per unit)."""
    @functools.lru_cache(maxsize=None)
    def m(ti, pi):
        if pi == len(toks):
            return ti == len(us)
        tok = toks[pi]
        if tok[0] == "any":
            return any(m(k, pi + 1) for k in range(ti, len(us) + 1))
        if ti >= len(us):
            return False
        if tok[0] == "one":
            return m(ti + 1, pi + 1)
        return us[ti] == tok[1] and m(ti + 1, pi + 1)
    return m(0, 0)


def like_positions(us, toks):
    """The same relation as a set of reachable unit positions per token (any cell length)."""
    reach = {0}
    for tok in toks:
        if not reach:
            return False
        if tok[0] == "any":
            reach = set(range(min(reach), len(us) + 1))
        elif tok[0] == "one":
            reach = {i + 1 for i in reach if i < len(us)}
        else:
            reach = {i + 1 for i in reach if i < len(us) and us[i] == tok[1]}
    return len(us) in reach


def like_one(cell: bytes, pattern: bytes, escape: bytes = b"\\", utf8: bool = True):
    us, toks = units(cell, utf8), like_tokens(pattern, escape, utf8)
    return like_recursive(tuple(us), tuple(toks)) if len(us) <= 64 else like_positions(us, toks)


def o_map(rows, fn):
    return [None if r is None else fn(r) for r in rows]


def o_compare(rows, other, op):
    """other: bytes / None scalar, or a list of rows."""
    f = CMP_OPS[op]
    if isinstance(other, list):
        return [None if a is None or b is None else f(a, b) for a, b in zip(rows, other)]
    return [None if a is None or other is None else f(a, other) for a in rows]


def o_match(rows, kind, pattern: bytes, escape: bytes = b"\\", utf8: bool = True):
    if kind == "starts_with":
        return o_map(rows, lambda r: r.startswith(pattern))
    if kind == "ends_with":
        return o_map(rows, lambda r: r.endswith(pattern))
    if kind == "contains":
        return o_map(rows, lambda r: pattern in r)
    return o_map(rows, lambda r: like_one(r, pattern, escape, utf8))


def o_length(rows, unit):
    if unit == "bytes":
        return o_map(rows, len)
    return o_map(rows, lambda r: sum(1 for x in r if not 0x80 <= x <= 0xBF))


# ---------------------------------------------------------------- builders
def build_column(ctx, rows, binary=False, name="s", garbage=None, lead=0, force_validity=False):
    """A string / binary column made of torch tensors, zero-copy (as Table.from_torch makes its
    columns): the byte tensor ends exactly at the last row's last byte and begins `lead` bytes into
    its allocation, so its address is unaligned.  A None row is null; its underlying bytes are
    `garbage` (bytes, or a function of the row number), which the engine must never read."""
    chunks, offs, valid, pos = [], [0], [], 0
    for i, r in enumerate(rows):
        if r is None:
            g = garbage(i) if callable(garbage) else (garbage or b"")
            chunks.append(g)
            pos += len(g)
            valid.append(0)
        else:
            chunks.append(r)
            pos += len(r)
            valid.append(1)
        offs.append(pos)
    raw = b"\xee" * lead + b"".join(chunks)
    dev = ctx.device
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)[lead:] if raw else \
        torch.empty(0, dtype=torch.uint8, device=dev)
    offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
    validity = None
    if force_validity or any(v == 0 for v in valid):
        validity = torch.tensor(valid, dtype=torch.uint8, device=dev)
    typ = C.DataType(C.Type.BINARY if binary else C.Type.STRING)
    return C.Column(name, typ, len(rows), data, offsets, validity)


def build_table(ctx, rows, **kw):
    return table_of(ctx, [build_column(ctx, rows, **kw)])


def table_of(ctx, cols):
    return Table(context=ctx, _native=C.Table(ctx._ctx, list(cols)))


def sliced(ctx, rows, lo, hi, pad=b"zzabcab", **kw):
    """rows[lo:hi] as a slice of a longer table, whose neighbours hold bytes that would match."""
    full = [pad] * lo + list(rows) + [pad] * 3
    t = build_table(ctx, full, **kw)
    return t.slice(lo, len(rows))


def col_result(col):
    """values (None where null) of a fixed-width result column, and whether it has a validity array"""
    vals = col.data.cpu().tolist()
    if col.type.type == C.Type.BOOL:
        vals = [bool(v) for v in vals]
    if col.validity is None:
        return vals, False
    valid = col.validity.cpu().tolist()
    return [v if ok else None for v, ok in zip(vals, valid)], True


def result(table, i=0):
    return col_result(table.native.column(i))[0]
