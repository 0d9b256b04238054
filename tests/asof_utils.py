"""Engine-independent oracle for the as-of join (docs/semantics.md "As-of join").

Plain Python over to_pylist() cells.  The right rows are grouped by their `by` key, with the sort's
equality spelled out as one canonical key for null, one for NaN and one for -0.0 / +0.0; rows whose
`on` is null or NaN are dropped; each group is sorted by (on, row number) and every left row is
answered with bisect:
  backward   the last y <= x (< x without exact matches): among equal y the highest row number
  forward    the first y >= x (> x): among equal y the lowest row number
  nearest    the backward and the forward candidate, the nearer one, the backward one on a tie
Distances are Python ints (exact) for integer and temporal `on` columns and one float subtraction for
float ones (0.0 for equal values, so two equal infinities are 0 apart); a match farther away than the
tolerance is dropped, for nearest after the choice.  The result is the right row number per left row,
None for no match, compared with ==.  Nothing is re-sorted."""
import bisect

import pyarrow as pa
import torch

from cylon_amd import Table
from cylon_amd._lib import C
from window_utils import _as_list, _is_nan, _names, _same_cell, traced

DIRECTIONS = ("backward", "forward", "nearest")


def _canon(v):
    if v is None:
        return ("null",)
    if _is_nan(v):
        return ("nan",)
    if isinstance(v, float) and v == 0:
        return 0.0
    return v


def _on_cells(col):
    """the `on` values as Python numbers: temporal types as their integer"""
    typ = col.type
    if pa.types.is_temporal(typ):
        col = col.cast(pa.int32() if typ.bit_width == 32 else pa.int64())
    return col.to_pylist()


def _keys(kw, left, right):
    on = kw.get("on")
    lo, ro = (on, on) if on is not None else (kw["left_on"], kw["right_on"])
    by = kw.get("by")
    lb, rb = (by, by) if by is not None else (kw.get("left_by"), kw.get("right_by"))
    return (_names([lo], left)[0], _names([ro], right)[0], _names(_as_list(lb), left), _names(_as_list(rb), right))


def _distance(a, b):
    if isinstance(a, float):
        return 0.0 if a == b else (a - b if a > b else b - a)
    return abs(a - b)


def expected(left: pa.Table, right: pa.Table, **kw):
    """the right row number of every left row, None for no match"""
    lo, ro, lb, rb = _keys(kw, left, right)
    direction = kw.get("direction", "backward")
    exact = kw.get("allow_exact_matches", True)
    tol = kw.get("tolerance")
    assert direction in DIRECTIONS
    ly, ry = _on_cells(left.column(lo)), _on_cells(right.column(ro))
    lk = list(zip(*[[_canon(v) for v in left.column(c).to_pylist()] for c in lb])) or [()] * left.num_rows
    rk = list(zip(*[[_canon(v) for v in right.column(c).to_pylist()] for c in rb])) or [()] * right.num_rows
    groups = {}
    for j in range(right.num_rows):
        if ry[j] is not None and not _is_nan(ry[j]):
            groups.setdefault(rk[j], []).append((ry[j], j))
    for g in groups.values():
        g.sort()
    ys = {k: [y for y, _ in g] for k, g in groups.items()}
    out = []
    for i in range(left.num_rows):
        x, g = ly[i], groups.get(lk[i])
        if x is None or _is_nan(x) or not g:
            out.append(None)
            continue
        y = ys[lk[i]]
        b = (bisect.bisect_right(y, x) if exact else bisect.bisect_left(y, x)) - 1
        f = bisect.bisect_left(y, x) if exact else bisect.bisect_right(y, x)
        b = g[b] if b >= 0 else None
        f = g[f] if f < len(g) else None
        if direction == "backward":
            m = b
        elif direction == "forward":
            m = f
        elif b is None or (f is not None and _distance(x, f[0]) < _distance(x, b[0])):
            m = f
        else:
            m = b
        if m is not None and tol is not None and not _distance(x, m[0]) <= tol:
            m = None
        out.append(None if m is None else m[1])
    return out


def assert_asof(got: pa.Table, left: pa.Table, right: pa.Table, row_id=None, exp=None, **kw):
    """got = left's columns unchanged in left's row order, then right's columns gathered from the
    expected rows (null for no match), all names prefixed.  row_id: a unique int column of left; got
    may then hold left's rows in any order (distributed results) and is matched by it."""
    if exp is None:
        exp = expected(left, right, **kw)
    lp, rp = kw.get("left_prefix", ""), kw.get("right_prefix", "")
    names = [lp + c for c in left.column_names] + [rp + c for c in right.column_names]
    assert got.column_names == names, (got.column_names, names)
    assert got.num_rows == left.num_rows, (got.num_rows, left.num_rows)
    nlc = left.num_columns
    if row_id is None:
        at = list(range(left.num_rows))
    else:
        where = {v: i for i, v in enumerate(left.column(row_id).to_pylist())}
        at = [where[v] for v in got.column(left.column_names.index(row_id)).to_pylist()]
        assert sorted(at) == list(range(left.num_rows))
    for c in range(nlc):
        assert got.column(c).type == left.column(c).type, names[c]
        g, e = got.column(c).to_pylist(), left.column(c).to_pylist()
        assert all(_same_cell(g[k], e[at[k]]) for k in range(len(g))), "left column %s changed" % names[c]
    for c in range(right.num_columns):
        col = got.column(nlc + c)
        assert col.type == right.column(c).type, names[nlc + c]
        g, src = col.to_pylist(), right.column(c).to_pylist()
        want = [None if exp[at[k]] is None else src[exp[at[k]]] for k in range(len(g))]
        assert col.null_count == sum(w is None for w in want), names[nlc + c]  # null exactly where expected
        for k in range(len(g)):
            assert _same_cell(g[k], want[k]), (names[nlc + c], k, g[k], want[k], exp[at[k]])


def _args(tl: Table, tr: Table, kw):
    k = {n: kw.get(n) for n in ("on", "left_on", "right_on", "by", "left_by", "right_by")}
    return tl._asof_args(tr, k["on"], k["left_on"], k["right_on"], k["by"], k["left_by"], k["right_by"],
                         kw.get("direction", "backward"), kw.get("allow_exact_matches", True), kw.get("tolerance"))


def run_asof(ctx, left: pa.Table, right: pa.Table, carry_step_tiles=0, tables=None, **kw):
    """Table.asof_join on ctx (through C.asof_join when the carry step is lowered)
    -> (arrow result, C.asof_join_indices as a list with None for -1, counters of the table call)"""
    tl, tr = tables if tables is not None else (Table(left, ctx), Table(right, ctx))
    args = _args(tl, tr, kw)
    idx = C.asof_join_indices(tl.native, tr.native, *args, carry_step_tiles)
    assert idx.dtype == torch.int64 and idx.numel() == left.num_rows
    idx = [None if v < 0 else v for v in idx.cpu().tolist()]
    if carry_step_tiles:
        lp, rp = kw.get("left_prefix", ""), kw.get("right_prefix", "")
        got, c = traced(lambda: tl._wrap(C.asof_join(tl.native, tr.native, *args, lp, rp, carry_step_tiles)).to_arrow())
    else:
        got, c = traced(lambda: tl.asof_join(tr, **kw).to_arrow())
    return got, idx, c


def check_asof(ctx, left: pa.Table, right: pa.Table, carry_step_tiles=0, exp=None, tables=None, **kw):
    """Table.asof_join and C.asof_join_indices on ctx against the oracle; returns the trace counters."""
    if exp is None:
        exp = expected(left, right, **kw)
    got, idx, c = run_asof(ctx, left, right, carry_step_tiles, tables, **kw)
    assert idx == exp, [(i, a, b) for i, (a, b) in enumerate(zip(idx, exp)) if a != b][:10]
    assert_asof(got, left, right, exp=exp, **kw)
    if left.num_rows and right.num_rows:
        nearest = kw.get("direction", "backward") == "nearest"
        assert c.get("asof.scan") == (2 if nearest else 1), c
        assert c.get("asof.sort") == (2 if nearest and not kw.get("allow_exact_matches", True) else 1), c
        assert c.get("asof.tiles", 0) >= c["asof.scan"], c
        assert c.get("asof.matched") == sum(e is not None for e in exp), c
    return c
