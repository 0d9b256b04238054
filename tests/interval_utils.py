"""Engine-independent oracle for the interval join (docs/semantics.md "Interval join").

Plain Python over to_pylist() cells.  The right rows are grouped by their `by` key, with the sort's
equality spelled out as one canonical key for null, one for NaN and one for -0.0 / +0.0; rows whose
`on` is null or NaN are dropped; each group is sorted by (on, row number).  A left row whose bounds are
neither null nor NaN is answered with two bisects over its group's `on` values:
  first   bisect_left(lower) where the lower end is closed ("both", "left"), else bisect_right(lower)
  end     bisect_right(upper) where the upper end is closed ("both", "right"), else bisect_left(upper)
and owns the group's rows [first, end) in that order (none when end <= first).  The result is the list
of (left row, right row) pairs ordered by left row, then right `on`, then right row; how="left" puts
(left row, None) in the place of a left row without a match.  Nothing is re-sorted."""
import bisect

import pyarrow as pa
import torch

from cylon_amd import Table
from cylon_amd._lib import C
from asof_utils import _canon, _on_cells
from window_utils import _as_list, _is_nan, _names, _same_cell, traced

CLOSED = ("both", "left", "right", "neither")
HOWS = ("inner", "left")


def _keys(kw, left, right):
    by = kw.get("by")
    lb, rb = (by, by) if by is not None else (kw.get("left_by"), kw.get("right_by"))
    return (_names([kw["lower"]], left)[0], _names([kw["upper"]], left)[0], _names([kw["on"]], right)[0],
            _names(_as_list(lb), left), _names(_as_list(rb), right))


def _usable(v):
    return v is not None and not _is_nan(v)


def expected(left: pa.Table, right: pa.Table, **kw):
    """the (left row, right row | None) pairs in the specified order"""
    lo, up, on, lb, rb = _keys(kw, left, right)
    closed, how = kw.get("closed", "both"), kw.get("how", "inner")
    assert closed in CLOSED and how in HOWS
    lows, ups, ry = _on_cells(left.column(lo)), _on_cells(left.column(up)), _on_cells(right.column(on))
    lk = list(zip(*[[_canon(v) for v in left.column(c).to_pylist()] for c in lb])) or [()] * left.num_rows
    rk = list(zip(*[[_canon(v) for v in right.column(c).to_pylist()] for c in rb])) or [()] * right.num_rows
    groups = {}
    for j in range(right.num_rows):
        if _usable(ry[j]):
            groups.setdefault(rk[j], []).append((ry[j], j))
    for g in groups.values():
        g.sort()
    ys = {k: [y for y, _ in g] for k, g in groups.items()}
    pairs = []
    for i in range(left.num_rows):
        g = groups.get(lk[i])
        own = []
        if g and _usable(lows[i]) and _usable(ups[i]):
            y = ys[lk[i]]
            first = bisect.bisect_left(y, lows[i]) if closed in ("both", "left") else bisect.bisect_right(y, lows[i])
            end = bisect.bisect_right(y, ups[i]) if closed in ("both", "right") else bisect.bisect_left(y, ups[i])
            own = [j for _, j in g[first:end]]
        if own:
            pairs += [(i, j) for j in own]
        elif how == "left":
            pairs.append((i, None))
    return pairs


def counts_of(pairs, nl):
    c = [0] * nl
    for i, j in pairs:
        c[i] += j is not None
    return c


def assert_table(got: pa.Table, left: pa.Table, right: pa.Table, pairs, **kw):
    """got = Gather(left, li) ++ GatherNullable(right, ri) of the pairs, cell for cell"""
    lp, rp = kw.get("left_prefix", ""), kw.get("right_prefix", "")
    names = [lp + c for c in left.column_names] + [rp + c for c in right.column_names]
    assert got.column_names == names, (got.column_names, names)
    assert got.num_rows == len(pairs), (got.num_rows, len(pairs))
    nlc = left.num_columns
    for c in range(nlc):
        assert got.column(c).type == left.column(c).type, names[c]
        g, src = got.column(c).to_pylist(), left.column(c).to_pylist()
        assert got.column(c).null_count == sum(src[i] is None for i, _ in pairs), names[c]
        assert all(_same_cell(g[k], src[i]) for k, (i, _) in enumerate(pairs)), "left column %s" % names[c]
    for c in range(right.num_columns):
        col = got.column(nlc + c)
        assert col.type == right.column(c).type, names[nlc + c]
        g, src = col.to_pylist(), right.column(c).to_pylist()
        want = [None if j is None else src[j] for _, j in pairs]
        assert col.null_count == sum(w is None for w in want), names[nlc + c]  # null exactly where expected
        for k in range(len(g)):
            assert _same_cell(g[k], want[k]), (names[nlc + c], k, g[k], want[k], pairs[k])


def assert_multiset(got: pa.Table, left: pa.Table, right: pa.Table, pairs, left_id, right_id, **kw):
    """got holds the rows of assert_table in any order (distributed results): they are matched by a
    unique int column of each side (right_id null in a filler row) and compared as a multiset"""
    lp, rp = kw.get("left_prefix", ""), kw.get("right_prefix", "")
    lw = {v: i for i, v in enumerate(left.column(left_id).to_pylist())}
    rw = {v: j for j, v in enumerate(right.column(right_id).to_pylist())}
    gl, gr = got.column(lp + left_id).to_pylist(), got.column(rp + right_id).to_pylist()
    seen = [(lw[a], None if b is None else rw[b]) for a, b in zip(gl, gr)]
    key = lambda p: (p[0], -1 if p[1] is None else p[1])
    order = sorted(range(len(seen)), key=lambda k: key(seen[k]))
    assert [seen[k] for k in order] == sorted(pairs, key=key)
    assert_table(got.take(pa.array(order, pa.int64())), left, right, sorted(pairs, key=key), **kw)


def _args(tl: Table, tr: Table, kw, with_how=True):
    k = {n: kw.get(n) for n in ("lower", "upper", "on", "by", "left_by", "right_by")}
    return tl._interval_args(tr, k["lower"], k["upper"], k["on"], k["by"], k["left_by"], k["right_by"],
                             kw.get("closed", "both"), kw.get("how", "inner") if with_how else None)


def check_interval(ctx, left: pa.Table, right: pa.Table, carry_step_tiles=0, exp=None, tables=None, **kw):
    """C.interval_join_indices, C.interval_join_counts and Table.interval_join on ctx against the oracle;
    returns the trace counters of the table call.  The counters are held where both sides have rows
    (nothing is sorted otherwise)."""
    if exp is None:
        exp = expected(left, right, **kw)
    tl, tr = tables if tables is not None else (Table(left, ctx), Table(right, ctx))
    args = _args(tl, tr, kw)
    li, ri = C.interval_join_indices(tl.native, tr.native, *args, carry_step_tiles)
    assert li.dtype == torch.int64 and ri.dtype == torch.int64 and li.numel() == ri.numel()
    got = list(zip(li.cpu().tolist(), [None if v < 0 else v for v in ri.cpu().tolist()]))
    assert len(got) == len(exp), (len(got), len(exp))
    assert got == exp, [(k, a, b) for k, (a, b) in enumerate(zip(got, exp)) if a != b][:10]
    cnt = C.interval_join_counts(tl.native, tr.native, *_args(tl, tr, kw, with_how=False), carry_step_tiles)
    assert cnt.dtype == torch.int64 and cnt.cpu().tolist() == counts_of(exp, left.num_rows)
    lp, rp = kw.get("left_prefix", ""), kw.get("right_prefix", "")
    if carry_step_tiles:
        out, c = traced(lambda: tl._wrap(C.interval_join(tl.native, tr.native, *args, lp, rp, carry_step_tiles)).to_arrow())
    else:
        out, c = traced(lambda: tl.interval_join(tr, **kw).to_arrow())
    assert_table(out, left, right, exp, **kw)
    if left.num_rows and right.num_rows:
        T = C.interval_tile_rows()
        assert c.get("interval.sort") == 1, c
        assert c.get("interval.rank_tiles") == -(-(right.num_rows + 2 * left.num_rows) // C.window_tile_rows()), c
        assert c.get("interval.pairs") == len(exp), c
        assert c.get("interval.matched") == sum(j is not None for _, j in exp), c
        if exp:
            assert c.get("interval.tiles") == -(-len(exp) // T), c
    return c
