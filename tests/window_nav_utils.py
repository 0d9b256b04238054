"""Engine-independent oracle for the navigation and distribution window functions (docs/semantics.md
"Navigation and distribution functions"): FIRST / LAST / NTH_VALUE, FFILL / BFILL, NTILE, PERCENT_RANK and
CUME_DIST.

The rows are put into window order by window_utils.sorted_partitions and every partition is walked with
plain loops over Python cells (None = null; NaN is a value).  Everything is compared with == in input row
order, null positions included: a fill or a navigation function copies a cell, so floats must come back
bit for bit (NaN as NaN, -0.0 as -0.0), and the two float64 distribution functions are one correctly
rounded division of two Python ints."""
import math

import pyarrow as pa

from cylon_amd import Table
from cylon_amd._lib import C
from window_utils import _as_list, _cells, _names, sorted_partitions, traced

NO_COLUMN = ("ntile", "percent_rank", "cume_dist")
NAV = ("first_value", "last_value", "nth_value", "ffill", "bfill") + NO_COLUMN


def _spec(spec):
    return (spec,) if isinstance(spec, str) else tuple(spec)


def default_name(spec, t):
    spec = _spec(spec)
    return spec[0] if spec[0] in NO_COLUMN else "%s_%s" % (spec[0], _names([spec[1]], t)[0])


def result_type(t, spec):
    spec = _spec(spec)
    if spec[0] == "ntile":
        return pa.int64()
    if spec[0] in NO_COLUMN:
        return pa.float64()
    return t.column(_names([spec[1]], t)[0]).type


def _fill(cells, rows, limit):
    """the cells of `rows` with every null replaced by the last non-null cell at most `limit` rows back"""
    out, last = [], None
    for j, r in enumerate(rows):
        if cells[r] is not None:
            last = j
        ok = last is not None and (limit is None or j - last <= limit)
        out.append(cells[rows[last]] if ok else None)
    return out


def _ntile(s, k):
    """buckets of sizes that differ by at most one, the larger ones first"""
    q, m = divmod(s, k)
    out = []
    for b in range(min(k, s)):  # the buckets past the s-th are empty
        out += [b + 1] * (q + 1 if b < m else q)
    assert len(out) == s
    return out


def expected(t: pa.Table, partition_by, order_by, ascending, funcs: dict) -> dict:
    """output name -> list over the INPUT rows"""
    parts = sorted_partitions(t, partition_by, order_by, ascending)
    out = {}
    for name, spec in funcs.items():
        spec = _spec(spec)
        fn = spec[0]
        assert fn in NAV, fn
        res = [None] * t.num_rows
        cells = None if fn in NO_COLUMN else _cells(t.column(_names([spec[1]], t)[0]))
        for rows, peers in parts:
            s = len(rows)
            if fn in ("first_value", "last_value"):
                ignore = len(spec) > 2 and bool(spec[2])
                walk = rows if fn == "first_value" else rows[::-1]
                v = None
                for r in walk:
                    v = cells[r]
                    if v is not None or not ignore:
                        break
                vals = [v] * s
            elif fn == "nth_value":
                vals = [cells[rows[spec[2] - 1]] if spec[2] <= s else None] * s
            elif fn == "ffill":
                vals = _fill(cells, rows, spec[2] if len(spec) > 2 else None)
            elif fn == "bfill":
                vals = _fill(cells, rows[::-1], spec[2] if len(spec) > 2 else None)[::-1]
            elif fn == "ntile":
                vals = _ntile(s, spec[1])
            elif fn == "percent_rank":
                vals, rank = [], 0
                for j in range(s):
                    if j == 0 or peers[j] != peers[j - 1]:
                        rank = j + 1
                    vals.append(0.0 if s == 1 else (rank - 1) / (s - 1))
            else:  # cume_dist: the rows at or before the row's last peer
                vals = [0.0] * s
                j = s - 1
                last = s
                while j >= 0:
                    if j < s - 1 and peers[j] != peers[j + 1]:
                        last = j + 1
                    vals[j] = last / s
                    j -= 1
            for r, v in zip(rows, vals):
                res[r] = v
        out[name if name else default_name(spec, t)] = res
    return out


def same_cell(g, e):
    if g is None or e is None:
        return g is None and e is None
    if isinstance(e, float):
        if e != e:
            return isinstance(g, float) and g != g
        return g == e and math.copysign(1.0, g) == math.copysign(1.0, e)
    return g == e and type(g) is type(e)


def assert_nav(got: pa.Table, t: pa.Table, partition_by, order_by, ascending, funcs: dict, row_id=None, exp=None):
    """got = t's columns unchanged in t's row order, then the oracle's columns.  row_id: a unique int column
    of t; got may then hold t's rows in any order (distributed results) and is matched by it."""
    if exp is None:
        exp = expected(t, partition_by, order_by, ascending, funcs)
    assert got.column_names == t.column_names + list(exp), (got.column_names, list(exp))
    assert got.num_rows == t.num_rows, (got.num_rows, t.num_rows)
    if row_id is None:
        at = list(range(t.num_rows))
    else:
        where = {v: i for i, v in enumerate(t.column(row_id).to_pylist())}
        at = [where[v] for v in got.column(row_id).to_pylist()]
        assert sorted(at) == list(range(t.num_rows))
    for c in t.column_names:
        g, e = _cells(got.column(c)), _cells(t.column(c))
        assert got.column(c).type == t.column(c).type, c
        assert all(same_cell(g[k], e[at[k]]) for k in range(len(g))), "input column %s changed" % c
    for (name, e), spec in zip(exp.items(), funcs.values()):
        assert got.column(name).type == result_type(t, spec), (name, got.column(name).type)
        g = _cells(got.column(name))
        for k in range(len(g)):
            assert same_cell(g[k], e[at[k]]), (name, k, g[k], e[at[k]])


def run_nav(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, carry_step_tiles=0, table=None):
    """Table.window on ctx (through C.window_nav when the carry step is lowered) -> (arrow result, counters)"""
    tt = table if table is not None else Table(t, ctx)
    if carry_step_tiles:
        args = tt._window_nav_args(partition_by, order_by, ascending, funcs)
        return traced(lambda: tt._wrap(C.window_nav(tt.native, *args, carry_step_tiles)).to_arrow())
    return traced(lambda: tt.window(partition_by, order_by, ascending, funcs).to_arrow())


def check_nav(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, carry_step_tiles=0, exp=None):
    """Table.window on ctx against the oracle; returns the trace counters."""
    got, c = run_nav(ctx, t, partition_by, order_by, ascending, funcs, carry_step_tiles)
    assert_nav(got, t, partition_by, order_by, ascending, funcs, exp=exp)
    if t.num_rows and funcs:
        assert c.get("window.sort") == (1 if _as_list(partition_by) or _as_list(order_by) else 0), c
        assert c.get("window.tiles", 0) == c.get("window.scan", 0) * -(-t.num_rows // C.window_tile_rows()), c
    return c
