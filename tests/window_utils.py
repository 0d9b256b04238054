"""Engine-independent oracle for the window functions (docs/semantics.md "Window functions").

Rows are ordered by a Python sort key that spells the documented order out: per key column the pair
(class, rank) with class 0 = a number or string, 1 = NaN, 2 = null -- so NaN follows every number and
null follows NaN in both directions --, rank = the position of the value among the column's distinct
values (-0.0 == +0.0), negated for a descending order column; partition columns always ascend; ties
keep the row number.  Each partition is then walked with plain loops.

Float running sums are exact (fractions.Fraction over the prefix) and come with the bound
gamma_m * A_m, gamma_m = m u / (1 - m u), u = 2^-53, m = non-null values of the partition up to the row,
A_m = the sum of their magnitudes.  Everything else is compared with ==, null positions included, in
input row order: nothing is re-sorted."""
from fractions import Fraction

import pyarrow as pa

from cylon_amd import Table
from cylon_amd._lib import C

U = Fraction(1, 2 ** 53)
RANKING = ("row_number", "rank", "dense_rank")


def _is_nan(v):
    return isinstance(v, float) and v != v


def _cells(col):
    return col.to_pylist()


def _column_key(cells, asc):
    distinct = sorted({v for v in cells if v is not None and not _is_nan(v)})
    rank = {v: r for r, v in enumerate(distinct)}  # -0.0 and 0.0 hash and compare equal
    out = []
    for v in cells:
        if v is None:
            out.append((2, 0))
        elif _is_nan(v):
            out.append((1, 0))
        else:
            out.append((0, rank[v] if asc else -rank[v]))
    return out


def _names(names, t):
    return [t.column_names[c] if isinstance(c, int) else c for c in names]


def _as_list(x):
    if x is None:
        return []
    return [x] if isinstance(x, (str, int)) else list(x)


def sorted_partitions(t: pa.Table, partition_by, order_by, ascending):
    """[(rows of the partition in window order, their peer keys)] in partition order"""
    part, order = _names(_as_list(partition_by), t), _names(_as_list(order_by), t)
    asc = [ascending] * len(order) if isinstance(ascending, bool) else list(ascending)
    n = t.num_rows
    pk = [_column_key(_cells(t.column(c)), True) for c in part]
    ok = [_column_key(_cells(t.column(c)), a) for c, a in zip(order, asc)]
    pkey = [tuple(k[i] for k in pk) for i in range(n)]
    okey = [tuple(k[i] for k in ok) for i in range(n)]
    rows = sorted(range(n), key=lambda i: (pkey[i], okey[i], i))
    parts = []
    for i in rows:
        if not parts or pkey[parts[-1][0][-1]] != pkey[i]:
            parts.append(([], []))
        parts[-1][0].append(i)
        parts[-1][1].append(okey[i])
    return parts


def _image_key(v):
    """the order of kernels/order_image.hpp: NaN above every number"""
    return (1, 0) if _is_nan(v) else (0, v)


def _wrap(total, typ):
    total &= (1 << 64) - 1
    if pa.types.is_unsigned_integer(typ) or pa.types.is_boolean(typ):
        return total
    return total - (1 << 64) if total >= 1 << 63 else total


def default_name(spec, t):
    spec = (spec,) if isinstance(spec, str) else tuple(spec)
    return spec[0] if spec[0] in RANKING else "%s_%s" % (spec[0], _names([spec[1]], t)[0])


def expected(t: pa.Table, partition_by, order_by, ascending, funcs: dict) -> dict:
    """output name -> list over the INPUT rows; a float cumsum cell is (exact sum, bound) as Fractions"""
    parts = sorted_partitions(t, partition_by, order_by, ascending)
    n = t.num_rows
    out = {}
    for name, spec in funcs.items():
        spec = (spec,) if isinstance(spec, str) else tuple(spec)
        fn = spec[0]
        res = [None] * n
        cells = typ = None
        if fn not in RANKING:
            col = t.column(_names([spec[1]], t)[0])
            cells, typ = _cells(col), col.type
        for rows, peers in parts:
            if fn in RANKING:
                rank = dense = 0
                for j, r in enumerate(rows):
                    if j == 0 or peers[j] != peers[j - 1]:
                        rank, dense = j + 1, dense + 1
                    res[r] = {"row_number": j + 1, "rank": rank, "dense_rank": dense}[fn]
            elif fn == "cumcount":
                c = 0
                for r in rows:
                    c += cells[r] is not None
                    res[r] = c
            elif fn == "cumsum" and pa.types.is_floating(typ):
                s, a, m = Fraction(0), Fraction(0), 0
                for r in rows:
                    if cells[r] is None:
                        continue
                    x = Fraction(cells[r])  # exact; raises on NaN / inf: keep those out of float sums
                    s, a, m = s + x, a + abs(x), m + 1
                    res[r] = (s, m * U / (1 - m * U) * a)
            elif fn == "cumsum":
                s = 0
                for r in rows:
                    if cells[r] is None:
                        continue
                    s += int(cells[r])
                    res[r] = _wrap(s, typ)
            elif fn in ("cummin", "cummax"):
                best = None
                for r in rows:
                    v = cells[r]
                    if v is None:
                        continue
                    if best is None or (_image_key(v) < _image_key(best) if fn == "cummin"
                                        else _image_key(v) > _image_key(best)):
                        best = v
                    res[r] = best
            elif fn in ("lag", "lead"):
                off = spec[2] if len(spec) > 2 else 1
                for j, r in enumerate(rows):
                    k = j - off if fn == "lag" else j + off
                    res[r] = cells[rows[k]] if 0 <= k < len(rows) else None
            else:
                raise ValueError(fn)
        out[name if name else default_name(spec, t)] = res
    return out


def _same_cell(g, e):
    if g is None or e is None:
        return g is None and e is None
    if _is_nan(e):
        return _is_nan(g)
    return g == e and not _is_nan(g)


def result_type(t: pa.Table, spec):
    spec = (spec,) if isinstance(spec, str) else tuple(spec)
    fn = spec[0]
    if fn in RANKING or fn == "cumcount":
        return pa.int64()
    typ = t.column(_names([spec[1]], t)[0]).type
    if fn == "cumsum":
        if pa.types.is_floating(typ):
            return pa.float64()
        return pa.uint64() if pa.types.is_unsigned_integer(typ) or pa.types.is_boolean(typ) else pa.int64()
    return typ


def assert_window(got: pa.Table, t: pa.Table, partition_by, order_by, ascending, funcs: dict, row_id=None, exp=None):
    """got = t's columns unchanged in t's row order, then the oracle's columns.  row_id: a unique int
    column of t; got may then hold t's rows in any order (distributed results) and is matched by it.
    exp: expected(...) of the same arguments, when the caller shares it between contexts."""
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
        assert all(_same_cell(g[k], e[at[k]]) for k in range(len(g))), "input column %s changed" % c
    for (name, e), spec in zip(exp.items(), funcs.values()):
        assert got.column(name).type == result_type(t, spec), (name, got.column(name).type)
        g = _cells(got.column(name))
        for k in range(len(g)):
            ek = e[at[k]]
            if isinstance(ek, tuple):  # a float running sum: exact value and bound
                assert g[k] is not None, (name, k)
                err = abs(Fraction(g[k]) - ek[0])
                assert err <= ek[1], (name, k, g[k], float(ek[0]), float(err), float(ek[1]))
            else:
                assert _same_cell(g[k], ek), (name, k, g[k], ek)


def traced(fn):
    """(result, trace counters of the call)"""
    C.trace_enable(True)
    C.trace_reset()
    try:
        out = fn()
        return out, dict(C.trace_counters())
    finally:
        C.trace_enable(False)


def run_window(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, carry_step_tiles=0, table=None):
    """Table.window on ctx (through C.window when the carry step is lowered) -> (arrow result, counters)"""
    tt = table if table is not None else Table(t, ctx)
    if carry_step_tiles:
        args = tt._window_args(partition_by, order_by, ascending, funcs)
        return traced(lambda: tt._wrap(C.window(tt.native, *args, carry_step_tiles)).to_arrow())
    return traced(lambda: tt.window(partition_by, order_by, ascending, funcs).to_arrow())


def check_window(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, carry_step_tiles=0, exp=None):
    """Table.window on ctx against the oracle; returns the trace counters."""
    got, c = run_window(ctx, t, partition_by, order_by, ascending, funcs, carry_step_tiles)
    assert_window(got, t, partition_by, order_by, ascending, funcs, exp=exp)
    if t.num_rows and funcs:
        assert c.get("window.scan", 0) > 0 and c.get("window.tiles", 0) >= c["window.scan"], c
        assert c.get("window.sort") == (1 if _as_list(partition_by) or _as_list(order_by) else 0), c
    return c
