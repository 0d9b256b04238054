"""Engine-independent oracle for the RANGE frames (docs/semantics.md "Framed aggregates", RANGE).

The order and the partitions come from window_utils.sorted_partitions.  Inside a partition the frame
of a row is [lo, hi] in local positions, straight from the definition:
  * a number's bounded side is the first (last) number whose key is not beyond the bound.  For an
    integer or temporal key the bound is an exact Python integer (o - a never wraps); for a float key
    it is ONE numpy.float64 operation on the key widened to float64 (an integer offset converted
    first), inf - inf = NaN being replaced by the key itself;
  * a NaN or null row's bounded side ends at its peer group (the NaN rows, the null rows);
  * an unbounded side (None) is positional: the partition's first / last row, for every row.
The values then come exactly as rolling_utils computes them from lo / hi: counts, integer sums, exact
float sums and magnitudes as differences of exact prefixes (int / Fraction), NaN and +-inf counted by
prefixes of their own, min / max through rolling_utils._extremes.  A float sum is (exact sum,
gamma_m A), a mean (exact mean, gamma_{m+1} A / m); everything else is compared with ==, null positions
included, in input row order."""
import math
from bisect import bisect_left, bisect_right
from fractions import Fraction

import numpy as np
import pyarrow as pa

import rolling_utils as ru
import window_utils as wu
from cylon_amd import Table

RANGE = ("range_count", "range_sum", "range_mean", "range_min", "range_max")


def is_range(spec):
    return not isinstance(spec, str) and spec[0] in RANGE


def as_rolling(spec):
    """the ROLLING spec whose result rules (type, name pattern aside) the range spec shares"""
    spec = tuple(spec)
    return ("rolling_" + spec[0][len("range_"):],) + spec[1:]


def order_keys(t: pa.Table, order_by):
    """(cells of the one order column as exact Python numbers / None, 'int' | 'float')"""
    name = wu._names(wu._as_list(order_by), t)
    assert len(name) == 1, name
    col = t.column(name[0])
    typ = col.type
    if pa.types.is_floating(typ):
        return col.to_pylist(), "float"
    if pa.types.is_integer(typ):
        return col.to_pylist(), "int"
    width = pa.int32() if typ.bit_width == 32 else pa.int64()  # temporal: the integer in the column's unit
    return col.cast(width).to_pylist(), "int"


def _bound(o, d, minus, kind):
    """the key bound d away from o, below (minus) or above it"""
    if kind == "int":
        return o - d if minus else o + d
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.float64(o) - np.float64(d) if minus else np.float64(o) + np.float64(d)
    return float(o) if math.isnan(b) else float(b)


def frame_bounds(keys, kind, asc, pre, fol):
    """local (lo, hi) per row of a partition whose keys are in window order"""
    n = len(keys)
    cls = [2 if k is None else 1 if wu._is_nan(k) else 0 for k in keys]
    assert cls == sorted(cls)
    first = [cls.index(c) if c in cls else n for c in (0, 1, 2)]
    last = [n - 1 - cls[::-1].index(c) if c in cls else -1 for c in (0, 1, 2)]
    nums = keys[:cls.count(0)]
    walk = nums if asc else [-k for k in nums]  # never decreases; negation is exact
    assert all(walk[j] <= walk[j + 1] for j in range(len(walk) - 1))
    lo, hi = [], []
    for j in range(n):
        c = cls[j]
        if pre is None:
            lo.append(0)
        elif c:
            lo.append(first[c])
        else:  # asc: the first key >= o - pre; desc: the first key <= o + pre
            b = _bound(keys[j], pre, asc, kind)
            lo.append(bisect_left(walk, b if asc else -b))
        if fol is None:
            hi.append(n - 1)
        elif c:
            hi.append(last[c])
        else:  # asc: the last key <= o + fol; desc: the last key >= o - fol
            b = _bound(keys[j], fol, not asc, kind)
            hi.append(bisect_right(walk, b if asc else -b) - 1)
        assert 0 <= lo[-1] <= j <= hi[-1] < n, (j, lo[-1], hi[-1])
    return lo, hi


def frame_values(fn, vals, typ, lo, hi, minp):
    """rolling_utils._partition's values for given frames; fn is a rolling_* name"""
    n = len(vals)
    cnt = [0]
    for v in vals:
        cnt.append(cnt[-1] + (v is not None))
    m = [cnt[hi[j] + 1] - cnt[lo[j]] for j in range(n)]
    if fn == "rolling_count":
        return m
    if fn in ("rolling_min", "rolling_max"):
        ext = ru._extremes(vals, lo, hi, fn == "rolling_min")
        return [ext[j] if m[j] >= minp else None for j in range(n)]
    is_float = pa.types.is_floating(typ)
    s, a, nan, pinf, ninf = [0], [0], [0], [0], [0]
    for v in vals:
        fin = v is not None and not (is_float and (wu._is_nan(v) or math.isinf(v)))
        x = (Fraction(v) if is_float else int(v)) if fin else 0
        s.append(s[-1] + x)
        a.append(a[-1] + abs(x))
        nan.append(nan[-1] + (v is not None and wu._is_nan(v)))
        pinf.append(pinf[-1] + (v is not None and is_float and v == math.inf))
        ninf.append(ninf[-1] + (v is not None and is_float and v == -math.inf))
    out = []
    for j in range(n):
        l, h, k = lo[j], hi[j] + 1, m[j]
        if k < minp:
            out.append(None)
            continue
        tot, mag = s[h] - s[l], a[h] - a[l]
        if is_float:
            if nan[h] - nan[l] or (pinf[h] - pinf[l] and ninf[h] - ninf[l]):
                out.append(math.nan)
            elif pinf[h] - pinf[l] or ninf[h] - ninf[l]:
                out.append(math.inf if pinf[h] - pinf[l] else -math.inf)
            elif fn == "rolling_sum":
                out.append((tot, ru._gamma(k) * mag))
            else:
                out.append((tot / k, ru._gamma(k + 1) * mag / k))
        elif fn == "rolling_sum":
            out.append(wu._wrap(tot, typ))
        else:  # the wrapped integer sum, converted and divided: two roundings
            wrapped = wu._wrap(tot, typ)
            out.append((Fraction(wrapped, k), ru._gamma(k + 1) * Fraction(max(mag, abs(wrapped)), k)))
    return out


def default_name(spec, t):
    return wu.default_name(tuple(spec)[:2], t)


def expected(t: pa.Table, partition_by, order_by, ascending, funcs: dict) -> dict:
    """output name -> list over the INPUT rows; a bounded float cell is (exact value, bound)"""
    parts = keys = kind = None
    bounds = {}
    out = {}
    for name, spec in funcs.items():
        if not is_range(spec):
            out.update(ru.expected(t, partition_by, order_by, ascending, {name: spec}))
            continue
        if parts is None:
            parts = wu.sorted_partitions(t, partition_by, order_by, ascending)
            keys, kind = order_keys(t, order_by)
        asc = ascending if isinstance(ascending, bool) else list(ascending)[0]
        spec = tuple(spec)
        pre, fol = spec[2], spec[3]
        minp = spec[4] if len(spec) > 4 else 1
        if (pre, fol) not in bounds:
            bounds[(pre, fol)] = [frame_bounds([keys[r] for r in rows], kind, asc, pre, fol) for rows, _ in parts]
        col = t.column(wu._names([spec[1]], t)[0])
        cells, res = col.to_pylist(), [None] * t.num_rows
        for (rows, _), (lo, hi) in zip(parts, bounds[(pre, fol)]):
            vals = frame_values(as_rolling(spec)[0], [cells[r] for r in rows], col.type, lo, hi, minp)
            for r, v in zip(rows, vals):
                res[r] = v
        out[name if name else default_name(spec, t)] = res
    return out


def assert_range(got: pa.Table, t: pa.Table, partition_by, order_by, ascending, funcs: dict, row_id=None, exp=None):
    """as rolling_utils.assert_rolling, for specs of every kind"""
    if exp is None:
        exp = expected(t, partition_by, order_by, ascending, funcs)
    typed = {k: as_rolling(s) if is_range(s) else s for k, s in funcs.items()}  # the result types are the twins'
    ru.assert_rolling(got, t, partition_by, order_by, ascending, typed, row_id=row_id, exp=exp)


def check_range(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, exp=None):
    """Table.window on ctx against the oracle; returns the trace counters"""
    got, c = wu.traced(lambda: Table(t, ctx).window(partition_by, order_by, ascending, funcs).to_arrow())
    assert_range(got, t, partition_by, order_by, ascending, funcs, exp=exp)
    if t.num_rows:
        assert c.get("window.frame.range", 0) == sum(is_range(s) for s in funcs.values()), c
    return c
