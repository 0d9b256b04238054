"""Engine-independent oracle for the framed aggregates (docs/semantics.md "Framed aggregates").

The order and the partitions come from window_utils.sorted_partitions.  Inside a partition the frame
of local position j is [max(j - preceding, 0), min(j + following, len - 1)], and the engine's block
scans are not imitated:
  * counts, integer sums, exact float sums and A = the sum of magnitudes are differences of exact
    prefixes (Python int / fractions.Fraction: nothing is lost by subtracting);
  * NaN, +inf and -inf are counted by prefixes of their own and decide the float result of exactly
    the frames that hold them;
  * min / max slide a monotonic deque over the order images.
A float sum comes as (exact sum, gamma_m A), a mean as (exact mean, gamma_{m+1} A / m), with
gamma_k = k u / (1 - k u), u = 2^-53, m = the frame's non-null values.  Everything else, null positions
included, is compared with ==, in input row order."""
import math
from collections import deque
from fractions import Fraction

import pyarrow as pa

import window_utils as wu
from cylon_amd import Table

U = wu.U
ROLLING = ("rolling_count", "rolling_sum", "rolling_mean", "rolling_min", "rolling_max")


def is_rolling(spec):
    return not isinstance(spec, str) and spec[0] in ROLLING


def _gamma(k):
    return k * U / (1 - k * U)


def default_name(spec, t):
    return wu.default_name(tuple(spec)[:2], t)


def result_type(t, spec):
    if not is_rolling(spec):
        return wu.result_type(t, spec)
    fn = spec[0]
    if fn == "rolling_count":
        return pa.int64()
    if fn == "rolling_mean":
        return pa.float64()
    typ = t.column(wu._names([spec[1]], t)[0]).type
    if fn == "rolling_sum":
        return wu.result_type(t, ("cumsum", spec[1]))
    return typ


def _extremes(vals, lo, hi, smallest):
    """min (max) of vals[lo[j] .. hi[j]] by order image, None skipped; lo and hi never decrease"""
    out, dq, nxt = [], deque(), 0  # dq: positions whose images increase (decrease) towards the back
    for j in range(len(vals)):
        while nxt <= hi[j]:
            v = vals[nxt]
            if v is not None:
                k = wu._image_key(v)
                while dq and (wu._image_key(vals[dq[-1]]) >= k if smallest else wu._image_key(vals[dq[-1]]) <= k):
                    dq.pop()
                dq.append(nxt)
            nxt += 1
        while dq and dq[0] < lo[j]:
            dq.popleft()
        out.append(vals[dq[0]] if dq else None)
    return out


def _partition(fn, vals, typ, pre, fol, minp):
    n = len(vals)
    lo = [max(j - pre, 0) if pre is not None else 0 for j in range(n)]
    hi = [min(j + fol, n - 1) if fol is not None else n - 1 for j in range(n)]
    cnt = [0]
    for v in vals:
        cnt.append(cnt[-1] + (v is not None))
    m = [cnt[hi[j] + 1] - cnt[lo[j]] for j in range(n)]
    if fn == "rolling_count":
        return m
    if fn in ("rolling_min", "rolling_max"):
        ext = _extremes(vals, lo, hi, fn == "rolling_min")
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
                out.append((tot, _gamma(k) * mag))
            else:
                out.append((tot / k, _gamma(k + 1) * mag / k))
        elif fn == "rolling_sum":
            out.append(wu._wrap(tot, typ))
        else:  # the wrapped integer sum, converted and divided: two roundings
            wrapped = wu._wrap(tot, typ)
            out.append((Fraction(wrapped, k), _gamma(k + 1) * Fraction(max(mag, abs(wrapped)), k)))
    return out


def expected(t: pa.Table, partition_by, order_by, ascending, funcs: dict) -> dict:
    """output name -> list over the INPUT rows; a bounded float cell is (exact value, bound)"""
    parts = None
    out = {}
    for name, spec in funcs.items():
        if not is_rolling(spec):
            out.update(wu.expected(t, partition_by, order_by, ascending, {name: spec}))
            continue
        if parts is None:
            parts = wu.sorted_partitions(t, partition_by, order_by, ascending)
        spec = tuple(spec)
        fn, pre, fol = spec[0], spec[2], spec[3]
        minp = spec[4] if len(spec) > 4 else 1
        col = t.column(wu._names([spec[1]], t)[0])
        cells, res = col.to_pylist(), [None] * t.num_rows
        for rows, _ in parts:
            for r, v in zip(rows, _partition(fn, [cells[r] for r in rows], col.type, pre, fol, minp)):
                res[r] = v
        out[name if name else default_name(spec, t)] = res
    return out


def assert_rolling(got: pa.Table, t: pa.Table, partition_by, order_by, ascending, funcs: dict, row_id=None, exp=None):
    """as window_utils.assert_window, for specs of both kinds"""
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
        g, e = got.column(c).to_pylist(), t.column(c).to_pylist()
        assert got.column(c).type == t.column(c).type, c
        assert all(wu._same_cell(g[k], e[at[k]]) for k in range(len(g))), "input column %s changed" % c
    for (name, e), spec in zip(exp.items(), funcs.values()):
        assert got.column(name).type == result_type(t, spec), (name, got.column(name).type)
        g = got.column(name).to_pylist()
        for k in range(len(g)):
            ek = e[at[k]]
            if isinstance(ek, tuple):  # exact value and bound
                assert g[k] is not None and math.isfinite(g[k]), (name, k, g[k], float(ek[0]))
                err = abs(Fraction(g[k]) - ek[0])
                assert err <= ek[1], (name, k, g[k], float(ek[0]), float(err), float(ek[1]))
            else:
                assert wu._same_cell(g[k], ek), (name, k, g[k], ek)


def frame_counters(t, funcs, lds_rows):
    """the (window.frame.lds, window.frame.wide) counts of a call"""
    n, lds, wide = t.num_rows, 0, 0
    for spec in funcs.values():
        if is_rolling(spec):
            w = min(n if spec[2] is None else spec[2], n) + min(n if spec[3] is None else spec[3], n) + 1
            lds, wide = lds + (w <= lds_rows), wide + (w > lds_rows)
    return lds, wide


def check_rolling(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, exp=None, lds_rows=None):
    """Table.window on ctx against the oracle; returns the trace counters"""
    got, c = wu.traced(lambda: Table(t, ctx).window(partition_by, order_by, ascending, funcs).to_arrow())
    assert_rolling(got, t, partition_by, order_by, ascending, funcs, exp=exp)
    if t.num_rows and lds_rows is not None:
        assert (c.get("window.frame.lds", 0), c.get("window.frame.wide", 0)) == frame_counters(t, funcs, lds_rows), c
    return c
