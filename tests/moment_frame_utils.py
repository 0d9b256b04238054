"""Engine-independent oracle for the framed VAR / STD (docs/semantics.md "Framed aggregates", VAR / STD):
rolling_var / rolling_std over ROWS frames, range_var / range_std over RANGE frames.

Frames.  The order and the partitions come from window_utils.sorted_partitions; inside a partition a
ROWS frame is rolling_utils._partition's rule, [max(j - preceding, 0), min(j + following, len - 1)], and a
RANGE frame is range_frame_utils.frame_bounds over range_frame_utils.order_keys.

Values.  Every non-null value is converted to float64 first.  Per value column the finite images are
put over one power-of-two denominator and the prefix sums of x, x^2 and |x| are Python ints, so per frame

    n,  S = sum x,  mu = S / n,  M2 = sum x^2 - S^2 / n,  A = sum |x|

are exact differences of prefixes (rational arithmetic: nothing cancels), O(1) per frame whatever its
length.  Prefixes of the NaN / +inf / -inf counts decide the non-finite cells, as rolling_utils does.
A cell is null where m < min_periods or m - ddof <= 0 (m = the frame's non-null values, NaN and
infinities included), else NaN where the frame holds a NaN or an infinity, else finite.

Comparison.  As test_moments_oracle.judge: null masks and NaN cells with ==; a finite VAR through
|got (n - ddof) - M2| <= tol, a finite STD through its square, |got^2 - v| <= tol_v + 3 u (v + tol_v) with
v = M2 / (n - ddof), tol_v = tol / (n - ddof); got >= 0 and never -0.0.

The bound tol (derived, not measured).  u = 2^-53; gamma(k) = k u / (1 - k u) >= (1 + u)^k - 1.
test_moments_oracle.tol_m2(loose) is written for ONE flat merge of parts that each meet the tight bound.
A framed result is instead the root of a tree of binary merges (frame_moments_common.hpp)

    d = mean_b - mean_a,  n = n_a + n_b,  mean = mean_a + d (n_b / n),  M2 = M2_a + M2_b + d d (n_a n_b / n)

whose leaves are single values (n = 1, mean = x, M2 = 0, all exact).  A merge with an empty state is
exact (it returns the other state), so only merges of two non-empty states count.  Let D bound the
number of such merges on any path from a leaf to the root.

* D from the frame length w (positions, nulls included).  The query takes one S and one P piece per
  level on which lo and hi lie in different blocks of 8, and then at most 8 entries of the next level.
  A level is crossed only while the range still has w_l >= 2 entries, and the blocks strictly between
  the two pieces leave w_(l+1) <= (w_l - 2) // 8 entries; L(w) = the number of levels crossed.  An entry
  of level l is a chain of 7 merges of entries of level l - 1 (depth 7 l); a P / S piece adds at most 7
  more; the left (right) pieces are chained with one merge per level, so after L levels their depth is
  at most 7 L + 1; the middle run has depth at most 7 L + 7; the two final merges give
  D <= 7 L + 9 <= 8 L + 8 (and D <= 7 for L = 0): at most 8 per level crossed, plus 8.
* Means.  Write m^ = mu + eps for the computed mean of a node.  In exact arithmetic the merged mean of
  perturbed inputs is (n_a m^_a + n_b m^_b) / n = mu + a convex combination of eps_a and eps_b.  The
  computed one is fl(m^_a + fl(fl(m^_b - m^_a) fl(n_b / n))): three roundings on a product of magnitude at
  most |m^_b - m^_a| <= 2 (X + eps), one on a sum of magnitude at most X + eps, where X >= max |x| over
  the frame bounds every exact mean.  So eps_k <= eps_(k-1) (1 + 7 u) + 7 u X (1 + O(u)) with eps_0 = 0,
  and every node of the tree has |eps| <= delta_D = gamma(7 D + 1) X (the + 1 covers the second-order
  terms; 7 D u < 1e-12).  X = min(A, |mu| + sqrt(M2)): every |x| <= A, and (x - mu)^2 <= M2.  For one flat
  pass this is test_moments_oracle's delta = 2 u A with the merge count 7 D / 2 in place of 1.
* Cross terms.  Along the tree M2 = sum over the merge nodes v of c_v = w_v d_v^2 exactly, with
  w_v = n_a n_b / n and d_v = mu_b - mu_a.  The computed d differs from d_v by at most 2 delta_D, so
  |c~_v - c_v| <= w_v (4 delta_D |d_v| + 4 delta_D^2), and by Cauchy-Schwarz
  sum_v w_v |d_v| <= sqrt(W sum_v w_v d_v^2) = sqrt(W M2) with W = sum_v w_v.  w_v <= min(n_a, n_b) <= n_v / 2,
  and a value lies in at most D merge nodes, so W <= n D / 2:
      cross = 4 delta_D sqrt(n D M2 / 2) + 2 n D delta_D^2  =  sqrt(2 D) * [2 delta_D sqrt(n M2)] + 2 D n delta_D^2,
  tol_m2's cross term 2 delta sqrt(n M2) with delta -> delta_D and the factor sqrt(2 D) of the nesting.
* Roundings.  Every term is non-negative, so rounding only scales it: with c~_v = w_v (m^_b - m^_a)^2 of the
  computed means, the computed term carries 8 roundings (the difference d, twice since it is squared, d d,
  n_a n_b, / n, the product, and the two additions of its merge) and then passes through at most D - 1
  further merges of 2 additions each, a factor within (1 + u)^(2 D + 6) of 1:
      rounding = gamma(2 D + 6) (M2 + cross),
  which takes the place of tol_m2's 4 u M2.
* What is left of tol_m2 is its tight form with delta_D for delta,
      (n + 4) u (M2 + n delta_D^2) + n delta_D^2 + 2 u M2,
  whose last term is the division by n - ddof (and the multiplication back); the first terms are kept
  as tol_m2 has them and only add slack of the order n u M2.
tol = tight(delta_D) + cross + rounding.  A one-value frame has D = 0 merges and M2 = 0 exactly.

The self-tests of test_window_moments.py run no project code: a plain-Python pyramid of exactly this
merge meets the bound on every value class, and the textbook sum x^2 - (sum x)^2 / n violates it on the
`offset` and `const` data."""
import math
from fractions import Fraction

import pyarrow as pa

import range_frame_utils as rfu
import window_nav_utils as nu
import window_utils as wu
from cylon_amd import Table
from test_moments_oracle import U, Stats, _ratio, _sqrt_up, tol_m2

MOMENT = ("rolling_var", "rolling_std", "range_var", "range_std")
RADIX = 8


def is_moment(spec):
    return not isinstance(spec, str) and spec[0] in MOMENT


def _gamma(k):
    return k * U / (1 - k * U)


def levels_crossed(w):
    """L(w): the pyramid levels on which a frame of w positions can have lo and hi in different blocks"""
    levels = 0
    while w >= 2:
        levels += 1
        w = (w - 2) // RADIX
    return levels


def merge_depth(w):
    """D(w): at most 8 per level crossed, plus 8; a single position is no merge at all"""
    return 0 if w <= 1 else RADIX * levels_crossed(w) + 8


def tol_frame(st, depth):
    """the bound on |M2^ - M2| of a frame with exact Stats st whose merge tree has depth <= depth"""
    n, M2 = st.n, st.M2
    if depth == 0 or n <= 1:
        return Fraction(0)
    X = min(st.A, abs(st.mu) + _sqrt_up(M2))
    delta = _gamma(7 * depth + 1) * X
    tight = tol_m2(st._replace(A=delta / (2 * U)), False)  # tol_m2's delta is 2 u A
    cross = 4 * delta * _sqrt_up(Fraction(n * depth, 2) * M2) + 2 * n * depth * delta * delta
    return tight + cross + _gamma(2 * depth + 6) * (M2 + cross)


def tol_frame_float(st, depth):
    """tol_frame in float64, term for term (every term is positive: no cancellation, so it is within
    1e-12 of tol_frame, which test_window_moments.py checks).  judge_cell accepts a cell on it only with
    a margin of 1e-6 and falls back to the exact bound otherwise: it saves time, it decides nothing."""
    n, M2 = st.n, float(st.M2)
    if depth == 0 or n <= 1:
        return 0.0
    u = 2.0 ** -53
    X = min(float(st.A), abs(float(st.mu)) + math.sqrt(M2) * (1 + 2.0 ** -40))
    k = 7 * depth + 1
    delta = k * u / (1 - k * u) * X
    tight = (n + 4) * u * (M2 + n * delta * delta) + n * delta * delta + 2 * u * M2
    cross = 4 * delta * math.sqrt(n * depth / 2 * M2) * (1 + 2.0 ** -40) + 2 * n * depth * delta * delta
    k = 2 * depth + 6
    return tight + cross + k * u / (1 - k * u) * (M2 + cross)


# ---- exact frame statistics from prefix sums
class Prefixes:
    """exact prefixes of one partition's values (None = null) as float64 images"""

    def __init__(self, vals):
        ratios = []
        for v in vals:
            f = None if v is None else float(v)
            ratios.append(f.as_integer_ratio() if f is not None and math.isfinite(f) else None)
        self.den = max([d for r in ratios if r is not None for d in (r[1],)], default=1)
        self.cnt, self.s, self.q, self.a, self.bad = [0], [0], [0], [0], [0]
        for v, r in zip(vals, ratios):
            x = 0 if r is None else r[0] * (self.den // r[1])
            self.cnt.append(self.cnt[-1] + (v is not None))
            self.bad.append(self.bad[-1] + (v is not None and r is None))  # NaN, +inf, -inf
            self.s.append(self.s[-1] + x)
            self.q.append(self.q[-1] + x * x)
            self.a.append(self.a[-1] + abs(x))

    def frame(self, lo, hi):
        """(non-null values, how many of them are not finite, Stats of the finite ones) of [lo, hi]"""
        h = hi + 1
        m, bad = self.cnt[h] - self.cnt[lo], self.bad[h] - self.bad[lo]
        n = m - bad
        if n == 0:
            return m, bad, Stats(0, Fraction(0), None, None, Fraction(0), 0)
        S, Q, A, D = self.s[h] - self.s[lo], self.q[h] - self.q[lo], self.a[h] - self.a[lo], self.den
        return m, bad, Stats(n, Fraction(S, D), Fraction(S, n * D), Fraction(n * Q - S * S, n * D * D), Fraction(A, D), 0)


def rows_bounds(n, pre, fol):
    """rolling_utils._partition's frames"""
    lo = [max(j - pre, 0) if pre is not None else 0 for j in range(n)]
    hi = [min(j + fol, n - 1) if fol is not None else n - 1 for j in range(n)]
    return lo, hi


def _parse(spec):
    spec = tuple(spec)
    minp = spec[4] if len(spec) > 4 else 1
    ddof = spec[5] if len(spec) > 5 else 1
    return spec[0], spec[2], spec[3], minp, ddof


def partition_cells(fn, pf, lo, hi, minp, ddof):
    """per local position: None (null) | nan | ('var' | 'std', ddof, Stats, merge depth)"""
    out = []
    for l, h in zip(lo, hi):
        m, bad, st = pf.frame(l, h)
        if m < minp or m - ddof <= 0:
            out.append(None)
        elif bad:
            out.append(math.nan)
        else:
            out.append((fn[-3:], ddof, st, merge_depth(h - l + 1)))
    return out


def default_name(spec, t):
    return wu.default_name(tuple(spec)[:2], t)


def expected(t: pa.Table, partition_by, order_by, ascending, funcs: dict) -> dict:
    """output name -> list over the INPUT rows, for the moment specs of funcs only"""
    parts = keys = kind = None
    prefixes, bounds, out = {}, {}, {}
    for name, spec in funcs.items():
        if not is_moment(spec):
            continue
        if parts is None:
            parts = wu.sorted_partitions(t, partition_by, order_by, ascending)
        fn, pre, fol, minp, ddof = _parse(spec)
        colname = wu._names([spec[1]], t)[0]
        if colname not in prefixes:
            cells = t.column(colname).to_pylist()
            prefixes[colname] = [Prefixes([cells[r] for r in rows]) for rows, _ in parts]
        bkey = (fn.startswith("range_"), pre, fol)
        if bkey not in bounds:
            if bkey[0]:
                if keys is None:
                    keys, kind = rfu.order_keys(t, order_by)
                asc = ascending if isinstance(ascending, bool) else list(ascending)[0]
                bounds[bkey] = [rfu.frame_bounds([keys[r] for r in rows], kind, asc, pre, fol) for rows, _ in parts]
            else:
                bounds[bkey] = [rows_bounds(len(rows), pre, fol) for rows, _ in parts]
        res = [None] * t.num_rows
        for (rows, _), pf, (lo, hi) in zip(parts, prefixes[colname], bounds[bkey]):
            for r, v in zip(rows, partition_cells(fn, pf, lo, hi, minp, ddof)):
                res[r] = v
        out[name if name else default_name(spec, t)] = res
    return out


def judge_cell(got, exp):
    """(verdict, error / bound): verdict None = right; ratio None = an exact comparison"""
    if exp is None:
        return (None if got is None else f"{got!r} where null is due"), None
    if got is None:
        return "null where a value is due", None
    if isinstance(exp, float):  # NaN
        return (None if got != got else f"{got!r} where NaN is due"), None
    op, ddof, st, depth = exp
    if not got >= 0 or math.copysign(1.0, got) < 0:
        return f"{op} {got!r} is negative, -0.0 or NaN", None
    if math.isinf(got):
        return f"{op} {got!r}", None
    n = st.n
    err = abs(Fraction(got) ** (1 if op == "var" else 2) * (n - ddof) - st.M2)  # of M2, exactly
    quick = tol_frame_float(st, depth)  # the std's own 3 u (v + tol_v) only adds to it
    if float(err) <= quick * (1 - 1e-6):
        return None, (float(err) / quick if quick > 0 else 0.0)
    t2 = tol_frame(st, depth)
    if op == "var":
        tol = t2
    else:
        v, tv = st.M2 / (n - ddof), t2 / (n - ddof)
        err, tol = abs(Fraction(got) ** 2 - v), tv + 3 * U * (v + tv)
    return (None if err <= tol else f"{op} {got!r} (exact M2 {float(st.M2)!r}, n {n}, depth {depth})"), _ratio(err, tol)


def assert_moments(got: pa.Table, t: pa.Table, partition_by, order_by, ascending, funcs: dict, row_id=None, exp=None,
                   what=""):
    """got = t's columns, then one column per entry of funcs.  Moment columns are held to this oracle,
    every other column to the oracle of its kind.  Returns the worst error / bound of the moment cells."""
    names = [n if n else (nu.default_name(s, t) if nu._spec(s)[0] in nu.NAV else default_name(nu._spec(s), t))
             for n, s in funcs.items()]
    assert got.num_rows == t.num_rows, (got.num_rows, t.num_rows)
    assert got.column_names == t.column_names + names, (got.column_names, names)
    if exp is None:
        exp = expected(t, partition_by, order_by, ascending, funcs)
    if row_id is None:
        at = list(range(t.num_rows))
    else:
        where = {v: i for i, v in enumerate(t.column(row_id).to_pylist())}
        at = [where[v] for v in got.column(row_id).to_pylist()]
        assert sorted(at) == list(range(t.num_rows))
    worst, bad = 0.0, []
    for name, spec in zip(names, funcs.values()):
        if not is_moment(spec):
            continue
        assert got.column(name).type == pa.float64(), (name, got.column(name).type)
        g, e = got.column(name).to_pylist(), exp[name]
        for k in range(len(g)):
            verdict, ratio = judge_cell(g[k], e[at[k]])
            if ratio is not None:
                worst = max(worst, ratio)
            if verdict is not None:
                bad.append((name, k, verdict, ratio))
    print(f"[window moments] {what}: worst error / bound {worst:.3g}")
    assert not bad, f"{what}: {len(bad)} cells off, (column, row, what, error / bound): {bad[:6]}"
    # the other specs of a mixed call
    nav = {n: s for n, s in zip(names, funcs.values()) if nu._spec(s)[0] in nu.NAV}
    rest = {n: s for n, s in zip(names, funcs.values()) if not is_moment(s) and n not in nav}
    if nav:
        nu.assert_nav(got.select(t.column_names + list(nav)), t, partition_by, order_by, ascending, nav, row_id=row_id)
    if rest:
        rfu.assert_range(got.select(t.column_names + list(rest)), t, partition_by, order_by, ascending, rest,
                         row_id=row_id)
    if not nav and not rest:
        for c in t.column_names:
            assert got.column(c).type == t.column(c).type, c
            g, e = got.column(c).to_pylist(), t.column(c).to_pylist()
            assert all(wu._same_cell(g[k], e[at[k]]) for k in range(len(g))), "input column %s changed" % c
    return worst


def check_moments(ctx, t: pa.Table, partition_by, order_by, ascending, funcs, exp=None, what=""):
    """Table.window on ctx against the oracle; returns (trace counters, worst error / bound)"""
    got, c = wu.traced(lambda: Table(t, ctx).window(partition_by, order_by, ascending, funcs).to_arrow())
    worst = assert_moments(got, t, partition_by, order_by, ascending, funcs, exp=exp, what=what)
    if t.num_rows:
        assert c.get("window.frame.moment", 0) == sum(is_moment(s) for s in funcs.values()), c
        cols = {wu._names([s[1]], t)[0] for s in funcs.values() if is_moment(s)}
        assert c.get("window.moment.pyramids", 0) == len(cols), c
    return c, worst
