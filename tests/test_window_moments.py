"""Framed VAR / STD (rolling_var / rolling_std / range_var / range_std) on CPU contexts against the exact
oracle of moment_frame_utils, whose docstring derives the bound.  The self-tests at the top run no project
code.  Every comparison prints its worst error / bound (`pytest -s` shows them)."""
import ctypes
import math
import os
import statistics
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

import cylon_amd.ops as ops
import moment_frame_utils as mu
import window_utils as wu
from cylon_amd import CylonContext, CylonEnv, DataFrame, Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from test_moments_oracle import CLASSES, _values

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "input")
ROWS_FRAMES = [(0, 0), (1, 0), (6, 0), (3, 3), (0, 5), (None, 0), (0, None), (None, None)]
DDOF_MINP = [(0, 1), (1, 1), (2, 1), (1, 3), (0, 3), (2, 3)]


@pytest.fixture(scope="module")
def cpu():
    return CylonContext(config=None, distributed=False, device="cpu")


# ---- self-tests: no project code
def _merge(a, b):
    """the merge of frame_moments_common.hpp on (n, mean, M2, depth); depth counts the merges of two
    non-empty states on the longest path below the state"""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    na, nb = float(a[0]), float(b[0])
    n = na + nb
    d = b[1] - a[1]
    return (a[0] + b[0], a[1] + d * (nb / n), a[2] + b[2] + d * d * (na * nb / n), max(a[3], b[3]) + 1)


IDENT = (0, 0.0, 0.0, 0)


class PyPyramid:
    """the radix-8 two-sided scan pyramid and its query, in plain Python"""

    def __init__(self, xs):
        self.levels = []  # (entries, P, S) per level
        ent = [IDENT if x is None else (1, x, x - x, 0) for x in xs]
        while True:
            P, S = [None] * len(ent), [None] * len(ent)
            nxt = []
            for j0 in range(0, len(ent), 8):
                blk = range(j0, min(j0 + 8, len(ent)))
                acc = IDENT
                for j in blk:
                    acc = _merge(acc, ent[j])
                    P[j] = acc
                nxt.append(acc)
                acc = IDENT
                for j in reversed(blk):
                    acc = _merge(ent[j], acc)
                    S[j] = acc
            self.levels.append((ent, P, S))
            if len(ent) <= 8:
                break
            ent = nxt

    def query(self, lo, hi):
        left = right = mid = IDENT
        for ent, P, S in self.levels:
            if lo >> 3 == hi >> 3:
                for j in range(lo, hi + 1):
                    mid = _merge(mid, ent[j])
                break
            left, right = _merge(left, S[lo]), _merge(P[hi], right)
            lo, hi = (lo >> 3) + 1, (hi >> 3) - 1
            if lo > hi:
                break
        return _merge(_merge(left, mid), right)


def _frames(n, rng, count=300):
    """single rows, runs inside a block, aligned blocks, two blocks, every level's edges, random ones"""
    out = [(0, 0), (n - 1, n - 1), (0, n - 1), (3, 5), (8, 15), (8, 23), (7, 8), (0, 63), (64, 511), (1, n - 2)]
    out += [(8 ** k, 2 * 8 ** k - 1) for k in range(1, 5) if 2 * 8 ** k <= n]
    out += [(8 ** k - 1, 2 * 8 ** k) for k in range(1, 5) if 2 * 8 ** k < n]
    while len(out) < count:
        w = int(rng.integers(1, n + 1)) if len(out) % 2 else int(rng.integers(1, 70))
        lo = int(rng.integers(0, n - w + 1))
        out.append((lo, lo + w - 1))
    return [(lo, hi) for lo, hi in out if 0 <= lo <= hi < n]


@pytest.mark.parametrize("cls", CLASSES)
def test_python_pyramid_meets_the_bound_and_the_textbook_formula_does_not(cls):
    n = 4097
    rng = np.random.default_rng([5, CLASSES.index(cls)])
    raw = _values(cls, rng, n)
    vals = [None if k % 11 == 3 else v for k, v in enumerate(raw.tolist())]
    xs = [None if v is None else float(v) for v in vals]
    pyr, pf = PyPyramid(xs), mu.Prefixes(vals)
    worst, deepest, broke, judged = 0.0, 0, 0, 0
    for lo, hi in _frames(n, rng):
        m, bad, st = pf.frame(lo, hi)
        got = pyr.query(lo, hi)
        assert got[0] == m == st.n and bad == 0
        depth = mu.merge_depth(hi - lo + 1)
        assert got[3] <= depth, (lo, hi, got[3], depth)
        deepest = max(deepest, got[3])
        if m == 0:
            continue
        tol = mu.tol_frame(st, depth)
        err = abs(Fraction(got[2]) - st.M2)
        assert err <= tol, (cls, lo, hi, float(err), float(tol))
        assert got[2] >= 0 and math.copysign(1.0, got[2]) > 0
        worst = max(worst, float(err / tol) if tol else 0.0)
        assert abs(mu.tol_frame_float(st, depth) - float(tol)) <= 1e-12 * float(tol)
        if m >= 2:
            x = np.array([v for v in xs[lo:hi + 1] if v is not None])
            textbook = float(np.dot(x, x) - x.sum() ** 2 / len(x))
            judged += 1
            broke += abs(Fraction(textbook) - st.M2) > tol
    print(f"[window moments] self-test {cls}: pyramid/bound {worst:.3g}, deepest chain {deepest}, "
          f"textbook breaks the bound in {broke} of {judged} frames")
    if cls in ("offset", "const"):
        assert broke > judged // 2, "the textbook formula passes: the data do not discriminate"


def test_merge_depth_is_8_per_level_crossed_plus_8():
    assert [mu.levels_crossed(w) for w in (1, 2, 9, 10, 17, 18, 145, 146, 1170)] == [0, 1, 1, 1, 1, 2, 2, 3, 4]
    assert mu.merge_depth(1) == 0 and mu.merge_depth(2) == 16 and mu.merge_depth(18) == 24
    # the worst alignment of every length reaches no deeper
    pyr = PyPyramid([float(k) for k in range(700)])
    for w in list(range(1, 80)) + [127, 128, 129, 511, 512, 513, 600]:
        assert max(pyr.query(lo, lo + w - 1)[3] for lo in range(0, 700 - w + 1)) <= mu.merge_depth(w), w


def test_oracle_matches_statistics_on_small_frames():
    rng = np.random.default_rng(2)
    vals = [None if k % 5 == 4 else int(v) for k, v in enumerate(rng.integers(-1000, 1000, 60))]
    vals[7], vals[30] = 0.1, -2.5
    pf = mu.Prefixes(vals)
    for lo in range(0, 60, 3):
        for hi in range(lo, min(lo + 14, 60)):
            x = [Fraction(float(v)) for v in vals[lo:hi + 1] if v is not None]
            m, bad, st = pf.frame(lo, hi)
            assert (m, bad, st.n) == (len(x), 0, len(x))
            if x:
                assert st.M2 == statistics.pvariance(x) * len(x) and st.A == sum(abs(v) for v in x)
                assert st.mu == statistics.mean(x)
            if len(x) > 1:
                assert st.M2 / (len(x) - 1) == statistics.variance(x)
    m, bad, st = mu.Prefixes([1.0, math.nan, None, math.inf, 2.0]).frame(0, 4)
    assert (m, bad, st.n, st.S) == (4, 2, 2, 3)


# ---- CPU context against the oracle
def _layout_table(cls, nulls, seed=0):
    """partitions of 1, 2, 7, 8, 9, 65 and 300 rows and one whose values are all null; rows shuffled"""
    rng = np.random.default_rng([seed, CLASSES.index(cls), int(nulls)])
    sizes = [1, 2, 7, 8, 9, 65, 300, 12]
    g = np.repeat(np.arange(len(sizes)), sizes)
    n = len(g)
    v = _values(cls, rng, n)
    mask = (rng.random(n) < 0.25) if nulls else np.zeros(n, bool)
    mask |= g == len(sizes) - 1
    p = rng.permutation(n)
    return pa.table({"g": g[p].astype(np.int32), "o": np.arange(n)[p], "v": pa.array(v[p], mask=mask[p])})


def _all_rows_specs(col="v", frames=ROWS_FRAMES, kind="rolling"):
    f = {}
    for k, (pre, fol) in enumerate(frames):
        for ddof, minp in DDOF_MINP:
            fn = f"{kind}_{'std' if (k + ddof) % 2 else 'var'}"
            f[f"{fn}_{k}_{ddof}_{minp}"] = (fn, col, pre, fol, minp, ddof)
    return f


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("cls", CLASSES)
def test_rows_frames_match_the_oracle(cpu, cls, nulls):
    t = _layout_table(cls, nulls)
    f = _all_rows_specs()
    f["std_default"] = ("rolling_std", "v", 6, 0)  # min_periods 1, ddof 1
    c, _ = mu.check_moments(cpu, t, "g", "o", True, f, what=f"cpu rows {cls}")
    assert c["window.moment.pyramids"] == 1 and "window.range.bounds" not in c, c
    # the expanding form, descending
    mu.check_moments(cpu, t, "g", "o", False, {"e": ("rolling_std", "v", None, 0), "v2": ("rolling_var", "v", 2, 9, 2, 0)},
                     what=f"cpu rows desc {cls}")


def _range_table(order, seed, n=700):
    """order keys with ties; float keys also with -inf / inf, NaN and null keys"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 5, n).astype(np.int32)
    v = pa.array(1e6 + rng.standard_normal(n), mask=rng.random(n) < 0.25)
    k = rng.integers(-200, 200, n)
    if order == "int":
        o = pa.array(k.astype(np.int64))
    elif order == "timestamp":
        o = pa.array((k + 1000) * 1_000_000, pa.timestamp("us"))
    else:
        o = (k / 4.0).astype(np.float64)
        o[rng.random(n) < 0.05] = np.nan
        o[:3], o[3:6] = -np.inf, np.inf
        o = pa.array(o, mask=rng.random(n) < 0.05)
    return pa.table({"g": g, "o": o, "v": v, "w": pa.array(rng.integers(-128, 128, n).astype(np.int8))})


RANGE_FRAMES = {"int": [(0, 0), (3, 0), (0, 40), (25, 25), (None, 2), (1, None), (None, None), (10 ** 12, 0)],
                "timestamp": [(0, 0), (5_000_000, 0), (60_000_000, 60_000_000), (None, 1_000_000), (0, None)],
                "float": [(0.0, 0.0), (0.5, 0.25), (3, 0.75), (2, 2), (None, 1.5), (0.25, None), (None, None),
                          (float("inf"), 0.0)]}


@pytest.mark.parametrize("asc", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("order", ["int", "timestamp", "float"])
def test_range_frames_match_the_oracle(cpu, order, asc):
    t = _range_table(order, 31 + len(order))
    f = _all_rows_specs(frames=RANGE_FRAMES[order], kind="range")
    f["w_std"] = ("range_std", "w", RANGE_FRAMES[order][1][0], RANGE_FRAMES[order][1][1])
    c, _ = mu.check_moments(cpu, t, "g", "o", asc, f, what=f"cpu range {order}")
    assert c["window.range.bounds"] == len(RANGE_FRAMES[order]) and c["window.moment.pyramids"] == 2, c
    assert "window.frame.range" not in c and "window.range.pyramids" not in c, c


def test_non_finite_values(cpu):
    n = 400
    rng = np.random.default_rng(41)
    v = rng.standard_normal(n) * 100
    for k, x in ((5, np.inf), (6, -np.inf), (50, np.nan), (120, np.inf), (121, np.inf), (200, -np.inf), (399, np.nan)):
        v[k] = x
    t = pa.table({"g": np.repeat([0, 1], n // 2).astype(np.int32), "o": np.arange(n),
                  "v": pa.array(v, mask=rng.random(n) < 0.2), "f": pa.array(v.astype(np.float32))})
    f = {"a": ("rolling_var", "v", 3, 3), "b": ("rolling_std", "v", None, 0, 1, 0), "c": ("range_std", "v", 9, 0, 3),
         "d": ("range_var", "f", None, None, 1, 2), "e": ("rolling_std", "f", 0, 0, 1, 0)}
    mu.check_moments(cpu, t, "g", "o", True, f, what="cpu non-finite")
    got = Table(t, cpu).window("g", "o", True, f).to_arrow()
    assert any(x is not None and x != x for x in got["a"].to_pylist())  # NaN is a value, not a null
    # a single infinite value with ddof 0 is NaN (x - x), a finite one is exactly +0.0
    e = got["e"].to_pylist()
    assert e[5] != e[5] and e[50] != e[50] and e[0] == 0.0 and math.copysign(1.0, e[0]) > 0


def test_value_types_and_wide_unsigned(cpu):
    n = 300
    rng = np.random.default_rng(43)
    cols = {"g": rng.integers(0, 3, n).astype(np.int32), "o": rng.permutation(n)}
    for dt in ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64"):
        info = np.iinfo(dt)
        cols[dt] = pa.array(rng.integers(info.min, info.max, n, dtype=dt), mask=rng.random(n) < 0.2)
    cols["uint64"] = pa.array(rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64))
    cols["float32"] = pa.array((1e4 + rng.standard_normal(n)).astype(np.float32))
    t = pa.table(cols)
    f = {}
    for c in t.column_names[2:]:
        f["r_" + c] = ("rolling_std", c, 4, 4)
        f["g_" + c] = ("range_var", c, 20, 0, 2, 0)
    c, _ = mu.check_moments(cpu, t, "g", "o", True, f, what="cpu types")
    assert c["window.moment.pyramids"] == 9 and c["window.range.bounds"] == 1, c


def test_empty_table_and_default_names(cpu):
    e = pa.table({"g": pa.array([], pa.int64()), "o": pa.array([], pa.int64()), "v": pa.array([], pa.float32())})
    f = {"a": ("rolling_var", "v", 1, 1), "b": ("range_std", "v", 1, None), None: ("rolling_std", "v", 0, 0)}
    got = Table(e, cpu).window("g", "o", True, f).to_arrow()
    assert got.num_rows == 0 and got.column_names == ["g", "o", "v", "a", "b", "rolling_std_v"]
    assert [got[c].type for c in ("a", "b", "rolling_std_v")] == [pa.float64()] * 3
    t = pa.table({"g": [1, 1, 2], "o": [1, 2, 3], "v": [1.0, 3.0, 5.0]})
    for fn in mu.MOMENT:
        got = Table(t, cpu).window("g", "o", True, {None: (fn, "v", None, None)}).to_arrow()
        assert got.column_names == ["g", "o", "v", fn + "_v"]
        want = [2.0, 2.0, None] if fn.endswith("var") else [math.sqrt(2.0), math.sqrt(2.0), None]
        assert got[fn + "_v"].to_pylist() == want


# ---- moment specs among the other kinds
def test_mixed_calls(cpu):
    t = _range_table("int", 51)
    f = {"rn": "row_number", "cs": ("cumsum", "w"), "rm": ("rolling_mean", "v", 6, 0), "gs": ("range_sum", "w", 3, 0),
         "ff": ("ffill", "v"), "cd": "cume_dist", "s1": ("rolling_std", "v", 6, 0), "v1": ("range_var", "v", 3, 0),
         "gm": ("range_mean", "v", 3, 0), "s2": ("range_std", "w", 3, 0, 2, 0), "v2": ("rolling_var", "w", None, None)}
    c, _ = mu.check_moments(cpu, t, "g", "o", True, f, what="cpu mixed")
    assert c["window.moment.pyramids"] == 2 and c["window.frame.moment"] == 4, c
    # range_sum, range_mean, range_var and range_std share the one frame (3, 0)
    assert c["window.range.bounds"] == 1 and c["window.frame.range"] == 2, c
    tt = Table(t, cpu)
    all_ = tt.window("g", "o", True, f).to_arrow()
    for name, spec in f.items():
        assert tt.window("g", "o", True, {name: spec}).to_arrow()[name].equals(all_[name]), name


def test_existing_specs_count_what_they_counted(cpu):
    """a call without a moment spec reports no moment counter and the counters it always reported"""
    t = _range_table("int", 52)
    f = {"cs": ("cumsum", "w"), "rs": ("rolling_sum", "w", 2, 1), "wide": ("rolling_max", "w", 400, 400),
         "gs": ("range_sum", "w", 3, 0), "gm": ("range_mean", "v", 3, 0), "rk": "rank"}
    _, c = wu.traced(lambda: Table(t, cpu).window("g", "o", True, f).to_arrow())
    assert not any("moment" in k for k in c), c
    assert (c["window.frame.lds"], c["window.frame.wide"], c["window.frame.range"], c["window.range.bounds"]) == \
        (1, 1, 2, 1), c
    assert c["window.range.pyramids"] == 3 and c["window.scan"] == 7 and c["window.tiles"] == 7, c


# ---- refusals and plumbing
def test_invalid_arguments(cpu):
    t = Table(pa.table({"g": [1, 1, 2], "o": [1, 2, 3], "p": [1.0, 2.0, 3.0], "v": pa.array([1, None, 3]),
                        "s": ["a", "b", "c"]}), cpu)
    for fn in mu.MOMENT:
        with pytest.raises(Exception, match="ddof"):
            t.window("g", "o", True, {"x": (fn, "v", 1, 0, 1, -1)})
        with pytest.raises(Exception, match="min_periods"):
            t.window("g", "o", True, {"x": (fn, "v", 1, 0, 0)})
        with pytest.raises(Exception, match="numeric"):
            t.window("g", "o", True, {"x": (fn, "s", 1, 0)})
        with pytest.raises(Exception, match="frame of"):
            t.window("g", "o", True, {"x": (fn, "v", -1, 0)})
        with pytest.raises(ValueError, match="expected"):
            t.window("g", "o", True, {"x": (fn, "v", 1)})
        with pytest.raises(ValueError, match="expected"):
            t.window("g", "o", True, {"x": (fn, "v", 1, 0, 1, 1, 1)})
        with pytest.raises(Exception, match="already exists"):
            t.window("g", "o", True, {"v": (fn, "v", 1, 0)})
    for fn in ("range_var", "range_std"):
        with pytest.raises(Exception, match="exactly one order column"):
            t.window("g", ["o", "p"], True, {"x": (fn, "v", 1, 0)})
        with pytest.raises(Exception, match="order column"):
            t.window("g", "s", True, {"x": (fn, "v", 1, 0)})
        with pytest.raises(Exception, match="float offset"):
            t.window("g", "o", True, {"x": (fn, "v", 0.5, 0)})
    mom = lambda funcs, cols, ddof=(1,), names=("x",): C.window_moment_frames(  # noqa: E731
        t.native, [0], [1], [True], funcs, cols, [0], list(names), [0], [0], [0.0], [0.0], [False], [1], [False], [0],
        list(ddof))
    assert t._wrap(mom([28], [3])).column_count == 6
    for bad in (31, -1):
        with pytest.raises(Exception, match=f"window function {bad}"):
            mom([bad], [3])
    for kw in ({"ddof": ()}, {"ddof": (1, 1)}, {"names": ()}):
        with pytest.raises(Exception, match="window spec lists differ in length"):
            mom([27], [3], **kw)
    with pytest.raises(Exception, match="of column"):
        mom([27], [9])
    # the older entry points still stop where they stopped
    with pytest.raises(Exception, match="window function 27"):
        C.window_nav(t.native, [0], [1], [True], [27], [3], [0], ["x"], [0], [0], [0.0], [0.0], [False], [1], [False], [0])


def test_table_frame_and_ops_surface(cpu):
    t = _range_table("int", 53, n=300)
    f = {"s": ["rolling_std", "v", 4, 0], "gv": ("range_var", "v", 5, 5, 2, 0), "rn": "row_number",
         "lv": ("last_value", "w")}
    tt = Table(t, cpu)
    exp = mu.expected(t, "g", "o", True, f)
    for what, got in (("table", tt.window("g", "o", True, f)), ("ops", ops.window(tt, "g", "o", True, f)),
                      ("ops distributed", ops.distributed_window(tt, "g", "o", True, f)),
                      ("world 1", tt.distributed_window("g", "o", True, f)),
                      ("frame", DataFrame(t).window("g", "o", True, f)),
                      ("frame env", DataFrame(t).window("g", "o", True, f, env=CylonEnv(distributed=False, device="cpu")))):
        mu.assert_moments(got.to_arrow(), t, "g", "o", True, f, exp=exp, what=what)
    assert len(tt._window_moment_args("g", "o", True, f)) == 16
    args = tt._window_moment_args("g", "o", True, f)
    assert args[3] == [28, 29, 0, 20] and args[-1] == [1, 0, 1, 1] and args[12] == [1, 2, 1, 1]
    # calls without a moment spec go where they went
    assert len(tt._window_nav_args("g", "o", True, {"lv": ("last_value", "w")})) == 15


def test_c_abi_window_moment_frames(cpu):
    from cylon_amd.api import capi_library
    lib = capi_library()
    assert lib.cylon_init(b"cpu") == 0
    assert lib.cylon_read_csv(os.path.join(DATA, "csv1_0.csv").encode(), b"MOM_A") == 0
    whole = Table(context=cpu, _native=C.registry_get("MOM_A")).to_arrow()
    k, v = whole.column_names[0], whole.column_names[1]
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    names = (ctypes.c_char_p * 4)(b"rs", None, b"gv", b"rn")
    rc = lib.cylon_window_moment_frames(b"MOM_A", (i32 * 1)(0), 1, (i32 * 1)(1), (i32 * 1)(1), 1,
                                        (i32 * 4)(28, 27, 29, 0), (i32 * 4)(1, 1, 1, -1), None,
                                        (i64 * 4)(2, 2 ** 63 - 1, 3, 0), (i64 * 4)(0, 1, 2 ** 63 - 1, 0), None, None, None,
                                        (i64 * 4)(1, 2, 1, 1), None, None, (i32 * 4)(1, 0, 2, 1), names, 4, 0, b"MOM_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=cpu, _native=C.registry_get("MOM_OUT")).to_arrow()
    f = {"rs": ("rolling_std", v, 2, 0), "rolling_var_" + v: ("rolling_var", v, None, 1, 2, 0),
         "gv": ("range_var", v, 3, None, 1, 2), "rn": "row_number"}
    mu.assert_moments(out, whole, k, v, True, f, what="c abi")
    # ddof may be NULL (1)
    rc = lib.cylon_window_moment_frames(b"MOM_A", (i32 * 1)(0), 1, (i32 * 1)(1), None, 1, (i32 * 1)(30), (i32 * 1)(1),
                                        None, (i64 * 1)(1), (i64 * 1)(1), None, None, None, None, None, None, None, None,
                                        1, 0, b"MOM_OUT")
    assert rc == 0, lib.cylon_last_error()
    out = Table(context=cpu, _native=C.registry_get("MOM_OUT")).to_arrow()
    mu.assert_moments(out, whole, k, v, True, {None: ("range_std", v, 1, 1)}, what="c abi defaults")
    for funcs, ddof, msg in (((i32 * 1)(31), None, b"window function 31"), ((i32 * 1)(27), (i32 * 1)(-1), b"ddof")):
        assert lib.cylon_window_moment_frames(b"MOM_A", (i32 * 1)(0), 1, (i32 * 1)(1), None, 1, funcs, (i32 * 1)(1), None,
                                              None, None, None, None, None, None, None, None, ddof, None, 1, 0,
                                              b"MOM_X") != 0
        assert msg in lib.cylon_last_error()
    assert lib.cylon_window_nav(b"MOM_A", None, 0, None, None, 0, (i32 * 1)(27), (i32 * 1)(1), None, None, None, None,
                                None, None, None, None, None, None, 1, 0, b"MOM_X") != 0  # still stops at 26
    for t in (b"MOM_A", b"MOM_OUT"):
        assert lib.cylon_remove_table(t) == 0


def _global():
    n = 1500
    rng = np.random.default_rng(61)
    return pa.table({"g": rng.integers(0, 40, n), "o": rng.permutation(n),
                     "v": pa.array(1e9 + rng.standard_normal(n), mask=rng.random(n) < 0.3), "row": np.arange(n)})


DIST_FUNCS = {"s": ("rolling_std", "v", 6, 0), "e": ("rolling_var", "v", None, 0, 3, 0), "gs": ("range_std", "v", 50, 50),
              "rm": ("rolling_mean", "v", 6, 0), "ff": ("ffill", "v")}


def _dist(ctx):
    """rank r holds rows r, r + W, ... of the global table"""
    rank, world = ctx.get_rank(), ctx.get_world_size()
    g = _global()
    tt = Table(g.take(pa.array(np.arange(rank, g.num_rows, world))), ctx)
    return tt.distributed_window("g", "o", True, DIST_FUNCS).to_arrow()


def test_distributed_window_two_ranks():
    res = run_distributed(_dist, 2)
    g = _global()
    on = [set(r["g"].to_pylist()) for r in res]  # every partition is on one rank
    assert on[0].isdisjoint(on[1]) and on[0] | on[1] == set(g["g"].to_pylist())
    # `o` is unique, so the window order does not depend on which rank held a row
    mu.assert_moments(pa.concat_tables(res), g, "g", "o", True, DIST_FUNCS, row_id="row", what="cpu 2 ranks")
