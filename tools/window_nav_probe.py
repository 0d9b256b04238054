"""Navigation / distribution window-function timing driver: N rows (int64 partition key, float64 order
key, float64 value with 25 % nulls), Table.window over PARTITION BY key ORDER BY order, next to CUMMAX and
LAG of the same column and to the floor of the operator, SortIndices on the two key columns alone -- all in
one run, so that the ratios compare like with like.

usage: python tools/window_nav_probe.py [N] [partitions[,partitions...]] [reps] [specs] [--once]
Partition counts default to 1e7,1e3,1; specs (comma separated) to all of
  ffill      FFILL(value)                         (gather, fill scan, scatter: value mode)
  bfill      BFILL(value)                         (the same over the reversed order)
  ffill3     FFILL(value, limit 3)
  firstlast  FIRST_VALUE + LAST_VALUE             (one rank scan each way, two element-wise launches)
  lastlive   LAST_VALUE(value IGNORE NULLS)       (the reversed rank scan, the fill scan, one launch)
  dist       NTILE(4) + PERCENT_RANK + CUME_DIST  (one rank scan each way, three element-wise launches)
  cummax     CUMMAX(value)                        (the yardstick: one value scan)
  lag        LAG(value, 1)                        (the yardstick: rank scan, shift, GatherColumn)
One JSON line per (partitions, specs): median ms of Window over reps (after one warm-up), SortIndices
alone, their difference, the trace counters and a spot check; then one line per partition count with
the ffill / cummax and ffill / lag ratios of the after-sort times.

Run one partition count per process, each under its own time limit, the steps chained with &&:
  timeout 600 python tools/window_nav_probe.py 1e8 1e7 3 && timeout 600 python tools/window_nav_probe.py 1e8 1e3 3 \\
      && timeout 600 python tools/window_nav_probe.py 1e8 1 3

--once: one untimed Window call per configuration and nothing else, for a `rocprofv3 --kernel-trace
--stats` run of its own (the per-kernel times of k_win_tile / k_nav_fill_tile / k_win_carry /
k_nav_fill_apply and the sort)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cylon_amd import CylonContext, Table  # noqa: E402
from cylon_amd._lib import C  # noqa: E402
from cylon_amd.data import arrow_bridge as ab  # noqa: E402

SPECS = {"ffill": {"f": ("ffill", "v")}, "bfill": {"b": ("bfill", "v")}, "ffill3": {"f": ("ffill", "v", 3)},
         "firstlast": {"fv": ("first_value", "v"), "lv": ("last_value", "v")},
         "lastlive": {"lv": ("last_value", "v", True)},
         "dist": {"nt": ("ntile", 4), "pr": "percent_rank", "cd": "cume_dist"},
         "cummax": {"m": ("cummax", "v")}, "lag": {"p": ("lag", "v", 1)}}

args = [a for a in sys.argv[1:] if not a.startswith("--")]
once = "--once" in sys.argv
n = int(float(args[0])) if len(args) > 0 else 1_000_000_000
parts = [int(float(x)) for x in (args[1] if len(args) > 1 else "1e7,1e3,1").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
which = (args[3] if len(args) > 3 else ",".join(SPECS)).split(",")
assert torch.cuda.is_available(), "window_nav_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def table_of(rows, npart):
    k = torch.randint(0, npart, (rows,), generator=g, device="cuda")
    o = torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)
    v = torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)
    valid = torch.rand(rows, generator=g, device="cuda") >= 0.25
    cols = [ab.column_from_tensor("k", k), ab.column_from_tensor("o", o), ab.column_from_tensor("v", v, valid)]
    return Table(context=ctx, _native=C.Table(ctx._ctx, cols)), valid


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1000 * (time.perf_counter() - t0)


def median_ms(fn):
    timed(fn)  # warm-up
    return round(statistics.median(timed(fn)[1] for _ in range(reps)), 3)


def counted(fn):
    C.trace_enable(True)
    C.trace_reset()
    out = fn()
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("window.")}
    C.trace_enable(False)
    return out, c


def spot_check(out, funcs, valid):
    """a fill keeps every non-null cell and leaves at most the input's nulls; the distribution functions
    stay inside their ranges"""
    cols = {c.name: c for c in out.native.columns()}
    ok = True
    for name in ("f", "b"):
        if name in funcs:
            c = cols[name]
            ok &= bool((c.data[valid] == cols["v"].data[valid]).all()) and bool(c.validity[valid].all())
            ok &= int(c.validity.sum()) >= int(valid.sum())
    if "cd" in funcs:
        ok &= bool(((cols["cd"].data > 0) & (cols["cd"].data <= 1)).all())
        ok &= bool(((cols["pr"].data >= 0) & (cols["pr"].data <= 1)).all())
        ok &= bool(((cols["nt"].data >= 1) & (cols["nt"].data <= 4)).all())
    return ok


for npart in parts:
    T, valid = table_of(n, npart)
    sort_ms = None if once else median_ms(lambda: C.sort_indices(T.native, [0, 1], [True, True], False))
    after = {}
    for name in which:
        funcs = SPECS[name]
        out, counters = counted(lambda: T.window("k", "o", True, funcs))
        if once:
            del out
            continue
        agree = spot_check(out, funcs, valid)
        del out
        ms = median_ms(lambda: T.window("k", "o", True, funcs))
        after[name] = round(ms - sort_ms, 3)
        print(json.dumps({"n": n, "partitions": npart, "specs": name, "window_ms": ms, "sort_indices_ms": sort_ms,
                          "after_sort_ms": after[name], "spot_check": bool(agree), "counters": counters}), flush=True)
    if all(k in after for k in ("ffill", "cummax", "lag")):
        print(json.dumps({"n": n, "partitions": npart,
                          "ffill_over_cummax_after_sort": round(after["ffill"] / after["cummax"], 3),
                          "ffill_over_lag_after_sort": round(after["ffill"] / after["lag"], 3)}), flush=True)
    del T, valid
