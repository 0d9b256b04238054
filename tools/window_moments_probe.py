"""Framed VAR / STD timing driver: N rows (int64 partition key, float64 order key uniform in [0, 1), float64
value), Table.window over PARTITION BY key ORDER BY order, in one process and on one table:
  sort         SortIndices on the two key columns (the floor of the operator)
  cumsum       CUMSUM(value): a running sum
  rolling_sum  at every width w (ROWS BETWEEN w - 1 PRECEDING AND CURRENT ROW)          \\ the yardsticks: a
  range_sum    at the first width                                                         / moment state is
  rolling_std  at every width, and unbounded (expanding)                                    2.5x a sum's
  range_std    at the first width (the offset that frames about w rows)                    bytes
  shared       rolling_var + rolling_std + range_var + range_std of the one column in one call

usage: python tools/window_moments_probe.py [N] [partitions[,partitions...]] [reps] [widths] [--once]
Defaults: N = 1e8, partitions 1e6,1e3,1, 3 reps, widths 7,20,252,unbounded.  One JSON line per measurement:
median ms over reps after one warm-up, ms after the sort, ns per row after the sort, the ratio to the sum of
the same frame kind (and width), the trace counters, and a spot check (at a partition's first row a
trailing frame holds the row alone: its population std is 0 and its sample std null).

--once: one untimed call per moment configuration and nothing else, for a `rocprofv3 --kernel-trace
--stats` run of its own (k_fm_level, k_fm_apply, the bounds search and the sort)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cylon_amd import CylonContext, Table  # noqa: E402
from cylon_amd._lib import C  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
once = "--once" in sys.argv
n = int(float(args[0])) if len(args) > 0 else 100_000_000
parts = [int(float(x)) for x in (args[1] if len(args) > 1 else "1e6,1e3,1").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
widths = [None if x == "unbounded" else int(float(x))
          for x in (args[3] if len(args) > 3 else "7,20,252,unbounded").split(",")]
assert torch.cuda.is_available(), "window_moments_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def table_of(rows, npart):
    return Table.from_torch(ctx, {"k": torch.randint(0, npart, (rows,), generator=g, device="cuda"),
                                  "o": torch.rand(rows, generator=g, device="cuda", dtype=torch.float64),
                                  "v": 1e6 + torch.randn(rows, generator=g, device="cuda", dtype=torch.float64)})


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1000 * (time.perf_counter() - t0)


def median_ms(fn):
    timed(fn)  # warm-up
    return statistics.median(round(timed(fn)[1], 3) for _ in range(reps))


def counted(fn):
    C.trace_enable(True)
    C.trace_reset()
    out = fn()
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("window.")}
    C.trace_enable(False)
    return out, c


def spot_check(T, out, pop, sample):
    """the first 2^20 sorted positions: the heads' population std is 0.0 and their sample std null"""
    cols = out.to_torch()
    perm = C.sort_indices(T.native, [0, 1], [True, True], False)[: 1 << 20]
    k = cols["k"][perm]
    head = torch.ones_like(k, dtype=torch.bool)
    head[1:] = k[1:] != k[:-1]
    nulls = out.to_arrow()[sample].is_null().to_numpy(zero_copy_only=False)
    return bool((cols[pop][perm][head] == 0).all()) and bool(nulls[perm[head].cpu().numpy()].all())


def report(**kw):
    print(json.dumps(kw), flush=True)


def after(fn, sort_ms):
    return round(median_ms(fn) - sort_ms, 3)


for npart in parts:
    T = table_of(n, npart)
    m = n / npart
    w0 = widths[0]
    a0 = None if w0 is None else min((w0 - 1) / m, 2.0)  # the RANGE offset that frames about w0 rows
    rows = [None if w is None else w - 1 for w in widths]
    if once:
        for r in rows:
            T.window("k", "o", True, {"s": ("rolling_std", "v", r, 0)})
        T.window("k", "o", True, {"s": ("range_std", "v", a0, 0.0)})
        continue
    sort_ms = median_ms(lambda: C.sort_indices(T.native, [0, 1], [True, True], False))
    cumsum = after(lambda: T.window("k", "o", True, {"s": ("cumsum", "v")}), sort_ms)
    report(n=n, partitions=npart, spec="cumsum", sort_indices_ms=sort_ms, after_sort_ms=cumsum)
    for w, r in zip(widths, rows):
        out, counters = counted(lambda: T.window("k", "o", True, {"p": ("rolling_std", "v", r, 0, 1, 0),
                                                                  "s": ("rolling_std", "v", r, 0)}))
        ok = spot_check(T, out, "p", "s")
        del out
        std = after(lambda: T.window("k", "o", True, {"s": ("rolling_std", "v", r, 0)}), sort_ms)
        rsum = after(lambda: T.window("k", "o", True, {"s": ("rolling_sum", "v", r, 0)}), sort_ms)
        report(n=n, partitions=npart, spec="rolling_std", width=w, after_sort_ms=std, rolling_sum_after_sort_ms=rsum,
               ratio_to_rolling_sum=round(std / rsum, 3), ratio_to_cumsum=round(std / cumsum, 3),
               ns_per_row_after_sort=round(1e6 * std / n, 3), spot_check=ok, counters=counters)
    gstd = after(lambda: T.window("k", "o", True, {"s": ("range_std", "v", a0, 0.0)}), sort_ms)
    gsum = after(lambda: T.window("k", "o", True, {"s": ("range_sum", "v", a0, 0.0)}), sort_ms)
    report(n=n, partitions=npart, spec="range_std", aimed_width=w0, offset=a0, after_sort_ms=gstd,
           range_sum_after_sort_ms=gsum, ratio_to_range_sum=round(gstd / gsum, 3),
           ratio_to_cumsum=round(gstd / cumsum, 3), ns_per_row_after_sort=round(1e6 * gstd / n, 3))
    four = {"rv": ("rolling_var", "v", rows[0], 0), "rs": ("rolling_std", "v", rows[0], 0),
            "gv": ("range_var", "v", a0, 0.0), "gs": ("range_std", "v", a0, 0.0)}
    shared = after(lambda: T.window("k", "o", True, four), sort_ms)
    report(n=n, partitions=npart, spec="shared", width=w0, after_sort_ms=shared,
           ratio_to_cumsum=round(shared / cumsum, 3))
    del T
