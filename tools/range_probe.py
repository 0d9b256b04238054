"""RANGE-frame timing driver: N rows (int64 partition key, float64 order key uniform in [0, 1), float64
value), Table.window over PARTITION BY key ORDER BY order with one frame RANGE BETWEEN a PRECEDING AND
CURRENT ROW per spec, against rolling_sum at the matching width, CUMSUM(value) and SortIndices alone in
the same process.

usage: python tools/range_probe.py [N] [partitions[,partitions...]] [reps] [lengths] [--once]
Partition counts default to 1e7,1e3,1; lengths (comma separated, default 7,513,1000000,unbounded) are
the mean frame lengths aimed at: a partition holds m = N / partitions rows on average, one per 1 / m of
the key range, so the offset a = (w - 1) / m gives frames of about w rows (never more than the
partition; the measured mean is reported).  Per partition count:
  sort      SortIndices on the two key columns (the floor of the operator)
  cumsum    CUMSUM(value) alone: the yardstick
  range     range_sum alone per length, and rolling_sum at w = that length
  five      range_count, range_sum, range_mean, range_min, range_max together at the first length
One JSON line each: median ms over reps (after one warm-up), ms after the sort, the ratio to CUMSUM and
to rolling_sum after the sort, the measured mean frame length, the trace counters, and a spot check (a
partition's first row: a trailing frame is the row and its peers, here the row alone).

--once: one untimed call per range configuration and nothing else, for a `rocprofv3 --kernel-trace
--stats` run of its own (k_fr_keys, k_fr_bounds, k_fr_level, k_fr_apply and the sort)."""
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
n = int(float(args[0])) if len(args) > 0 else 1_000_000_000
parts = [int(float(x)) for x in (args[1] if len(args) > 1 else "1e7,1e3,1").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
lengths = [None if x == "unbounded" else int(float(x))
           for x in (args[3] if len(args) > 3 else "7,513,1000000,unbounded").split(",")]
assert torch.cuda.is_available(), "range_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def table_of(rows, npart):
    return Table.from_torch(ctx, {"k": torch.randint(0, npart, (rows,), generator=g, device="cuda"),
                                  "o": torch.rand(rows, generator=g, device="cuda", dtype=torch.float64),
                                  "v": torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)})


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


def spot_check(T, out, col):
    """the first 2^20 sorted positions: at a partition's first row a trailing frame is the row alone"""
    cols = out.to_torch()
    perm = C.sort_indices(T.native, [0, 1], [True, True], False)[: 1 << 20]
    k = cols["k"][perm]
    head = torch.ones_like(k, dtype=torch.bool)
    head[1:] = k[1:] != k[:-1]
    return bool((cols[col][perm][head] == cols["v"][perm][head]).all())


def report(**kw):
    print(json.dumps(kw), flush=True)


for npart in parts:
    T = table_of(n, npart)
    m = n / npart
    specs = [(w, (None if w is None else min((w - 1) / m, 2.0))) for w in lengths]
    if once:
        for w, a in specs:
            T.window("k", "o", True, {"s": ("range_sum", "v", a, 0.0)})
        continue
    sort_ms = median_ms(lambda: C.sort_indices(T.native, [0, 1], [True, True], False))
    cumsum_after = round(median_ms(lambda: T.window("k", "o", True, {"s": ("cumsum", "v")})) - sort_ms, 3)
    report(n=n, partitions=npart, spec="cumsum", sort_indices_ms=sort_ms, after_sort_ms=cumsum_after)
    for w, a in specs:
        funcs = {"s": ("range_sum", "v", a, 0.0), "c": ("range_count", "v", a, 0.0)}
        out, counters = counted(lambda: T.window("k", "o", True, funcs))
        agree = spot_check(T, out, "s")
        mean_len = float(out.to_torch()["c"].double().mean())
        del out
        range_after = round(median_ms(lambda: T.window("k", "o", True, {"s": funcs["s"]})) - sort_ms, 3)
        rows = None if w is None else w - 1
        roll_after = round(median_ms(lambda: T.window("k", "o", True, {"s": ("rolling_sum", "v", rows, 0)})) - sort_ms, 3)
        report(n=n, partitions=npart, spec="range_sum", aimed_length=w, offset=a, mean_frame_rows=round(mean_len, 2),
               after_sort_ms=range_after, rolling_sum_after_sort_ms=roll_after,
               ratio_to_rolling_sum=round(range_after / roll_after, 3),
               ratio_to_cumsum=round(range_after / cumsum_after, 3), ns_per_row_after_sort=round(1e6 * range_after / n, 3),
               spot_check=agree, counters=counters)
    w, a = specs[0]
    five = {k: ("range_" + k, "v", a, 0.0) for k in ("count", "sum", "mean", "min", "max")}
    five_after = round(median_ms(lambda: T.window("k", "o", True, five)) - sort_ms, 3)
    report(n=n, partitions=npart, spec="five", aimed_length=w, after_sort_ms=five_after,
           ratio_to_cumsum=round(five_after / cumsum_after, 3))
    del T
