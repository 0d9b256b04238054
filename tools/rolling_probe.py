"""Framed-aggregate timing driver: N rows (int64 partition key, float64 order key, float64 value),
Table.window over PARTITION BY key ORDER BY order with one trailing frame ROWS BETWEEN w - 1 PRECEDING
AND CURRENT ROW per spec, against CUMSUM(value) and SortIndices alone in the same process.

usage: python tools/rolling_probe.py [N] [partitions[,partitions...]] [reps] [configs] [--once]
Partition counts default to 1e7,1e3,1.  Per partition count:
  sort      SortIndices on the two key columns (the floor of the operator)
  cumsum    CUMSUM(value) alone: the yardstick, with its spread (min, max) over the reps
  sum / max rolling_sum / rolling_max alone at w = 7, 1001, L, L + 1, 10^6 and unbounded
            (L = C.window_frame_lds_rows(): up to L the one-launch LDS kernel, above it the wide path)
  four      rolling_sum, rolling_mean, rolling_min, rolling_max together at w = 7
configs (comma separated, default all): cumsum, four, sum:W, max:W with W a width or `unbounded`.
One JSON line each: median ms over reps (after one warm-up), ms after the sort, the ratio of that to
CUMSUM's, the trace counters, and a spot check (a partition's first row: the frame is the row itself).

--once: one untimed call per configuration and nothing else, for a `rocprofv3 --kernel-trace --stats`
run of its own (k_roll_lds, k_roll_tile / k_win_carry / k_roll_scan / k_roll_combine and the sort)."""
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
only = set(args[3].split(",")) if len(args) > 3 else None
L = C.window_frame_lds_rows()
WIDTHS = [7, 1001, L, L + 1, 1_000_000, None]
assert torch.cuda.is_available(), "rolling_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def frame(w):
    return (None, 0) if w is None else (w - 1, 0)


def configs():
    yield "cumsum", None, {"s": ("cumsum", "v")}
    for fn in ("sum", "max"):
        for w in WIDTHS:
            yield fn, w, {"s": ("rolling_" + fn, "v", *frame(w))}
    yield "four", 7, {k: ("rolling_" + k, "v", 6, 0) for k in ("sum", "mean", "min", "max")}


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


def all_ms(fn):
    timed(fn)  # warm-up
    return [round(timed(fn)[1], 3) for _ in range(reps)]


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


for npart in parts:
    T = table_of(n, npart)
    sort_ms = None if once else statistics.median(all_ms(lambda: C.sort_indices(T.native, [0, 1], [True, True], False)))
    cumsum_after = None
    for name, w, funcs in configs():
        label = name if name in ("cumsum", "four") else "%s:%s" % (name, "unbounded" if w is None else w)
        if only is not None and label not in only:
            continue
        out, counters = counted(lambda: T.window("k", "o", True, funcs))
        if once:
            del out
            continue
        agree = spot_check(T, out, "s" if "s" in funcs else "sum")
        del out
        ms = all_ms(lambda: T.window("k", "o", True, funcs))
        med = statistics.median(ms)
        after = round(med - sort_ms, 3)
        if name == "cumsum":
            cumsum_after = after
        print(json.dumps({"n": n, "partitions": npart, "spec": name, "w": w, "window_ms": med, "min_ms": min(ms),
                          "max_ms": max(ms), "sort_indices_ms": sort_ms, "after_sort_ms": after,
                          "ratio_to_cumsum": round(after / cumsum_after, 3) if cumsum_after else None, "spot_check": agree,
                          "counters": counters}), flush=True)
    del T
