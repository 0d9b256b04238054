"""Window-function timing driver: N rows (int64 partition key, float64 order key, float64 value),
Table.window over PARTITION BY key ORDER BY order, against the floor of the operator: SortIndices on
the same two columns alone.

usage: python tools/window_probe.py [N] [partitions[,partitions...]] [reps] [specs] [--once]
Partition counts default to 1e7,1e3,1; specs (comma separated) to rn,cumsum,all:
  rn      ROW_NUMBER alone            (one scan of the flags)
  cumsum  CUMSUM(value) alone         (one value scan: gather, carry, scatter)
  all     both plus LAG(value, 1)     (two scans, the shift and one gather of the value column)
One JSON line per (partitions, specs): median ms of Window and of SortIndices over reps (after one
warm-up each), their difference (flags + scans + outputs), the trace counters, and a spot check of
the result against torch on the sorted order.

--once: one untimed Window call per configuration and nothing else, for a `rocprofv3 --kernel-trace
--stats` run of its own (the per-kernel times of k_win_tile / k_win_carry / k_win_apply and the sort)."""
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
which = (args[3] if len(args) > 3 else "rn,cumsum,all").split(",")
SPECS = {"rn": {"rn": "row_number"}, "cumsum": {"s": ("cumsum", "v")},
         "all": {"rn": "row_number", "s": ("cumsum", "v"), "prev": ("lag", "v", 1)}}
assert torch.cuda.is_available(), "window_probe needs an MI355X"
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
    return round(statistics.median(timed(fn)[1] for _ in range(reps)), 3)


def counted(fn):
    C.trace_enable(True)
    C.trace_reset()
    out = fn()
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("window.")}
    C.trace_enable(False)
    return out, c


def spot_check(T, out, funcs):
    """the first 2^20 sorted positions against torch: row numbers restart at key changes, the running
    sum of a partition's first row is its value"""
    cols = out.to_torch()
    perm = C.sort_indices(T.native, [0, 1], [True, True], False)[: 1 << 20]
    k = cols["k"][perm]
    head = torch.ones_like(k, dtype=torch.bool)
    head[1:] = k[1:] != k[:-1]
    ok = True
    if "rn" in funcs:
        rn = cols["rn"][perm]
        ok &= bool((rn[head] == 1).all()) and bool((rn[1:][~head[1:]] == rn[:-1][~head[1:]] + 1).all())
    if "s" in funcs:
        ok &= bool((cols["s"][perm][head] == cols["v"][perm][head]).all())
    return ok


for npart in parts:
    T = table_of(n, npart)
    sort_ms = None if once else median_ms(lambda: C.sort_indices(T.native, [0, 1], [True, True], False))
    for name in which:
        funcs = SPECS[name]
        out, counters = counted(lambda: T.window("k", "o", True, funcs))
        if once:
            del out
            continue
        agree = spot_check(T, out, funcs)
        del out
        ms = median_ms(lambda: T.window("k", "o", True, funcs))
        print(json.dumps({"n": n, "partitions": npart, "specs": name, "window_ms": ms, "sort_indices_ms": sort_ms,
                          "after_sort_ms": round(ms - sort_ms, 3), "spot_check": bool(agree), "counters": counters}),
              flush=True)
    del T
