"""Top-k timing driver: N rows (int64 key + 3 float64 payload columns), k rows by the key, against the
only way the engine answered ORDER BY key LIMIT k before: Table.sort(...).slice(0, k).  `sort` is not
touched by the top-k work, so the baseline is the earlier behaviour measured on the same box.

usage: python tools/topk_probe.py [N] [k[,k...]] [reps] [dists] [--crossover]
Key distributions (dists, comma separated): uniform63 (uniform over 63 bits), ties20 (uniform over a
2^20 range: heavy ties), sorted (ascending, spanning 63 bits).  Both sides run alternately in this one
process on the same table, ascending and descending.  One JSON line per (distribution, direction, k):
median ms of each side over reps (after one warm-up each), topk.passes, topk.key_reads, the achieved
TB/s over key_reads x 8 B x N, and whether keys, row order and payload agree with the baseline.

--crossover: instead, the three thresholds of ops/topk.cpp at smaller shapes --
  rows  (topk_select_min_rows): k = 100, N from 2^14 to 2^24, select against the sort fallback;
  k     (topk_max_k):           N = 2^26, k from 2^16 to 2^24, select against sort + slice;
  cand  (topk_candidates):      N = 2^28 uniform keys, k = 10^4, candidate limits 2^12 .. 2^24."""
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
crossover = "--crossover" in sys.argv
n = int(float(args[0])) if len(args) > 0 else 1_000_000_000
ks = [int(float(x)) for x in (args[1] if len(args) > 1 else "100,1e4,1e6").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
dists = (args[3] if len(args) > 3 else "uniform63,ties20,sorted").split(",")
assert torch.cuda.is_available(), "topk_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def keys_of(dist, rows):
    if dist == "uniform63":
        return torch.randint(0, (1 << 63) - 1, (rows,), generator=g, device="cuda")
    if dist == "ties20":
        return torch.randint(0, 1 << 20, (rows,), generator=g, device="cuda")
    return torch.arange(rows, device="cuda") * ((1 << 63) // max(rows, 1))  # sorted ascending


def table_of(dist, rows):
    return Table.from_torch(ctx, {"k": keys_of(dist, rows),
                                  **{f"v{i}": torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)
                                     for i in range(3)}})


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1000 * (time.perf_counter() - t0)


def counted(fn):
    C.trace_enable(True)
    C.trace_reset()
    out = fn()
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("topk.")}
    C.trace_enable(False)
    return out, c


def median_ms(fn, r=reps):
    timed(fn)  # warm-up
    return round(statistics.median(timed(fn)[1] for _ in range(r)), 3)


def same(a, b):
    ca, cb = a.to_torch(), b.to_torch()
    return a.row_count == b.row_count and all(torch.equal(ca[c], cb[c]) for c in a.column_names)


def compare(T, dist, asc, k):
    top, counters = counted(lambda: T.topk(k, "k", asc))
    base = T.sort("k", asc).slice(0, k)
    agree = same(top, base)
    del top, base
    ms = median_ms(lambda: T.topk(k, "k", asc))
    base_ms = median_ms(lambda: T.sort("k", asc).slice(0, k))
    reads = counters.get("topk.key_reads", 0)
    print(json.dumps({"dist": dist, "n": T.row_count, "k": k, "ascending": asc, "topk_ms": ms,
                      "sort_slice_ms": base_ms, "passes": counters.get("topk.passes"), "key_reads": reads,
                      "key_TBps": round(reads * 8 * T.row_count / (ms * 1e-3) / 1e12, 3) if reads else None,
                      "outputs_agree": bool(agree), "counters": counters}), flush=True)


if not crossover:
    for dist in dists:
        T = table_of(dist, n)
        for asc in (True, False):
            for k in ks:
                compare(T, dist, asc, k)
        del T
else:
    for e in (14, 16, 18, 20, 22, 24):
        T = table_of("uniform63", 1 << e)
        ctx.add_config("topk_select_min_rows", "0")
        sel = median_ms(lambda: T.topk(100, "k", True), 5)
        ctx.add_config("topk_select_min_rows", str(1 << 62))
        fb = median_ms(lambda: T.topk(100, "k", True), 5)
        print(json.dumps({"crossover": "rows", "n": 1 << e, "k": 100, "select_ms": sel, "sort_fallback_ms": fb}),
              flush=True)
        del T
    ctx.add_config("topk_select_min_rows", "0")
    ctx.add_config("topk_max_k", str(1 << 62))
    ctx.add_config("topk_rows_per_k", "1")
    T = table_of("uniform63", 1 << 26)
    srt = median_ms(lambda: T.sort("k", True).slice(0, 1 << 16))
    for e in (16, 18, 20, 22, 24):
        sel = median_ms(lambda: T.topk(1 << e, "k", True))
        print(json.dumps({"crossover": "k", "n": 1 << 26, "k": 1 << e, "select_ms": sel, "sort_slice_ms": srt}),
              flush=True)
    del T
    T = table_of("uniform63", 1 << 28)
    for e in (12, 16, 20, 24):
        ctx.add_config("topk_candidates", str(1 << e))
        _, c = counted(lambda: T.topk(10_000, "k", True))
        sel = median_ms(lambda: T.topk(10_000, "k", True))
        print(json.dumps({"crossover": "cand", "n": 1 << 28, "k": 10_000, "topk_candidates": 1 << e, "select_ms": sel,
                          "passes": c.get("topk.passes"), "key_reads": c.get("topk.key_reads")}), flush=True)
