"""Interval join timing driver: N left x N right rows (int64 `by` key, float64 bounds and `on`, three
float64 payload columns on the right), Table.interval_join(lower, upper, on, by) with how="inner" at a
mean of about 0, 1 and 4 matches per left row, against yardsticks timed in the same run on the same rows:
  counts_ms        Table.interval_join_counts alone: the sort and the rank pass, no pair output
  sort_indices_ms  SortIndices of the 3N concatenated (key, value) rows alone: the floor of the operator
  asof_ms          Table.asof_join BACKWARD of the same tables (on = lower)

usage: python tools/interval_probe.py [N] [groups[,groups...]] [reps] [--once] [--layouts]
Groups default to 1e7,1e3,1.  One JSON line per (groups, matches): median ms over reps (after one
warm-up each, device events around synchronised work), the trace counters, and a spot check of the
counts against torch.searchsorted on one group.

--layouts: one group, three layouts with the pair total of the uniform 1-match case (N): uniform, one
left row owning every pair, and Zipf-distributed counts.  The claim to check in a kernel trace is that
k_interval_expand's time stays within the repeat-to-repeat spread of the uniform layout.

--once: one untimed call per configuration and nothing else, for a `rocprofv3 --kernel-trace --stats`
run of its own: k_interval_rank_tile / k_win_carry / k_interval_rank, k_interval_counts and
k_interval_expand, whose bytes per second (16 B stored and 8 B gathered per pair, 16 B staged per left
row) are to be held against the copy rate of profiles/membench.txt."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cylon_amd import CylonContext, Table  # noqa: E402
from cylon_amd._lib import C  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
once = "--once" in sys.argv
layouts = "--layouts" in sys.argv
n = int(float(args[0])) if len(args) > 0 else 1_000_000_000
groups = [int(float(x)) for x in (args[1] if len(args) > 1 else "1e7,1e3,1").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
MATCHES = (0.01, 1.0, 4.0)
KW = dict(lower="lo", upper="hi", on="t", by="k", right_prefix="r_")
assert torch.cuda.is_available(), "interval_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def rand(rows):
    return torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(stop)


def median_ms(fn):
    timed(fn)  # warm-up
    return round(statistics.median(timed(fn)[1] for _ in range(reps)), 3)


def counted(fn):
    C.trace_enable(True)
    C.trace_reset()
    out = fn()
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("interval.")}
    C.trace_enable(False)
    return out, c


def spot_check(L, R):
    """interval_join_counts for the left rows of the first left row's group against torch.searchsorted
    over that group's right rows (closed both)"""
    got = L.interval_join_counts(R, "lo", "hi", "t", by="k")
    lc, rc = L.to_torch(), R.to_torch()
    key = lc["k"][0]
    li, ri = (lc["k"] == key).nonzero().flatten()[: 1 << 16], (rc["k"] == key).nonzero().flatten()
    ry = torch.sort(rc["t"][ri]).values
    want = torch.searchsorted(ry, lc["hi"][li], right=True) - torch.searchsorted(ry, lc["lo"][li], right=False)
    return bool((got[li] == want.clamp(min=0)).all())


def right_table(ng):
    return Table.from_torch(ctx, {"k": torch.randint(0, ng, (n,), generator=g, device="cuda"), "t": rand(n),
                                  "p0": rand(n), "p1": rand(n), "p2": rand(n)})


def left_table(ng, widths):
    lo = rand(n)
    return Table.from_torch(ctx, {"k": torch.randint(0, ng, (n,), generator=g, device="cuda"), "lo": lo,
                                  "hi": lo + widths})


def run(name, ng, L, R, extra):
    """one configuration; a case whose output does not fit the device (4 matches per row at N = 1e9 are
    4e9 rows of eight 8-byte columns) is reported as such and the run goes on"""
    try:
        measure(name, ng, L, R, extra)
    except (RuntimeError, MemoryError) as e:
        if "out of memory" not in str(e).lower():
            raise
        torch.cuda.empty_cache()
        print(json.dumps({"n_left": n, "n_right": n, "groups": ng, "case": name, "error": "out of memory"}), flush=True)


def measure(name, ng, L, R, extra):
    if once:
        L.interval_join(R, **KW)
        return
    counters = counted(lambda: L.interval_join(R, **KW))[1]
    agree = spot_check(L, R)
    ms = median_ms(lambda: L.interval_join(R, **KW))
    counts_ms = median_ms(lambda: L.interval_join_counts(R, "lo", "hi", "t", by="k"))
    print(json.dumps(dict({"n_left": n, "n_right": n, "groups": ng, "case": name, "interval_ms": ms,
                           "counts_ms": counts_ms, "after_counts_ms": round(ms - counts_ms, 3), "spot_check": agree,
                           "counters": counters}, **extra)), flush=True)


if layouts:
    R = right_table(1)
    rank = torch.arange(1, n + 1, device="cuda", dtype=torch.float64)
    zipf = 1.0 / rank
    zipf = (zipf / zipf.sum())[torch.randperm(n, generator=g, device="cuda")]  # expected counts add up to n
    one = torch.full((n,), -1.0, device="cuda", dtype=torch.float64)  # lower > upper: no pair
    cases = {"uniform": torch.full((n,), 1.0 / n, device="cuda", dtype=torch.float64), "zipf": zipf, "one_row": one}
    for name, widths in cases.items():
        L = left_table(1, widths)
        if name == "one_row":  # row n / 2 owns every right row
            c = L.to_torch()
            c["lo"][n // 2], c["hi"][n // 2] = -float("inf"), float("inf")
            L = Table.from_torch(ctx, c)
        run(name, 1, L, R, {})
        del L
        torch.cuda.empty_cache()
    sys.exit(0)

for ng in groups:
    R = right_table(ng)
    extra = {}
    for m in MATCHES:
        L = left_table(ng, torch.full((n,), m * ng / n, device="cuda", dtype=torch.float64))
        if not once and not extra:
            W = Table.merge([L.project(["k", "lo"]), R.project(["k", "t"]), L.project(["k", "hi"])])  # the 3N key rows
            extra["sort_indices_ms"] = median_ms(lambda: C.sort_indices(W.native, [0, 1], [True, True], False))
            del W
            torch.cuda.empty_cache()
            extra["asof_ms"] = median_ms(lambda: L.asof_join(R, left_on="lo", right_on="t", by="k", right_prefix="r_"))
        run("matches_%g" % m, ng, L, R, extra)
        del L
        torch.cuda.empty_cache()
    del R
    torch.cuda.empty_cache()
