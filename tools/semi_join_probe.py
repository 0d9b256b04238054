"""Left semi / anti join timing driver: NL left rows (int64 key + 3 float64) filtered by NR right
rows of int64 keys, against the only way the engine answered the question before these join types
existed: an inner hash join with the distinct right keys, projected to the left columns.

usage: python tools/semi_join_probe.py [NL] [NR[,NR...]] [how: semi | anti | both] [reps]
Both sides of the comparison run alternately in this one process on the same tables.  Prints one
JSON line per join type: median ms of each side over reps (after one warm-up each), the output rows
and whether row counts, key sums and payload sums agree (anti has no inner-join form: its baseline
is the left table minus the semi baseline's rows, compared by counts and sums only).
Bytes the mark kernels must move (for GB/s from a kernel trace): 8 * NR (right keys) + 8 * NL
(left keys, + 8 * NL row ids when partitioned) + one byte per matching row."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cylon_amd import CylonContext, Table  # noqa: E402
from cylon_amd._lib import C  # noqa: E402

nl = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
nrs = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1e6,1e8,1e9").split(",")]
how = sys.argv[3] if len(sys.argv) > 3 else "both"
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
assert torch.cuda.is_available(), "semi_join_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)
hi = 2 * nl  # about half of a right side as long as the left matches; fewer for shorter ones
L = Table.from_torch(ctx, {"k": torch.randint(0, hi, (nl,), generator=g, device="cuda"),
                           **{f"v{i}": torch.rand(nl, generator=g, device="cuda", dtype=torch.float64)
                              for i in range(3)}})


def sums(t):
    cols = t.to_torch()
    return [t.row_count] + [float(cols[c].sum(dtype=torch.float64 if cols[c].is_floating_point() else torch.int64))
                            for c in t.column_names]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1000 * (time.perf_counter() - t0)


def new(R, kind):
    return L.join(R, kind, "hash", on=["k"])


def baseline(R):
    j = L.join(R.unique(["k"]), "inner", "hash", on=["k"], left_prefix="", right_prefix="r_")
    return j.project(["k", "v0", "v1", "v2"])


total = sums(L)
for nr in nrs:
    R = Table.from_torch(ctx, {"k": torch.randint(0, hi, (nr,), generator=g, device="cuda")})
    for kind in (("semi", "anti") if how == "both" else (how,)):
        tn, tb, sn, sb = [], [], None, None
        for i in range(reps + 1):
            C.trace_enable(i == 0)
            C.trace_reset()
            out, ms = timed(lambda: new(R, kind))
            counters = dict(C.trace_counters()) if i == 0 else counters
            C.trace_enable(False)
            if i:
                tn.append(ms)
            sn = sums(out)
            del out
            out, ms = timed(lambda: baseline(R))
            if i:
                tb.append(ms)
            sb = sums(out)
            del out
        if kind == "anti":  # left minus the semi baseline
            sb = [a - b for a, b in zip(total, sb)]
        agree = sn[0] == sb[0] and all(abs(a - b) <= 1e-9 * max(1.0, abs(a)) for a, b in zip(sn[1:], sb[1:]))
        print(json.dumps({"how": kind, "nl": nl, "nr": nr, "ms": round(statistics.median(tn), 3),
                          "baseline_inner_unique_ms": round(statistics.median(tb), 3),
                          "all_ms": [round(x, 2) for x in tn], "all_baseline_ms": [round(x, 2) for x in tb],
                          "rows": sn[0], "outputs_agree": bool(agree),
                          "counters": {k: v for k, v in counters.items() if k.startswith("join.semi")}}), flush=True)
    del R
