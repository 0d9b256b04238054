"""As-of join timing driver: N left x N right rows (int64 `by` key, float64 `on`, three float64 payload
columns on the right), Table.asof_join(on, by) for BACKWARD, NEAREST and BACKWARD with a tolerance,
against three yardsticks timed in the same run on the same tables' rows:
  sort_indices_ms  SortIndices of the 2N concatenated (key, on) rows alone: the floor of the operator
  cummax_ms        Table.window CUMMAX(on) PARTITION BY key ORDER BY on over a table of 2N rows: the same
                   sort plus one value scan (tile + carry + apply), no gather of payload columns
  left_join_ms     a LEFT equality join of two N-row tables of the same width on a key with about N
                   distinct values (an equality join on the `by` key itself would emit N^2 / groups rows)

usage: python tools/asof_probe.py [N] [groups[,groups...]] [reps] [--once]
Groups default to 1e7,1e3,1.  One JSON line per (groups, mode): median ms over reps (after one warm-up
each), the time after the sort (flags + scans + pick + the gather of the right columns), the trace
counters and a spot check of the indices against torch.searchsorted on one group (not for NEAREST).

--once: one untimed call per configuration of asof_join BACKWARD and of the CUMMAX window and nothing
else, for a `rocprofv3 --kernel-trace --stats` run of its own (k_asof_tile / k_win_carry / k_asof_apply
against k_win_tile / k_win_carry / k_win_apply)."""
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
groups = [int(float(x)) for x in (args[1] if len(args) > 1 else "1e7,1e3,1").split(",")]
reps = int(args[2]) if len(args) > 2 else 3
MODES = {"backward": dict(direction="backward"), "nearest": dict(direction="nearest"),
         "backward_tolerance": dict(direction="backward", tolerance=0.25 / n)}
assert torch.cuda.is_available(), "asof_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def rand(rows):
    return torch.rand(rows, generator=g, device="cuda", dtype=torch.float64)


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
    c = {k: v for k, v in dict(C.trace_counters()).items() if k.startswith("asof.")}
    C.trace_enable(False)
    return out, c


def spot_check(L, R, kw):
    """C.asof_join_indices for the left rows of the first left row's group against torch.searchsorted over
    that group's right rows"""
    args = L._asof_args(R, "t", None, None, "k", None, None, kw["direction"], True, kw.get("tolerance"))
    got = C.asof_join_indices(L.native, R.native, *args)
    lc, rc = L.to_torch(), R.to_torch()
    key = lc["k"][0]
    li, ri = (lc["k"] == key).nonzero().flatten()[: 1 << 16], (rc["k"] == key).nonzero().flatten()
    if ri.numel() == 0:
        return bool((got[li] == -1).all())
    ry, order = torch.sort(rc["t"][ri], stable=True)
    x = lc["t"][li]
    pos = torch.searchsorted(ry, x, right=True) - 1  # the last y <= x; equal y are unique with probability 1
    ok = pos >= 0
    if "tolerance" in kw:
        ok &= x - ry[pos.clamp(min=0)] <= kw["tolerance"]
    want = torch.where(ok, ri[order[pos.clamp(min=0)]], torch.full_like(pos, -1))
    return bool((got[li] == want).all())


if not once:
    # the equality join: its own key with about n distinct values, the same column widths
    J1 = Table.from_torch(ctx, {"j": torch.randint(0, n, (n,), generator=g, device="cuda"), "t": rand(n)})
    J2 = Table.from_torch(ctx, {"j": torch.randint(0, n, (n,), generator=g, device="cuda"), "t": rand(n),
                                "p0": rand(n), "p1": rand(n), "p2": rand(n)})
    join_ms = median_ms(lambda: J1.join(J2, "left", "hash", on=["j"], left_prefix="l_", right_prefix="r_"))
    del J1, J2
    torch.cuda.empty_cache()

for ng in groups:
    L = Table.from_torch(ctx, {"k": torch.randint(0, ng, (n,), generator=g, device="cuda"), "t": rand(n)})
    R = Table.from_torch(ctx, {"k": torch.randint(0, ng, (n,), generator=g, device="cuda"), "t": rand(n),
                               "p0": rand(n), "p1": rand(n), "p2": rand(n)})
    W = Table.merge([L, R.project(["k", "t"])])  # the 2N key rows
    if once:
        L.asof_join(R, on="t", by="k", right_prefix="r_")
        W.window("k", "t", True, {"m": ("cummax", "t")})
        del L, R, W
        continue
    sort_ms = median_ms(lambda: C.sort_indices(W.native, [0, 1], [True, True], False))
    cummax_ms = median_ms(lambda: W.window("k", "t", True, {"m": ("cummax", "t")}))
    del W
    torch.cuda.empty_cache()
    for name, kw in MODES.items():
        counters = counted(lambda: L.asof_join(R, on="t", by="k", right_prefix="r_", **kw))[1]
        agree = spot_check(L, R, kw) if name != "nearest" else None
        ms = median_ms(lambda: L.asof_join(R, on="t", by="k", right_prefix="r_", **kw))
        print(json.dumps({"n_left": n, "n_right": n, "groups": ng, "mode": name, "asof_ms": ms,
                          "sort_indices_ms": sort_ms, "after_sort_ms": round(ms - sort_ms * counters["asof.sort"], 3),
                          "cummax_ms": cummax_ms, "cummax_after_sort_ms": round(cummax_ms - sort_ms, 3),
                          "left_join_ms": join_ms, "spot_check": agree, "counters": counters}), flush=True)
    del L, R
    torch.cuda.empty_cache()
