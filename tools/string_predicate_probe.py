"""String predicate timing driver: one string column of N rows in HBM, each operation through the public
compute functions on the device engine (kernels/strmatch.hip) next to two baselines taken in the same
run: the same call under compute_engine="arrow" (the column copied to the host, Arrow's kernel, the
result copied back -- what every one of these calls did before the device kernels) and the read floor,
(bytes read + 8 (n + 1) offset bytes + validity + output bytes) / the sequential copy rate of
profiles/membench.txt (copy1, 4.74 TB/s).

usage: python tools/string_predicate_probe.py [shape] [N] [reps] [ops] [--nulls=P]
  --nulls=P  a fraction P of the rows (of both columns) is null: the columns carry validity bytes, and a
             staged block with a null row copies its bytes row by row instead of by 16-byte vectors
  shape  keys: rows of 8-32 bytes over the alphabet abcd (the README's string-join shape; N defaults to 2e8)
         text: rows of 200-300 bytes (N defaults to 2e7); 256 rows span more than C.string_tile_bytes(),
               so the whole-row kernels take their long-row path
  ops    comma separated, default all of
    eq        column == "abcdabcd"            (prefix kind: bytes read = min(len, 9) per row)
    starts    starts_with("abc")              (prefix kind: min(len, 4) per row)
    contains  contains("abcabc")              (whole-row kind: every byte)
    like      like("%ab%cd")                  (whole-row kind, the general matcher)
    len       length in code points           (whole-row kind)
    lt        column < a second column        (whole-row kind, both columns; the floor counts every byte of
                                               both, which the kernel's early exit does not read)
One JSON line per operation: median ms of the device call over reps (after one warm-up), ms of one Arrow-
engine call (after a warm-up on a small slice), the floor, both ratios and a spot check of the first
100 000 device results against pyarrow.compute.

Run one shape per process, each under its own time limit, the steps chained with &&:
  timeout 900 python tools/string_predicate_probe.py keys && timeout 900 python tools/string_predicate_probe.py text
"""
import json
import operator
import os
import statistics
import sys
import time

import pyarrow.compute as pc
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cylon_amd import CylonContext, Table  # noqa: E402
from cylon_amd._lib import C  # noqa: E402
from cylon_amd.data import compute  # noqa: E402

COPY_RATE = 4.74e12  # bytes / s, profiles/membench.txt copy1 sequential
SAMPLE = 100_000

args = [a for a in sys.argv[1:] if not a.startswith("--")]
nulls = max([float(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--nulls=")] or [0.0])
shape = args[0] if len(args) > 0 else "keys"
assert shape in ("keys", "text"), shape
n = int(float(args[1])) if len(args) > 1 else (200_000_000 if shape == "keys" else 20_000_000)
reps = int(args[2]) if len(args) > 2 else 5
lo, hi = (8, 32) if shape == "keys" else (200, 300)
assert torch.cuda.is_available(), "string_predicate_probe needs an MI355X"
ctx = CylonContext(device="cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)


def string_table(name):
    lens = torch.randint(lo, hi + 1, (n,), generator=g, device="cuda")
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=offs[1:])
    total = int(offs[-1])
    data = torch.empty(total, dtype=torch.uint8, device="cuda")
    step = 1 << 30
    for b in range(0, total, step):  # letters a-d
        m = min(step, total - b)
        data[b:b + m] = torch.randint(97, 101, (m,), generator=g, device="cuda", dtype=torch.uint8)
    valid = (torch.rand(n, generator=g, device="cuda") >= nulls).to(torch.uint8) if nulls > 0 else None
    col = C.Column(name, C.DataType(C.Type.STRING), n, data, offs, valid)
    return Table(context=ctx, _native=C.Table(ctx._ctx, [col])), lens, total


T, lens, total = string_table("s")
OPS = {
    "eq": (lambda t, o, e: compute.binary_op(t, "abcdabcd", operator.eq, e), lambda a, b: pc.equal(a, "abcdabcd"), 9),
    "starts": (lambda t, o, e: compute.str_starts_with(t, "abc", e), lambda a, b: pc.starts_with(a, "abc"), 4),
    "contains": (lambda t, o, e: compute.str_contains(t, "abcabc", e), lambda a, b: pc.match_substring(a, "abcabc"),
                 None),
    "like": (lambda t, o, e: compute.str_like(t, "%ab%cd", "\\", e), lambda a, b: pc.match_like(a, "%ab%cd"), None),
    "len": (lambda t, o, e: compute.str_length(t, "chars", e), lambda a, b: pc.utf8_length(a), None),
    "lt": (lambda t, o, e: compute.binary_op(t, o, operator.lt, e), lambda a, b: pc.less(a, b), None),
}
which = (args[3] if len(args) > 3 else ",".join(OPS)).split(",")
O, total_o = None, 0
if "lt" in which:
    O, _, total_o = string_table("o")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1000 * (time.perf_counter() - t0)


def median_ms(fn):
    timed(fn)  # warm-up
    return round(statistics.median(timed(fn)[1] for _ in range(reps)), 3)


k = min(SAMPLE, n)
head, ohead = T.slice(0, k), (O.slice(0, k) if O is not None else None)
ahead = head.to_arrow().column(0)
aohead = ohead.to_arrow().column(0) if ohead is not None else None
for name in which:
    call, ref, need = OPS[name]
    out = call(T, O, "device")
    oc = out.native.column(0)
    got = oc.data[:k].cpu().tolist()
    live = oc.validity[:k].cpu().tolist() if oc.validity is not None else [1] * k
    want = ref(ahead, aohead).to_pylist()
    agree = [int(x) if ok else None for x, ok in zip(got, live)] == [None if x is None else int(x) for x in want]
    out_bytes = out.native.column(0).data.element_size() * n
    del out
    dev_ms = median_ms(lambda: call(T, O, "device"))
    timed(lambda: call(head, ohead, "arrow"))  # warm-up of the Arrow path on the small slice
    arrow_ms = round(timed(lambda: call(T, O, "arrow"))[1], 3)
    read = int(torch.clamp(lens, max=need).sum()) if need is not None else total + (total_o if name == "lt" else 0)
    offs_bytes = (8 * (n + 1) + (n if nulls > 0 else 0)) * (2 if name == "lt" else 1)  # offsets + validity
    floor_ms = max(round(1000 * (read + offs_bytes + out_bytes) / COPY_RATE, 4), 1e-4)
    print(json.dumps({"shape": shape, "n": n, "nulls": nulls, "bytes": total, "op": name, "device_ms": dev_ms, "arrow_engine_ms": arrow_ms,
                      "floor_ms": floor_ms, "arrow_over_device": round(arrow_ms / dev_ms, 1),
                      "device_over_floor": round(dev_ms / floor_ms, 2), "spot_check": bool(agree)}), flush=True)
