"""String transform timing driver: one string column of N rows in HBM, each transform through the public
compute functions on the device engine (kernels/strxform.hip) next to three baselines taken in the same
run:
  1. the same call under compute_engine="arrow" (the column copied to the host, Arrow's kernel, the
     result copied back -- the only way to these results before the device kernels);
  2. the traffic floor: (bytes read per pass + bytes written) / the sequential copy rate of
     profiles/membench.txt (copy1, 4.74 TB/s).  A function whose lengths pass needs the row bytes
     (code-point slice, strip, replace) reads them twice; every function reads the offsets (and the
     validity bytes) in both passes and writes 8 (n + 1) length and offset bytes twice (lengths, scan)
     plus the output bytes;
  3. the engine's wave-per-row writer on an identity copy: `where` with an all-true condition
     (kernels/select.hip k_select_var_bytes), against slice(0, None), which copies the same bytes.

usage: python tools/string_transform_probe.py [shape] [N] [reps] [ops] [--nulls=P]
  --nulls=P  a fraction P of the rows (of both columns) is null
  shape  keys: rows of 8-32 bytes over the alphabet abcd (the README's string-join shape; N defaults to 2e8)
         text: rows of 200-300 bytes (N defaults to 2e7); 256 rows span more than C.string_tile_bytes(),
               so every block takes the long-row path
  ops    comma separated, default all of
    slice_id  slice(0, None)                  (the identity copy; code-point slice, bytes read twice)
    where_id  where(all true)                 (the wave-per-row writer; no Arrow figure)
    slice     slice(1, 5)
    strip     strip()                         (ASCII whitespace; nothing to strip in this data)
    upper     upper()                         (flat map without nulls; staged with)
    replace   replace("ab", "x")
    concat    column + "_" + second column
One JSON line per operation: median ms of the device call over reps (after one warm-up), ms of one Arrow-
engine call, the floor, the ratios and a spot check of the first 100 000 device results against
pyarrow.compute.

Run one shape per process, each under its own time limit, the steps chained with &&:
  timeout 900 python tools/string_transform_probe.py keys && timeout 900 python tools/string_transform_probe.py text
"""
import json
import os
import statistics
import sys
import time

import pyarrow as pa
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
assert torch.cuda.is_available(), "string_transform_probe needs an MI355X"
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
    return Table(context=ctx, _native=C.Table(ctx._ctx, [col])), total


T, total = string_table("s")
ALL_TRUE = torch.ones(n, dtype=torch.uint8, device="cuda")


def where_identity(t, o, e):
    return t._wrap(C.Table(t.native.context(), [C.select_var(t.native.column(0), None, ALL_TRUE[:t.row_count])]))


# name: (call(table, other, engine), arrow reference on the sample (None: the input itself), passes over
#        the input bytes, other column read too)
OPS = {
    "slice_id": (lambda t, o, e: compute.str_slice(t, 0, None, e), lambda a, b: a, 2, False),
    "where_id": (where_identity, lambda a, b: a, 1, False),
    "slice": (lambda t, o, e: compute.str_slice(t, 1, 5, e), lambda a, b: pc.utf8_slice_codeunits(a, 1, 5), 2, False),
    "strip": (lambda t, o, e: compute.str_strip(t, None, e), lambda a, b: pc.ascii_trim_whitespace(a), 2, False),
    "upper": (lambda t, o, e: compute.str_upper(t, False, e), lambda a, b: pc.ascii_upper(a), 1, False),
    "replace": (lambda t, o, e: compute.str_replace(t, "ab", "x", -1, e),
                lambda a, b: pc.replace_substring(a, "ab", "x"), 2, False),
    "concat": (lambda t, o, e: compute.str_concat(t, o, "_", e),
               lambda a, b: pc.binary_join_element_wise(a, b, "_"), 1, True),
}
which = (args[3] if len(args) > 3 else ",".join(OPS)).split(",")
O, total_o = None, 0
if "concat" in which:
    O, total_o = string_table("o")


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
    call, ref, passes, two = OPS[name]
    out = call(T, O, "device")
    oc = out.native.column(0)
    out_bytes = int(oc.data.numel())
    got = out.slice(0, k).to_arrow().column(0).to_pylist()
    want = ref(ahead, aohead)
    want = want.to_pylist() if isinstance(want, (pa.Array, pa.ChunkedArray)) else list(want)
    agree = got == want
    del out, oc
    dev_ms = median_ms(lambda: call(T, O, "device"))
    arrow_ms = None
    if name != "where_id":
        timed(lambda: call(head, ohead, "arrow"))  # warm-up of the Arrow path on the small slice
        arrow_ms = round(timed(lambda: call(T, O, "arrow"))[1], 3)
    if name == "upper" and nulls == 0:
        meta = 8 * (n + 1) * 2  # the flat map: offsets read once, written once
    else:
        meta = (2 * (8 * (n + 1) + (n if nulls > 0 else 0))) * (2 if two else 1) + 4 * 8 * (n + 1)
    read = passes * total + (total_o if two else 0)
    floor_ms = max(round(1000 * (read + meta + out_bytes) / COPY_RATE, 4), 1e-4)
    print(json.dumps({"shape": shape, "n": n, "nulls": nulls, "bytes": total, "op": name, "out_bytes": out_bytes,
                      "device_ms": dev_ms, "arrow_engine_ms": arrow_ms, "floor_ms": floor_ms,
                      "arrow_over_device": None if arrow_ms is None else round(arrow_ms / dev_ms, 1),
                      "device_over_floor": round(dev_ms / floor_ms, 2), "spot_check": bool(agree)}), flush=True)
