"""Shared by the oracle suites (test_moments_oracle.py, test_extremes_oracle.py,
test_join_float_oracle.py): the group-size ladder, wide int64 group keys, arrow columns from and to
raw bit patterns, the special float patterns, traced calls and one spawn of ranks per distributed
configuration."""
import numpy as np
import pyarrow as pa

from cylon_amd._lib import C

from dist_utils import run_distributed

INT64_MIN = -(1 << 63)
LADDER = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
FLOAT_FIELDS = {2: (5, 10), 4: (8, 23), 8: (11, 52)}  # width -> (exponent bits, mantissa bits)


def fspecials(w):
    """name -> bit pattern of the special values of a float of w bytes"""
    e, m = FLOAT_FIELDS[w]
    S, E = 1 << (8 * w - 1), ((1 << e) - 1) << m
    return dict(pnan=E | 1 << (m - 1), nnan=S | E | 1 << (m - 1), psnan=E | 1, nsnan=S | E | 1, pinf=E, ninf=S | E,
                pzero=0, nzero=S, pden=1, nden=S | 1, pmax=E - 1, nmax=S | (E - 1))


def width_kind(typ):
    """(bytes, "f" / "i" / "u") of a fixed-width arrow type"""
    if pa.types.is_boolean(typ):
        return 1, "u"
    kind = "f" if pa.types.is_floating(typ) else ("i" if pa.types.is_signed_integer(typ) else "u")
    return typ.bit_width // 8, kind


def column_bits(col):
    """bit pattern of every row (None for null), read from the column's data buffer"""
    a = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(a, pa.ChunkedArray):  # (older pyarrow: a chunked array of one chunk)
        a = a.chunk(0) if a.num_chunks else pa.array([], type=a.type)
    if pa.types.is_boolean(a.type):
        return [None if v is None else int(v) for v in a.to_pylist()]
    w = a.type.bit_width // 8
    raw = a.buffers()[1].to_pybytes() if a.buffers()[1] is not None else b""
    valid = a.is_valid().to_pylist()
    return [int.from_bytes(raw[(a.offset + i) * w:(a.offset + i + 1) * w], "little") if valid[i] else None
            for i in range(len(a))]


def make_array(bits, typ, nullable):
    """arrow array of `typ` with exactly these bit patterns (None: null)"""
    w, kind = width_kind(typ)
    raw = np.array([0 if b is None else b for b in bits], dtype=f"u{w}")
    vals = raw.astype(bool) if pa.types.is_boolean(typ) else (raw.view(f"f{w}") if kind == "f" else
                                                                 (raw.view(f"i{w}") if kind == "i" else raw))
    if not nullable:
        assert None not in bits
        return pa.array(vals, type=typ)
    return pa.array(vals, type=typ, mask=np.array([b is None for b in bits], dtype=bool))


def wide_keys(rng, count):
    """distinct int64 keys of both signs with the high half set, none INT64_MIN"""
    keys = set()
    while len(keys) < count:
        k = int(rng.integers(1 << 40, 1 << 62)) * (1 if len(keys) % 2 else -1)
        keys.add(k)
    return sorted(keys, key=lambda k: (abs(k) % 1009, k))


def traced(fn):
    """(fn(), the trace counters it left)"""
    C.trace_enable(True)
    C.trace_reset()
    try:
        return fn(), dict(C.trace_counters())
    finally:
        C.trace_enable(False)


def deal_round_robin(key_rows, rank, world):
    """Row numbers of this rank's share: row j of a group (in table order) lives on rank j mod world,
    so every group of at least 2 rows spans ranks.  key_rows: the group key (a tuple) of each row."""
    seen, mine = {}, []
    for i, kk in enumerate(key_rows):
        j = seen.get(kk, 0)
        seen[kk] = j + 1
        if j % world == rank:
            mine.append(i)
    return mine


def spawn_once(spawned, worker, cases, world, device, chunks, rccl_forced=False):
    """One spawn of worker(ctx, cases, chunks, rccl_forced) per configuration, ever: a failed spawn is
    remembered in `spawned`, not repeated.  Returns the list of per-rank results."""
    cfg = (world, device, chunks, rccl_forced)
    if cfg not in spawned:
        env = {"CYLON_TEST_COMM": "rccl"} if rccl_forced else None
        try:
            spawned[cfg] = run_distributed(worker, world, cases, chunks, rccl_forced, device=device, env=env)
        except BaseException as e:
            spawned[cfg] = e
            raise
    if isinstance(spawned[cfg], BaseException):
        raise AssertionError(f"the ranks of {cfg} failed before: {spawned[cfg]!r}")
    return spawned[cfg]
