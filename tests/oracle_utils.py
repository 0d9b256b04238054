"""Shared by the oracle suites (test_moments_oracle.py, test_extremes_oracle.py): the group-size
ladder, wide int64 group keys, traced calls and one spawn of ranks per distributed configuration."""
from cylon_amd._lib import C

from dist_utils import run_distributed

INT64_MIN = -(1 << 63)
LADDER = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)


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
