"""Tile and round edges of the radix join's two hot kernels (kernels/radix_join.hip k_rows_pass in
slot mode, kernels/lds_join.hip k_rj_write).

Slot pass: a tile is 8192 rows.  The first pass cuts the table into 8 chunks of n / 8 rows, the
second pass reads the 8 x 2^db1 slots the first one filled; a tile never straddles a chunk / slot,
so each ends in one short tile.  A full tile takes the unpredicated column loop with the next
tile's key prefetch from clamped addresses, a short one the predicated loop; the cases put the
switch between the two at every place it can sit.

Write kernel: each of a partition's 16 waves emits its slice of the probe rows in rounds of 64; the
cases choose partition sizes around the round edges.

Every case is compared with the CPU twin of the same join, whole frame."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C

pytestmark = pytest.mark.gpu

TILE = 8192


def _join(gpu_ctx, ctx, a, b, how, monkeypatch, extra_bits=None):
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1024")
    if extra_bits is not None:
        monkeypatch.setenv("CYLON_RJ_EXTRA_BITS", str(extra_bits))
    kw = dict(left_on=["k"], right_on=["k"], left_prefix="l_", right_prefix="r_")
    C.trace_enable(True)
    C.trace_reset()
    got = Table(a, gpu_ctx).join(Table(b, gpu_ctx), how, "hash", **kw)
    c = dict(C.trace_counters())
    C.trace_enable(False)
    exp = Table(a, ctx).join(Table(b, ctx), how, "hash", **kw)
    return got.to_pandas(), exp.to_pandas(), c


def _canon(df):
    df = df[sorted(df.columns)]
    return df.sort_values(list(df.columns), kind="mergesort", na_position="last").reset_index(drop=True)


def _assert_same_rows(got, exp, how="inner"):
    """Whole-frame equality up to row order (the radix join's output order is unspecified)."""
    assert sorted(got.columns) == sorted(exp.columns)
    assert len(got) == len(exp)
    if how != "inner":  # nulls: pandas' ordering
        pd.testing.assert_frame_equal(_canon(got), _canon(exp), check_dtype=False)
        return
    # inner joins have no nulls: order by (key, first payload of each side) -- random doubles, so
    # no two rows tie -- and compare every column bit for bit (much cheaper than an 8-column sort)
    by = [n for n in sorted(exp.columns) if n.endswith(("k", "v0", "w0"))]
    assert len(by) >= 3, by

    def order(df):
        return np.lexsort(tuple(df[n].to_numpy() for n in reversed(by)))

    og, oe = order(got), order(exp)
    for name in sorted(exp.columns):
        assert np.array_equal(got[name].to_numpy()[og], exp[name].to_numpy()[oe]), name


def _sides(rng, nl, nr, key_range, ncols_l=3, ncols_r=3, lo=0):
    a = {"k": rng.integers(lo, lo + key_range, nl)}
    b = {"k": rng.integers(lo, lo + key_range, nr)}
    for i in range(ncols_l):
        a[f"v{i}"] = rng.random(nl)
    for i in range(ncols_r):
        b[f"w{i}"] = rng.random(nr)
    return pa.table(a), pa.table(b)


# ---- slot pass: int64 key + 3 float64 columns per side, both sides through the two slot passes
# rows per side -> (rows, CYLON_RJ_EXTRA_BITS: lifts these small joins to the >= 11 partition bits
# of slot mode)
SLOT_CASES = {
    # first-pass chunks of 1023 / 1024 / 1025 rows: short tiles only, the smallest two-pass joins
    "8191": (8191, 11),
    "8192": (8192, 11),
    "8193": (8193, 11),
    # 8 chunks of exactly one full tile: every first-pass tile takes the full-tile path and has no
    # next tile (the key prefetch is all clamped rows) or a full next tile
    "8x8192": (8 * TILE, 11),
    # chunks of 8191 rows (the largest short tile) and of 8193 (a full tile, then a 1-row tile: the
    # prefetch under a full tile reads 1 real row and 8191 clamped ones)
    "8x8191": (8 * (TILE - 1), 11),
    "8x8193": (8 * (TILE + 1), 11),
    # every second-pass slot holds ~78 rows: every second-pass tile is short
    "40k": (40_000, 11),
    # second-pass slots of ~8984 rows (sigma ~95): one full tile followed by one short tile in every
    # slot (3M rows would leave the 512 slots at ~5859 rows, below one tile); first-pass chunks of 70
    # full tiles and a short one
    "4.6M": (4_600_000, 1),
}


@pytest.mark.parametrize("case", list(SLOT_CASES))
def test_slot_pass_tile_edges(gpu_ctx, ctx, monkeypatch, case):
    n, xb = SLOT_CASES[case]
    rng = np.random.default_rng(701)
    a, b = _sides(rng, n, n, max(n, 2), lo=-(1 << 40))
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=xb)
    assert c.get("join.radix.slot_sides", 0) == 2 and c.get("join.radix.slot_overflow", 0) == 0, c
    assert c.get("join.radix.narrow_keys", 0) == 1 and c.get("join.radix.narrow_fallback", 0) == 0, c
    assert c["join.radix.rows_out"] == len(exp)
    _assert_same_rows(got, exp)


def test_slot_pass_full_tiles_report_wide_keys_exactly(gpu_ctx, ctx, monkeypatch):
    """One key outside the uint32 offset range, in a row that only the key prefetch under a full tile
    loads, next to clamped rows: the pass must report it (join.radix.narrow_fallback; the cases above
    check that clamped rows alone report nothing).  2.4M rows are 8 chunks of 300000 rows = 36 full
    tiles + a 5088-row tile; a pass runs 32 blocks per chunk, block j takes tiles j, j + 32, ..., so the
    short tile 36 is prefetched under the full tile 4."""
    n = 2_400_000
    rng = np.random.default_rng(702)
    a, b = _sides(rng, n, n, n)
    ka = a["k"].to_numpy().copy()
    ka[36 * TILE + 5000] = 1 << 40
    a = a.set_column(0, "k", pa.array(ka))
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=2)
    assert c.get("join.radix.narrow_fallback", 0) == 1 and c.get("join.radix.slot_sides", 0) == 2, c
    assert c["join.radix.rows_out"] == len(exp)
    _assert_same_rows(got, exp)


# ---- write kernel
def test_write_kernel_eight_byte_keys(gpu_ctx, ctx, monkeypatch):
    """Keys spanning more than 2^32: the first pass reports it and both sides join as int64 keys
    (the write kernel's 8-byte key instance)."""
    rng = np.random.default_rng(703)
    n = 300_000
    a, b = _sides(rng, n, n, 1 << 41, lo=-(1 << 40))
    kb = b["k"].to_numpy().copy()
    kb[: n // 2] = a["k"].to_numpy()[rng.integers(0, n, n // 2)]  # plenty of matches
    b = b.set_column(0, "k", pa.array(kb))
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch)
    assert c.get("join.radix.narrow_fallback", 0) == 1, c
    assert c["join.radix.rows_out"] == len(exp) >= n // 2
    _assert_same_rows(got, exp)


def test_write_kernel_outer_join(gpu_ctx, ctx, monkeypatch):
    rng = np.random.default_rng(704)
    a, b = _sides(rng, 300_000, 400_000, 500_000)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "outer", monkeypatch)
    assert c.get("join.radix.outer", 0) > 0, c
    assert c["join.radix.rows_out"] == len(exp)
    _assert_same_rows(got, exp, "outer")


def test_write_kernel_six_probe_payload_columns(gpu_ctx, ctx, monkeypatch):
    """6 payload columns on the larger (probe) side: more probe columns than the kernel holds in
    registers, the rest are re-read per output row (pc.n > MAXP)."""
    rng = np.random.default_rng(705)
    a, b = _sides(rng, 400_000, 300_000, 350_000, ncols_l=6, ncols_r=1)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch)
    assert c["join.radix.rows_out"] == len(exp)
    _assert_same_rows(got, exp)


# probe rows per partition decide the emit rounds: each of the 16 waves owns ceil(rows / 16) of them
# and emits 64 per round.  (build rows, probe rows, probe key range, extra bits) -> partitions:
ROUND_CASES = {
    # 4096 partitions, probe keys in 1/32 of the build's key range: most partitions see 0 probe rows,
    # the others a handful (most waves none)
    "no_probe_rows": (50_000, 60_000, 60_000 // 32, 8),
    # 2048 partitions of ~146 probe rows: ~10 per wave, one partial round
    "under_64_per_wave": (200_000, 300_000, 400_000, 5),
    # 1024 partitions of ~977 probe rows (sigma ~31): wave slices of 58..66 rows -- partitions on both
    # sides of 1024 rows, where every wave has exactly one full round
    "one_round_per_wave": (200_000, 1_000_000, 1_200_000, 4),
    # 256 partitions of ~3906 probe rows: 4 rounds per wave, the last one partial
    "four_rounds_per_wave": (200_000, 1_000_000, 1_200_000, 2),
}


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("case", list(ROUND_CASES))
def test_write_kernel_round_edges(gpu_ctx, ctx, monkeypatch, case, how):
    nb, npr, prange, xb = ROUND_CASES[case]
    rng = np.random.default_rng(706)
    a = pa.table({"k": rng.integers(0, prange, npr), "v0": rng.random(npr), "v1": rng.random(npr),
                  "v2": rng.random(npr)})  # left = the larger side = probe
    b = pa.table({"k": rng.integers(0, max(prange, nb), nb), "w0": rng.random(nb), "w1": rng.random(nb),
                  "w2": rng.random(nb)})
    got, exp, c = _join(gpu_ctx, ctx, a, b, how, monkeypatch, extra_bits=xb)
    assert c["join.radix.rows_out"] == len(exp) > 0
    _assert_same_rows(got, exp, how)


def test_write_kernel_round_expands_to_many_store_iterations(gpu_ctx, ctx, monkeypatch):
    """A key duplicated 200 times on the build side and 300 times on the probe side: a round whose 64
    probe rows all carry it produces 12800 output rows, 200 store iterations."""
    rng = np.random.default_rng(707)
    nb, npr = 200_000, 300_000
    kb = rng.integers(0, 400_000, nb)
    kp = rng.integers(0, 400_000, npr)
    kb[rng.choice(nb, 200, replace=False)] = 123_457
    kp[1000:1300] = 123_457  # adjacent probe rows: whole rounds of the hot key
    a = pa.table({"k": kp, "v0": rng.random(npr), "v1": rng.random(npr), "v2": rng.random(npr)})
    b = pa.table({"k": kb, "w0": rng.random(nb), "w1": rng.random(nb), "w2": rng.random(nb)})
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch)
    assert c["join.radix.rows_out"] == len(exp) >= 200 * 300
    _assert_same_rows(got, exp)
