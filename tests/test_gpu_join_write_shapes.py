"""The radix join's exact-shape write kernel (kernels/lds_join.hip k_rj_write_exact): which joins take
it (trace counter join.radix.write_exact), that phase D emits what phase C's single probe found,
and the round / iteration edges of its emit loop.

The kernel takes inner joins of all-8-byte columns whose probe side (the larger table) is the key
plus 1..3 payload columns and whose build side is the key plus 1..3 payload columns, on narrowed
(uint32 offset) keys or, for a single partition, 8-byte keys; every other join keeps k_rj_write.

Partition sizes: without CYLON_RJ_EXTRA_BITS a build side of up to ~4000 rows is ONE partition (no
pass runs, so the rows keep their order and the keys stay 8 bytes wide): wave w of the block owns
probe rows [w * per, (w + 1) * per), per = ceil(rows / 16), and emits them in rounds of 64.  With
extra bits the keys are narrowed and the rows are spread over 2^bits partitions by their hash.

Every case is compared with the CPU twin of the same join, whole frame, up to row order."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C

pytestmark = pytest.mark.gpu

EXACT = "join.radix.write_exact"
KEPT_ROUNDS = 8  # lds_join.hip kRJKeptRounds: rounds of a wave slice whose probe result phase C keeps


def _join(gpu_ctx, ctx, a, b, how, monkeypatch, extra_bits=None, min_rows=1024, split_rows=None):
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", str(min_rows))
    if extra_bits is not None:
        monkeypatch.setenv("CYLON_RJ_EXTRA_BITS", str(extra_bits))
    if split_rows is not None:
        monkeypatch.setenv("CYLON_RJ_SPLIT_ROWS", str(split_rows))
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


def _assert_same_rows(got, exp):
    """Whole-frame equality up to row order (the radix join's output order is unspecified)."""
    assert sorted(got.columns) == sorted(exp.columns)
    assert len(got) == len(exp)
    by = [n for n in sorted(exp.columns) if n.endswith(("k", "v0", "w0"))]
    if exp.isna().any().any() or len(by) < 4:  # nulls or a key-only side: pandas' ordering of whole rows
        pd.testing.assert_frame_equal(_canon(got), _canon(exp), check_dtype=False)
        return
    # (key, first payload of each side): random doubles, no two rows tie; every column bit for bit
    og = np.lexsort(tuple(got[n].to_numpy() for n in reversed(by)))
    oe = np.lexsort(tuple(exp[n].to_numpy() for n in reversed(by)))
    for name in sorted(exp.columns):
        assert np.array_equal(got[name].to_numpy()[og], exp[name].to_numpy()[oe]), name


def _table(rng, keys, prefix, ncols, dtype=np.float64):
    cols = {"k": np.asarray(keys, dtype=np.int64)}
    for i in range(ncols):
        cols[f"{prefix}{i}"] = rng.random(len(keys)).astype(dtype)
    return pa.table(cols)


def _sides(rng, npr, nb, key_range, ncols_p=3, ncols_b=3, lo=0):
    """left = probe (the larger side), right = build"""
    assert npr > nb
    return (_table(rng, rng.integers(lo, lo + key_range, npr), "v", ncols_p),
            _table(rng, rng.integers(lo, lo + key_range, nb), "w", ncols_b))


def _ran_exact(c, narrow):
    assert c.get(EXACT, 0) >= 1, c
    assert c.get("join.radix.split_items", 0) == 0, c
    assert c.get("join.radix.narrow_keys", 0) == (1 if narrow else 0), c
    assert c.get("join.radix.narrow_fallback", 0) == 0, c


# ---- shape dispatch
@pytest.mark.parametrize("keys", ["narrow", "single_partition"])
@pytest.mark.parametrize("nb_cols", [1, 2, 3])
@pytest.mark.parametrize("np_cols", [1, 2, 3])
def test_every_exact_shape(gpu_ctx, ctx, monkeypatch, np_cols, nb_cols, keys):
    """key + np_cols payload columns on the probe side, key + nb_cols on the build side; narrowed keys
    over 8 partitions, and one partition of 8-byte keys."""
    rng = np.random.default_rng(1200 + 10 * np_cols + nb_cols)
    a, b = _sides(rng, 4000, 2500, 3000, np_cols, nb_cols, lo=-(1 << 40))
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=3 if keys == "narrow" else None)
    _ran_exact(c, keys == "narrow")
    assert c["join.radix.rows_out"] == len(exp) > 1000
    _assert_same_rows(got, exp)


def _outside(name, rng):
    """(left, right, how) of the joins just outside the exact shapes"""
    how = "inner"
    if name == "five_probe_columns":
        a, b = _sides(rng, 4000, 2500, 3000, 4, 3)
    elif name == "four_build_payload_columns":
        a, b = _sides(rng, 4000, 2500, 3000, 3, 4)
    elif name == "key_only_build_side":
        a, b = _sides(rng, 4000, 2500, 3000, 3, 0)
    elif name == "key_only_probe_side":
        a, b = _sides(rng, 4000, 2500, 3000, 0, 3)
    elif name == "float32_payload_column":
        a, b = _sides(rng, 4000, 2500, 3000, 3, 2)
        b = b.append_column("w2", pa.array(rng.random(2500).astype(np.float32)))
    elif name == "wide_keys":  # keys spanning more than 2^32: reported by the first pass, joined as int64 keys
        a, b = _sides(rng, 4000, 2500, 1 << 41, 3, 3, lo=-(1 << 40))
        kb = b["k"].to_numpy().copy()
        kb[:1500] = a["k"].to_numpy()[rng.integers(0, 4000, 1500)]  # plenty of matches
        b = b.set_column(0, "k", pa.array(kb))
    else:
        a, b = _sides(rng, 4000, 2500, 3000, 3, 3)
        how = name
    return a, b, how


@pytest.mark.parametrize("name", ["five_probe_columns", "four_build_payload_columns", "key_only_build_side",
                                  "key_only_probe_side", "float32_payload_column", "wide_keys", "left", "outer"])
def test_shapes_just_outside_take_the_generic_kernel(gpu_ctx, ctx, monkeypatch, name):
    rng = np.random.default_rng(1230)
    a, b, how = _outside(name, rng)
    got, exp, c = _join(gpu_ctx, ctx, a, b, how, monkeypatch, extra_bits=3)
    assert EXACT not in c, c
    if name == "wide_keys":
        assert c.get("join.radix.narrow_fallback", 0) == 1, c
    assert c["join.radix.rows_out"] == len(exp) > 1000
    _assert_same_rows(got, exp)


# ---- probe once
HOT = 200  # duplicates of the hot build key: one bucket filled by one key's matches


def _dup_sides(rng, counts, nb, n_twice=300, n_once=600):
    """Probe rows in the given order, row i with counts[i] in {0, 1, 2, HOT} matches, against nb build
    rows: one key HOT times, n_twice keys twice, n_once keys once, the rest keys no probe row asks for."""
    counts = np.asarray(counts)
    assert set(np.unique(counts)) <= {0, 1, 2, HOT}
    named = 1 + n_twice + n_once
    nfill = nb - (HOT + 2 * n_twice + n_once)
    assert nfill >= 0 and len(counts) > nb  # the probe side is the larger one
    ids = rng.permutation(1_000_000)[: named + nfill + 500] + 7  # distinct key values
    hot, twice, once = ids[:1], ids[1: 1 + n_twice], ids[1 + n_twice: named]
    fill, absent = ids[named: named + nfill], ids[named + nfill:]
    bkeys = np.concatenate([np.repeat(hot, HOT), np.repeat(twice, 2), once, fill])
    pkeys = np.empty(len(counts), dtype=np.int64)
    for m, pool in ((0, absent), (1, once), (2, twice), (HOT, hot)):
        sel = counts == m
        pkeys[sel] = pool[rng.integers(0, len(pool), int(sel.sum()))]
    return _table(rng, pkeys, "v", 3), _table(rng, rng.permutation(bkeys), "w", 3), int(counts.sum())


@pytest.mark.parametrize("bits", [None, 2])
def test_probe_once_duplicate_counts(gpu_ctx, ctx, monkeypatch, bits):
    """Build keys with 0, 1, 2 and 200 duplicates in the same partition (4096 buckets for ~3000 rows: a
    key's two copies are often separated by another key of their bucket, the hot key's fill theirs),
    probe rows of every count mixed at random."""
    rng = np.random.default_rng(1240)
    counts = rng.choice([0, 1, 2, HOT], size=5000, p=[0.3, 0.4, 0.295, 0.005])
    a, b, rows = _dup_sides(rng, counts, 3000)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=bits)
    _ran_exact(c, bits is not None)
    assert c["join.radix.rows_out"] == len(exp) == rows
    _assert_same_rows(got, exp)


@pytest.mark.parametrize("bits", [None, 1])
def test_probe_once_unmatched_row_at_every_round_position(gpu_ctx, ctx, monkeypatch, bits):
    """4096 probe rows = 16 wave slices of 4 rounds: round r's row at position r % 64 has no match, so
    every position of a round (the first and the last among them) is unmatched once; the partition's
    first 70 and last 70 rows are unmatched too (a whole first round and more)."""
    rng = np.random.default_rng(1241)
    r = np.arange(4096)
    counts = np.where(r % 64 == (r // 64) % 64, 0, 1 + (r % 3 == 0))
    counts[:70] = 0
    counts[-70:] = 0
    a, b, rows = _dup_sides(rng, counts, 2000)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=bits)
    _ran_exact(c, bits is not None)
    assert c["join.radix.rows_out"] == len(exp) == rows
    _assert_same_rows(got, exp)


@pytest.mark.parametrize("bits", [None, 1])
def test_probe_partition_with_more_rounds_than_kept(gpu_ctx, ctx, monkeypatch, bits):
    """20 000 probe rows on few keys against a small build side: wave slices of 1250 rows (20 rounds) in
    one partition, ~10 rounds in each of two -- more than the rounds whose probe result phase C keeps,
    so the later rounds are probed again in phase D."""
    rng = np.random.default_rng(1242)
    counts = rng.choice([0, 1, 2], size=20_000, p=[0.5, 0.3, 0.2])
    a, b, rows = _dup_sides(rng, counts, 1400)
    assert 20_000 / 2 / 16 / 64 > KEPT_ROUNDS
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=bits)
    _ran_exact(c, bits is not None)
    assert c["join.radix.rows_out"] == len(exp) == rows
    _assert_same_rows(got, exp)


# ---- round and iteration edges
@pytest.mark.parametrize("per", [63, 64, 65, 129])
def test_wave_slices_of_exact_sizes(gpu_ctx, ctx, monkeypatch, per):
    """One partition of 16 * per probe rows: every wave slice holds exactly per rows (a partial round,
    one full round, a full round + 1 row, two full rounds + 1 row)."""
    rng = np.random.default_rng(1250 + per)
    counts = rng.choice([0, 1, 2], size=16 * per, p=[0.2, 0.6, 0.2])
    a, b, rows = _dup_sides(rng, counts, 800, n_twice=100, n_once=300)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, min_rows=512)
    _ran_exact(c, False)
    assert c["join.radix.rows_out"] == len(exp) == rows
    _assert_same_rows(got, exp)


def test_wave_slices_of_one_row(gpu_ctx, ctx, monkeypatch):
    """2048 probe rows over 128 partitions (mean 16, most between 8 and 24): slices of one row, waves
    without a row, and partitions where the last waves' slices are empty."""
    rng = np.random.default_rng(1251)
    a, b = _sides(rng, 2048, 1500, 1800)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=7)
    _ran_exact(c, True)
    assert c["join.radix.rows_out"] == len(exp) > 1000
    _assert_same_rows(got, exp)


def test_rounds_of_0_64_65_and_128_output_rows(gpu_ctx, ctx, monkeypatch):
    """One partition of 1536 probe rows: slices of 96 rows = a full round and a half one.  Wave 0's
    full round emits 0 rows, wave 1's 64 (one full store iteration), wave 2's 65 (a second iteration
    with one row), wave 3's 128 (two full iterations), wave 4's 64 from 32 rows with two matches each
    between unmatched rows; the other rounds a random mix."""
    rng = np.random.default_rng(1252)
    counts = rng.choice([0, 1, 2], size=1536, p=[0.3, 0.4, 0.3])
    per = 96
    counts[0 * per: 0 * per + 64] = 0
    counts[0 * per + 64: 1 * per] = 1
    counts[1 * per: 1 * per + 64] = 1
    counts[1 * per + 64: 2 * per] = 0
    counts[2 * per: 2 * per + 64] = 1
    counts[2 * per + 17] = 2
    counts[3 * per: 3 * per + 64] = 2
    counts[4 * per: 4 * per + 64] = 0
    counts[4 * per + 5: 4 * per + 37] = 2  # 32 rows x 2 = 64, between unmatched rows
    a, b, rows = _dup_sides(rng, counts, 1400)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch)
    _ran_exact(c, False)
    assert c["join.radix.rows_out"] == len(exp) == rows
    _assert_same_rows(got, exp)


def test_empty_build_and_empty_probe_partitions(gpu_ctx, ctx, monkeypatch):
    """4096 partitions (the fused count: rows claimed from a cursor) for 1500 build rows and 2048 probe
    rows on 300 keys: ~70 % of the partitions hold no build row, ~93 % no probe row, some only one
    side's rows."""
    rng = np.random.default_rng(1253)
    bk = rng.permutation(3000)[:1500]
    pk = rng.permutation(3000)[:300]
    a = _table(rng, pk[rng.integers(0, 300, 2048)], "v", 3)
    b = _table(rng, bk, "w", 3)
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=12)
    _ran_exact(c, True)
    assert c["join.radix.rows_out"] == len(exp) > 500
    _assert_same_rows(got, exp)


# ---- skew
def test_skewed_join_with_split_items(gpu_ctx, ctx, monkeypatch):
    """A build key with 1500 duplicates among 4000 build rows, build chunks of 1024 rows: its partition
    runs as split items (the generic kernel's), the result is the same."""
    rng = np.random.default_rng(1260)
    a, b = _sides(rng, 6000, 4000, 5000)
    kb, ka = b["k"].to_numpy().copy(), a["k"].to_numpy().copy()
    kb[rng.choice(4000, 1500, replace=False)] = 4242
    ka[rng.choice(6000, 20, replace=False)] = 4242
    a, b = a.set_column(0, "k", pa.array(ka)), b.set_column(0, "k", pa.array(kb))
    got, exp, c = _join(gpu_ctx, ctx, a, b, "inner", monkeypatch, extra_bits=2, split_rows=1024)
    assert c.get("join.radix.split_items", 0) > 0, c
    assert c["join.radix.rows_out"] == len(exp) >= 1500 * 20
    _assert_same_rows(got, exp)
