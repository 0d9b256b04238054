"""Left semi / anti joins on the MI355X: the LDS key-set kernels (kernels/semi_join.hip k_sj_build /
k_sj_probe) behind ops/join_semi.cpp semi_join_local.  Every case is compared, WITHOUT sorting (local
joins keep left's row order), with a Python-set oracle that does not use the engine
(semi_join_utils) and with the same call on the CPU context.

The no-fallback assertions are conditions, not measurements: the partition-bits rule puts the mean
partition 8 sigma below the LDS set's capacity for uniform keys, and each case checks its own
inputs' largest partition with the CPU mirror of fmix64 before it joins."""
import numpy as np
import pyarrow as pa
import pytest

from cylon_amd import Table
from cylon_amd._lib import C
from dist_utils import run_distributed
from semi_join_utils import (assert_same_rows, canon, expected, fmix64_inv, max_distinct_per_partition,
                             semi_mask, semi_partition_bits)

pytestmark = pytest.mark.gpu

N = 300_000
CAP = 4096  # semi_join.hip kSJCap
I64 = np.iinfo(np.int64)


def _payload(rng, n):
    return {"f": rng.random(n),
            "ni": pa.array(rng.integers(-9, 9, n), mask=rng.random(n) < 0.2),
            "s": pa.array(np.char.add("row", np.arange(n).astype(str)))}


def _run(gpu_ctx, ctx, a, b, on, monkeypatch, extra_bits=None, algorithm="hash"):
    """semi and anti on the GPU against the oracle and the CPU context; the GPU counters per type"""
    monkeypatch.setenv("CYLON_RADIX_JOIN_MIN_ROWS", "1024")
    if extra_bits is not None:
        monkeypatch.setenv("CYLON_RJ_EXTRA_BITS", str(extra_bits))
    counters = {}
    kw = dict(on=on, left_prefix="l_", right_prefix="r_")
    for how in ("semi", "anti"):
        C.trace_enable(True)
        C.trace_reset()
        got = Table(a, gpu_ctx).join(Table(b, gpu_ctx), how, algorithm, **kw).to_arrow()
        counters[how] = dict(C.trace_counters())
        C.trace_enable(False)
        exp = expected(a, b, how, on, prefix="l_")
        print(how, "rows", got.num_rows, "expected", exp.num_rows, counters[how])
        assert_same_rows(got, exp)
        assert_same_rows(Table(a, ctx).join(Table(b, ctx), how, algorithm, **kw).to_arrow(), exp)
    return counters


def _radix_no_fallback(counters, parts=None):
    for how, c in counters.items():
        assert c.get("join.semi.radix") == 1, c
        assert c.get("join.semi.overflow_fallback", 0) == 0 and "join.semi.general" not in c, c
        if parts is not None:
            assert c.get("join.semi.parts") == parts, c


@pytest.mark.parametrize("algorithm", ["hash", "sort"])
def test_int64_key_half_matching(gpu_ctx, ctx, monkeypatch, algorithm):
    rng = np.random.default_rng(21)
    a = pa.table({"k": rng.integers(0, N, N), **_payload(rng, N)})
    b = pa.table({"k": rng.integers(0, 2 * N, N), "w": rng.random(N)})
    bits = semi_partition_bits(N)
    assert bits > 0 and max_distinct_per_partition(b["k"].to_numpy(), bits) <= CAP
    m = semi_mask(a, b, ["k"])
    assert 0.3 < m.mean() < 0.5
    assert np.array_equal(m, np.isin(a["k"].to_numpy(), b["k"].to_numpy()))
    c = _run(gpu_ctx, ctx, a, b, ["k"], monkeypatch, algorithm=algorithm)
    _radix_no_fallback(c, parts=1 << bits)
    assert c["semi"]["join.semi.matched"] == c["anti"]["join.semi.matched"] == m.sum()


@pytest.mark.parametrize("nr", [2000, N])
@pytest.mark.parametrize("zero_on", ["left", "right", "both"])
def test_edge_key_values(gpu_ctx, ctx, monkeypatch, zero_on, nr):
    """INT64_MIN, -1, 0, 1, INT64_MAX as keys; 0 is the kernel's empty-slot value and must be neither
    always present (zero only on the left) nor absent (zero on both)."""
    rng = np.random.default_rng(22)
    edges = np.array([I64.min, -1, 1, I64.max, I64.min + 1, I64.max - 1], np.int64)
    lk = np.where(rng.random(N) < 0.3, rng.choice(edges, N), rng.integers(-N, N, N))
    lk[lk == 0] = 7
    lk[:6] = edges
    rk = np.where(rng.random(nr) < 0.01, rng.choice(edges[:4], nr), rng.integers(-N, N, nr))
    rk[rk == 0] = 9
    rk[:4] = edges[:4]
    if zero_on in ("left", "both"):
        lk[10 + rng.choice(N - 10, 5000, replace=False)] = 0
    if zero_on in ("right", "both"):
        rk[10 + rng.choice(nr - 10, 3, replace=False)] = 0
    a = pa.table({"k": lk, **_payload(rng, N)})
    b = pa.table({"k": rk})
    bits = semi_partition_bits(nr)
    assert max_distinct_per_partition(rk, bits) <= CAP
    m = semi_mask(a, b, ["k"])
    zeros = lk == 0
    assert (m[zeros].all() if zero_on == "both" else not m[zeros].any())
    assert m[lk == I64.min].all() and m[lk == I64.max].all() and not m[lk == I64.max - 1].any()
    _radix_no_fallback(_run(gpu_ctx, ctx, a, b, ["k"], monkeypatch), parts=1 << bits)


def test_hot_right_key_never_overflows(gpu_ctx, ctx, monkeypatch):
    rng = np.random.default_rng(23)
    rk = np.concatenate([np.full(200_000, 123_456), rng.choice(N, 1000, replace=False)])
    rng.shuffle(rk)
    a = pa.table({"k": rng.integers(0, N, N), **_payload(rng, N)})
    a = a.set_column(0, "k", pa.array(np.where(rng.random(N) < 0.1, 123_456, a["k"].to_numpy())))
    b = pa.table({"k": rk})
    bits = semi_partition_bits(len(rk))
    assert bits > 0 and max_distinct_per_partition(rk, bits) <= CAP
    _radix_no_fallback(_run(gpu_ctx, ctx, a, b, ["k"], monkeypatch), parts=1 << bits)


@pytest.mark.parametrize("present", [True, False])
def test_hot_left_key(gpu_ctx, ctx, monkeypatch, present):
    """250k left rows share one key: their partition is probed by many workgroups (slices)"""
    rng = np.random.default_rng(24)
    hot = 2 * N + 5
    lk = np.concatenate([np.full(250_000, hot), rng.integers(0, N, N - 250_000)])
    rng.shuffle(lk)
    rk = rng.integers(0, 2 * N, N)
    if present:
        rk[1234] = hot
    a = pa.table({"k": lk, **_payload(rng, N)})
    b = pa.table({"k": rk})
    bits = semi_partition_bits(N)
    assert max_distinct_per_partition(rk, bits) <= CAP
    assert semi_mask(a, b, ["k"])[lk == hot].all() == present
    _radix_no_fallback(_run(gpu_ctx, ctx, a, b, ["k"], monkeypatch), parts=1 << bits)


@pytest.mark.parametrize("nl,nr", [(N, 500), (N, 0), (0, 500), (N + 12_345, 3000)])
def test_tiny_right_is_one_partition(gpu_ctx, ctx, monkeypatch, nl, nr):
    """A right side that fits one LDS set: no partition pass, the kernel reads the keys in place"""
    rng = np.random.default_rng(25)
    a = pa.table({"k": rng.integers(0, 1000, nl), **_payload(rng, nl)})
    b = pa.table({"k": rng.integers(0, 2000, nr), "w": rng.random(nr)})
    c = _run(gpu_ctx, ctx, a, b, ["k"], monkeypatch)
    if nl and nr:
        _radix_no_fallback(c, parts=1)
        assert not any(k.startswith("partition.") for k in c["semi"]), c


@pytest.mark.parametrize("nkeys", [1, 2])
def test_nullable_int_keys(gpu_ctx, ctx, monkeypatch, nkeys):
    rng = np.random.default_rng(26)

    def side(n, extra):
        km = np.zeros(n, bool)
        km[rng.choice(n, 40, replace=False)] = True
        cols = {"k": pa.array(rng.integers(-50_000, 150_000, n), mask=km)}
        if nkeys == 2:
            gm = np.zeros(n, bool)
            gm[rng.choice(n, 2500, replace=False)] = True
            cols["g"] = pa.array(rng.integers(0, 4, n).astype(np.int16), mask=gm)
        return pa.table({**cols, **extra})

    a, b = side(N, _payload(rng, N)), side(N, {"w": rng.random(N)})
    on = ["k", "g"][:nkeys]
    m = semi_mask(a, b, on)
    nulls = np.array([None in t for t in zip(*[a[c].to_pylist() for c in on])])
    assert (m & nulls).any()  # nulls match nulls
    c = _run(gpu_ctx, ctx, a, b, on, monkeypatch)
    _radix_no_fallback(c)
    assert c["semi"].get("join.radix.composite_key") == 1, c


def test_two_pass_partition(gpu_ctx, ctx, monkeypatch):
    """12 partition bits: two LSD passes of the (key, row id) pairs at this size"""
    rng = np.random.default_rng(27)
    a = pa.table({"k": rng.integers(-N, N, N), **_payload(rng, N)})
    b = pa.table({"k": rng.integers(-N, 3 * N, N)})
    bits = semi_partition_bits(N)
    assert bits + 5 == 12
    _radix_no_fallback(_run(gpu_ctx, ctx, a, b, ["k"], monkeypatch, extra_bits=5), parts=1 << 12)


def test_overflow_falls_back_to_general_path(gpu_ctx, ctx, monkeypatch):
    """6000 distinct right keys built to share one partition (fmix64 inverted on the host) exceed the
    LDS set: the kernel reports it, the mask is discarded and the general path answers"""
    rng = np.random.default_rng(28)
    bits = semi_partition_bits(N)
    tail = rng.choice(1 << 40, 6000, replace=False)
    crafted = np.array([fmix64_inv((5 << (64 - bits)) | int(t)) for t in tail], np.uint64).view(np.int64)
    rk = np.concatenate([crafted, rng.integers(0, 2 * N, N - 6000)])
    rng.shuffle(rk)
    assert max_distinct_per_partition(rk, bits) > CAP + 1000
    lk = np.where(rng.random(N) < 0.2, rng.choice(crafted, N), rng.integers(0, N, N))
    a = pa.table({"k": lk, **_payload(rng, N)})
    b = pa.table({"k": rk})
    c = _run(gpu_ctx, ctx, a, b, ["k"], monkeypatch)
    for how in c:
        assert c[how].get("join.semi.radix") == 1 and c[how].get("join.semi.overflow_fallback") == 1, c
        assert c[how].get("join.semi.general") == 1, c


def test_string_key_takes_general_path(gpu_ctx, ctx, monkeypatch):
    rng = np.random.default_rng(29)
    a = pa.table({"k": pa.array(np.char.add("key-", rng.integers(0, N, N).astype(str))), **_payload(rng, N)})
    b = pa.table({"k": pa.array(np.char.add("key-", rng.integers(0, 2 * N, N).astype(str)))})
    c = _run(gpu_ctx, ctx, a, b, ["k"], monkeypatch)
    for how in c:
        assert "join.semi.radix" not in c[how] and c[how].get("join.semi.general") == 1, c


def _forced(ctx, n):
    """world-1 RCCL context with force_shuffle: the distributed operator's exchange path on one GPU
    (set up as tests/test_gpu_rccl_forced.py does)"""
    from cylon_amd import CylonContext
    assert ctx.get_world_size() == 1 and ctx.on_gpu and ctx.is_distributed()
    ctx.add_config("force_shuffle", "1")
    ctx.add_config("shuffle_self_rccl", "1")
    ctx.add_config("shuffle_chunks", "2")
    rng = np.random.default_rng(30)
    a = pa.table({"k": rng.integers(0, n, n), "f": rng.random(n),
                  "s": pa.array(np.char.add("row", np.arange(n).astype(str)))})
    b = pa.table({"w": rng.random(n), "k": rng.integers(0, 2 * n, n)})
    out = {}
    for how in ("semi", "anti"):
        C.trace_enable(True)
        C.trace_reset()
        got = Table(a, ctx).distributed_join(Table(b, ctx), how, "hash", on=["k"], left_prefix="l_").to_arrow()
        out[how] = (got, dict(C.trace_counters()))
        C.trace_enable(False)
    return a, b, out


def test_distributed_forced_rccl_exchange():
    env = {"CYLON_TEST_COMM": "rccl", "CYLON_RADIX_JOIN_MIN_ROWS": "4096"}
    a, b, out = run_distributed(_forced, 1, N, device="cuda:0", env=env)[0]
    for how, (got, c) in out.items():
        exp = expected(a, b, how, ["k"], prefix="l_")
        assert got.column_names == exp.column_names
        assert canon(got) == canon(exp), how
        assert c.get("shuffle.chunks") == 2 and c.get("join.semi.radix") == 2, c
