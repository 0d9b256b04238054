"""Framed VAR / STD on the MI355X: kernels/frame_moments.hip behind ops/window.cpp, held to the exact oracle
of moment_frame_utils (never to the CPU twin), in input row order.

Shapes: the edges of pyramid levels 1 - 4 (8, 64, 512, 4096 rows; 100 003 rows reach level 5) and of the
tile T = C.window_tile_rows().  The order key is the sorted position (optionally with ties), so a RANGE
offset is a frame length like a ROWS one: single rows, runs inside one 8-block, whole aligned blocks
(ties of 8, 64, 512, 4096), two adjacent blocks, frames that climb every level, unbounded sides.  The worst
error / bound per case is printed (`pytest -s`)."""
import numpy as np
import pyarrow as pa
import pytest

import moment_frame_utils as mu
from cylon_amd import CylonContext
from cylon_amd._lib import C
from test_moments_oracle import _values

pytestmark = pytest.mark.gpu

T = C.window_tile_rows()
BIG = 100_003
SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, T - 1, T, T + 1]
VALUE_CLASSES = ["offset", "mixed", "const", "int8"]


@pytest.fixture(scope="module")
def gpu():
    return CylonContext(config=None, distributed=False, device="cuda:0")


def _partition_ids(layout, n, rng):
    """a partition id per sorted position, non-decreasing"""
    if layout == "one":
        return np.zeros(n, np.int64)
    if layout == "each":
        return np.arange(n, dtype=np.int64)
    if layout == "blocks":  # heads on block boundaries of every level
        sizes = np.array([8, 64, 512, 8, 8, 64] * (n // 8 + 1))
        return np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int64)
    assert layout == "straddle"  # partitions that straddle the blocks of levels 0 and 1
    sizes = rng.integers(1, 201, n)
    return np.repeat(np.arange(n), sizes)[:n].astype(np.int64)


def _table(layout, n, seed, cls="offset", nullable=False, ties=1, mask=None, values=None):
    """rows shuffled; o = the sorted position // ties"""
    rng = np.random.default_rng(seed)
    ids = _partition_ids(layout, n, rng)
    p = rng.permutation(n)
    v = _values(cls, rng, n) if values is None else values
    if mask is None:
        mask = rng.random(n) < 0.25 if nullable else np.zeros(n, bool)
    o = np.arange(n, dtype=np.int64) // ties
    return pa.table({"g": ids[p].astype(np.int32), "o": o[p], "v": pa.array(v[p], mask=mask[p])})


def four(pre, fol, minp=1, ddof=1):
    """the ROWS and the RANGE form of a frame, VAR and STD"""
    return {"rv": ("rolling_var", "v", pre, fol, minp, ddof), "rs": ("rolling_std", "v", pre, fol, minp, ddof),
            "gv": ("range_var", "v", pre, fol, minp, ddof), "gs": ("range_std", "v", pre, fol, minp, ddof)}


@pytest.mark.parametrize("layout", ["one", "blocks", "each", "straddle"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_layouts(gpu, n, layout):
    cls = VALUE_CLASSES[(SIZES.index(n) + len(layout)) % 4]
    t = _table(layout, n, n * 7 + len(layout), cls=cls, nullable=n % 2 == 1)
    f = {"one": ("rolling_var", "v", 0, 0, 1, 0), "in": ("rolling_std", "v", 2, 3), "gin": ("range_var", "v", 2, 3, 3, 2),
         "two": ("range_std", "v", 8, 0, 1, 0), "all": ("rolling_std", "v", None, None), "gall": ("range_var", "v", None, 0)}
    c, w = mu.check_moments(gpu, t, "g", "o", True, f, what=f"gpu {n} rows, {layout}, {cls}")
    assert c["window.moment.pyramids"] == 1 and c["window.range.bounds"] == 3, c


FRAMES = [(0, 0), (3, 4), (7, 0), (0, 7), (8, 8), (63, 64), (64, 0), (511, 512), (4095, 0), (0, 4096), (None, 0),
          (0, None), (None, None)]


@pytest.mark.parametrize("cls", VALUE_CLASSES)
@pytest.mark.parametrize("frame", FRAMES, ids=str)
def test_frames(gpu, frame, cls):
    t = _table("one" if FRAMES.index(frame) % 2 else "blocks", 4097 + 13, 11, cls=cls, nullable=True)
    mu.check_moments(gpu, t, "g", "o", frame != (3, 4), four(*frame), what=f"gpu frame {frame} {cls}")


@pytest.mark.parametrize("ties", [8, 64, 512, 4096])
def test_aligned_blocks_of_every_level(gpu, ties):
    """ties of 8^k in one partition: RANGE (0, 0) is lo at a block start and hi at a block end on level
    k - 1, (1, 0) two such runs, (1, 1) three"""
    n = 2 * 4096 + 77
    t = _table("one", n, 13 + ties, cls="offset", nullable=True, ties=ties)
    f = {"b1": ("range_var", "v", 0, 0), "b2": ("range_std", "v", 1, 0), "b3": ("range_var", "v", 1, 1, 1, 0),
         "r": ("rolling_std", "v", ties - 1, 0)}
    c, _ = mu.check_moments(gpu, t, "g", "o", True, f, what=f"gpu ties {ties}")
    assert c["window.moment.pyramids"] == 1 and c["window.range.bounds"] == 3, c


@pytest.mark.parametrize("cls,spec", [("offset", ("rolling_std", "v", 40_000, 300)),
                                      ("mixed", ("range_var", "v", 5, 33_000, 1, 0))], ids=["rows-offset", "range-mixed"])
def test_every_pyramid_level(gpu, cls, spec):
    """100 003 rows in one partition (levels of 12 501, 1 563, 196, 25 and 4 entries), several grid strides;
    one spec per case keeps the exact oracle's 100 003 cells within a few seconds"""
    t = _table("one", BIG, 15, cls=cls, nullable=cls == "mixed")
    f = {"climb": spec}
    c, _ = mu.check_moments(gpu, t, "g", "o", True, f, what=f"gpu {BIG} rows {cls}")
    assert c["window.moment.pyramids"] == 1, c


def test_long_null_runs_and_non_finite_values(gpu):
    n = 3 * 512 + 5
    rng = np.random.default_rng(17)
    v = 1e6 + rng.standard_normal(n)
    mask = rng.random(n) < 0.1
    mask[100:100 + 70] = True     # longer than a level-1 block
    mask[512:512 + 600] = True    # longer than a level-2 block
    for k, x in ((5, np.inf), (6, -np.inf), (50, np.nan), (300, np.inf), (301, np.inf), (1300, -np.inf), (n - 1, np.nan)):
        v[k], mask[k] = x, False
    t = _table("one", n, 18, mask=mask, values=v)
    f = four(5, 5)
    f.update(e=("rolling_std", "v", None, 0, 3, 0), w=("range_var", "v", 700, 0, 1, 2), s=("rolling_var", "v", 0, 0, 1, 0))
    mu.check_moments(gpu, t, "g", "o", True, f, what="gpu null runs, non-finite")
    mu.check_moments(gpu, _table("straddle", n, 19, mask=mask, values=v), "g", "o", False, f,
                     what="gpu null runs, non-finite, partitions")


def test_ddof_and_min_periods(gpu):
    t = _table("straddle", T + 500, 20, cls="int8", nullable=True)
    for minp, ddof in ((1, 0), (3, 1), (40, 2), (1, 5)):
        mu.check_moments(gpu, t, "g", "o", True, four(20, 20, minp, ddof), what=f"gpu min_periods {minp} ddof {ddof}")


def test_one_pyramid_per_column_and_mixed_specs(gpu):
    t = _table("straddle", 2 * T + 77, 21, cls="offset", nullable=True)
    f = {"a": ("rolling_var", "v", 6, 0), "b": ("rolling_std", "v", 400, 400, 2, 0), "c": ("range_var", "v", 6, 0),
         "d": ("range_std", "v", None, 3, 1, 2)}
    c, _ = mu.check_moments(gpu, t, "g", "o", True, f, what="gpu shared pyramid")
    assert c["window.moment.pyramids"] == 1 and c["window.frame.moment"] == 4 and c["window.range.bounds"] == 2, c
    f.update(rn="row_number", cs=("cumsum", "o"), rm=("rolling_mean", "v", 6, 0), gm=("range_mean", "v", 6, 0),
             ff=("ffill", "v"), cd="cume_dist", o2=("rolling_std", "o", 6, 0))
    c, _ = mu.check_moments(gpu, t, "g", "o", True, f, what="gpu mixed")
    assert c["window.moment.pyramids"] == 2 and c["window.range.bounds"] == 2 and c["window.frame.range"] == 1, c
