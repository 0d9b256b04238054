// Interval join: the rank pass over the merged order of the key rows and the tiled expansion of the
// per-left-row (first, count) ranges into output index pairs, gfx950.  Semantics: docs/semantics.md
// "Interval join"; the CPU twin (cpu_interval.cpp) is the definition.
//
// The operator (ops/interval.cpp) concatenates three blocks of key rows (by .., value) -- the right
// rows with value = on, the left rows with value = lower (L-copies) and with value = upper
// (U-copies), in an order that encodes `closed` -- and sorts them once (SortIndices, stable).  The
// side of sorted position p is read from the range perm[p] falls in (IntervalLayout).
//   k_interval_rank_tile   one tile of kWinTile positions per block step: 16-byte loads of perm, the
//                          number of right rows in the tile (tile flag 0: the scan is unsegmented).
//   window_carry           (window.hip, words 1, func COUNT) unchanged: each tile's 64-bit carry-in.
//   k_interval_rank        re-reads the tile and scans "is a right row" with the carry-in as prefix.
//                          With c = the right rows strictly before the position: an L-copy stores
//                          lo[left row] = c, a U-copy hi[left row] = c, a right row
//                          rrows[c] = its row number.  Those scatters are the only random writes.
//   k_interval_counts      one thread per left row: cnt = hi - lo where both bounds are usable and
//                          hi > lo, else 0; the matched pairs are summed by a wave reduction and one
//                          atomic add per wave.  For a LEFT join cnt becomes max(cnt, 1) and
//                          empty[row] remembers that the one row is a filler.
//   k_interval_expand      one block emits one tile of kIvTile consecutive output rows, whatever the
//                          counts are.  The left rows of the tile are [first, last], found by binary
//                          search of the tile's first and last output row in off (nl + 1 offsets).
//                          When last - first < kIvSlice the block stages off and lo of those rows in
//                          LDS (lo = -1 for a filler) and every thread searches there; else -- only
//                          possible when the tile spans left rows with no output at all -- every
//                          thread searches off[first .. last] in global memory.  A thread owns pairs
//                          of adjacent output rows and writes li and ri with 16-byte stores; the rrows
//                          gather is the only irregular read, contiguous within one left row.
//
// Bounds: perm is a whole allocation of n = nr + 2 nl elements, 16-byte aligned, a permutation of
// [0, n): each left row's lo and hi and each slot of rrows (nr entries; c < nr at a right row) are
// written exactly once.  off[0] = 0, off is non-decreasing and off[nl] = total, so a search for
// o < total over [0, nl - 1] stays inside and ends at a row with off[l] <= o < off[l + 1]; then
// lo[l] + (o - off[l]) < lo[l] + cnt[l] <= hi[l] <= nr.  The rrows read is guarded by < nr all the same.
#include "interval_common.hpp"
#include "window_scan.hpp"

namespace cylon {
namespace hip {

using IvScan = ValScan<WF_SUM_I>;

constexpr int kIvThreads = 256;
constexpr int kIvItems = 8;  // output rows per thread and tile: four 16-byte stores to li, four to ri
constexpr int kIvTile = kIvThreads * kIvItems;
constexpr int kIvSlice = kIvTile;  // left rows staged in LDS: a tile whose left rows all emit fits

__device__ __forceinline__ bool iv_in(int64_t r, int64_t base, int64_t len) {
  return (uint64_t)(r - base) < (uint64_t)len;
}

__global__ __launch_bounds__(kWinThreads) void k_interval_rank_tile(const int64_t *__restrict__ perm, int64_t n,
                                                                    int64_t rbase, int64_t nr,
                                                                    int64_t *__restrict__ tagg,
                                                                    uint8_t *__restrict__ tflag) {
  using T = IvScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t row[kWinItems];
    win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
    uint64_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) cnt += ((full || i0 + k < n) && iv_in((int64_t)row[k], rbase, nr)) ? 1 : 0;
    WinVal tot;
    win_block_exclusive<T>(WinVal{cnt, 0u}, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      tagg[t] = (int64_t)tot.a;
      tflag[t] = 0;
    }
  }
}

__global__ __launch_bounds__(kWinThreads) void k_interval_rank(const int64_t *__restrict__ perm, int64_t n,
                                                               IntervalLayout y, const int64_t *__restrict__ carry,
                                                               int64_t *__restrict__ lo, int64_t *__restrict__ hi,
                                                               int64_t *__restrict__ rrows) {
  using T = IvScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t row[kWinItems];
    win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
    uint64_t cnt = 0;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) cnt += ((full || i0 + k < n) && iv_in((int64_t)row[k], y.rbase, y.nr)) ? 1 : 0;
    WinVal tot;
    const WinVal ex = win_block_exclusive<T>(WinVal{cnt, 0u}, WinVal{(uint64_t)carry[t], 0u}, lds, &tot);
    int64_t c = (int64_t)ex.a;  // right rows strictly before position i0
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      if (full || i0 + k < n) {
        const int64_t r = (int64_t)row[k];  // in [0, n): exactly one of the three ranges
        if (iv_in(r, y.rbase, y.nr)) {
          if (c < y.nr) rrows[c] = r - y.rbase;
          ++c;
        } else if (iv_in(r, y.lbase, y.nl)) {
          lo[r - y.lbase] = c;
        } else if (iv_in(r, y.ubase, y.nl)) {
          hi[r - y.ubase] = c;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_interval_counts(ColView lower, ColView upper,
                                                            const int64_t *__restrict__ lo,
                                                            const int64_t *__restrict__ hi, int64_t nl, int left,
                                                            int64_t *__restrict__ cnt, uint8_t *__restrict__ empty,
                                                            int64_t *matched) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t sum = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += stride) {
    const bool lv = lower.valid == nullptr || lower.valid[i] != 0;
    const bool uv = upper.valid == nullptr || upper.valid[i] != 0;
    const bool usable = interval_usable(lv, load_bits(lower.data, i, lower.width), lower.width, lower.kind) &&
                        interval_usable(uv, load_bits(upper.data, i, upper.width), upper.width, upper.kind);
    const int64_t c = interval_count(usable, lo[i], hi[i]);
    sum += c;
    if (left) {
      empty[i] = c == 0 ? 1 : 0;
      cnt[i] = c == 0 ? 1 : c;
    } else {
      cnt[i] = c;
    }
  }
  // every lane of the wave reaches the reduction
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, kWave);
  if (matched != nullptr && lane_id() == 0 && sum != 0)
    atomicAdd(reinterpret_cast<unsigned long long *>(matched), (unsigned long long)sum);
}

// the last l in [a, b] with off[l] <= o, given off[a] <= o
template <typename P>
__device__ __forceinline__ int64_t iv_find(P off, int64_t a, int64_t b, int64_t o) {
  while (a < b) {
    const int64_t m = a + (b - a + 1) / 2;
    if (off[m] <= o) a = m;
    else b = m - 1;
  }
  return a;
}

template <bool VEC>
__global__ __launch_bounds__(kIvThreads) void k_interval_expand(const int64_t *__restrict__ off,
                                                                const int64_t *__restrict__ lo,
                                                                const uint8_t *__restrict__ empty,
                                                                const int64_t *__restrict__ rrows, int64_t nl,
                                                                int64_t nr, int64_t total, int64_t *__restrict__ li,
                                                                int64_t *__restrict__ ri) {
  __shared__ int64_t s_off[kIvSlice];
  __shared__ int64_t s_lo[kIvSlice];
  const int64_t ntiles = (total + kIvTile - 1) / kIvTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t o0 = t * kIvTile;
    const int64_t o1 = o0 + kIvTile < total ? o0 + kIvTile : total;  // o0 < o1
    // the same two searches in every thread: their addresses depend on the block alone
    const int64_t first = iv_find(off, (int64_t)0, nl - 1, o0);
    const int64_t last = iv_find(off, first, nl - 1, o1 - 1);
    const int64_t span = last - first + 1;
    const bool staged = span <= (int64_t)kIvSlice;
    if (staged) {
      for (int64_t k = threadIdx.x; k < span; k += kIvThreads) {
        const int64_t l = first + k;
        s_off[k] = off[l];
        s_lo[k] = (empty != nullptr && empty[l] != 0) ? -1 : lo[l];
      }
    }
    __syncthreads();
    int64_t row[kIvItems], src[kIvItems];  // the left row and the slot of rrows (-1: a filler) of each output row
#pragma unroll
    for (int p = 0; p < kIvItems / 2; ++p) {
      const int64_t o = o0 + (int64_t)p * (2 * kIvThreads) + 2 * (int64_t)threadIdx.x;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = 2 * p + h, qp = q > 0 ? q - 1 : 0;
        row[q] = -1;
        src[q] = -1;
        if (o + h < o1) {
          int64_t l, at, base;
          if (staged) {
            // the second row of a pair starts from the first one's left row
            const int64_t k0 = h == 0 ? 0 : row[qp] - first;
            const int64_t k = iv_find(s_off, k0, span - 1, o + h);
            l = first + k;
            at = s_off[k];
            base = s_lo[k];
          } else {
            l = iv_find(off, h == 0 ? first : row[qp], last, o + h);
            at = off[l];
            base = (empty != nullptr && empty[l] != 0) ? -1 : lo[l];
          }
          row[q] = l;
          src[q] = base < 0 ? -1 : base + (o + h - at);
        }
      }
    }
    int64_t rr[kIvItems];
#pragma unroll
    for (int q = 0; q < kIvItems; ++q) rr[q] = (src[q] >= 0 && src[q] < nr) ? rrows[src[q]] : -1;
#pragma unroll
    for (int p = 0; p < kIvItems / 2; ++p) {
      const int64_t o = o0 + (int64_t)p * (2 * kIvThreads) + 2 * (int64_t)threadIdx.x;
      if (VEC && o + 1 < o1) {  // o is even: 16-byte aligned in 16-byte aligned outputs
        *reinterpret_cast<longlong2 *>(li + o) = make_longlong2(row[2 * p], row[2 * p + 1]);
        *reinterpret_cast<longlong2 *>(ri + o) = make_longlong2(rr[2 * p], rr[2 * p + 1]);
      } else {
        if (o < o1) {
          li[o] = row[2 * p];
          ri[o] = rr[2 * p];
        }
        if (o + 1 < o1) {
          li[o + 1] = row[2 * p + 1];
          ri[o + 1] = rr[2 * p + 1];
        }
      }
    }
    __syncthreads();  // the slice is restaged by the next tile
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t interval_tile_rows() { return kIvTile; }

static int64_t iv_rank_tiles(int64_t n) { return (n + kWinTile - 1) / kWinTile; }

// tile counts, carries (int64 each) and the tile flags (bytes, rounded up to whole words)
int64_t interval_rank_workspace(int64_t n) {
  const int64_t t = iv_rank_tiles(n);
  return 2 * t + (t + 7) / 8;
}

void interval_rank(const int64_t *perm, int64_t nl, int64_t nr, int64_t lbase, int64_t rbase, int64_t ubase,
                   int64_t step, int64_t *ws, int64_t *lo, int64_t *hi, int64_t *rrows, void *stream) {
  const IntervalLayout y{nl, nr, lbase, rbase, ubase};
  CYLON_CHECK(interval_layout_ok(y), Code::Invalid,
              "interval: blocks at " << lbase << ", " << rbase << ", " << ubase << " of " << nl << " left and " << nr
                                     << " right rows");
  const int64_t n = nr + 2 * nl;
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  CYLON_CHECK(perm != nullptr && reinterpret_cast<uintptr_t>(perm) % 16 == 0, Code::Invalid,
              "interval: perm must be a 16-byte aligned buffer");
  CYLON_CHECK(ws != nullptr && (nl == 0 || (lo != nullptr && hi != nullptr)) && (nr == 0 || rrows != nullptr),
              Code::Invalid, "interval: rank outputs");
  const int64_t ntiles = iv_rank_tiles(n);
  int64_t *tagg = ws, *carry = ws + ntiles;
  uint8_t *tflag = reinterpret_cast<uint8_t *>(ws + 2 * ntiles);
  const dim3 g(grid_for(ntiles, 1)), b(kWinThreads);
  hipLaunchKernelGGL(k_interval_rank_tile, g, b, 0, s, perm, n, rbase, nr, tagg, tflag);
  HIP_LAUNCH_CHECK();
  window_carry(tagg, tflag, ntiles, 1, WF_COUNT, step, carry, stream);
  hipLaunchKernelGGL(k_interval_rank, g, b, 0, s, perm, n, y, carry, lo, hi, rrows);
  HIP_LAUNCH_CHECK();
}

static void iv_check_bound(const ColView &c) {
  const bool isf = c.kind == static_cast<int>(ValueKind::FLOAT);
  const bool w = isf ? (c.width == 4 || c.width == 8) : (c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8);
  CYLON_CHECK(w && c.kind <= static_cast<int>(ValueKind::FLOAT) && c.data != nullptr, Code::Invalid,
              "interval: bound column of width " << c.width << ", kind " << c.kind);
}

void interval_counts(const ColView &lower, const ColView &upper, const int64_t *lo, const int64_t *hi, int64_t nl,
                     bool left, int64_t *cnt, uint8_t *empty, int64_t *matched, void *stream) {
  if (nl == 0) return;
  iv_check_bound(lower);
  iv_check_bound(upper);
  CYLON_CHECK(lo != nullptr && hi != nullptr && cnt != nullptr && (!left || empty != nullptr), Code::Invalid,
              "interval: counts buffers");
  hipLaunchKernelGGL(k_interval_counts, dim3(grid_for(nl)), dim3(kBlock), 0, as_stream(stream), lower, upper, lo, hi,
                     nl, left ? 1 : 0, cnt, empty, matched);
  HIP_LAUNCH_CHECK();
}

void interval_expand(const int64_t *off, const int64_t *lo, const uint8_t *empty, const int64_t *rrows, int64_t nl,
                     int64_t nr, int64_t total, int64_t *li, int64_t *ri, void *stream) {
  if (total == 0) return;
  CYLON_CHECK(total > 0 && nl > 0 && nr >= 0, Code::Invalid,
              "interval: " << total << " pairs of " << nl << " left rows");
  CYLON_CHECK(off != nullptr && lo != nullptr && li != nullptr && ri != nullptr && (nr == 0 || rrows != nullptr),
              Code::Invalid, "interval: expansion buffers");
  const bool vec = reinterpret_cast<uintptr_t>(li) % 16 == 0 && reinterpret_cast<uintptr_t>(ri) % 16 == 0;
  const dim3 g(grid_for((total + kIvTile - 1) / kIvTile, 1)), b(kIvThreads);
  if (vec)
    hipLaunchKernelGGL(k_interval_expand<true>, g, b, 0, as_stream(stream), off, lo, empty, rrows, nl, nr, total, li, ri);
  else
    hipLaunchKernelGGL(k_interval_expand<false>, g, b, 0, as_stream(stream), off, lo, empty, rrows, nl, nr, total, li,
                       ri);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_interval() { preload_code(reinterpret_cast<const void *>(&k_interval_counts)); }

}  // namespace hip
}  // namespace cylon
