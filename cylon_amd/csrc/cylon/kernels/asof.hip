// As-of join: "the last right row seen since the partition head" over the merged order of both
// sides' key rows, gfx950.  Semantics: docs/semantics.md "As-of join"; the CPU twin (cpu_asof.cpp) is
// the definition.
//
// The operator (ops/asof.cpp) concatenates the key columns of the two sides (nfirst rows of the first
// side, then the second side's), sorts them once (SortIndices, stable) and marks the partition heads
// (segment_heads over the `by` columns).  A sorted position holds a right row where
// (perm[i] < nfirst) == right_first.  Its scan element is "scan position + 1" for a right row whose
// `on` is neither null nor NaN, else 0, and the scan is the segmented running maximum: ValScan<WF_MAX>
// of window_scan.hpp, in the three launches of window.hip with no hand-off between workgroups:
//   k_asof_tile    one tile of kWinTile positions per block step.  A thread owns kWinItems consecutive
//                  positions: it streams perm and the restarts with 16 / 8-byte loads, reads the `on`
//                  value and validity byte of row perm[i] -- the only random reads --, stores the code
//                  byte (asof_common.hpp) densely in scan order and reduces its elements, then the
//                  block, to the tile's (flag, aggregate) pair.
//   window_carry   (window.hip, words 1, func 3) unchanged: each tile's carry-in.
//   k_asof_apply   re-scans the tile from the code bytes with the carry-in as the prefix; every LEFT
//                  position writes match[left row] = the right row at the carried scan position (-1 for
//                  none, or when the left row's `on` is null or NaN).  That scatter is the only random
//                  write; nothing is sorted back.
// REV: the scan runs over the reversed order (scan position k is sorted position n - 1 - k, read
// element by element as rolling.hip does); rst is then window_rev_flags' output, in scan order.
//   k_asof_pick    one thread per left row: the NEAREST choice between the backward and the forward
//                  candidate and the tolerance (asof_pick_one), skipped when neither applies.
// k_asof_apply or k_asof_pick, whichever runs last, also counts the matched left rows: a wave
// reduction and one atomic add per wave.
//
// Bounds: perm, rst and code are whole allocations of n elements (checked to be 16-byte aligned); a
// full tile is read unpredicated, the last partial tile element by element with k < n.  perm is a
// permutation of [0, n): the `on` column (n rows) is addressed only through it, a left row number is
// perm[i] minus its side's base and lies in [0, n - nright), a carried scan position p lies in [1, n]
// and is read back as perm at position p - 1.
#include "asof_common.hpp"
#include "window_scan.hpp"

namespace cylon {
namespace hip {

using AsofScan = ValScan<WF_MAX>;

// kWinItems rows of perm from scan position k0
template <bool REV>
__device__ __forceinline__ void asof_load_rows(const int64_t *__restrict__ perm, int64_t k0, int64_t n, bool full,
                                               uint64_t *row) {
  if (!REV) {
    win_load8_u64(reinterpret_cast<const uint64_t *>(perm), k0, n, full, row);
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) row[k] = (full || k0 + k < n) ? (uint64_t)perm[n - 1 - (k0 + k)] : 0;
  }
}

template <bool REV>
__global__ __launch_bounds__(kWinThreads) void k_asof_tile(ColView on, const int64_t *__restrict__ perm,
                                                           const uint8_t *__restrict__ rst, int64_t n,
                                                           int64_t nfirst, int right_first,
                                                           uint8_t *__restrict__ code, int64_t *__restrict__ tagg,
                                                           uint8_t *__restrict__ tflag) {
  using T = AsofScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t row[kWinItems];
    uint8_t fl[kWinItems], cd[kWinItems];
    win_load8_u8(rst, k0, n, full, fl);
    asof_load_rows<REV>(perm, k0, n, full, row);
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      const bool in = full || k0 + k < n;  // row[k] < n
      cd[k] = 0;
      if (in) {
        const bool right = ((int64_t)row[k] < nfirst) == (right_first != 0);
        const bool valid = on.valid == nullptr || on.valid[row[k]] != 0;
        cd[k] = asof_code(right, valid, load_bits(on.data, (int64_t)row[k], on.width), on.width, on.kind);
      }
      const uint64_t x = cd[k] == (kAsofRight | kAsofUsable) ? (uint64_t)(k0 + k + 1) : 0ull;
      agg = T::combine(agg, WinVal{x, (uint32_t)(fl[k] & 1)});
    }
    win_store8_u8(code, k0, n, full, cd);
    WinVal tot;
    win_block_exclusive<T>(agg, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      tagg[t] = (int64_t)tot.a;
      tflag[t] = (uint8_t)tot.f;
    }
  }
}

// adds this thread's count to *total: a wave reduction, one atomic per wave
__device__ __forceinline__ void asof_count(int cnt, int64_t *total) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, kWave);
  if (lane_id() == 0 && cnt != 0) atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)cnt);
}

template <bool REV>
__global__ __launch_bounds__(kWinThreads) void k_asof_apply(const int64_t *__restrict__ perm,
                                                            const uint8_t *__restrict__ rst,
                                                            const uint8_t *__restrict__ code, int64_t n,
                                                            int64_t nfirst, int right_first,
                                                            const int64_t *__restrict__ carry,
                                                            int64_t *__restrict__ match, int64_t *matched) {
  using T = AsofScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  const int64_t lbase = right_first ? nfirst : 0, rbase = right_first ? 0 : nfirst;
  int cnt = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t row[kWinItems], x[kWinItems];
    uint8_t fl[kWinItems], cd[kWinItems];
    win_load8_u8(rst, k0, n, full, fl);
    win_load8_u8(code, k0, n, full, cd);  // 0 past n
    asof_load_rows<REV>(perm, k0, n, full, row);
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      x[k] = cd[k] == (kAsofRight | kAsofUsable) ? (uint64_t)(k0 + k + 1) : 0ull;
      agg = T::combine(agg, WinVal{x[k], (uint32_t)(fl[k] & 1)});
    }
    WinVal tot;
    const WinVal ex = win_block_exclusive<T>(agg, WinVal{(uint64_t)carry[t], 0u}, lds, &tot);
    uint64_t run = ex.a;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      run = (fl[k] & 1) ? x[k] : win_op<WF_MAX>(run, x[k]);
      if ((full || k0 + k < n) && !(cd[k] & kAsofRight)) {  // a left row: row[k] - lbase in [0, n - nright)
        int64_t m = -1;
        if ((cd[k] & kAsofUsable) && run != 0) {  // 1 <= run <= k0 + k: a candidate's scan position + 1
          const int64_t p = (int64_t)run - 1;
          m = perm[REV ? n - 1 - p : p] - rbase;
          ++cnt;
        }
        match[(int64_t)row[k] - lbase] = m;
      }
    }
  }
  if (matched != nullptr) asof_count(cnt, matched);
}

// back may be match itself (a one-directional join with a tolerance): no __restrict__ on the two
__global__ __launch_bounds__(kBlock) void k_asof_pick(ColView lon, ColView ron, int64_t nl, AsofPick p,
                                                      const int64_t *back, const int64_t *__restrict__ fwd,
                                                      int64_t *match, int64_t *matched) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += stride) {
    const int64_t b = back[i], f = fwd != nullptr ? fwd[i] : -1;  // -1, or a right row
    const uint64_t x = (b >= 0 || f >= 0) ? load_bits(lon.data, i, p.width) : 0;
    const uint64_t yb = b >= 0 ? load_bits(ron.data, b, p.width) : 0;
    const uint64_t yf = f >= 0 ? load_bits(ron.data, f, p.width) : 0;
    const int64_t m = asof_pick_one(p, x, b, yb, f, yf);
    match[i] = m;
    cnt += m >= 0 ? 1 : 0;
  }
  // every lane of the wave reaches the reduction
  if (matched != nullptr) asof_count(cnt, matched);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void asof_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "asof: " << what << " must be a 16-byte aligned buffer");
}

static void asof_check_on(const ColView &c) {
  const bool isf = c.kind == static_cast<int>(ValueKind::FLOAT);
  const bool w = isf ? (c.width == 4 || c.width == 8) : (c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8);
  CYLON_CHECK(w && c.kind <= static_cast<int>(ValueKind::FLOAT) && c.data != nullptr, Code::Invalid,
              "asof: `on` column of width " << c.width << ", kind " << c.kind);
}

static dim3 asof_grid(int64_t n) { return dim3(grid_for((n + kWinTile - 1) / kWinTile, 1)); }

void asof_tile(const ColView &on, const int64_t *perm, const uint8_t *restarts, int64_t n, int64_t nfirst,
               bool right_first, bool reverse, uint8_t *code, int64_t *tile_agg, uint8_t *tile_flag, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  asof_check_on(on);
  asof_aligned(perm, "perm");
  asof_aligned(restarts, "restarts");
  asof_aligned(code, "codes");
  CYLON_CHECK(nfirst >= 0 && nfirst <= n, Code::Invalid, "asof: " << nfirst << " first rows of " << n);
  CYLON_CHECK(tile_agg != nullptr && tile_flag != nullptr, Code::Invalid, "asof: tile pairs");
  const dim3 g = asof_grid(n), b(kWinThreads);
  if (reverse)
    hipLaunchKernelGGL(k_asof_tile<true>, g, b, 0, s, on, perm, restarts, n, nfirst, right_first ? 1 : 0, code, tile_agg,
                       tile_flag);
  else
    hipLaunchKernelGGL(k_asof_tile<false>, g, b, 0, s, on, perm, restarts, n, nfirst, right_first ? 1 : 0, code,
                       tile_agg, tile_flag);
  HIP_LAUNCH_CHECK();
}

void asof_apply(const int64_t *perm, const uint8_t *restarts, const uint8_t *code, int64_t n, int64_t nfirst,
                bool right_first, bool reverse, const int64_t *carry, int64_t *match, int64_t *matched, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  asof_aligned(perm, "perm");
  asof_aligned(restarts, "restarts");
  asof_aligned(code, "codes");
  CYLON_CHECK(nfirst >= 0 && nfirst <= n, Code::Invalid, "asof: " << nfirst << " first rows of " << n);
  CYLON_CHECK(carry != nullptr, Code::Invalid, "asof: carry");
  // every row may be a left row as far as this launch can tell: match must exist unless there is none
  CYLON_CHECK(match != nullptr || (right_first ? nfirst == n : nfirst == 0), Code::Invalid, "asof: match");
  const dim3 g = asof_grid(n), b(kWinThreads);
  if (reverse)
    hipLaunchKernelGGL(k_asof_apply<true>, g, b, 0, s, perm, restarts, code, n, nfirst, right_first ? 1 : 0, carry,
                       match, matched);
  else
    hipLaunchKernelGGL(k_asof_apply<false>, g, b, 0, s, perm, restarts, code, n, nfirst, right_first ? 1 : 0, carry,
                       match, matched);
  HIP_LAUNCH_CHECK();
}

void asof_pick(const ColView &left_on, const ColView &right_on, int64_t nl, const int64_t *back, const int64_t *fwd,
               bool has_tolerance, int64_t tolerance_i, double tolerance_f, int64_t *match, int64_t *matched,
               void *stream) {
  if (nl == 0) return;
  asof_check_on(left_on);
  CYLON_CHECK(right_on.data != nullptr && right_on.width == left_on.width && right_on.kind == left_on.kind,
              Code::Invalid, "asof: `on` columns of different types");
  CYLON_CHECK(back != nullptr && match != nullptr, Code::Invalid, "asof: candidates and output");
  const AsofPick p{left_on.width, left_on.kind, has_tolerance ? 1 : 0, tolerance_i, tolerance_f};
  hipLaunchKernelGGL(k_asof_pick, dim3(grid_for(nl)), dim3(kBlock), 0, as_stream(stream), left_on, right_on, nl, p,
                     back, fwd, match, matched);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_asof() { preload_code(reinterpret_cast<const void *>(&k_asof_pick)); }

}  // namespace hip
}  // namespace cylon
