// Window functions (ROW_NUMBER / RANK / DENSE_RANK, running SUM / MIN / MAX / COUNT, LAG / LEAD) over
// the sorted positions of a permutation, gfx950.  Semantics: docs/semantics.md "Window functions";
// the CPU twin (cpu_window.cpp) is the definition.
//
// The operator (ops/window.cpp) sorts once (SortIndices) and marks every sorted position with a flag
// byte: bit 0 = the position starts a partition, bit 1 = it starts a run of peers.  Everything here
// is a segmented scan along that order, in three launches with no hand-off between workgroups inside
// a launch (no look-back, no waits):
//   k_win_tile    one tile of kWinTile positions per block step.  A thread owns kWinItems
//                 consecutive positions: it streams perm and the flags with 16 / 8-byte loads, gathers
//                 the value (widths 1, 2, 4, 8) and its validity byte from row perm[i] -- the only
//                 random reads of the operator --, stores both densely in sorted order and reduces its
//                 items, then the block, to the tile's (flag, aggregate) pair.  A later function on the
//                 same column starts from the dense arrays instead (gather = 0).
//   k_win_carry   one block: the exclusive segmented scan of the tile pairs,
//                 (f1, a1) (+) (f2, a2) = (f1 | f2, f2 ? a2 : a1 o a2), kWinCarryItems tiles per thread,
//                 looping while tiles remain, the running pair carried from step to step.
//   k_win_apply   re-scans each tile from the dense values with the tile's carry-in as the prefix
//                 and scatters the running value (and the validity byte) to out[perm[i]].
// Inside a tile: a serial scan of the thread's items, a wave64 scan of the thread aggregates with six
// __shfl_up steps, the four wave totals through LDS.
//
// A running sum is therefore only ever the sum of values of its own partition: no prefix of another
// partition is added and subtracted again (the float accuracy contract of docs/semantics.md).
//
// The ranking functions read no column: the same three phases over the flags alone carry
// (last partition head, last peer head, peer heads since the partition head) and give all three
// functions and, for LAG / LEAD, the partition head of every position in one scan.
//
// Bounds: perm, flags, dense and the tile arrays are whole allocations of the operator (checked to be
// 16-byte aligned); a full tile is read unpredicated, the last partial tile element by element with
// i < n; rows are addressed only through perm[i] in [0, n).
#include "window_scan.hpp"

namespace cylon {
namespace hip {

// ---------------------------------------------------------------------------
// value scans
// ---------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(kWinThreads) void k_win_tile(ColView c, const int64_t *__restrict__ perm,
                                                          const uint8_t *__restrict__ flags, int64_t n,
                                                          uint64_t *__restrict__ dense,
                                                          uint8_t *__restrict__ dvalid, int gather,
                                                          int64_t *__restrict__ tagg, uint8_t *__restrict__ tflag) {
  using T = ValScan<F>;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t bits[kWinItems];
    uint8_t live[kWinItems], fl[kWinItems];
    win_load8_u8(flags, i0, n, full, fl);
    if (gather) {
      uint64_t row[kWinItems];
      win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) {
        const bool in = full || i0 + k < n;  // row[k] < n
        bits[k] = in ? load_bits(c.data, (int64_t)row[k], c.width) : 0;
        live[k] = in ? (c.valid == nullptr ? 1 : (c.valid[row[k]] != 0)) : 0;
      }
      win_store8_u64(dense, i0, n, full, bits);
      if (dvalid != nullptr) win_store8_u8(dvalid, i0, n, full, live);
    } else {
      win_load8_u64(dense, i0, n, full, bits);
      if (dvalid != nullptr) {
        win_load8_u8(dvalid, i0, n, full, live);
      } else {
#pragma unroll
        for (int k = 0; k < kWinItems; ++k) live[k] = (full || i0 + k < n) ? 1 : 0;
      }
    }
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      agg = T::combine(agg, WinVal{win_widen<F>(bits[k], live[k] != 0, c.width, c.kind), (uint32_t)(fl[k] & 1)});
    WinVal tot;
    win_block_exclusive<T>(agg, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      tagg[t] = (int64_t)tot.a;
      tflag[t] = (uint8_t)tot.f;
    }
  }
}

// carry[t] = the pairs of tiles [0, t) combined; step <= kWinCarryTiles tiles per loop step
template <typename T>
__global__ __launch_bounds__(kWinThreads) void k_win_carry(const int64_t *__restrict__ tagg,
                                                           const uint8_t *__restrict__ tflag, int64_t ntiles,
                                                           int64_t step, int64_t *__restrict__ carry) {
  using S = typename T::S;
  __shared__ S lds[kWinWaves];
  S run = T::identity();
  for (int64_t base = 0; base < ntiles; base += step) {
    const int64_t end = base + step < ntiles ? base + step : ntiles;
    const int64_t t0 = base + (int64_t)threadIdx.x * kWinCarryItems;
    S v[kWinCarryItems];
    S agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinCarryItems; ++k) {
      v[k] = t0 + k < end ? T::load(tagg, tflag, t0 + k) : T::identity();
      agg = T::combine(agg, v[k]);
    }
    S tot;
    S ex = win_block_exclusive<T>(agg, run, lds, &tot);
#pragma unroll
    for (int k = 0; k < kWinCarryItems; ++k) {
      if (t0 + k < end) T::store(carry, t0 + k, ex);
      ex = T::combine(ex, v[k]);
    }
    run = tot;
  }
}

template <int F>
__global__ __launch_bounds__(kWinThreads) void k_win_apply(ColView c, const int64_t *__restrict__ perm,
                                                           const uint8_t *__restrict__ flags, int64_t n,
                                                           const uint64_t *__restrict__ dense,
                                                           const uint8_t *__restrict__ dvalid,
                                                           const int64_t *__restrict__ carry,
                                                           uint8_t *__restrict__ out, uint8_t *__restrict__ ovalid) {
  using T = ValScan<F>;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t x[kWinItems], row[kWinItems];
    uint8_t live[kWinItems], fl[kWinItems];
    win_load8_u8(flags, i0, n, full, fl);
    win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
    win_load8_u64(dense, i0, n, full, x);
    if (dvalid != nullptr) {
      win_load8_u8(dvalid, i0, n, full, live);
    } else {
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) live[k] = (full || i0 + k < n) ? 1 : 0;
    }
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      x[k] = win_widen<F>(x[k], live[k] != 0, c.width, c.kind);
      agg = T::combine(agg, WinVal{x[k], (uint32_t)(fl[k] & 1)});
    }
    WinVal tot;
    const WinVal ex = win_block_exclusive<T>(agg, WinVal{(uint64_t)carry[t], 0u}, lds, &tot);
    uint64_t run = ex.a;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      run = (fl[k] & 1) ? x[k] : win_op<F>(run, x[k]);
      if (full || i0 + k < n) {  // row[k] < n
        if (F == WF_MIN || F == WF_MAX)
          win_store_bits(out, (int64_t)row[k], c.width, order_unimage(run, c.width, c.kind));
        else
          reinterpret_cast<uint64_t *>(out)[row[k]] = run;
        if (ovalid != nullptr) ovalid[row[k]] = live[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// the rank scan
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWinThreads) void k_win_rank_tile(const uint8_t *__restrict__ flags, int64_t n,
                                                               int64_t *__restrict__ tagg,
                                                               uint8_t *__restrict__ tflag) {
  using T = RankScan;
  __shared__ WinRank lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint8_t fl[kWinItems];
    win_load8_u8(flags, i0, n, full, fl);  // 0 past n: the identity element
    WinRank agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) agg = T::combine(agg, T::element(fl[k], i0 + k));
    WinRank tot;
    win_block_exclusive<T>(agg, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      T::store(tagg, t, tot);
      tflag[t] = (uint8_t)tot.f;
    }
  }
}

__global__ __launch_bounds__(kWinThreads) void k_win_rank_apply(const int64_t *__restrict__ perm,
                                                                const uint8_t *__restrict__ flags, int64_t n,
                                                                const int64_t *__restrict__ carry,
                                                                int64_t *__restrict__ row_number,
                                                                int64_t *__restrict__ rank,
                                                                int64_t *__restrict__ dense_rank,
                                                                int64_t *__restrict__ phead) {
  using T = RankScan;
  __shared__ WinRank lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint8_t fl[kWinItems];
    uint64_t row[kWinItems];
    win_load8_u8(flags, i0, n, full, fl);
    win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
    WinRank agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) agg = T::combine(agg, T::element(fl[k], i0 + k));
    WinRank tot;
    const WinRank cin{carry[3 * t], carry[3 * t + 1], carry[3 * t + 2], 0u};
    WinRank run = win_block_exclusive<T>(agg, cin, lds, &tot);
    uint64_t ph[kWinItems];
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      run = T::combine(run, T::element(fl[k], i0 + k));
      ph[k] = (uint64_t)run.p;
      if (full || i0 + k < n) {  // position 0 is a partition head, so run.p >= 0; row[k] < n
        const int64_t i = i0 + k;
        if (row_number != nullptr) row_number[row[k]] = i - run.p + 1;
        if (rank != nullptr) rank[row[k]] = run.q - run.p + 1;
        if (dense_rank != nullptr) dense_rank[row[k]] = run.d;
      }
    }
    if (phead != nullptr) win_store8_u64(reinterpret_cast<uint64_t *>(phead), i0, n, full, ph);
  }
}

// LAG (delta < 0) / LEAD (delta > 0) source rows; |delta| <= n
__global__ void k_win_shift(const int64_t *__restrict__ perm, const int64_t *__restrict__ phead, int64_t n,
                            int64_t delta, int64_t *__restrict__ src) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t j = i + delta;
    const bool ok = j >= 0 && j < n && phead[j] == phead[i];
    src[perm[i]] = ok ? perm[j] : -1;
  }
}

// flags[i] = (part[i] != 0) | (peer[i] != 0) << 1 from 0 / 1 head bytes; peer == nullptr: the partition heads
// (flags may be part itself: no __restrict__)
__global__ void k_win_flags(const uint8_t *part, const uint8_t *peer, int64_t n, uint8_t *flags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = n / 16;
  const uint4 *a4 = reinterpret_cast<const uint4 *>(part);
  const uint4 *b4 = reinterpret_cast<const uint4 *>(peer);
  uint4 *o4 = reinterpret_cast<uint4 *>(flags);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t v = tid; v < nv; v += stride) {
    const uint4 a = a4[v];
    const uint4 b = peer != nullptr ? b4[v] : a;
    o4[v] = make_uint4(a.x | (b.x << 1), a.y | (b.y << 1), a.z | (b.z << 1), a.w | (b.w << 1));
  }
  for (int64_t i = nv * 16 + tid; i < n; i += stride)
    flags[i] = (uint8_t)(part[i] | ((peer != nullptr ? peer[i] : part[i]) << 1));
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t window_tile_rows() { return kWinTile; }
int64_t window_carry_tiles() { return kWinCarryTiles; }

static void win_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "window: " << what << " must be a 16-byte aligned buffer");
}

static int64_t win_tiles(int64_t n) { return (n + kWinTile - 1) / kWinTile; }
static dim3 win_grid(int64_t n) { return dim3(grid_for(win_tiles(n), 1)); }

static void win_check_value(const ColView &c, int func) {
  CYLON_CHECK(func >= WF_SUM_I && func <= WF_COUNT, Code::Invalid, "window: value function " << func);
  if (func == WF_COUNT) return;
  const bool w = c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
  CYLON_CHECK(w && c.kind <= static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "window: value column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_F || (c.kind == static_cast<int>(ValueKind::FLOAT) && c.width >= 4), Code::Invalid,
              "window: float sum of a column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_I || c.kind != static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "window: integer sum of a float column");
}

void window_flags(const uint8_t *part, const uint8_t *peer, int64_t n, uint8_t *flags, void *stream) {
  if (n == 0) return;
  win_aligned(part, "partition heads");
  win_aligned(flags, "flags");
  if (peer != nullptr) win_aligned(peer, "peer heads");
  hipLaunchKernelGGL(k_win_flags, dim3(grid_for(n, (int64_t)kBlock * 16)), dim3(kBlock), 0, as_stream(stream), part,
                     peer, n, flags);
  HIP_LAUNCH_CHECK();
}

#define WIN_DISPATCH(kernel, func, ...)                                                                  \
  do {                                                                                                   \
    const dim3 g = win_grid(n), b(kWinThreads);                                                          \
    switch (func) {                                                                                      \
      case WF_SUM_I: hipLaunchKernelGGL(kernel<WF_SUM_I>, g, b, 0, s, __VA_ARGS__); break;               \
      case WF_SUM_F: hipLaunchKernelGGL(kernel<WF_SUM_F>, g, b, 0, s, __VA_ARGS__); break;               \
      case WF_MIN: hipLaunchKernelGGL(kernel<WF_MIN>, g, b, 0, s, __VA_ARGS__); break;                   \
      case WF_MAX: hipLaunchKernelGGL(kernel<WF_MAX>, g, b, 0, s, __VA_ARGS__); break;                   \
      default: hipLaunchKernelGGL(kernel<WF_COUNT>, g, b, 0, s, __VA_ARGS__); break;                     \
    }                                                                                                    \
    HIP_LAUNCH_CHECK();                                                                                  \
  } while (0)

void window_tile(const ColView &col, const int64_t *perm, const uint8_t *flags, int64_t n, int func, uint64_t *dense,
                 uint8_t *dense_valid, bool gather, int64_t *tile_agg, uint8_t *tile_flag, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  win_check_value(col, func);
  win_aligned(perm, "perm");
  win_aligned(flags, "flags");
  win_aligned(dense, "dense values");
  if (dense_valid != nullptr) win_aligned(dense_valid, "dense validity");
  CYLON_CHECK(tile_agg != nullptr && tile_flag != nullptr, Code::Invalid, "window: tile pairs");
  // a column with nulls must come with a dense validity array, in both modes
  CYLON_CHECK(!gather || col.valid == nullptr || dense_valid != nullptr, Code::Invalid,
              "window: nullable column without a dense validity buffer");
  ColView c = col;
  if (!(c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8)) c.width = 0;  // COUNT: validity only
  WIN_DISPATCH(k_win_tile, func, c, perm, flags, n, dense, dense_valid, gather ? 1 : 0, tile_agg, tile_flag);
}

void window_carry(const int64_t *tile_agg, const uint8_t *tile_flag, int64_t ntiles, int words, int func,
                  int64_t step, int64_t *carry, void *stream) {
  if (ntiles == 0) return;
  hipStream_t s = as_stream(stream);
  if (step <= 0) step = kWinCarryTiles;
  CYLON_CHECK(step <= kWinCarryTiles, Code::Invalid, "window: carry step of " << step << " tiles");
  CYLON_CHECK((func == WF_RANK) == (words == 3) && (func == WF_RANK || words == 1) && func >= 0 && func <= WF_RANK,
              Code::Invalid, "window: carry of function " << func << " with " << words << " words");
  const dim3 g(1), b(kWinThreads);
  switch (func) {
    case WF_SUM_I:
    case WF_COUNT: hipLaunchKernelGGL(k_win_carry<ValScan<WF_SUM_I>>, g, b, 0, s, tile_agg, tile_flag, ntiles, step, carry); break;
    case WF_SUM_F: hipLaunchKernelGGL(k_win_carry<ValScan<WF_SUM_F>>, g, b, 0, s, tile_agg, tile_flag, ntiles, step, carry); break;
    case WF_MIN: hipLaunchKernelGGL(k_win_carry<ValScan<WF_MIN>>, g, b, 0, s, tile_agg, tile_flag, ntiles, step, carry); break;
    case WF_MAX: hipLaunchKernelGGL(k_win_carry<ValScan<WF_MAX>>, g, b, 0, s, tile_agg, tile_flag, ntiles, step, carry); break;
    default: hipLaunchKernelGGL(k_win_carry<RankScan>, g, b, 0, s, tile_agg, tile_flag, ntiles, step, carry); break;
  }
  HIP_LAUNCH_CHECK();
}

void window_apply(const ColView &col, const int64_t *perm, const uint8_t *flags, int64_t n, int func,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry, uint8_t *out,
                  uint8_t *out_valid, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  win_check_value(col, func);
  win_aligned(perm, "perm");
  win_aligned(flags, "flags");
  win_aligned(dense, "dense values");
  if (dense_valid != nullptr) win_aligned(dense_valid, "dense validity");
  CYLON_CHECK(carry != nullptr && out != nullptr, Code::Invalid, "window: carry and output");
  ColView c = col;
  if (!(c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8)) c.width = 0;
  const int ow = (func == WF_MIN || func == WF_MAX) ? c.width : 8;
  CYLON_CHECK(reinterpret_cast<uintptr_t>(out) % ow == 0, Code::Invalid, "window: unaligned output");
  WIN_DISPATCH(k_win_apply, func, c, perm, flags, n, dense, dense_valid, carry, out, out_valid);
}

void window_rank_tile(const uint8_t *flags, int64_t n, int64_t *tile_agg, uint8_t *tile_flag, void *stream) {
  if (n == 0) return;
  win_aligned(flags, "flags");
  CYLON_CHECK(tile_agg != nullptr && tile_flag != nullptr, Code::Invalid, "window: tile pairs");
  hipLaunchKernelGGL(k_win_rank_tile, win_grid(n), dim3(kWinThreads), 0, as_stream(stream), flags, n, tile_agg,
                     tile_flag);
  HIP_LAUNCH_CHECK();
}

void window_rank_apply(const int64_t *perm, const uint8_t *flags, int64_t n, const int64_t *carry,
                       int64_t *row_number, int64_t *rank, int64_t *dense_rank, int64_t *phead, void *stream) {
  if (n == 0) return;
  win_aligned(perm, "perm");
  win_aligned(flags, "flags");
  if (phead != nullptr) win_aligned(phead, "partition heads");
  CYLON_CHECK(carry != nullptr, Code::Invalid, "window: carry");
  hipLaunchKernelGGL(k_win_rank_apply, win_grid(n), dim3(kWinThreads), 0, as_stream(stream), perm, flags, n, carry,
                     row_number, rank, dense_rank, phead);
  HIP_LAUNCH_CHECK();
}

void window_shift(const int64_t *perm, const int64_t *phead, int64_t n, int64_t delta, int64_t *src, void *stream) {
  if (n == 0) return;
  CYLON_CHECK(delta >= -n && delta <= n, Code::Invalid, "window: shift of " << delta << " over " << n << " rows");
  hipLaunchKernelGGL(k_win_shift, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), perm, phead, n, delta, src);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_window() { preload_code(reinterpret_cast<const void *>(&k_win_shift)); }

}  // namespace hip
}  // namespace cylon
