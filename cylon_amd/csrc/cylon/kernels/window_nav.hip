// Navigation and distribution window functions (FIRST / LAST / NTH_VALUE, FFILL / BFILL, NTILE,
// PERCENT_RANK, CUME_DIST) over the sorted positions of a permutation, gfx950.  Semantics:
// docs/semantics.md "Navigation and distribution functions"; the CPU twin (cpu_window_nav.cpp) is the
// definition.
//
// Everything starts from what the window operator (ops/window.cpp) already holds: perm, the flag byte
// of every sorted position, the dense (sorted-order) values and validity bytes of k_win_tile, phead
// from the rank scan and rtail from the same scan over the reversed flags.
//
// A fill is "the nearest non-null position at or before me in my partition": the segmented running
// maximum of "scan position + 1 where the validity byte is set, else 0", ValScan<WF_MAX> of
// window_scan.hpp in the three launches of window.hip, with no hand-off between workgroups:
//   k_nav_fill_tile    one tile of kWinTile positions per block step: streams the restarts and the
//                      validity bytes (8-byte loads), reduces to the tile's (flag, aggregate) pair.
//   window_carry       (window.hip, words 1, func 3) unchanged: each tile's carry-in.
//   k_nav_fill_apply   re-scans the tile with its carry-in, applies the limit, and then either copies
//                      the value (widths 1, 2, 4, 8: out[perm[i]] = dense[j], one scatter, no position
//                      array in between) or names the source row (src[perm[i]] = perm[j]) for
//                      GatherColumn; IGNORE NULLS forms also take the position itself (pos[i] = j).
// REV: the scan runs over the reversed order (scan position k is sorted position n - 1 - k, read
// element by element as rolling.hip does); rst is then window_rev_flags' output, in scan order.
//   k_nav_pick         one thread per sorted position: the position FIRST / LAST / NTH_VALUE read.
//   k_nav_rev_peer     the reversed flags with the peer tails in bit 1.
//   k_nav_rank_heads   the rank scan's apply that keeps the p and q words (partition head, peer head)
//                      in scan order.
//   k_nav_dist         NTILE / PERCENT_RANK / CUME_DIST from those, element-wise.
//
// Bounds: perm, rst, dense, dvalid, phead, rtail and pos are whole allocations of n elements (checked
// to be 16-byte aligned where a tile reads them); a full tile is read unpredicated, the last partial
// tile element by element with k < n; rows are addressed only through perm[i] in [0, n).  A carried
// scan value `run` at scan position k is 0 or the scan position + 1 of a position at or before k, so
// run - 1 lies in [0, k] and its sorted position (run - 1, or n - run when reversed) in [0, n).
// phead[i] lies in [0, i] and the tail n - 1 - rtail[n - 1 - i] in [i, n): both are positions the rank
// scan met; a fill position read through them is -1 or a position of the same partition.
#include "window_scan.hpp"

namespace cylon {
namespace hip {

using NavScan = ValScan<WF_MAX>;

enum NavForm : int { NAV_FIRST = 0, NAV_LAST = 1, NAV_NTH = 2, NAV_FIRST_LIVE = 3, NAV_LAST_LIVE = 4 };
enum NavDist : int { NAV_NTILE = 0, NAV_PERCENT_RANK = 1, NAV_CUME_DIST = 2 };

// kWinItems validity bytes from scan position k0
template <bool REV>
__device__ __forceinline__ void nav_load_live(const uint8_t *__restrict__ dvalid, int64_t k0, int64_t n, bool full,
                                              uint8_t *live) {
  if (!REV) {
    win_load8_u8(dvalid, k0, n, full, live);
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) live[k] = (full || k0 + k < n) ? dvalid[n - 1 - (k0 + k)] : 0;
  }
}

// kWinItems 8-byte words (perm, dense) from scan position k0
template <bool REV>
__device__ __forceinline__ void nav_load_u64(const uint64_t *__restrict__ p, int64_t k0, int64_t n, bool full,
                                             uint64_t *v) {
  if (!REV) {
    win_load8_u64(p, k0, n, full, v);
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) v[k] = (full || k0 + k < n) ? p[n - 1 - (k0 + k)] : 0;
  }
}

// ---------------------------------------------------------------------------
// the fill scan
// ---------------------------------------------------------------------------
template <bool REV>
__global__ __launch_bounds__(kWinThreads) void k_nav_fill_tile(const uint8_t *__restrict__ rst,
                                                               const uint8_t *__restrict__ dvalid, int64_t n,
                                                               int64_t *__restrict__ tagg,
                                                               uint8_t *__restrict__ tflag) {
  using T = NavScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint8_t fl[kWinItems], live[kWinItems];
    win_load8_u8(rst, k0, n, full, fl);  // 0 past n
    nav_load_live<REV>(dvalid, k0, n, full, live);
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      agg = T::combine(agg, WinVal{live[k] != 0 ? (uint64_t)(k0 + k + 1) : 0ull, (uint32_t)(fl[k] & 1)});
    WinVal tot;
    win_block_exclusive<T>(agg, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      tagg[t] = (int64_t)tot.a;
      tflag[t] = (uint8_t)tot.f;
    }
  }
}

// MODE: bit 0 = value mode (out, ovalid), bit 1 = source mode (src); pos is written where not nullptr
template <bool REV, int MODE>
__global__ __launch_bounds__(kWinThreads) void k_nav_fill_apply(int width, const int64_t *__restrict__ perm,
                                                                const uint8_t *__restrict__ rst,
                                                                const uint64_t *__restrict__ dense,
                                                                const uint8_t *__restrict__ dvalid, int64_t n,
                                                                int64_t limit, const int64_t *__restrict__ carry,
                                                                uint8_t *__restrict__ out,
                                                                uint8_t *__restrict__ ovalid,
                                                                int64_t *__restrict__ src,
                                                                int64_t *__restrict__ pos) {
  using T = NavScan;
  __shared__ WinVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t row[kWinItems], own[kWinItems], x[kWinItems];
    uint8_t fl[kWinItems], live[kWinItems];
    win_load8_u8(rst, k0, n, full, fl);
    nav_load_live<REV>(dvalid, k0, n, full, live);
    if (MODE != 0) nav_load_u64<REV>(reinterpret_cast<const uint64_t *>(perm), k0, n, full, row);
    if (MODE & 1) nav_load_u64<REV>(dense, k0, n, full, own);
    WinVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      x[k] = live[k] != 0 ? (uint64_t)(k0 + k + 1) : 0ull;
      agg = T::combine(agg, WinVal{x[k], (uint32_t)(fl[k] & 1)});
    }
    WinVal tot;
    const WinVal ex = win_block_exclusive<T>(agg, WinVal{(uint64_t)carry[t], 0u}, lds, &tot);
    uint64_t run = ex.a;
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      run = (fl[k] & 1) ? x[k] : win_op<WF_MAX>(run, x[k]);
      if (full || k0 + k < n) {  // row[k] < n
        const int64_t kk = k0 + k;
        // 0, or 1 <= run <= kk + 1: a non-null position of this partition at or before kk, + 1
        const bool has = run != 0 && (limit == 0 || kk + 1 - (int64_t)run <= limit);
        const int64_t i = REV ? n - 1 - kk : kk;
        const int64_t j = has ? (REV ? n - (int64_t)run : (int64_t)run - 1) : -1;  // in [0, n), or none
        if (MODE & 1) {
          const uint64_t v = (has && j != i) ? dense[j] : own[k];
          win_store_bits(out, (int64_t)row[k], width, v);
          ovalid[row[k]] = has ? 1 : 0;
        }
        if (MODE & 2) src[row[k]] = has ? perm[j] : -1;
        if (pos != nullptr) pos[i] = j;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// FIRST / LAST / NTH_VALUE
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_nav_pick(int width, const int64_t *__restrict__ perm,
                                                     const int64_t *__restrict__ phead,
                                                     const int64_t *__restrict__ rtail,
                                                     const int64_t *__restrict__ fillpos, int64_t n, int form,
                                                     int64_t nth, const uint64_t *__restrict__ dense,
                                                     const uint8_t *__restrict__ dvalid, uint8_t *__restrict__ out,
                                                     uint8_t *__restrict__ ovalid, int64_t *__restrict__ src) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t hd = phead != nullptr ? phead[i] : 0;                   // in [0, i]
    const int64_t tl = rtail != nullptr ? n - 1 - rtail[n - 1 - i] : 0;  // in [i, n)
    int64_t j;
    switch (form) {
      case NAV_FIRST: j = hd; break;
      case NAV_LAST: j = tl; break;
      case NAV_NTH: j = nth - 1 <= tl - hd ? hd + nth - 1 : -1; break;
      case NAV_FIRST_LIVE: j = fillpos[hd]; break;
      default: j = fillpos[tl]; break;
    }
    const int64_t r = perm[i];
    if (out != nullptr) {
      win_store_bits(out, r, width, j >= 0 ? dense[j] : 0ull);
      ovalid[r] = j >= 0 ? (dvalid != nullptr ? (uint8_t)(dvalid[j] != 0) : (uint8_t)1) : (uint8_t)0;
    }
    if (src != nullptr) src[r] = j >= 0 ? perm[j] : -1;
  }
}

// ---------------------------------------------------------------------------
// distribution functions
// ---------------------------------------------------------------------------
// rflags[k]: bit 0 = sorted position n - 1 - k is a partition's last one, bit 1 = it is the last of a
// run of peers (the next position's flag bits; the table's last position ends both)
__global__ void k_nav_rev_peer(const uint8_t *__restrict__ flags, int64_t n, uint8_t *__restrict__ rflags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
    rflags[k] = k == 0 ? (uint8_t)3 : (uint8_t)(flags[n - k] & 3);
}

__global__ __launch_bounds__(kWinThreads) void k_nav_rank_heads(const uint8_t *__restrict__ flags, int64_t n,
                                                                const int64_t *__restrict__ carry,
                                                                int64_t *__restrict__ phead,
                                                                int64_t *__restrict__ qhead) {
  using T = RankScan;
  __shared__ WinRank lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint8_t fl[kWinItems];
    win_load8_u8(flags, i0, n, full, fl);
    WinRank agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) agg = T::combine(agg, T::element(fl[k], i0 + k));
    WinRank tot;
    const WinRank cin{carry[3 * t], carry[3 * t + 1], carry[3 * t + 2], 0u};
    WinRank run = win_block_exclusive<T>(agg, cin, lds, &tot);
    uint64_t ph[kWinItems], qh[kWinItems];
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      run = T::combine(run, T::element(fl[k], i0 + k));
      ph[k] = (uint64_t)run.p;  // position 0 carries both bits: p, q >= 0
      qh[k] = (uint64_t)run.q;
    }
    if (phead != nullptr) win_store8_u64(reinterpret_cast<uint64_t *>(phead), i0, n, full, ph);
    if (qhead != nullptr) win_store8_u64(reinterpret_cast<uint64_t *>(qhead), i0, n, full, qh);
  }
}

__global__ __launch_bounds__(kBlock) void k_nav_dist(const int64_t *__restrict__ perm,
                                                     const int64_t *__restrict__ phead,
                                                     const int64_t *__restrict__ rtail,
                                                     const int64_t *__restrict__ qhead,
                                                     const int64_t *__restrict__ rqhead, int64_t n, int func,
                                                     int64_t nb, uint8_t *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t hd = phead[i];                   // in [0, i]
    const int64_t tl = n - 1 - rtail[n - 1 - i];  // in [i, n)
    const int64_t s = tl - hd + 1, r = i - hd;
    const int64_t row = perm[i];
    if (func == NAV_NTILE) {
      const int64_t q = s / nb, m = s % nb;  // m < nb, so m * (q + 1) <= s
      const int64_t big = m * (q + 1);
      const int64_t b = r < big ? r / (q + 1) + 1 : m + (r - big) / (q > 0 ? q : 1) + 1;
      reinterpret_cast<int64_t *>(out)[row] = b;
    } else if (func == NAV_PERCENT_RANK) {
      reinterpret_cast<double *>(out)[row] = s == 1 ? 0.0 : (double)(qhead[i] - hd) / (double)(s - 1);
    } else {
      const int64_t pt = n - 1 - rqhead[n - 1 - i];  // the last peer of i, in [i, tl]
      reinterpret_cast<double *>(out)[row] = (double)(pt - hd + 1) / (double)s;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void nav_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "window: " << what << " must be a 16-byte aligned buffer");
}

static dim3 nav_grid(int64_t n) { return dim3(grid_for((n + kWinTile - 1) / kWinTile, 1)); }

static bool nav_plain_width(int w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// the value mode's buffers, or none of them
static void nav_check_value(const ColView &col, const uint64_t *dense, const uint8_t *out, const uint8_t *out_valid) {
  if (out == nullptr) return;
  CYLON_CHECK(nav_plain_width(col.width), Code::Invalid, "window: value mode on a column of width " << col.width);
  CYLON_CHECK(out_valid != nullptr && reinterpret_cast<uintptr_t>(out) % col.width == 0, Code::Invalid,
              "window: value mode output");
  nav_aligned(dense, "dense values");
}

void window_fill_tile(const uint8_t *restarts, int64_t n, bool reverse, const uint8_t *dense_valid,
                      int64_t *tile_agg, uint8_t *tile_flag, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  nav_aligned(restarts, "restarts");
  nav_aligned(dense_valid, "dense validity");
  CYLON_CHECK(tile_agg != nullptr && tile_flag != nullptr, Code::Invalid, "window: tile pairs");
  const dim3 g = nav_grid(n), b(kWinThreads);
  if (reverse) hipLaunchKernelGGL(k_nav_fill_tile<true>, g, b, 0, s, restarts, dense_valid, n, tile_agg, tile_flag);
  else hipLaunchKernelGGL(k_nav_fill_tile<false>, g, b, 0, s, restarts, dense_valid, n, tile_agg, tile_flag);
  HIP_LAUNCH_CHECK();
}

void window_fill_apply(const ColView &col, const int64_t *perm, const uint8_t *restarts, int64_t n, bool reverse,
                       int64_t limit, const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry,
                       uint8_t *out, uint8_t *out_valid, int64_t *src, int64_t *pos, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  CYLON_CHECK(limit >= 0, Code::Invalid, "window: fill limit " << limit);
  CYLON_CHECK(out != nullptr || src != nullptr || pos != nullptr, Code::Invalid, "window: fill without an output");
  CYLON_CHECK(out == nullptr || src == nullptr, Code::Invalid, "window: fill in value mode and source mode at once");
  nav_aligned(perm, "perm");
  nav_aligned(restarts, "restarts");
  nav_aligned(dense_valid, "dense validity");
  if (pos != nullptr) nav_aligned(pos, "fill positions");
  nav_check_value(col, dense, out, out_valid);
  CYLON_CHECK(carry != nullptr, Code::Invalid, "window: carry");
  const dim3 g = nav_grid(n), b(kWinThreads);
#define NAV_LAUNCH(REV, MODE)                                                                                    \
  hipLaunchKernelGGL((k_nav_fill_apply<REV, MODE>), g, b, 0, s, col.width, perm, restarts, dense, dense_valid, n, \
                     limit, carry, out, out_valid, src, pos)
  switch ((out != nullptr ? 1 : 0) | (src != nullptr ? 2 : 0)) {
    case 0: if (reverse) NAV_LAUNCH(true, 0); else NAV_LAUNCH(false, 0); break;
    case 1: if (reverse) NAV_LAUNCH(true, 1); else NAV_LAUNCH(false, 1); break;
    default: if (reverse) NAV_LAUNCH(true, 2); else NAV_LAUNCH(false, 2); break;
  }
#undef NAV_LAUNCH
  HIP_LAUNCH_CHECK();
}

void window_nav_pick(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail,
                     const int64_t *fillpos, int64_t n, int form, int64_t k, const uint64_t *dense,
                     const uint8_t *dense_valid, uint8_t *out, uint8_t *out_valid, int64_t *src, void *stream) {
  if (n == 0) return;
  CYLON_CHECK(form >= NAV_FIRST && form <= NAV_LAST_LIVE, Code::Invalid, "window: navigation form " << form);
  CYLON_CHECK(perm != nullptr && (out != nullptr || src != nullptr), Code::Invalid, "window: navigation outputs");
  CYLON_CHECK(phead != nullptr || form == NAV_LAST || form == NAV_LAST_LIVE, Code::Invalid, "window: partition heads");
  CYLON_CHECK(rtail != nullptr || form == NAV_FIRST || form == NAV_FIRST_LIVE, Code::Invalid, "window: reversed tails");
  CYLON_CHECK(fillpos != nullptr || form < NAV_FIRST_LIVE, Code::Invalid, "window: fill positions");
  CYLON_CHECK(form != NAV_NTH || k >= 1, Code::Invalid, "window: nth_value of row " << k);
  nav_check_value(col, dense, out, out_valid);
  hipLaunchKernelGGL(k_nav_pick, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), col.width, perm, phead, rtail,
                     fillpos, n, form, k, dense, dense_valid, out, out_valid, src);
  HIP_LAUNCH_CHECK();
}

void window_rev_peer_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *stream) {
  if (n == 0) return;
  CYLON_CHECK(flags != nullptr && rflags != nullptr, Code::Invalid, "window: flags");
  hipLaunchKernelGGL(k_nav_rev_peer, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), flags, n, rflags);
  HIP_LAUNCH_CHECK();
}

void window_rank_heads(const uint8_t *flags, int64_t n, const int64_t *carry, int64_t *phead, int64_t *qhead,
                       void *stream) {
  if (n == 0) return;
  nav_aligned(flags, "flags");
  if (phead != nullptr) nav_aligned(phead, "partition heads");
  if (qhead != nullptr) nav_aligned(qhead, "peer heads");
  CYLON_CHECK(carry != nullptr, Code::Invalid, "window: carry");
  hipLaunchKernelGGL(k_nav_rank_heads, nav_grid(n), dim3(kWinThreads), 0, as_stream(stream), flags, n, carry, phead,
                     qhead);
  HIP_LAUNCH_CHECK();
}

void window_dist_apply(const int64_t *perm, const int64_t *phead, const int64_t *rtail, const int64_t *qhead,
                       const int64_t *rqhead, int64_t n, int func, int64_t k, uint8_t *out, void *stream) {
  if (n == 0) return;
  CYLON_CHECK(func >= NAV_NTILE && func <= NAV_CUME_DIST, Code::Invalid, "window: distribution function " << func);
  CYLON_CHECK(perm != nullptr && phead != nullptr && rtail != nullptr, Code::Invalid, "window: distribution inputs");
  CYLON_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % 8 == 0, Code::Invalid, "window: distribution output");
  CYLON_CHECK(func != NAV_NTILE || k >= 1, Code::Invalid, "window: ntile of " << k << " buckets");
  CYLON_CHECK(func != NAV_PERCENT_RANK || qhead != nullptr, Code::Invalid, "window: peer heads");
  CYLON_CHECK(func != NAV_CUME_DIST || rqhead != nullptr, Code::Invalid, "window: peer tails");
  hipLaunchKernelGGL(k_nav_dist, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), perm, phead, rtail, qhead,
                     rqhead, n, func, func == NAV_NTILE ? k : 1, out);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_window_nav() { preload_code(reinterpret_cast<const void *>(&k_nav_rev_peer)); }

}  // namespace hip
}  // namespace cylon
