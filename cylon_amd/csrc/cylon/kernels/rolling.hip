// Bounded ROWS frames (rolling COUNT / SUM / MEAN / MIN / MAX) over the sorted positions of a
// permutation, gfx950.  Semantics: docs/semantics.md "Framed aggregates"; the CPU twin
// (cpu_rolling.cpp) is the definition.
//
// The frame of sorted position i is [lo, hi] = [max(i - preceding, head), min(i + following, tail)] of
// i's partition, w = preceding + following + 1.  The positions are cut into blocks of w by absolute
// position and two segmented scans are formed, each restarting at every block and partition edge:
//   P[j] = x[max(block start, head)] o .. o x[j]      S[j] = x[j] o .. o x[min(block end, tail)]
// A frame is at most w long, so it holds at most one block start b after lo, and
//   b exists                       -> S[lo] o P[hi]   (two disjoint pieces of the frame)
//   lo is a block start or head    -> P[hi]
//   otherwise (hi is the tail)     -> S[lo]
// Every result is therefore a combination of values of its own frame only (nothing is subtracted),
// and the cost per row does not depend on w.  The non-null count m goes through the same two scans.
//
//   k_roll_lds      w <= kRollLdsRows.  One launch.  A tile of kWinTile positions loads the dense
//                   values, validity bytes and flags of [tile_lo - halo, tile_hi + halo] (halo = w - 1
//                   rounded up to 8) into registers kWinTile positions at a time, scans them forwards
//                   with the block scan of window_scan.hpp (the running state carried from one step
//                   to the next) and leaves P in LDS; after a barrier the backward scan re-reads the
//                   values from LDS in reverse order and leaves S there.  Then every thread forms the
//                   results of its kWinItems positions and scatters them to out[perm[i]].
//   k_roll_tile / window_carry / k_roll_scan
//                   the wide path: the three-phase scan of window.hip with the block edges as further
//                   restarts, once forwards and once over the reversed order (position k of the
//                   reversed order is position n - 1 - k), P and S (and the counts) written to HBM.
//   k_roll_combine  applies the rule above from P, S, phead and the reversed tails.
// No workgroup waits for another one.
//
// Bounds: perm, flags, dense, phead, rtail, P, S are whole allocations of n elements (16-byte
// aligned).  A run of kWinItems positions that lies inside [0, n) is read unpredicated; every other
// position -- the halo before 0 and past n, the last partial tile -- is tested element by element.
// LDS indices are lo - base and hi - base with base = tile_lo - halo <= lo <= hi < base + R.
#include "rolling_check.hpp"
#include "window_scan.hpp"

namespace cylon {
namespace hip {

constexpr int kRollBytesPerRow = 8 + 8 + 2 + 2;  // P, S, and the two counts

struct RollVal {
  uint64_t a;  // as WinVal::a
  uint32_t c;  // non-null values in the range
  uint32_t f;  // a restart lies in the range
};

template <int F>
struct RollScan {
  using S = RollVal;
  static __device__ __forceinline__ S identity() { return S{F == WF_MIN ? ~0ull : 0ull, 0u, 0u}; }
  static __device__ __forceinline__ S combine(const S &l, const S &r) {
    return S{r.f ? r.a : win_op<F>(l.a, r.a), r.f ? r.c : l.c + r.c, l.f | r.f};
  }
  static __device__ __forceinline__ S shfl_up(const S &s, int d) {
    return S{(uint64_t)__shfl_up((int64_t)s.a, d, kWave), (uint32_t)__shfl_up((int)s.c, d, kWave),
             (uint32_t)__shfl_up((int)s.f, d, kWave)};
  }
};

// the result of a frame: aggregate a over m non-null values
template <int F>
__device__ __forceinline__ void roll_emit(uint64_t a, uint32_t m, int w, int kind, int mean, int64_t minp,
                                          int64_t row, uint8_t *out, uint8_t *ovalid) {
  if (F == WF_MIN || F == WF_MAX) {
    win_store_bits(out, row, w, order_unimage(a, w, kind));
  } else if (mean) {
    double s;
    if (F == WF_SUM_F) s = __longlong_as_double((long long)a);
    else s = kind == static_cast<int>(ValueKind::SIGNED_INT) ? (double)(int64_t)a : (double)a;
    reinterpret_cast<double *>(out)[row] = s / (double)m;
  } else {
    reinterpret_cast<uint64_t *>(out)[row] = a;
  }
  if (ovalid != nullptr) ovalid[row] = (int64_t)m >= minp ? 1 : 0;
}

// which of P[hi], S[lo] make up the frame [lo, hi] of position i (i - w < lo <= i <= hi < i + w):
// bit 0 = S[lo], bit 1 = P[hi]
__device__ __forceinline__ int roll_pieces(int64_t i, int64_t imod, int64_t lo, int64_t hi, int64_t head,
                                           int64_t w) {
  const int64_t b = i - imod;  // the block start at or before i
  if (b > lo || b + w <= hi) return 3;
  return (lo == b || lo == head) ? 2 : 1;
}

// ---------------------------------------------------------------------------
// the LDS path
// ---------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(kWinThreads) void k_roll_lds(ColView c, const int64_t *__restrict__ perm,
                                                          const uint8_t *__restrict__ flags,
                                                          const uint64_t *__restrict__ dense,
                                                          const uint8_t *__restrict__ dvalid,
                                                          const int64_t *__restrict__ phead,
                                                          const int64_t *__restrict__ rtail, int64_t n, int p, int f,
                                                          int64_t minp, int mean, uint8_t *__restrict__ out,
                                                          uint8_t *__restrict__ ovalid) {
  using T = RollScan<F>;
  extern __shared__ __align__(16) uint8_t smem[];
  const int w = p + f + 1;
  const int halo = (w - 1 + 7) / 8 * 8;
  const int R = kWinTile + 2 * halo;  // a multiple of kWinItems
  RollVal *lds = reinterpret_cast<RollVal *>(smem);
  uint64_t *Pa = reinterpret_cast<uint64_t *>(smem + kWinWaves * sizeof(RollVal));
  uint64_t *Sa = Pa + R;
  uint16_t *Pc = reinterpret_cast<uint16_t *>(Sa + R);
  uint16_t *Sc = Pc + R;
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t tile_lo = t * kWinTile;
    const int64_t base = tile_lo - halo;  // a multiple of kWinItems, may be negative
    const int bmod = (int)(((base % w) + w) % w);

    // forwards: P, and the values and backward restarts parked in S's arrays
    RollVal run = T::identity();
    for (int c0 = 0; c0 < R; c0 += kWinTile) {
      const int q0 = c0 + (int)threadIdx.x * kWinItems;
      const bool in_r = q0 < R;
      const int64_t g0 = base + q0;
      const bool full = in_r && g0 >= 0 && g0 + kWinItems <= n;
      uint64_t bits[kWinItems];
      uint8_t live[kWinItems], fl[kWinItems + 1];
      if (full) {
        win_load8_u64(dense, g0, n, true, bits);
        win_load8_u8(flags, g0, n, true, fl);
        if (dvalid != nullptr) {
          win_load8_u8(dvalid, g0, n, true, live);
        } else {
#pragma unroll
          for (int k = 0; k < kWinItems; ++k) live[k] = 1;
        }
      } else {
#pragma unroll
        for (int k = 0; k < kWinItems; ++k) {
          const int64_t g = g0 + k;
          const bool in = in_r && g >= 0 && g < n;
          bits[k] = in ? dense[g] : 0;
          fl[k] = in ? flags[g] : 0;
          live[k] = in ? (dvalid != nullptr ? dvalid[g] : 1) : 0;
        }
      }
      {
        const int64_t g = g0 + kWinItems;
        fl[kWinItems] = (in_r && g >= 0 && g < n) ? flags[g] : 0;
      }
      int m = (bmod + q0) % w;  // (g0 + k) mod w, kept up item by item
      RollVal e[kWinItems];
      uint16_t back[kWinItems];
      RollVal agg = T::identity();
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) {
        const int64_t g = g0 + k;
        const bool lv = live[k] != 0;
        e[k] = RollVal{win_widen<F>(bits[k], lv, c.width, c.kind), lv ? 1u : 0u,
                       (uint32_t)((m == 0) | (fl[k] & 1))};
        m = m + 1 == w ? 0 : m + 1;
        // the backward scan restarts where a block or a partition ends, or the table does
        back[k] = (uint16_t)((lv ? 1 : 0) | (((m == 0) | (fl[k + 1] & 1) | (g + 1 >= n)) ? 2 : 0));
        agg = T::combine(agg, e[k]);
      }
      RollVal tot;
      RollVal x = win_block_exclusive<T>(agg, run, lds, &tot);
      run = tot;
      if (in_r) {
#pragma unroll
        for (int k = 0; k < kWinItems; ++k) {
          x = T::combine(x, e[k]);
          Pa[q0 + k] = x.a;
          Pc[q0 + k] = (uint16_t)x.c;
          Sa[q0 + k] = e[k].a;
          Sc[q0 + k] = back[k];
        }
      }
    }

    // The last forward step's stores to S's arrays are read below by other threads, for the wider
    // frames by threads of another wave; nothing before this orders the two.
    __syncthreads();
    // backwards, in place: within this pass a thread reads and writes only its own kWinItems slots
    run = T::identity();
    for (int c0 = 0; c0 < R; c0 += kWinTile) {
      const int r0 = c0 + (int)threadIdx.x * kWinItems;  // position in the reversed order
      const bool in_r = r0 < R;
      RollVal e[kWinItems];
      RollVal agg = T::identity();
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) {
        const int q = R - 1 - (r0 + k);
        e[k] = in_r ? RollVal{Sa[q], (uint32_t)(Sc[q] & 1), (uint32_t)(Sc[q] >> 1)} : T::identity();
        agg = T::combine(agg, e[k]);
      }
      RollVal tot;
      RollVal x = win_block_exclusive<T>(agg, run, lds, &tot);
      run = tot;
      if (in_r) {
#pragma unroll
        for (int k = 0; k < kWinItems; ++k) {
          const int q = R - 1 - (r0 + k);
          x = T::combine(x, e[k]);
          Sa[q] = x.a;
          Sc[q] = (uint16_t)x.c;
        }
      }
    }
    __syncthreads();

    // the results of this tile
    {
      const bool full = tile_lo + kWinTile <= n;
      const int64_t i0 = tile_lo + (int64_t)threadIdx.x * kWinItems;
      uint64_t row[kWinItems], head[kWinItems];
      win_load8_u64(reinterpret_cast<const uint64_t *>(perm), i0, n, full, row);
      win_load8_u64(reinterpret_cast<const uint64_t *>(phead), i0, n, full, head);
      int m = (int)((tile_lo % w + (int64_t)threadIdx.x * kWinItems) % w);  // i mod w
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) {
        const int64_t i = i0 + k;
        if (full || i < n) {  // row[k] < n
          const int64_t hd = (int64_t)head[k], tl = n - 1 - rtail[n - 1 - i];
          const int64_t lo = i - p > hd ? i - p : hd;
          const int64_t hi = i + f < tl ? i + f : tl;
          const int ql = (int)(lo - base), qh = (int)(hi - base);  // in [0, R)
          const int pieces = roll_pieces(i, m, lo, hi, hd, w);
          uint64_t a;
          uint32_t cnt;
          if (pieces == 3) {
            a = win_op<F>(Sa[ql], Pa[qh]);
            cnt = (uint32_t)Sc[ql] + Pc[qh];
          } else if (pieces == 2) {
            a = Pa[qh];
            cnt = Pc[qh];
          } else {
            a = Sa[ql];
            cnt = Sc[ql];
          }
          roll_emit<F>(a, cnt, c.width, c.kind, mean, minp, (int64_t)row[k], out, ovalid);
        }
        m = m + 1 == w ? 0 : m + 1;
      }
    }
    __syncthreads();  // before the next tile overwrites P and S
  }
}

// ---------------------------------------------------------------------------
// the wide path
// ---------------------------------------------------------------------------
// kWinItems elements from position k0 of the scan order.  REV: position k is sorted position
// n - 1 - k; rst is always in scan order (the flags, or window_rev_flags' output).
template <int F, bool REV>
__device__ __forceinline__ void roll_load(const ColView &c, const uint8_t *__restrict__ rst,
                                          const uint64_t *__restrict__ dense, const uint8_t *__restrict__ dvalid,
                                          int64_t n, int64_t w, int64_t k0, bool full, RollVal *e) {
  uint64_t bits[kWinItems];
  uint8_t live[kWinItems], fl[kWinItems];
  win_load8_u8(rst, k0, n, full, fl);
  if (!REV) {
    win_load8_u64(dense, k0, n, full, bits);
    if (dvalid != nullptr) {
      win_load8_u8(dvalid, k0, n, full, live);
    } else {
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) live[k] = (full || k0 + k < n) ? 1 : 0;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      const bool in = full || k0 + k < n;
      const int64_t g = n - 1 - (k0 + k);  // >= 0 when in
      bits[k] = in ? dense[g] : 0;
      live[k] = in ? (dvalid != nullptr ? dvalid[g] : 1) : 0;
    }
  }
  // forwards a block starts where g mod w == 0; backwards the scan restarts at a block's last
  // position, (g + 1) mod w == 0 with g + 1 = n - k
  int64_t m = REV ? (n - k0) % w : k0 % w;
#pragma unroll
  for (int k = 0; k < kWinItems; ++k) {
    const bool lv = live[k] != 0;
    e[k] = RollVal{win_widen<F>(bits[k], lv, c.width, c.kind), lv ? 1u : 0u, (uint32_t)((m == 0) | (fl[k] & 1))};
    if (REV) m = m == 0 ? w - 1 : m - 1;
    else m = m + 1 == w ? 0 : m + 1;
  }
}

template <int F, bool REV>
__global__ __launch_bounds__(kWinThreads) void k_roll_tile(ColView c, const uint8_t *__restrict__ rst,
                                                           const uint64_t *__restrict__ dense,
                                                           const uint8_t *__restrict__ dvalid, int64_t n, int64_t w,
                                                           int64_t *__restrict__ tagg, int64_t *__restrict__ tcnt,
                                                           uint8_t *__restrict__ tflag) {
  using T = RollScan<F>;
  __shared__ RollVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    RollVal e[kWinItems];
    roll_load<F, REV>(c, rst, dense, dvalid, n, w, k0, full, e);
    RollVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      if (full || k0 + k < n) agg = T::combine(agg, e[k]);
    RollVal tot;
    win_block_exclusive<T>(agg, T::identity(), lds, &tot);
    if (threadIdx.x == 0) {
      tagg[t] = (int64_t)tot.a;
      tcnt[t] = (int64_t)tot.c;
      tflag[t] = (uint8_t)tot.f;
    }
  }
}

template <int F, bool REV>
__global__ __launch_bounds__(kWinThreads) void k_roll_scan(ColView c, const uint8_t *__restrict__ rst,
                                                           const uint64_t *__restrict__ dense,
                                                           const uint8_t *__restrict__ dvalid, int64_t n, int64_t w,
                                                           const int64_t *__restrict__ carry,
                                                           const int64_t *__restrict__ carry_cnt,
                                                           uint64_t *__restrict__ scan, uint32_t *__restrict__ scan_cnt) {
  using T = RollScan<F>;
  __shared__ RollVal lds[kWinWaves];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t k0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    RollVal e[kWinItems];
    roll_load<F, REV>(c, rst, dense, dvalid, n, w, k0, full, e);
    RollVal agg = T::identity();
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      if (full || k0 + k < n) agg = T::combine(agg, e[k]);
    RollVal tot;
    RollVal x = win_block_exclusive<T>(agg, RollVal{(uint64_t)carry[t], (uint32_t)carry_cnt[t], 0u}, lds, &tot);
    uint64_t va[kWinItems];
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      x = T::combine(x, e[k]);
      va[k] = x.a;
      if (full || k0 + k < n) scan_cnt[k0 + k] = x.c;
    }
    win_store8_u64(scan, k0, n, full, va);
  }
}

// P in sorted order, S in reversed order (S of sorted position j at n - 1 - j)
template <int F>
__global__ void k_roll_combine(ColView c, const int64_t *__restrict__ perm, const int64_t *__restrict__ phead,
                               const int64_t *__restrict__ rtail, int64_t n, int64_t p, int64_t f, int64_t minp,
                               int mean, const uint64_t *__restrict__ P, const uint32_t *__restrict__ Pc,
                               const uint64_t *__restrict__ S, const uint32_t *__restrict__ Sc,
                               uint8_t *__restrict__ out, uint8_t *__restrict__ ovalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t w = p + f + 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t hd = phead[i], tl = n - 1 - rtail[n - 1 - i];
    const int64_t lo = i - p > hd ? i - p : hd;
    const int64_t hi = i + f < tl ? i + f : tl;
    const int pieces = roll_pieces(i, i % w, lo, hi, hd, w);
    uint64_t a;
    uint32_t cnt;
    if (pieces == 3) {
      a = win_op<F>(S[n - 1 - lo], P[hi]);
      cnt = Sc[n - 1 - lo] + Pc[hi];
    } else if (pieces == 2) {
      a = P[hi];
      cnt = Pc[hi];
    } else {
      a = S[n - 1 - lo];
      cnt = Sc[n - 1 - lo];
    }
    roll_emit<F>(a, cnt, c.width, c.kind, mean, minp, perm[i], out, ovalid);
  }
}

// rflags[k] = 3 where position k of the reversed order starts a partition there, i.e. sorted
// position n - 1 - k is a partition's last one; else 0
__global__ void k_roll_rev_flags(const uint8_t *__restrict__ flags, int64_t n, uint8_t *__restrict__ rflags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
    rflags[k] = (k == 0 || (flags[n - k] & 1)) ? 3 : 0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t window_frame_lds_rows() { return kRollLdsRows; }

static void roll_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "rolling: " << what << " must be a 16-byte aligned buffer");
}

static void roll_check_out(const ColView &c, int func, const uint8_t *out) {
  const int ow = (func == WF_MIN || func == WF_MAX) ? c.width : 8;
  CYLON_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % ow == 0, Code::Invalid, "rolling: output");
}

#define ROLL_DISPATCH(func, LAUNCH)        \
  do {                                     \
    switch (func) {                        \
      case WF_SUM_I: LAUNCH(WF_SUM_I); break; \
      case WF_SUM_F: LAUNCH(WF_SUM_F); break; \
      case WF_MIN: LAUNCH(WF_MIN); break;  \
      case WF_MAX: LAUNCH(WF_MAX); break;  \
      default: LAUNCH(WF_COUNT); break;    \
    }                                      \
    HIP_LAUNCH_CHECK();                    \
  } while (0)

void window_rev_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *stream) {
  if (n == 0) return;
  CYLON_CHECK(flags != nullptr && rflags != nullptr, Code::Invalid, "rolling: flags");
  hipLaunchKernelGGL(k_roll_rev_flags, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), flags, n, rflags);
  HIP_LAUNCH_CHECK();
}

void rolling_lds(const ColView &col, const int64_t *perm, const uint8_t *flags, const int64_t *phead,
                 const int64_t *rtail, int64_t n, int func, bool mean, int64_t preceding, int64_t following,
                 int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, uint8_t *out,
                 uint8_t *out_valid, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  const ColView c = rolling_check(col, func, n, preceding, following, min_periods, mean);
  CYLON_CHECK(preceding + following + 1 <= kRollLdsRows, Code::Invalid,
              "rolling: a frame of " << preceding + following + 1 << " rows does not fit the LDS path");
  roll_aligned(perm, "perm");
  roll_aligned(flags, "flags");
  roll_aligned(phead, "partition heads");
  roll_aligned(dense, "dense values");
  if (dense_valid != nullptr) roll_aligned(dense_valid, "dense validity");
  CYLON_CHECK(rtail != nullptr, Code::Invalid, "rolling: reversed tails");
  roll_check_out(c, func, out);
  const int p = (int)preceding, f = (int)following;
  const int halo = (p + f + 7) / 8 * 8;
  const size_t lds = kWinWaves * sizeof(RollVal) + (size_t)(kWinTile + 2 * halo) * kRollBytesPerRow;
  const dim3 g(grid_for((n + kWinTile - 1) / kWinTile, 1)), b(kWinThreads);
#define ROLL_LAUNCH(F)                                                                                          \
  hipLaunchKernelGGL(k_roll_lds<F>, g, b, lds, s, c, perm, flags, dense, dense_valid, phead, rtail, n, p, f, \
                     min_periods, mean ? 1 : 0, out, out_valid)
  ROLL_DISPATCH(func, ROLL_LAUNCH);
#undef ROLL_LAUNCH
}

void rolling_tile(const ColView &col, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
                  const uint64_t *dense, const uint8_t *dense_valid, int64_t *tile_agg, int64_t *tile_cnt,
                  uint8_t *tile_flag, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  const ColView c = rolling_check(col, func, n, 0, 0, 0, false);
  CYLON_CHECK(w >= 1, Code::Invalid, "rolling: frame of " << w << " rows");
  roll_aligned(restarts, "flags");
  roll_aligned(dense, "dense values");
  if (dense_valid != nullptr) roll_aligned(dense_valid, "dense validity");
  CYLON_CHECK(tile_agg != nullptr && tile_cnt != nullptr && tile_flag != nullptr, Code::Invalid, "rolling: tile pairs");
  const dim3 g(grid_for((n + kWinTile - 1) / kWinTile, 1)), b(kWinThreads);
#define ROLL_LAUNCH(F)                                                                                             \
  if (reverse)                                                                                                     \
    hipLaunchKernelGGL((k_roll_tile<F, true>), g, b, 0, s, c, restarts, dense, dense_valid, n, w, tile_agg, tile_cnt, \
                       tile_flag);                                                                                 \
  else                                                                                                             \
    hipLaunchKernelGGL((k_roll_tile<F, false>), g, b, 0, s, c, restarts, dense, dense_valid, n, w, tile_agg,       \
                       tile_cnt, tile_flag)
  ROLL_DISPATCH(func, ROLL_LAUNCH);
#undef ROLL_LAUNCH
}

void rolling_scan(const ColView &col, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry, const int64_t *carry_cnt,
                  uint64_t *scan, uint32_t *scan_cnt, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  const ColView c = rolling_check(col, func, n, 0, 0, 0, false);
  CYLON_CHECK(w >= 1, Code::Invalid, "rolling: frame of " << w << " rows");
  roll_aligned(restarts, "flags");
  roll_aligned(dense, "dense values");
  roll_aligned(scan, "scan");
  if (dense_valid != nullptr) roll_aligned(dense_valid, "dense validity");
  CYLON_CHECK(carry != nullptr && carry_cnt != nullptr && scan_cnt != nullptr, Code::Invalid, "rolling: carries");
  const dim3 g(grid_for((n + kWinTile - 1) / kWinTile, 1)), b(kWinThreads);
#define ROLL_LAUNCH(F)                                                                                            \
  if (reverse)                                                                                                    \
    hipLaunchKernelGGL((k_roll_scan<F, true>), g, b, 0, s, c, restarts, dense, dense_valid, n, w, carry, carry_cnt, \
                       scan, scan_cnt);                                                                           \
  else                                                                                                            \
    hipLaunchKernelGGL((k_roll_scan<F, false>), g, b, 0, s, c, restarts, dense, dense_valid, n, w, carry,         \
                       carry_cnt, scan, scan_cnt)
  ROLL_DISPATCH(func, ROLL_LAUNCH);
#undef ROLL_LAUNCH
}

void rolling_combine(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail, int64_t n,
                     int func, bool mean, int64_t preceding, int64_t following, int64_t min_periods,
                     const uint64_t *fwd, const uint32_t *fwd_cnt, const uint64_t *bwd, const uint32_t *bwd_cnt,
                     uint8_t *out, uint8_t *out_valid, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  const ColView c = rolling_check(col, func, n, preceding, following, min_periods, mean);
  CYLON_CHECK(perm != nullptr && phead != nullptr && rtail != nullptr && fwd != nullptr && fwd_cnt != nullptr &&
                  bwd != nullptr && bwd_cnt != nullptr,
              Code::Invalid, "rolling: combine inputs");
  roll_check_out(c, func, out);
  const dim3 g(grid_for(n)), b(kBlock);
#define ROLL_LAUNCH(F)                                                                                       \
  hipLaunchKernelGGL(k_roll_combine<F>, g, b, 0, s, c, perm, phead, rtail, n, preceding, following, min_periods, \
                     mean ? 1 : 0, fwd, fwd_cnt, bwd, bwd_cnt, out, out_valid)
  ROLL_DISPATCH(func, ROLL_LAUNCH);
#undef ROLL_LAUNCH
}

void preload_rolling() { preload_code(reinterpret_cast<const void *>(&k_roll_rev_flags)); }

}  // namespace hip
}  // namespace cylon
