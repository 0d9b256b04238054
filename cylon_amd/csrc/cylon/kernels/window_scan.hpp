// The scan states, the block-wide segmented scan and the tile loads / stores shared by the window
// kernels (window.hip, rolling.hip).  See window.hip for how the three phases use them.
#pragma once
#include "device_common.hpp"
#include "order_image.hpp"

namespace cylon {
namespace hip {

constexpr int kWinThreads = 256;
constexpr int kWinItems = 8;  // consecutive positions per thread: 64 B of perm, 8 flag bytes
constexpr int kWinTile = kWinThreads * kWinItems;
constexpr int kWinWaves = kWinThreads / kWave;
constexpr int kWinCarryItems = 8;  // tiles per thread and carry step
constexpr int kWinCarryTiles = kWinThreads * kWinCarryItems;

enum WinFunc : int { WF_SUM_I = 0, WF_SUM_F = 1, WF_MIN = 2, WF_MAX = 3, WF_COUNT = 4, WF_RANK = 5 };

// ---------------------------------------------------------------------------
// the two scan states
// ---------------------------------------------------------------------------
struct WinVal {
  uint64_t a;  // int64 / uint64 sum, float64 bits, order image, count
  uint32_t f;  // a partition head lies in the range
};

template <int F>
__device__ __forceinline__ uint64_t win_op(uint64_t x, uint64_t y) {
  if (F == WF_SUM_F) return (uint64_t)__double_as_longlong(__longlong_as_double((long long)x) + __longlong_as_double((long long)y));
  if (F == WF_MIN) return x < y ? x : y;
  if (F == WF_MAX) return x > y ? x : y;
  return x + y;
}

// raw column bits -> accumulator; a null value is the operator's identity
template <int F>
__device__ __forceinline__ uint64_t win_widen(uint64_t bits, bool live, int w, int kind) {
  if (!live) return F == WF_MIN ? ~0ull : 0ull;
  if (F == WF_COUNT) return 1;
  if (F == WF_SUM_I) return (uint64_t)extend_bits(bits, w, kind);
  if (F == WF_SUM_F)
    return w == 8 ? bits : (uint64_t)__double_as_longlong((double)__uint_as_float((unsigned int)bits));
  return order_image(bits, w, kind);
}

template <int F>
struct ValScan {
  using S = WinVal;
  static constexpr int kWords = 1;
  static __device__ __forceinline__ S identity() { return S{F == WF_MIN ? ~0ull : 0ull, 0u}; }
  static __device__ __forceinline__ S combine(const S &l, const S &r) {
    return S{r.f ? r.a : win_op<F>(l.a, r.a), l.f | r.f};
  }
  static __device__ __forceinline__ S shfl_up(const S &s, int d) {
    return S{(uint64_t)__shfl_up((int64_t)s.a, d, kWave), (uint32_t)__shfl_up((int)s.f, d, kWave)};
  }
  static __device__ __forceinline__ S load(const int64_t *agg, const uint8_t *flag, int64_t t) {
    return S{(uint64_t)agg[t], flag[t]};
  }
  static __device__ __forceinline__ void store(int64_t *agg, int64_t t, const S &s) { agg[t] = (int64_t)s.a; }
};

struct WinRank {
  int64_t p;  // sorted position of the last partition head (-1: none in the range)
  int64_t q;  // ... of the last peer head
  int64_t d;  // peer heads since the last partition head
  uint32_t f;
};

struct RankScan {
  using S = WinRank;
  static constexpr int kWords = 3;
  static __device__ __forceinline__ S identity() { return S{-1, -1, 0, 0u}; }
  static __device__ __forceinline__ S combine(const S &l, const S &r) {
    return S{l.p > r.p ? l.p : r.p, l.q > r.q ? l.q : r.q, r.f ? r.d : l.d + r.d, l.f | r.f};
  }
  static __device__ __forceinline__ S shfl_up(const S &s, int d) {
    return S{__shfl_up(s.p, d, kWave), __shfl_up(s.q, d, kWave), __shfl_up(s.d, d, kWave),
             (uint32_t)__shfl_up((int)s.f, d, kWave)};
  }
  static __device__ __forceinline__ S load(const int64_t *agg, const uint8_t *flag, int64_t t) {
    return S{agg[3 * t], agg[3 * t + 1], agg[3 * t + 2], flag[t]};
  }
  static __device__ __forceinline__ void store(int64_t *agg, int64_t t, const S &s) {
    agg[3 * t] = s.p;
    agg[3 * t + 1] = s.q;
    agg[3 * t + 2] = s.d;
  }
  static __device__ __forceinline__ S element(uint8_t flag, int64_t i) {
    return S{(flag & 1) ? i : -1, (flag & 2) ? i : -1, (flag & 2) ? 1 : 0, (uint32_t)(flag & 1)};
  }
};

// Block-wide exclusive segmented scan of one aggregate per thread, in thread order, with `carry` as the
// prefix of thread 0; *total = carry (+) every thread's aggregate.  lds: kWinWaves states.
template <typename T>
__device__ __forceinline__ typename T::S win_block_exclusive(const typename T::S &agg, const typename T::S &carry,
                                                             typename T::S *lds, typename T::S *total) {
  using S = typename T::S;
  const int lane = lane_id();
  const int wave = threadIdx.x / kWave;
  S inc = agg;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const S t = T::shfl_up(inc, d);
    if (lane >= d) inc = T::combine(t, inc);
  }
  if (lane == kWave - 1) lds[wave] = inc;
  __syncthreads();
  S pre = carry, tot = carry;
#pragma unroll
  for (int w = 0; w < kWinWaves; ++w) {
    const S x = lds[w];
    if (w < wave) pre = T::combine(pre, x);
    tot = T::combine(tot, x);
  }
  __syncthreads();
  S prev = T::shfl_up(inc, 1);
  if (lane == 0) prev = T::identity();
  *total = tot;
  return T::combine(pre, prev);
}

// ---------------------------------------------------------------------------
// tile loads: kWinItems consecutive positions from i0 (a multiple of kWinItems)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void win_load8_u64(const uint64_t *p, int64_t i0, int64_t n, bool full, uint64_t *v) {
  if (full) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p + i0);
#pragma unroll
    for (int k = 0; k < kWinItems / 2; ++k) {
      const uint4 x = q[k];
      v[2 * k] = (uint64_t)x.x | ((uint64_t)x.y << 32);
      v[2 * k + 1] = (uint64_t)x.z | ((uint64_t)x.w << 32);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) v[k] = (i0 + k < n) ? p[i0 + k] : 0;
  }
}

__device__ __forceinline__ void win_store8_u64(uint64_t *p, int64_t i0, int64_t n, bool full, const uint64_t *v) {
  if (full) {
    uint4 *q = reinterpret_cast<uint4 *>(p + i0);
#pragma unroll
    for (int k = 0; k < kWinItems / 2; ++k)
      q[k] = make_uint4((uint32_t)v[2 * k], (uint32_t)(v[2 * k] >> 32), (uint32_t)v[2 * k + 1],
                        (uint32_t)(v[2 * k + 1] >> 32));
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      if (i0 + k < n) p[i0 + k] = v[k];
  }
}

// bytes of positions at or past n read as 0
__device__ __forceinline__ void win_load8_u8(const uint8_t *p, int64_t i0, int64_t n, bool full, uint8_t *v) {
  if (full) {
    const uint2 x = *reinterpret_cast<const uint2 *>(p + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = (uint8_t)(x.x >> (8 * k));
      v[4 + k] = (uint8_t)(x.y >> (8 * k));
    }
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) v[k] = (i0 + k < n) ? p[i0 + k] : 0;
  }
}

__device__ __forceinline__ void win_store8_u8(uint8_t *p, int64_t i0, int64_t n, bool full, const uint8_t *v) {
  if (full) {
    uint2 x = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x.x |= (uint32_t)v[k] << (8 * k);
      x.y |= (uint32_t)v[4 + k] << (8 * k);
    }
    *reinterpret_cast<uint2 *>(p + i0) = x;
  } else {
#pragma unroll
    for (int k = 0; k < kWinItems; ++k)
      if (i0 + k < n) p[i0 + k] = v[k];
  }
}

__device__ __forceinline__ void win_store_bits(uint8_t *base, int64_t i, int w, uint64_t v) {
  switch (w) {
    case 1: base[i] = (uint8_t)v; break;
    case 2: reinterpret_cast<uint16_t *>(base)[i] = (uint16_t)v; break;
    case 4: reinterpret_cast<uint32_t *>(base)[i] = (uint32_t)v; break;
    default: reinterpret_cast<uint64_t *>(base)[i] = v; break;
  }
}

}  // namespace hip
}  // namespace cylon
