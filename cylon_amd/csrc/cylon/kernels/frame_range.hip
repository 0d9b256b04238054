// RANGE frames (value-based rolling COUNT / SUM / MEAN / MIN / MAX) over the sorted positions of a
// permutation, gfx950.  Semantics: docs/semantics.md "Framed aggregates", RANGE; the rules shared with
// the CPU twin (cpu_frame_range.cpp) are in frame_range_common.hpp.
//
// The frame of sorted position i is the contiguous range [lo(i), hi(i)] of its partition whose order
// keys lie within `preceding` below and `following` above i's.  Its length differs from row to row, so
// the fixed-width block scans of rolling.hip do not apply.  Instead:
//   k_fr_keys     one pass over the order column's dense values (window_tile's gather): the 64-bit
//                 search key and the class byte (number / NaN / null) of every position.
//   k_fr_bounds   once per distinct (preceding, following) of a call.  A tile of kWinTile positions
//                 stages the keys and classes of [tile_lo - kFrHalo, tile_hi + kFrHalo] in LDS; every
//                 thread finds lo and hi of its kWinItems positions by binary search there, restricted
//                 to [head, tail] of the partition.  Only when the staged window's first (last) key
//                 still lies inside the frame and is not the partition's head (tail) does the search
//                 run in global memory instead, over [head, window start] ([window end, tail]):
//                 neighbouring rows then probe the same few lines.  lo / hi are stored as uint32.
//   k_fr_level    one launch per pyramid level: a thread reads the 8 entries of one block, writes the
//                 block's 8 P (scan from the block's start) and 8 S (scan to the block's end) and the
//                 block's total = one entry of the next level.  No scan primitive, no restart: a frame
//                 never crosses a partition, so no query reads across one either.
//   k_fr_apply    one thread per position: S[lo] and P[hi] of every level on which lo and hi lie in
//                 different blocks, then at most 8 entries combined serially, so a frame of length w
//                 costs 2 log8(w) + 8 reads at most, whatever the data.  The result goes to
//                 out[perm[i]] with the validity byte (m >= min_periods).
// Every float result is a combination of the values of its own frame, each exactly once (nothing is
// subtracted); MIN / MAX combine order images.  No workgroup waits for another one.
//
// Bounds: keys, cls, dense, phead, lo, hi are whole allocations of n elements (16-byte aligned); a run
// of 8 positions inside [0, n) is read with vector loads, anything else element by element.  LDS
// indices are g - base with base = tile_lo - kFrHalo <= wlo <= g <= whi < base + kFrWin.  Pyramid
// indices: a level's P / S are written in whole blocks inside its fr_cap(n_l) slots and read at
// lo, hi < n_l; E at block < n_(l+1).
#include "frame_range_common.hpp"
#include "window_scan.hpp"

namespace cylon {
namespace hip {

constexpr int kFrWin = kWinTile + 2 * kFrHalo;  // staged keys of a bounds tile
static_assert(kFrHalo % kWinItems == 0 && kFrWin % kWinItems == 0, "the staging loop moves 8 keys at a time");

// ---------------------------------------------------------------------------
// keys
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWinThreads) void k_fr_keys(ColView c, const uint64_t *__restrict__ dense,
                                                         const uint8_t *__restrict__ dvalid, int64_t n, int desc,
                                                         uint64_t *__restrict__ keys, uint8_t *__restrict__ cls) {
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const bool full = (t + 1) * kWinTile <= n;
    const int64_t i0 = t * kWinTile + (int64_t)threadIdx.x * kWinItems;
    uint64_t bits[kWinItems], key[kWinItems];
    uint8_t live[kWinItems], cl[kWinItems];
    win_load8_u64(dense, i0, n, full, bits);
    if (dvalid != nullptr) {
      win_load8_u8(dvalid, i0, n, full, live);
    } else {
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) live[k] = 1;
    }
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) fr_key(bits[k], live[k] != 0, c.width, c.kind, desc != 0, &key[k], &cl[k]);
    win_store8_u64(keys, i0, n, full, key);
    win_store8_u8(cls, i0, n, full, cl);
  }
}

// ---------------------------------------------------------------------------
// bounds
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWinThreads) void k_fr_bounds(const uint64_t *__restrict__ keys,
                                                           const uint8_t *__restrict__ cls,
                                                           const int64_t *__restrict__ phead,
                                                           const int64_t *__restrict__ rtail, int64_t n, FrFrame fr,
                                                           uint32_t *__restrict__ lo32, uint32_t *__restrict__ hi32) {
  __shared__ __align__(16) uint64_t sk[kFrWin];
  __shared__ __align__(16) uint8_t sc[kFrWin];
  const int64_t ntiles = (n + kWinTile - 1) / kWinTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t tile_lo = t * kWinTile;
    const int64_t base = tile_lo - kFrHalo;  // a multiple of kWinItems, may be negative
    for (int q0 = (int)threadIdx.x * kWinItems; q0 < kFrWin; q0 += kWinThreads * kWinItems) {
      const int64_t g0 = base + q0;
      uint64_t k8[kWinItems];
      uint8_t c8[kWinItems];
      if (g0 >= 0 && g0 + kWinItems <= n) {
        win_load8_u64(keys, g0, n, true, k8);
        win_load8_u8(cls, g0, n, true, c8);
      } else {
#pragma unroll
        for (int k = 0; k < kWinItems; ++k) {
          const int64_t g = g0 + k;
          const bool in = g >= 0 && g < n;
          k8[k] = in ? keys[g] : 0;
          c8[k] = in ? cls[g] : 0;
        }
      }
#pragma unroll
      for (int k = 0; k < kWinItems; ++k) {
        sk[q0 + k] = k8[k];
        sc[q0 + k] = c8[k];
      }
    }
    __syncthreads();
    const int64_t wlo = base > 0 ? base : 0;                                  // staged positions [wlo, whi]
    const int64_t whi = (base + kFrWin < n ? base + kFrWin : n) - 1;
    // neighbouring lanes take neighbouring positions: their searches probe the same few keys, and
    // the 4-byte results leave as whole lines
#pragma unroll 1
    for (int k = 0; k < kWinItems; ++k) {
      const int64_t i = tile_lo + (int64_t)k * kWinThreads + threadIdx.x;
      if (i >= n) break;
      const int64_t hd = phead[i], tl = n - 1 - rtail[n - 1 - i];
      const uint8_t ci = sc[i - base];
      const uint64_t ki = sk[i - base];
      int64_t lo = hd, hi = tl;
      if (fr.pre_mode != FR_UNBOUNDED) {
        const uint64_t want = ci == FR_NUMBER ? fr_bound(ki, false, fr) : 0;
        int64_t a = hd > wlo ? hd : wlo, b = i;  // the first position >= (ci, want); position i is one
        if (a > hd && fr_ge(sc[a - base], sk[a - base], ci, want)) {
          b = a;
          a = hd;
          while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (fr_ge(cls[mid], keys[mid], ci, want)) b = mid;
            else a = mid + 1;
          }
        } else {
          while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (fr_ge(sc[mid - base], sk[mid - base], ci, want)) b = mid;
            else a = mid + 1;
          }
        }
        lo = a;
      }
      if (fr.fol_mode != FR_UNBOUNDED) {
        const uint64_t want = ci == FR_NUMBER ? fr_bound(ki, true, fr) : 0;
        int64_t a = i, b = tl < whi ? tl : whi;  // the last position <= (ci, want); position i is one
        if (b < tl && fr_ge(ci, want, sc[b - base], sk[b - base])) {
          a = b;
          b = tl;
          while (a < b) {
            const int64_t mid = (a + b + 1) >> 1;
            if (fr_ge(ci, want, cls[mid], keys[mid])) a = mid;
            else b = mid - 1;
          }
        } else {
          while (a < b) {
            const int64_t mid = (a + b + 1) >> 1;
            if (fr_ge(ci, want, sc[mid - base], sk[mid - base])) a = mid;
            else b = mid - 1;
          }
        }
        hi = a;
      }
      lo32[i] = (uint32_t)lo;
      hi32[i] = (uint32_t)hi;
    }
    __syncthreads();  // before the next tile overwrites the staged keys
  }
}

// ---------------------------------------------------------------------------
// the pyramid
// ---------------------------------------------------------------------------
// One block of 8 entries per thread.  LEVEL0: the entries are the dense column; else in[0 .. nl).
// P, S: this level's slots (nullptr when the level has one block); next: the next level's entries.
template <int F, bool LEVEL0>
__global__ __launch_bounds__(kBlock) void k_fr_level(FrPyramid src, const uint64_t *__restrict__ in, int64_t nl,
                                                     uint64_t *__restrict__ P, uint64_t *__restrict__ S,
                                                     uint64_t *__restrict__ next) {
  const int64_t nblocks = fr_up(nl);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += stride) {
    const int64_t j0 = b * kFrRadix;
    const bool full = j0 + kFrRadix <= nl;
    uint64_t e[kFrRadix], p[kFrRadix], s[kFrRadix];
    if (LEVEL0) {
      uint64_t bits[kFrRadix];
      uint8_t live[kFrRadix];
      win_load8_u64(src.dense, j0, nl, full, bits);
      if (src.dvalid != nullptr) {
        win_load8_u8(src.dvalid, j0, nl, full, live);
      } else {
#pragma unroll
        for (int k = 0; k < kFrRadix; ++k) live[k] = 1;
      }
#pragma unroll
      for (int k = 0; k < kFrRadix; ++k) e[k] = fr_entry0(F, bits[k], live[k] != 0, src.w, src.kind);
    } else {
      win_load8_u64(in, j0, nl, full, e);
    }
    const int cnt = full ? kFrRadix : (int)(nl - j0);
    uint64_t acc = fr_identity(F);
#pragma unroll
    for (int k = 0; k < kFrRadix; ++k) {
      if (k < cnt) acc = fr_op(F, acc, e[k]);
      p[k] = acc;
    }
    next[b] = acc;
    acc = fr_identity(F);
#pragma unroll
    for (int k = kFrRadix - 1; k >= 0; --k) {
      if (k < cnt) acc = fr_op(F, e[k], acc);
      s[k] = acc;
    }
    // whole blocks: the level's slots are fr_cap(nl)
    win_store8_u64(P, j0, nl, true, p);
    win_store8_u64(S, j0, nl, true, s);
  }
}

// ---------------------------------------------------------------------------
// the query
// ---------------------------------------------------------------------------
template <int F>
__global__ __launch_bounds__(kBlock) void k_fr_apply(ColView c, const int64_t *__restrict__ perm, int64_t n,
                                                     int64_t minp, int mean, const uint32_t *__restrict__ lo32,
                                                     const uint32_t *__restrict__ hi32, FrPyramid pyr, FrPyramid cnt,
                                                     uint8_t *__restrict__ out, uint8_t *__restrict__ ovalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t lo = lo32[i], hi = hi32[i], row = perm[i];
    const uint64_t m = cnt.dvalid == nullptr ? (uint64_t)(hi - lo + 1) : fr_query(FR_COUNT, cnt, n, lo, hi);
    const uint64_t a = F == WF_COUNT ? m : fr_query(F, pyr, n, lo, hi);
    if (F == WF_MIN || F == WF_MAX) {
      win_store_bits(out, row, c.width, order_unimage(a, c.width, c.kind));
    } else if (mean) {
      double s;
      if (F == WF_SUM_F) s = fr_bits_f64(a);
      else s = c.kind == static_cast<int>(ValueKind::SIGNED_INT) ? (double)(int64_t)a : (double)a;
      reinterpret_cast<double *>(out)[row] = s / (double)m;
    } else {
      reinterpret_cast<uint64_t *>(out)[row] = a;
    }
    if (ovalid != nullptr) ovalid[row] = (int64_t)m >= minp ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t window_range_radix() { return kFrRadix; }
int64_t window_range_halo() { return kFrHalo; }

static void fr_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "range frame: " << what << " must be a 16-byte aligned buffer");
}

static void fr_check_rows(int64_t n) {
  CYLON_CHECK(n < (int64_t(1) << 32), Code::Invalid, "range frame: " << n << " rows");  // lo / hi are 32-bit
}

// the view the kernels use; as rolling_check's
static ColView fr_check_value(const ColView &col, int func, bool mean) {
  CYLON_CHECK(func >= WF_SUM_I && func <= WF_COUNT, Code::Invalid, "range frame: value function " << func);
  CYLON_CHECK(!mean || func == WF_SUM_I || func == WF_SUM_F, Code::Invalid, "range frame: mean of function " << func);
  ColView c = col;
  const bool plain = c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
  if (func == WF_COUNT) {
    if (!plain) c.width = 0;
    return c;
  }
  CYLON_CHECK(plain && c.kind <= static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "range frame: value column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_F || (c.kind == static_cast<int>(ValueKind::FLOAT) && c.width >= 4), Code::Invalid,
              "range frame: float sum of a column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_I || c.kind != static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "range frame: integer sum of a float column");
  return c;
}

void frame_range_keys(const ColView &order_col, const uint64_t *dense, const uint8_t *dense_valid, int64_t n,
                      bool descending, uint64_t *keys, uint8_t *cls, void *stream) {
  if (n == 0) return;
  const bool is_float = order_col.kind == static_cast<int>(ValueKind::FLOAT);
  const int w = order_col.width;
  CYLON_CHECK(order_col.kind <= static_cast<int>(ValueKind::FLOAT) &&
                  (w == 4 || w == 8 || (!is_float && (w == 1 || w == 2))),
              Code::Invalid, "range frame: order column of width " << w << ", kind " << order_col.kind);
  fr_aligned(dense, "dense order values");
  if (dense_valid != nullptr) fr_aligned(dense_valid, "dense order validity");
  fr_aligned(keys, "keys");
  fr_aligned(cls, "key classes");
  hipLaunchKernelGGL(k_fr_keys, dim3(grid_for((n + kWinTile - 1) / kWinTile, 1)), dim3(kWinThreads), 0,
                     as_stream(stream), order_col, dense, dense_valid, n, descending ? 1 : 0, keys, cls);
  HIP_LAUNCH_CHECK();
}

void frame_range_bounds(const uint64_t *keys, const uint8_t *cls, const int64_t *phead, const int64_t *rtail,
                        int64_t n, bool float_keys, bool descending, int pre_mode, uint64_t pre_i, double pre_f,
                        int fol_mode, uint64_t fol_i, double fol_f, uint32_t *lo, uint32_t *hi, void *stream) {
  if (n == 0) return;
  fr_check_rows(n);
  const int bounded = float_keys ? FR_FLOAT : FR_INT;
  CYLON_CHECK((pre_mode == FR_UNBOUNDED || pre_mode == bounded) && (fol_mode == FR_UNBOUNDED || fol_mode == bounded),
              Code::Invalid, "range frame: offsets of modes " << pre_mode << ", " << fol_mode);
  CYLON_CHECK(!float_keys || (pre_f >= 0 && fol_f >= 0), Code::Invalid, "range frame: negative or NaN offset");
  fr_aligned(keys, "keys");
  fr_aligned(cls, "key classes");
  fr_aligned(phead, "partition heads");
  CYLON_CHECK(rtail != nullptr && lo != nullptr && hi != nullptr, Code::Invalid, "range frame: bounds buffers");
  const FrFrame fr{pre_mode, fol_mode, pre_i, fol_i, pre_f, fol_f, float_keys ? 1 : 0, descending ? 1 : 0};
  hipLaunchKernelGGL(k_fr_bounds, dim3(grid_for((n + kWinTile - 1) / kWinTile, 1)), dim3(kWinThreads), 0,
                     as_stream(stream), keys, cls, phead, rtail, n, fr, lo, hi);
  HIP_LAUNCH_CHECK();
}

#define FR_DISPATCH(func, LAUNCH)           \
  do {                                      \
    switch (func) {                         \
      case WF_SUM_I: LAUNCH(WF_SUM_I); break; \
      case WF_SUM_F: LAUNCH(WF_SUM_F); break; \
      case WF_MIN: LAUNCH(WF_MIN); break;   \
      case WF_MAX: LAUNCH(WF_MAX); break;   \
      default: LAUNCH(WF_COUNT); break;     \
    }                                       \
    HIP_LAUNCH_CHECK();                     \
  } while (0)

void frame_range_pyramid(const ColView &col, int64_t n, int func, const uint64_t *dense, const uint8_t *dense_valid,
                         uint64_t *P, uint64_t *S, uint64_t *E, void *stream) {
  if (n <= kFrRadix) return;  // one block: the query combines the column's own entries
  hipStream_t s = as_stream(stream);
  fr_check_rows(n);
  const ColView c = fr_check_value(col, func, false);
  fr_aligned(dense, "dense values");
  if (dense_valid != nullptr) fr_aligned(dense_valid, "dense validity");
  fr_aligned(P, "pyramid P");
  fr_aligned(S, "pyramid S");
  fr_aligned(E, "pyramid entries");
  const FrPyramid src{nullptr, nullptr, nullptr, dense, dense_valid, c.width, c.kind};
  int64_t nl = n, ps = 0, e = 0;  // this level's entries, its P / S offset, the next level's E offset
  const uint64_t *in = nullptr;
  for (bool level0 = true; nl > kFrRadix; level0 = false) {
    const dim3 g(grid_for(fr_up(nl))), b(kBlock);
    uint64_t *next = E + e;
#define FR_LAUNCH(F)                                                                                  \
  if (level0) hipLaunchKernelGGL((k_fr_level<F, true>), g, b, 0, s, src, in, nl, P + ps, S + ps, next); \
  else hipLaunchKernelGGL((k_fr_level<F, false>), g, b, 0, s, src, in, nl, P + ps, S + ps, next)
    FR_DISPATCH(func, FR_LAUNCH);
#undef FR_LAUNCH
    ps += fr_cap(nl);
    nl = fr_up(nl);
    in = next;
    e += fr_cap(nl);
  }
}

void frame_range_apply(const ColView &col, const int64_t *perm, int64_t n, int func, bool mean, int64_t min_periods,
                       const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo, const uint32_t *hi,
                       const uint64_t *P, const uint64_t *S, const uint64_t *E, const uint64_t *cP,
                       const uint64_t *cS, const uint64_t *cE, uint8_t *out, uint8_t *out_valid, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  fr_check_rows(n);
  const ColView c = fr_check_value(col, func, mean);
  CYLON_CHECK(min_periods >= 0, Code::Invalid, "range frame: min_periods " << min_periods);
  CYLON_CHECK(perm != nullptr && lo != nullptr && hi != nullptr && dense != nullptr, Code::Invalid,
              "range frame: apply inputs");
  const bool levels = n > kFrRadix;
  CYLON_CHECK(!levels || func == WF_COUNT || (P != nullptr && S != nullptr && E != nullptr), Code::Invalid,
              "range frame: value pyramid");
  CYLON_CHECK(!levels || dense_valid == nullptr || (cP != nullptr && cS != nullptr && cE != nullptr), Code::Invalid,
              "range frame: count pyramid of a column with nulls");
  const int ow = (func == WF_MIN || func == WF_MAX) ? c.width : 8;
  CYLON_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % ow == 0, Code::Invalid, "range frame: output");
  const FrPyramid pyr{P, S, E, dense, dense_valid, c.width, c.kind};
  const FrPyramid cnt{cP, cS, cE, dense, dense_valid, c.width, c.kind};
  const dim3 g(grid_for(n)), b(kBlock);
#define FR_LAUNCH(F) \
  hipLaunchKernelGGL(k_fr_apply<F>, g, b, 0, s, c, perm, n, min_periods, mean ? 1 : 0, lo, hi, pyr, cnt, out, out_valid)
  FR_DISPATCH(func, FR_LAUNCH);
#undef FR_LAUNCH
}

void preload_frame_range() { preload_code(reinterpret_cast<const void *>(&k_fr_keys)); }

}  // namespace hip
}  // namespace cylon
