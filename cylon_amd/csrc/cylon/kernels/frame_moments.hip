// Framed VAR / STD (ROWS and RANGE frames) over the sorted positions of a permutation, gfx950.
// Semantics: docs/semantics.md "Framed aggregates", VAR / STD; the state, its merge, the layout and the
// query shared with the CPU twin (cpu_frame_moments.cpp) are in frame_moments_common.hpp.
//
// A variance from framed sums of x and x^2 cancels catastrophically, and a sliding update subtracts.
// Instead every result is a merge of (count, mean, M2) states of disjoint pieces of its own frame, each
// value used once and nothing subtracted, read off one moment pyramid per value column: the radix-8
// two-sided scan pyramid of frame_range.hip with a three-word state.
//   k_fm_level   one launch per pyramid level: a thread reads the 8 entries of one block (level 0: the
//                dense values and validity bytes; above: the E planes), writes the block's 8 P states
//                during a forward sweep and its 8 S states during a backward sweep, and the block's
//                total = one entry of the next level.  Only the 8 entries and one running state are
//                live; the states leave two (means, M2s) resp. four (counts) at a time as 16-byte stores.
//   k_fm_apply   one thread per sorted position i.  A RANGE spec reads the frame [lo, hi] from
//                frame_range_bounds' uint32 arrays; a ROWS spec computes max(i - preceding, phead[i])
//                and min(i + following, tail(i)) itself, saturating so that "unbounded" (>= n) cannot
//                overflow.  Then fm_query: S[lo] and P[hi] of every level on which lo and hi lie in
//                different blocks, then at most 8 entries merged serially -- 2 log8(w) + 8 state reads at
//                most for a frame of w rows.  out[perm[i]] = M2 / (m - ddof) or its square root, with
//                the validity byte (m >= min_periods and m - ddof > 0).
// No LDS, no workgroup waits for another one, wave64, grid-stride loops.
//
// Bounds: dense, dvalid, perm, phead, rtail, lo, hi are whole allocations of n elements (16-byte
// aligned where read with vector loads); a run of 8 positions inside [0, n_l) is read with vector loads,
// anything else element by element.  Pyramid indices: a level's P / S planes are written in whole
// blocks inside its fr_cap(n_l) slots (b < fr_up(n_l), so 8 b + 7 < fr_cap(n_l)) and read at
// lo, hi < n_l; E is written at b < n_(l+1) and read at j < n_(l+1).  A frame lies inside [phead, tail]
// of its partition, so 0 <= lo <= i <= hi < n.
#include "frame_moments_common.hpp"
#include "window_scan.hpp"

namespace cylon {
namespace hip {

// kFrRadix consecutive uint32 from j0 (a multiple of 8); positions at or past n read as 0
__device__ __forceinline__ void fm_load8_u32(const uint32_t *p, int64_t j0, int64_t n, bool full, uint32_t *v) {
  if (full) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p + j0);
    const uint4 a = q[0], b = q[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < kFrRadix; ++k) v[k] = (j0 + k < n) ? p[j0 + k] : 0u;
  }
}

__device__ __forceinline__ void fm_store2(double *p, int64_t j, double a, double b) {
  *reinterpret_cast<double2 *>(p + j) = make_double2(a, b);
}

// ---------------------------------------------------------------------------
// the pyramid
// ---------------------------------------------------------------------------
// One block of 8 entries per thread.  LEVEL0: the entries are the dense column; else in's [0 .. nl).
// P, S: this level's planes (offset to the level); next: the next level's entries.
template <bool LEVEL0>
__global__ __launch_bounds__(kBlock) void k_fm_level(FmPyramid src, FmPlanes in, int64_t nl, FmMutPlanes P,
                                                     FmMutPlanes S, FmMutPlanes next) {
  const int64_t nblocks = fr_up(nl);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += stride) {
    const int64_t j0 = b * kFrRadix;
    const bool full = j0 + kFrRadix <= nl;
    // the 8 entries: positions at or past nl are the identity (count 0)
    uint32_t en[kFrRadix];
    double em[kFrRadix], e2[kFrRadix];
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
      for (int k = 0; k < kFrRadix; ++k) {
        const FmState s = fm_entry0(bits[k], live[k] != 0 && (full || j0 + k < nl), src.w, src.kind);
        en[k] = s.n, em[k] = s.mean, e2[k] = s.m2;
      }
    } else {
      uint64_t m[kFrRadix], q[kFrRadix];
      win_load8_u64(reinterpret_cast<const uint64_t *>(in.mean), j0, nl, full, m);
      win_load8_u64(reinterpret_cast<const uint64_t *>(in.m2), j0, nl, full, q);
      fm_load8_u32(in.n, j0, nl, full, en);
#pragma unroll
      for (int k = 0; k < kFrRadix; ++k) em[k] = fr_bits_f64(m[k]), e2[k] = fr_bits_f64(q[k]);
    }
    // forward: P, and the block's total.  Whole blocks: the level's slots are fr_cap(nl).
    FmState acc = fm_identity();
    double pm = 0.0, p2 = 0.0;
    uint32_t pn[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kFrRadix; ++k) {
      acc = fm_merge(acc, FmState{en[k], em[k], e2[k]});
      if (k & 1) {
        fm_store2(P.mean, j0 + k - 1, pm, acc.mean);
        fm_store2(P.m2, j0 + k - 1, p2, acc.m2);
      } else {
        pm = acc.mean, p2 = acc.m2;
      }
      if ((k & 3) == 3) *reinterpret_cast<uint4 *>(P.n + j0 + k - 3) = make_uint4(pn[0], pn[1], pn[2], acc.n);
      else pn[k & 3] = acc.n;
    }
    fm_store(next, b, acc);
    // backward: S
    acc = fm_identity();
#pragma unroll
    for (int k = kFrRadix - 1; k >= 0; --k) {
      acc = fm_merge(FmState{en[k], em[k], e2[k]}, acc);
      if (k & 1) {
        pm = acc.mean, p2 = acc.m2;
      } else {
        fm_store2(S.mean, j0 + k, acc.mean, pm);
        fm_store2(S.m2, j0 + k, acc.m2, p2);
      }
      if ((k & 3) == 0) *reinterpret_cast<uint4 *>(S.n + j0 + k) = make_uint4(acc.n, pn[0], pn[1], pn[2]);
      else pn[(k & 3) - 1] = acc.n;
    }
  }
}

// ---------------------------------------------------------------------------
// the query
// ---------------------------------------------------------------------------
// lo32 / hi32 != nullptr: a RANGE spec; else a ROWS spec of (preceding, following) over phead / rtail
template <bool STD>
__global__ __launch_bounds__(kBlock) void k_fm_apply(const int64_t *__restrict__ perm, int64_t n, int64_t ddof,
                                                     int64_t minp, const uint32_t *__restrict__ lo32,
                                                     const uint32_t *__restrict__ hi32,
                                                     const int64_t *__restrict__ phead,
                                                     const int64_t *__restrict__ rtail, int64_t preceding,
                                                     int64_t following, FmPyramid pyr, double *__restrict__ out,
                                                     uint8_t *__restrict__ ovalid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t lo, hi;
    if (lo32 != nullptr) {
      lo = lo32[i];
      hi = hi32[i];
    } else {
      fm_rows_frame(i, n, phead[i], n - 1 - rtail[n - 1 - i], preceding, following, &lo, &hi);
    }
    const int64_t row = perm[i];
    const FmState s = fm_query(pyr, n, lo, hi);
    uint8_t ok;
    out[row] = fm_result(s, STD, ddof, minp, &ok);
    ovalid[row] = ok;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void fm_aligned(const void *p, const char *what) {
  CYLON_CHECK(p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0, Code::Invalid,
              "moment frame: " << what << " must be a 16-byte aligned buffer");
}

static void fm_check_rows(int64_t n) {
  CYLON_CHECK(n < (int64_t(1) << 32), Code::Invalid, "moment frame: " << n << " rows");  // counts and lo / hi are 32-bit
}

static void fm_check_value(const ColView &c) {
  const bool is_float = c.kind == static_cast<int>(ValueKind::FLOAT);
  CYLON_CHECK(c.kind <= static_cast<int>(ValueKind::FLOAT) &&
                  (c.width == 4 || c.width == 8 || (!is_float && (c.width == 1 || c.width == 2))),
              Code::Invalid, "moment frame: value column of width " << c.width << ", kind " << c.kind);
}

void frame_moments_pyramid(const ColView &col, int64_t n, const uint64_t *dense, const uint8_t *dense_valid,
                           uint64_t *P, uint64_t *S, uint64_t *E, void *stream) {
  if (n <= kFrRadix) return;  // one block: the query merges the column's own entries
  hipStream_t s = as_stream(stream);
  fm_check_rows(n);
  fm_check_value(col);
  fm_aligned(dense, "dense values");
  if (dense_valid != nullptr) fm_aligned(dense_valid, "dense validity");
  fm_aligned(P, "pyramid P");
  fm_aligned(S, "pyramid S");
  fm_aligned(E, "pyramid entries");
  const FmPyramid src{FmPlanes{}, FmPlanes{}, FmPlanes{}, dense, dense_valid, col.width, col.kind};
  const FmMutPlanes p = fm_planes(P, fm_ps_slots(n)), sp = fm_planes(S, fm_ps_slots(n)),
                    ep = fm_planes(E, fm_e_slots(n));
  auto at = [](const FmMutPlanes &x, int64_t o) { return FmMutPlanes{x.mean + o, x.m2 + o, x.n + o}; };
  int64_t nl = n, ps = 0, e = 0;  // this level's entries, its P / S offset, the next level's E offset
  FmPlanes in{};
  for (bool level0 = true; nl > kFrRadix; level0 = false) {
    const dim3 g(grid_for(fr_up(nl))), b(kBlock);
    const FmMutPlanes next = at(ep, e);
    if (level0) hipLaunchKernelGGL(k_fm_level<true>, g, b, 0, s, src, in, nl, at(p, ps), at(sp, ps), next);
    else hipLaunchKernelGGL(k_fm_level<false>, g, b, 0, s, src, in, nl, at(p, ps), at(sp, ps), next);
    HIP_LAUNCH_CHECK();
    ps += fr_cap(nl);
    nl = fr_up(nl);
    in = FmPlanes{next.mean, next.m2, next.n};
    e += fr_cap(nl);
  }
}

void frame_moments_apply(const ColView &col, const int64_t *perm, int64_t n, bool std_dev, int64_t ddof,
                         int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo,
                         const uint32_t *hi, const int64_t *phead, const int64_t *rtail, int64_t preceding,
                         int64_t following, const uint64_t *P, const uint64_t *S, const uint64_t *E, uint8_t *out,
                         uint8_t *out_valid, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  fm_check_rows(n);
  fm_check_value(col);
  CYLON_CHECK(ddof >= 0, Code::Invalid, "moment frame: ddof " << ddof);
  CYLON_CHECK(min_periods >= 1, Code::Invalid, "moment frame: min_periods " << min_periods);
  CYLON_CHECK(perm != nullptr && dense != nullptr, Code::Invalid, "moment frame: apply inputs");
  const bool range = lo != nullptr || hi != nullptr;
  CYLON_CHECK(range ? (lo != nullptr && hi != nullptr)
                    : (phead != nullptr && rtail != nullptr && preceding >= 0 && following >= 0),
              Code::Invalid, "moment frame: frame bounds");
  CYLON_CHECK(n <= kFrRadix || (P != nullptr && S != nullptr && E != nullptr), Code::Invalid,
              "moment frame: pyramid");
  CYLON_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % 8 == 0 && out_valid != nullptr, Code::Invalid,
              "moment frame: output");
  const FmPyramid pyr{fm_planes(P, fm_ps_slots(n)), fm_planes(S, fm_ps_slots(n)), fm_planes(E, fm_e_slots(n)),
                      dense,                        dense_valid,                  col.width,
                      col.kind};
  const dim3 g(grid_for(n)), b(kBlock);
  double *o = reinterpret_cast<double *>(out);
  if (std_dev)
    hipLaunchKernelGGL(k_fm_apply<true>, g, b, 0, s, perm, n, ddof, min_periods, lo, hi, phead, rtail, preceding,
                       following, pyr, o, out_valid);
  else
    hipLaunchKernelGGL(k_fm_apply<false>, g, b, 0, s, perm, n, ddof, min_periods, lo, hi, phead, rtail, preceding,
                       following, pyr, o, out_valid);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_frame_moments() { preload_code(reinterpret_cast<const void *>(&k_fm_level<true>)); }

}  // namespace hip
}  // namespace cylon
