// What kernels/frame_moments.hip and its CPU twin (cpu_frame_moments.cpp) share, so that they agree by
// construction (docs/semantics.md "Framed aggregates", VAR / STD): the moment state of a run of
// values, its merge, the moment pyramid's layout and the query that reads the state of a frame off it.
//
// State.  (n, mean, M2) of the non-null values of a run of positions, every value converted to float64
// first: n their number, M2 = sum (x - mean)^2.  A live value x enters as (1, x, x - x): M2 is 0 for a
// finite x and NaN for a NaN or an infinity, and since every merge ADDS the M2 of both sides, a frame
// that holds a non-finite value has M2 = NaN whatever the order of the merges.  A null enters as the
// identity (0, 0, 0), and merging with the identity returns the other state bit for bit.
//
// Merge (Chan et al.) of two disjoint runs a, b:  d = mean_b - mean_a,  n = n_a + n_b,
//   mean = mean_a + d (n_b / n),   M2 = M2_a + M2_b + d d (n_a n_b / n).
// Nothing is subtracted from an M2: every term is >= +0, so M2 is never negative and never -0.0.
//
// The count is a uint32: a pyramid has fewer than 2^32 level-0 entries (the limit the RANGE frames'
// 32-bit bounds set anyway), so no count can exceed it, it converts to float64 exactly, and a state is
// 20 bytes rather than 24.
//
// Pyramid of n level-0 entries: the geometry of frame_range_common.hpp (radix kFrRadix, fr_cap, fr_up).
// P, S and E hold fr_ps_slots(n) resp. fr_e_slots(n) states each, as three planes (SoA) in one buffer of
// fm_words(slots) 64-bit words: the means, then the M2s, then the counts.  A level's slot count is a
// multiple of 8, so the 8 states of a block are 64 + 64 + 32 contiguous, 16-byte aligned bytes.
#pragma once
#include "frame_range_common.hpp"

namespace cylon {

struct FmState {
  uint32_t n;
  double mean, m2;
};

CYLON_HD FmState fm_identity() { return FmState{0u, 0.0, 0.0}; }

// a then b, in position order
CYLON_HD FmState fm_merge(const FmState &a, const FmState &b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  const double na = (double)a.n, nb = (double)b.n, n = na + nb;
  const double d = b.mean - a.mean;
  return FmState{a.n + b.n, a.mean + d * (nb / n), a.m2 + b.m2 + d * d * (na * nb / n)};
}

// raw column bits (the dense values window_tile gathers) -> float64, as the group-by VAR converts
CYLON_HD double fm_value(uint64_t bits, int w, int kind) {
  if (kind == static_cast<int>(ValueKind::FLOAT)) return fr_widen_float(bits, w);
  if (kind == static_cast<int>(ValueKind::SIGNED_INT)) return (double)fr_sign_extend(bits, w);
  return (double)(w == 8 ? bits : (bits & ((1ull << (8 * w)) - 1)));
}

CYLON_HD FmState fm_entry0(uint64_t bits, bool live, int w, int kind) {
  if (!live) return fm_identity();
  const double x = fm_value(bits, w, kind);
  return FmState{1u, x, x - x};
}

// ---------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------
// 64-bit words of `slots` states
CYLON_HD int64_t fm_words(int64_t slots) { return 2 * slots + (slots + 1) / 2; }
CYLON_HD int64_t fm_ps_slots(int64_t n) { return fr_ps_slots(n); }
CYLON_HD int64_t fm_e_slots(int64_t n) { return fr_e_slots(n); }

struct FmPlanes {
  const double *mean, *m2;
  const uint32_t *n;
};

struct FmMutPlanes {
  double *mean, *m2;
  uint32_t *n;
};

CYLON_HD FmPlanes fm_planes(const uint64_t *base, int64_t slots) {
  const double *d = reinterpret_cast<const double *>(base);
  return FmPlanes{d, d + slots, reinterpret_cast<const uint32_t *>(base + 2 * slots)};
}

CYLON_HD FmMutPlanes fm_planes(uint64_t *base, int64_t slots) {
  double *d = reinterpret_cast<double *>(base);
  return FmMutPlanes{d, d + slots, reinterpret_cast<uint32_t *>(base + 2 * slots)};
}

CYLON_HD FmState fm_load(const FmPlanes &p, int64_t j) { return FmState{p.n[j], p.mean[j], p.m2[j]}; }

CYLON_HD void fm_store(const FmMutPlanes &p, int64_t j, const FmState &s) {
  p.n[j] = s.n;
  p.mean[j] = s.mean;
  p.m2[j] = s.m2;
}

// ---------------------------------------------------------------------------
// the query
// ---------------------------------------------------------------------------
struct FmPyramid {
  FmPlanes P, S, E;
  // level 0: the dense column
  const uint64_t *dense;
  const uint8_t *dvalid;  // nullptr: no nulls
  int w, kind;
};

CYLON_HD FmState fm_level0(const FmPyramid &p, int64_t j) {
  return fm_entry0(p.dense[j], p.dvalid == nullptr || p.dvalid[j] != 0, p.w, p.kind);
}

// The state of level-0 entries lo .. hi (0 <= lo <= hi < n), each entry exactly once: fr_query's walk.
// The left pieces (S[lo] per level) are merged left to right and the right ones (P[hi]) right to left,
// so the order of the states is the order of the positions.
CYLON_HD FmState fm_query(const FmPyramid &p, int64_t n, int64_t lo, int64_t hi) {
  FmState left = fm_identity(), right = fm_identity(), mid = fm_identity();
  int64_t nl = n, ps = 0, e = 0;  // this level's entries, its offset in P / S, and (above level 0) in E
  bool level0 = true;
  for (;;) {
    if ((lo >> kFrShift) == (hi >> kFrShift)) {
      for (int64_t j = lo; j <= hi; ++j) mid = fm_merge(mid, level0 ? fm_level0(p, j) : fm_load(p.E, e + j));
      break;
    }
    left = fm_merge(left, fm_load(p.S, ps + lo));
    right = fm_merge(fm_load(p.P, ps + hi), right);
    lo = (lo >> kFrShift) + 1;
    hi = (hi >> kFrShift) - 1;
    if (lo > hi) break;
    ps += fr_cap(nl);
    if (!level0) e += fr_cap(nl);
    nl = fr_up(nl);
    level0 = false;
  }
  return fm_merge(fm_merge(left, mid), right);
}

// the ROWS frame of sorted position i inside [head, tail]; preceding, following >= 0, any size
CYLON_HD void fm_rows_frame(int64_t i, int64_t n, int64_t head, int64_t tail, int64_t preceding, int64_t following,
                            int64_t *lo, int64_t *hi) {
  const int64_t l = preceding > i ? 0 : i - preceding;             // never below 0
  const int64_t h = following >= n - 1 - i ? n - 1 : i + following;  // never above n - 1: no overflow
  *lo = l > head ? l : head;
  *hi = h < tail ? h : tail;
}

// VAR or STD of a frame's state; *valid = 0: null (the value is then 0)
CYLON_HD double fm_result(const FmState &s, bool std_dev, int64_t ddof, int64_t min_periods, uint8_t *valid) {
  const int64_t m = (int64_t)s.n;
  const bool ok = m >= min_periods && m - ddof > 0;
  *valid = ok ? 1 : 0;
  if (!ok) return 0.0;
  const double v = s.m2 / (double)(m - ddof);
  return std_dev ? __builtin_sqrt(v) : v;
}

}  // namespace cylon
