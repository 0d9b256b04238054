// CPU twin of kernels/rolling.hip, and the definition of the framed aggregates (docs/semantics.md
// "Framed aggregates"): the same two block scans and the same case split, as sequential loops, so the
// cost is O(n) whatever the frame.  Nothing is tiled: rolling_tile does nothing, rolling_scan walks
// all positions, and rolling_lds is the two scans and the combine step over buffers of its own.
#include <cstring>
#include <vector>

#include "kernels.hpp"
#include "order_image.hpp"
#include "rolling_check.hpp"

namespace cylon {
namespace cpu {

namespace {

enum : int { WF_SUM_I = 0, WF_SUM_F = 1, WF_MIN = 2, WF_MAX = 3, WF_COUNT = 4 };

inline double bits_f64(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

inline uint64_t f64_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

inline uint64_t identity(int func) { return func == WF_MIN ? ~0ull : 0ull; }

inline uint64_t op(int func, uint64_t x, uint64_t y) {
  switch (func) {
    case WF_SUM_F: return f64_bits(bits_f64(x) + bits_f64(y));
    case WF_MIN: return x < y ? x : y;
    case WF_MAX: return x > y ? x : y;
    default: return x + y;
  }
}

// raw column bits -> accumulator
inline uint64_t widen(int func, uint64_t b, int w, int kind) {
  switch (func) {
    case WF_COUNT: return 1;
    case WF_SUM_I:
      if (kind != static_cast<int>(ValueKind::SIGNED_INT)) return b;
      return w == 1 ? (uint64_t)(int64_t)(int8_t)b : w == 2 ? (uint64_t)(int64_t)(int16_t)b
             : w == 4 ? (uint64_t)(int64_t)(int32_t)b : b;
    case WF_SUM_F: {
      if (w == 8) return b;
      const uint32_t u = (uint32_t)b;
      float f;
      std::memcpy(&f, &u, 4);
      return f64_bits((double)f);
    }
    default: return order_image(b, w, kind);
  }
}

// scan[k], scan_cnt[k] over the scan order; reverse: position k is sorted position n - 1 - k
void scan_all(const ColView &c, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
              const uint64_t *dense, const uint8_t *dense_valid, uint64_t *scan, uint32_t *scan_cnt) {
  uint64_t acc = identity(func);
  uint32_t cnt = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t g = reverse ? n - 1 - k : k;
    const bool edge = reverse ? (g + 1) % w == 0 : g % w == 0;
    if (edge || (restarts[k] & 1)) {
      acc = identity(func);
      cnt = 0;
    }
    if (dense_valid == nullptr || dense_valid[g] != 0) {
      acc = op(func, acc, widen(func, dense[g], c.width, c.kind));
      ++cnt;
    }
    scan[k] = acc;
    scan_cnt[k] = cnt;
  }
}

void combine_all(const ColView &c, const int64_t *perm, const int64_t *phead, const int64_t *rtail, int64_t n,
                 int func, bool mean, int64_t p, int64_t f, int64_t minp, const uint64_t *P, const uint32_t *Pc,
                 const uint64_t *S, const uint32_t *Sc, uint8_t *out, uint8_t *ovalid) {
  const int64_t w = p + f + 1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t hd = phead[i], tl = n - 1 - rtail[n - 1 - i];
    const int64_t lo = i - p > hd ? i - p : hd;
    const int64_t hi = i + f < tl ? i + f : tl;
    const int64_t b = i - i % w;  // the block start at or before i
    uint64_t a;
    uint32_t m;
    if (b > lo || b + w <= hi) {  // a block starts inside (lo, hi]
      a = op(func, S[n - 1 - lo], P[hi]);
      m = Sc[n - 1 - lo] + Pc[hi];
    } else if (lo == b || lo == hd) {
      a = P[hi];
      m = Pc[hi];
    } else {  // hi is the partition's tail
      a = S[n - 1 - lo];
      m = Sc[n - 1 - lo];
    }
    const int64_t r = perm[i];
    if (func == WF_MIN || func == WF_MAX) {
      const uint64_t v = order_unimage(a, c.width, c.kind);  // a null row's bytes are unspecified
      std::memcpy(out + r * c.width, &v, (size_t)c.width);
    } else if (mean) {
      const double s = func == WF_SUM_F ? bits_f64(a)
                       : c.kind == static_cast<int>(ValueKind::SIGNED_INT) ? (double)(int64_t)a : (double)a;
      const double q = s / (double)m;
      std::memcpy(out + r * 8, &q, 8);
    } else {
      std::memcpy(out + r * 8, &a, 8);
    }
    if (ovalid != nullptr) ovalid[r] = (int64_t)m >= minp ? 1 : 0;
  }
}

}  // namespace

int64_t window_frame_lds_rows() { return kRollLdsRows; }

void window_rev_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *) {
  for (int64_t k = 0; k < n; ++k) rflags[k] = (k == 0 || (flags[n - k] & 1)) ? 3 : 0;
}

void rolling_tile(const ColView &col, const uint8_t *, int64_t n, int func, int64_t w, bool, const uint64_t *,
                  const uint8_t *, int64_t *, int64_t *, uint8_t *, void *) {
  rolling_check(col, func, n, 0, 0, 0, false);
  CYLON_CHECK(w >= 1, Code::Invalid, "rolling: frame of " << w << " rows");
}

void rolling_scan(const ColView &col, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *, const int64_t *, uint64_t *scan,
                  uint32_t *scan_cnt, void *) {
  const ColView c = rolling_check(col, func, n, 0, 0, 0, false);
  CYLON_CHECK(w >= 1, Code::Invalid, "rolling: frame of " << w << " rows");
  scan_all(c, restarts, n, func, w, reverse, dense, dense_valid, scan, scan_cnt);
}

void rolling_combine(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail, int64_t n,
                     int func, bool mean, int64_t preceding, int64_t following, int64_t min_periods,
                     const uint64_t *fwd, const uint32_t *fwd_cnt, const uint64_t *bwd, const uint32_t *bwd_cnt,
                     uint8_t *out, uint8_t *out_valid, void *) {
  const ColView c = rolling_check(col, func, n, preceding, following, min_periods, mean);
  combine_all(c, perm, phead, rtail, n, func, mean, preceding, following, min_periods, fwd, fwd_cnt, bwd, bwd_cnt, out,
              out_valid);
}

void rolling_lds(const ColView &col, const int64_t *perm, const uint8_t *flags, const int64_t *phead,
                 const int64_t *rtail, int64_t n, int func, bool mean, int64_t preceding, int64_t following,
                 int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, uint8_t *out,
                 uint8_t *out_valid, void *) {
  if (n == 0) return;
  const ColView c = rolling_check(col, func, n, preceding, following, min_periods, mean);
  const int64_t w = preceding + following + 1;
  CYLON_CHECK(w <= kRollLdsRows, Code::Invalid, "rolling: a frame of " << w << " rows does not fit the LDS path");
  std::vector<uint8_t> rflags((size_t)n);
  window_rev_flags(flags, n, rflags.data(), nullptr);
  std::vector<uint64_t> P((size_t)n), S((size_t)n);
  std::vector<uint32_t> Pc((size_t)n), Sc((size_t)n);
  scan_all(c, flags, n, func, w, false, dense, dense_valid, P.data(), Pc.data());
  scan_all(c, rflags.data(), n, func, w, true, dense, dense_valid, S.data(), Sc.data());
  combine_all(c, perm, phead, rtail, n, func, mean, preceding, following, min_periods, P.data(), Pc.data(), S.data(),
              Sc.data(), out, out_valid);
}

}  // namespace cpu
}  // namespace cylon
