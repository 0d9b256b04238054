// CPU twin of kernels/frame_range.hip, and the sequential definition of the RANGE frames
// (docs/semantics.md "Framed aggregates", RANGE).  The keys, the bounds in key space, the pyramid's
// layout and the query are the shared rules of frame_range_common.hpp; what differs is the walk: the
// bounds of a partition come from two pointers that only move forwards, and the pyramid's levels are
// built by one loop each.
#include <cstring>
#include <vector>

#include "frame_range_common.hpp"
#include "kernels.hpp"

namespace cylon {
namespace cpu {

namespace {

void check_rows(int64_t n) {
  CYLON_CHECK(n < (int64_t(1) << 32), Code::Invalid, "range frame: " << n << " rows");  // lo / hi are 32-bit
}

// the view the loops use; as rolling_check's
ColView check_value(const ColView &col, int func, bool mean) {
  CYLON_CHECK(func >= FR_SUM_I && func <= FR_COUNT, Code::Invalid, "range frame: value function " << func);
  CYLON_CHECK(!mean || func == FR_SUM_I || func == FR_SUM_F, Code::Invalid, "range frame: mean of function " << func);
  ColView c = col;
  const bool plain = c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
  if (func == FR_COUNT) {
    if (!plain) c.width = 0;
    return c;
  }
  CYLON_CHECK(plain && c.kind <= static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "range frame: value column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != FR_SUM_F || (c.kind == static_cast<int>(ValueKind::FLOAT) && c.width >= 4), Code::Invalid,
              "range frame: float sum of a column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != FR_SUM_I || c.kind != static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "range frame: integer sum of a float column");
  return c;
}

}  // namespace

int64_t window_range_radix() { return kFrRadix; }
int64_t window_range_halo() { return kFrHalo; }

void frame_range_keys(const ColView &order_col, const uint64_t *dense, const uint8_t *dense_valid, int64_t n,
                      bool descending, uint64_t *keys, uint8_t *cls, void *) {
  if (n == 0) return;
  const bool is_float = order_col.kind == static_cast<int>(ValueKind::FLOAT);
  const int w = order_col.width;
  CYLON_CHECK(order_col.kind <= static_cast<int>(ValueKind::FLOAT) &&
                  (w == 4 || w == 8 || (!is_float && (w == 1 || w == 2))),
              Code::Invalid, "range frame: order column of width " << w << ", kind " << order_col.kind);
  for (int64_t i = 0; i < n; ++i)
    fr_key(dense[i], dense_valid == nullptr || dense_valid[i] != 0, w, order_col.kind, descending, &keys[i], &cls[i]);
}

void frame_range_bounds(const uint64_t *keys, const uint8_t *cls, const int64_t *phead, const int64_t *rtail,
                        int64_t n, bool float_keys, bool descending, int pre_mode, uint64_t pre_i, double pre_f,
                        int fol_mode, uint64_t fol_i, double fol_f, uint32_t *lo, uint32_t *hi, void *) {
  if (n == 0) return;
  check_rows(n);
  const int bounded = float_keys ? FR_FLOAT : FR_INT;
  CYLON_CHECK((pre_mode == FR_UNBOUNDED || pre_mode == bounded) && (fol_mode == FR_UNBOUNDED || fol_mode == bounded),
              Code::Invalid, "range frame: offsets of modes " << pre_mode << ", " << fol_mode);
  CYLON_CHECK(!float_keys || (pre_f >= 0 && fol_f >= 0), Code::Invalid, "range frame: negative or NaN offset");
  const FrFrame fr{pre_mode, fol_mode, pre_i, fol_i, pre_f, fol_f, float_keys ? 1 : 0, descending ? 1 : 0};
  // both bounds never decrease along a partition: two pointers
  int64_t l = 0, h = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t hd = phead[i], tl = n - 1 - rtail[n - 1 - i];
    if (i == hd) l = h = hd;
    const uint8_t c = cls[i];
    if (pre_mode == FR_UNBOUNDED) {
      lo[i] = (uint32_t)hd;
    } else {
      const uint64_t want = c == FR_NUMBER ? fr_bound(keys[i], false, fr) : 0;
      while (!fr_ge(cls[l], keys[l], c, want)) ++l;  // position i ends it
      lo[i] = (uint32_t)l;
    }
    if (fol_mode == FR_UNBOUNDED) {
      hi[i] = (uint32_t)tl;
    } else {
      const uint64_t want = c == FR_NUMBER ? fr_bound(keys[i], true, fr) : 0;
      if (h < i) h = i;
      while (h < tl && fr_ge(c, want, cls[h + 1], keys[h + 1])) ++h;
      hi[i] = (uint32_t)h;
    }
  }
}

void frame_range_pyramid(const ColView &col, int64_t n, int func, const uint64_t *dense, const uint8_t *dense_valid,
                         uint64_t *P, uint64_t *S, uint64_t *E, void *) {
  if (n <= kFrRadix) return;
  check_rows(n);
  const ColView c = check_value(col, func, false);
  const FrPyramid src{nullptr, nullptr, nullptr, dense, dense_valid, c.width, c.kind};
  int64_t nl = n, ps = 0, e = 0;
  const uint64_t *in = nullptr;
  for (bool level0 = true; nl > kFrRadix; level0 = false) {
    uint64_t *next = E + e;
    for (int64_t b = 0; b < fr_up(nl); ++b) {
      const int64_t j0 = b * kFrRadix;
      const int cnt = j0 + kFrRadix <= nl ? kFrRadix : (int)(nl - j0);
      uint64_t ent[kFrRadix] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < cnt; ++k) ent[k] = level0 ? fr_level0(func, src, j0 + k) : in[j0 + k];
      next[b] = fr_block(func, ent, cnt, P + ps + j0, S + ps + j0);
    }
    ps += fr_cap(nl);
    nl = fr_up(nl);
    in = next;
    e += fr_cap(nl);
  }
}

void frame_range_apply(const ColView &col, const int64_t *perm, int64_t n, int func, bool mean, int64_t min_periods,
                       const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo, const uint32_t *hi,
                       const uint64_t *P, const uint64_t *S, const uint64_t *E, const uint64_t *cP,
                       const uint64_t *cS, const uint64_t *cE, uint8_t *out, uint8_t *out_valid, void *) {
  if (n == 0) return;
  check_rows(n);
  const ColView c = check_value(col, func, mean);
  CYLON_CHECK(min_periods >= 0, Code::Invalid, "range frame: min_periods " << min_periods);
  const bool levels = n > kFrRadix;
  CYLON_CHECK(!levels || func == FR_COUNT || (P != nullptr && S != nullptr && E != nullptr), Code::Invalid,
              "range frame: value pyramid");
  CYLON_CHECK(!levels || dense_valid == nullptr || (cP != nullptr && cS != nullptr && cE != nullptr), Code::Invalid,
              "range frame: count pyramid of a column with nulls");
  const FrPyramid pyr{P, S, E, dense, dense_valid, c.width, c.kind};
  const FrPyramid cnt{cP, cS, cE, dense, dense_valid, c.width, c.kind};
  for (int64_t i = 0; i < n; ++i) {
    const int64_t l = lo[i], h = hi[i], r = perm[i];
    const uint64_t m = dense_valid == nullptr ? (uint64_t)(h - l + 1) : fr_query(FR_COUNT, cnt, n, l, h);
    const uint64_t a = func == FR_COUNT ? m : fr_query(func, pyr, n, l, h);
    if (func == FR_MIN || func == FR_MAX) {
      const uint64_t v = order_unimage(a, c.width, c.kind);  // a null row's bytes are unspecified
      std::memcpy(out + r * c.width, &v, (size_t)c.width);
    } else if (mean) {
      const double s = func == FR_SUM_F ? fr_bits_f64(a)
                       : c.kind == static_cast<int>(ValueKind::SIGNED_INT) ? (double)(int64_t)a : (double)a;
      const double q = s / (double)m;
      std::memcpy(out + r * 8, &q, 8);
    } else {
      std::memcpy(out + r * 8, &a, 8);
    }
    if (out_valid != nullptr) out_valid[r] = (int64_t)m >= min_periods ? 1 : 0;
  }
}

}  // namespace cpu
}  // namespace cylon
