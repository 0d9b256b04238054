// Order images of fixed-width values: the one definition shared by the sort (sort.hip k_sort_keys
// and its CPU twin), the top-k select (topk.hip, cpu_topk.cpp), the window / rolling MIN and MAX and
// the group-by's and scalar MIN / MAX (groupby.hip, radix_groupby.hip, cpu_groupby.cpp).  Unsigned
// order of the images = the requested order of the values, so all of them agree by construction.
// Equal images = equal values under the engine's value equality (-0.0 == +0.0, every NaN one value).
#pragma once
#include <cstdint>

#include "../types.hpp"

#if defined(__HIPCC__)
#define CYLON_HD __host__ __device__ __forceinline__
#else
#define CYLON_HD inline
#endif

namespace cylon {

CYLON_HD uint64_t order_image(uint64_t bits, int w, int kind) {
  const int nb = 8 * w;
  const uint64_t mask = (nb == 64) ? ~0ull : ((1ull << nb) - 1);
  const uint64_t sign = 1ull << (nb - 1);
  bits &= mask;
  if (kind == static_cast<int>(ValueKind::SIGNED_INT)) return bits ^ sign;
  if (kind == static_cast<int>(ValueKind::FLOAT)) {
    // canonicalise -0.0 to +0.0 and every NaN to the positive quiet NaN (sorts last)
    if (bits == sign) bits = 0;
    const uint64_t exp_mask = (w == 8) ? 0x7ff0000000000000ull : (w == 4 ? 0x7f800000ull : 0x7c00ull);
    const uint64_t man_mask = (w == 8) ? 0x000fffffffffffffull : (w == 4 ? 0x007fffffull : 0x03ffull);
    if ((bits & exp_mask) == exp_mask && (bits & man_mask) != 0) bits = exp_mask | ((man_mask + 1) >> 1);
    return (bits & sign) ? (~bits & mask) : (bits | sign);
  }
  return bits;
}

// the value bits whose order_image is img (-0.0 comes back as +0.0, every NaN as the quiet NaN)
CYLON_HD uint64_t order_unimage(uint64_t img, int w, int kind) {
  const int nb = 8 * w;
  const uint64_t mask = (nb == 64) ? ~0ull : ((1ull << nb) - 1);
  const uint64_t sign = 1ull << (nb - 1);
  img &= mask;
  if (kind == static_cast<int>(ValueKind::SIGNED_INT)) return img ^ sign;
  if (kind == static_cast<int>(ValueKind::FLOAT)) return (img & sign) ? (img ^ sign) : (~img & mask);
  return img;
}

// the bits MIN / MAX give back for a float: -0.0 -> +0.0, every NaN -> the positive quiet NaN
CYLON_HD uint64_t canonical_float_bits(uint64_t bits, int w) {
  const int kind = static_cast<int>(ValueKind::FLOAT);
  return order_unimage(order_image(bits, w, kind), w, kind);
}

CYLON_HD bool is_nan_bits(uint64_t bits, int w) {
  if (w == 8) return (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (bits & 0x000fffffffffffffull);
  if (w == 4) return (bits & 0x7f800000ull) == 0x7f800000ull && (bits & 0x007fffffull);
  return (bits & 0x7c00ull) == 0x7c00ull && (bits & 0x03ffull);
}

// the sort key of a non-null value: order image, descending flip inside the value's bit width,
// NaN last in both directions
CYLON_HD uint64_t sort_key_image(uint64_t bits, int w, int kind, bool desc) {
  const int nb = 8 * w;
  const uint64_t mask = (nb == 64) ? ~0ull : ((1ull << nb) - 1);
  uint64_t k = order_image(bits, w, kind);
  if (desc) k = ~k & mask;
  if (kind == static_cast<int>(ValueKind::FLOAT) && is_nan_bits(bits, w)) k = mask;
  return k;
}

// bits [lo, hi) of v as a number (0 when the range is empty); 0 <= lo <= hi <= 64
CYLON_HD uint64_t bit_field(uint64_t v, int lo, int hi) {
  const int w = hi - lo;
  if (w <= 0) return 0;
  v >>= lo;  // lo < 64 here
  return w >= 64 ? v : (v & ((1ull << w) - 1));
}

}  // namespace cylon
