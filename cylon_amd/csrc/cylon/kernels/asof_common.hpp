// The as-of join's element code and its distance rules (docs/semantics.md "As-of join"): the one
// definition shared by kernels/asof.hip and its CPU twin cpu_asof.cpp, so the two agree bit for bit.
#pragma once
#include <cstdint>

#include "order_image.hpp"

namespace cylon {

// code byte of a position of the merged order: bit 0 = the row is a right row, bit 1 = its `on` value
// is neither null nor NaN.  3: a candidate, 2: a left row that may match, 0 / 1: neither.
constexpr uint8_t kAsofRight = 1, kAsofUsable = 2;

CYLON_HD uint8_t asof_code(bool right, bool valid, uint64_t bits, int w, int kind) {
  const bool nan = kind == static_cast<int>(ValueKind::FLOAT) && is_nan_bits(bits, w);
  return (uint8_t)((right ? kAsofRight : 0) | ((valid && !nan) ? kAsofUsable : 0));
}

CYLON_HD double asof_f64(uint64_t bits, int w) {
  if (w == 8) {
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
  }
  const uint32_t u = (uint32_t)bits;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return (double)f;  // exact
}

// |x - y| of two integer / temporal values: the difference of the order images, exact in uint64
CYLON_HD uint64_t asof_distance_int(uint64_t x, uint64_t y, int w, int kind) {
  const uint64_t a = order_image(x, w, kind), b = order_image(y, w, kind);
  return a > b ? a - b : b - a;
}

// |x - y| of two floats that are not NaN: 0 for equal values (-0.0 and +0.0, two equal infinities),
// else one float64 subtraction
CYLON_HD double asof_distance_float(uint64_t x, uint64_t y, int w) {
  const double a = asof_f64(x, w), b = asof_f64(y, w);
  if (a == b) return 0.0;
  return a > b ? a - b : b - a;
}

struct AsofPick {
  int32_t width, kind;
  int32_t has_tol;
  int64_t tol_i;  // integer / temporal `on`
  double tol_f;   // float `on`
};

// The final right row of one left row with `on` bits x: back / fwd = the backward and the forward
// candidate (-1: none; fwd is -1 for a one-directional join), yb / yf their `on` bits.  The nearer
// one is kept, the backward one on equal distances, and dropped when farther than the tolerance.
CYLON_HD int64_t asof_pick_one(const AsofPick &p, uint64_t x, int64_t back, uint64_t yb, int64_t fwd, uint64_t yf) {
  if (back < 0 && fwd < 0) return -1;
  if (p.kind == static_cast<int>(ValueKind::FLOAT)) {
    const double db = back >= 0 ? asof_distance_float(x, yb, p.width) : 0.0;
    const double df = fwd >= 0 ? asof_distance_float(x, yf, p.width) : 0.0;
    const bool take_f = fwd >= 0 && (back < 0 || df < db);
    const double d = take_f ? df : db;
    if (p.has_tol && !(d <= p.tol_f)) return -1;
    return take_f ? fwd : back;
  }
  const uint64_t db = back >= 0 ? asof_distance_int(x, yb, p.width, p.kind) : 0;
  const uint64_t df = fwd >= 0 ? asof_distance_int(x, yf, p.width, p.kind) : 0;
  const bool take_f = fwd >= 0 && (back < 0 || df < db);
  const uint64_t d = take_f ? df : db;
  if (p.has_tol && d > (uint64_t)p.tol_i) return -1;
  return take_f ? fwd : back;
}

}  // namespace cylon
