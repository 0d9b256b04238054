// The interval join's rules shared by kernels/interval.hip and its CPU twin cpu_interval.cpp
// (docs/semantics.md "Interval join"), so the two agree bit for bit.
#pragma once
#include <cstdint>

#include "order_image.hpp"

namespace cylon {

// Where the three blocks of key rows lie in the concatenation that was sorted: the right rows
// (value = on) at [rbase, rbase + nr), the left rows' L-copies (value = lower) at [lbase, lbase + nl)
// and their U-copies (value = upper) at [ubase, ubase + nl).  The three ranges tile [0, nr + 2 nl).
struct IntervalLayout {
  int64_t nl, nr;
  int64_t lbase, rbase, ubase;
};

// three ranges inside [0, n) whose lengths add up to n tile it exactly when no two of them overlap
inline bool interval_layout_ok(const IntervalLayout &y) {
  if (y.nl < 0 || y.nr < 0) return false;
  const int64_t n = y.nr + 2 * y.nl;
  const int64_t b[3] = {y.lbase, y.rbase, y.ubase}, len[3] = {y.nl, y.nr, y.nl};
  for (int k = 0; k < 3; ++k)
    if (b[k] < 0 || b[k] + len[k] > n) return false;
  for (int j = 0; j < 3; ++j)
    for (int k = j + 1; k < 3; ++k)
      if (len[j] > 0 && len[k] > 0 && b[j] < b[k] + len[k] && b[k] < b[j] + len[j]) return false;
  return true;
}

// a bound or an `on` value takes part in comparisons: neither null nor NaN
CYLON_HD bool interval_usable(bool valid, uint64_t bits, int w, int kind) {
  return valid && !(kind == static_cast<int>(ValueKind::FLOAT) && is_nan_bits(bits, w));
}

// matches of one left row: lo / hi = right rows sorted before its L-copy / its U-copy
CYLON_HD int64_t interval_count(bool usable, int64_t lo, int64_t hi) { return (usable && hi > lo) ? hi - lo : 0; }

}  // namespace cylon
