// What kernels/rolling.hip and its CPU twin (cpu_rolling.cpp) must agree on: the cap of the one-launch
// path and the argument checks of every entry point (host code only).
#pragma once
#include <cstdint>

#include "../types.hpp"
#include "kernels.hpp"

namespace cylon {

// the widest frame (preceding + following + 1) of rolling_lds: window_frame_lds_rows() of both twins
constexpr int kRollLdsRows = 513;

// func: kernels/window.hip WinFunc 0 .. 4 (sum of integers, sum of floats, min, max, count).  Returns the
// view the kernels use: a COUNT of a column that is not 1, 2, 4 or 8 bytes wide reads its validity only.
inline ColView rolling_check(const ColView &col, int func, int64_t n, int64_t preceding, int64_t following,
                             int64_t min_periods, bool mean) {
  constexpr int kSumI = 0, kSumF = 1, kCount = 4;
  CYLON_CHECK(func >= kSumI && func <= kCount, Code::Invalid, "rolling: value function " << func);
  CYLON_CHECK(n < (int64_t(1) << 32), Code::Invalid, "rolling: " << n << " rows");  // the counts are 32-bit
  CYLON_CHECK(preceding >= 0 && preceding <= n && following >= 0 && following <= n, Code::Invalid,
              "rolling: frame of " << preceding << " preceding and " << following << " following over " << n
                                   << " rows");
  CYLON_CHECK(min_periods >= 0, Code::Invalid, "rolling: min_periods " << min_periods);
  CYLON_CHECK(!mean || func == kSumI || func == kSumF, Code::Invalid, "rolling: mean of function " << func);
  ColView c = col;
  const bool plain = c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8;
  if (func == kCount) {
    if (!plain) c.width = 0;
    return c;
  }
  CYLON_CHECK(plain && c.kind <= static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "rolling: value column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != kSumF || (c.kind == static_cast<int>(ValueKind::FLOAT) && c.width >= 4), Code::Invalid,
              "rolling: float sum of a column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != kSumI || c.kind != static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "rolling: integer sum of a float column");
  return c;
}

}  // namespace cylon
