// Sizing rules of the radix partitions (LDS radix join, semi join, slot-mode partition passes, MSD
// key sort).  Pure host arithmetic, stated once: every user must agree on them (a bounded-memory
// chunk is only joinable when its bits equal the ones the join would have chosen).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace cylon {
namespace ops {
namespace sizing {

// Partition bits: the fewest bits whose mean build partition, ceil(rows / 2^bits), sits 8 Poisson
// sigma (+16 rows) below the LDS capacity `cap`.  The largest of ~2^18 uniform partitions then fits
// with ~1e-10 failure odds (an overflow only sends the join to its exact / global path).  1B rows:
// 18 bits -- two 9-bit passes -- for inner joins (cap 4544) and build-preserving outer joins (cap
// 4408) alike.
inline int partition_bits(int64_t rows, int64_t cap, int max_bits = 24) {
  int bits = 0;
  for (; bits < max_bits; ++bits) {
    const double mean = (double)((rows + (int64_t(1) << bits) - 1) >> bits);
    if (mean + 8.0 * std::sqrt(mean) + 16.0 <= (double)cap) break;
  }
  return bits;
}

// Slot rows of a slot-mode (histogram-free) pass: a partition of `mean` expected rows claims a
// fixed slot of mean + 8 Poisson sigma + 64 rows, rounded up to 8 rows.  A partition beyond its
// slot (skewed keys) raises the pass's overflow flag and the caller partitions exactly.
inline int64_t slot_rows(double mean) {
  return ((int64_t)(mean + 8.0 * std::sqrt(mean) + 64.0) + 7) & ~int64_t(7);
}

// Digit split of a two-pass (MSD) partition: the second (low) digit has <= 9 bits, the first
// (high) digit the rest, which the passes take up to 10 bits: 11 .. 19 partition bits run in two
// passes (callers check db1 <= 10).
struct Digits {
  int db1, db2;
};
inline Digits digit_split(int bits) {
  const int db2 = std::min(9, bits / 2);
  return {bits - db2, db2};
}

}  // namespace sizing
}  // namespace ops
}  // namespace cylon
