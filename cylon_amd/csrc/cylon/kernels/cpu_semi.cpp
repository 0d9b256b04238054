// CPU twin of kernels/semi_join.hip: left semi / anti join mark over partitioned int64 key images.
// One std::unordered_set per partition; any number of partitions; never overflows.  The work-item
// and workspace arguments of the device kernel are ignored.
#include <unordered_set>

#include "kernels.hpp"

namespace cylon {
namespace cpu {

int64_t semi_join_capacity() { return int64_t(1) << 62; }
int64_t semi_join_slice_rows() { return int64_t(1) << 62; }

void semi_join_mark(const int64_t *rkeys, const int64_t *roffs, const int64_t *lkeys, const int64_t *lrow,
                    const int64_t *loffs, int64_t nparts, int anti, uint8_t *mask, int64_t *matched, int *overflow,
                    const int64_t *, const int64_t *, int64_t, int64_t *, int64_t *, void *) {
  *matched = 0;
  *overflow = 0;
  const uint8_t val = anti ? 0 : 1;
  std::unordered_set<int64_t> set;
  for (int64_t p = 0; p < nparts; ++p) {
    const int64_t lb = loffs[p], le = loffs[p + 1];
    if (lb == le) continue;
    set.clear();
    set.insert(rkeys + roffs[p], rkeys + roffs[p + 1]);
    for (int64_t r = lb; r < le; ++r) {
      if (set.count(lkeys[r]) == 0) continue;
      mask[lrow ? lrow[r] : r] = val;
      ++*matched;
    }
  }
}

}  // namespace cpu
}  // namespace cylon
