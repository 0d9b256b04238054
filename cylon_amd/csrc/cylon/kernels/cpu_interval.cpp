// CPU twin of kernels/interval.hip, and the definition of the interval join's rank pass, counts and
// expansion (docs/semantics.md "Interval join"): plain sequential loops.  The tiles, carries and LDS
// slices of the device kernels have no part in it; the rank workspace and the carry step are unused.
#include <cstring>

#include "interval_common.hpp"
#include "kernels.hpp"

namespace cylon {
namespace cpu {

namespace {

constexpr int64_t kIvTile = 2048;  // interval.hip kIvTile: the counters report the same tiles

inline uint64_t raw_bits(const ColView &c, int64_t i) {
  uint64_t b = 0;
  std::memcpy(&b, c.data + i * c.width, (size_t)c.width);  // little endian
  return b;
}

void check_bound(const ColView &c) {
  const bool isf = c.kind == static_cast<int>(ValueKind::FLOAT);
  const bool w = isf ? (c.width == 4 || c.width == 8) : (c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8);
  CYLON_CHECK(w && c.kind <= static_cast<int>(ValueKind::FLOAT) && c.data != nullptr, Code::Invalid,
              "interval: bound column of width " << c.width << ", kind " << c.kind);
}

inline bool in(int64_t r, int64_t base, int64_t len) { return r >= base && r - base < len; }

}  // namespace

int64_t interval_tile_rows() { return kIvTile; }
int64_t interval_rank_workspace(int64_t) { return 1; }

void interval_rank(const int64_t *perm, int64_t nl, int64_t nr, int64_t lbase, int64_t rbase, int64_t ubase, int64_t,
                   int64_t *, int64_t *lo, int64_t *hi, int64_t *rrows, void *) {
  const IntervalLayout y{nl, nr, lbase, rbase, ubase};
  CYLON_CHECK(interval_layout_ok(y), Code::Invalid,
              "interval: blocks at " << lbase << ", " << rbase << ", " << ubase << " of " << nl << " left and " << nr
                                     << " right rows");
  const int64_t n = nr + 2 * nl;
  int64_t c = 0;  // right rows strictly before position p
  for (int64_t p = 0; p < n; ++p) {
    const int64_t r = perm[p];
    if (in(r, rbase, nr)) rrows[c++] = r - rbase;
    else if (in(r, lbase, nl)) lo[r - lbase] = c;
    else hi[r - ubase] = c;
  }
}

void interval_counts(const ColView &lower, const ColView &upper, const int64_t *lo, const int64_t *hi, int64_t nl,
                     bool left, int64_t *cnt, uint8_t *empty, int64_t *matched, void *) {
  if (nl == 0) return;
  check_bound(lower);
  check_bound(upper);
  CYLON_CHECK(lo != nullptr && hi != nullptr && cnt != nullptr && (!left || empty != nullptr), Code::Invalid,
              "interval: counts buffers");
  int64_t sum = 0;
  for (int64_t i = 0; i < nl; ++i) {
    const bool lv = lower.valid == nullptr || lower.valid[i] != 0;
    const bool uv = upper.valid == nullptr || upper.valid[i] != 0;
    const bool usable = interval_usable(lv, raw_bits(lower, i), lower.width, lower.kind) &&
                        interval_usable(uv, raw_bits(upper, i), upper.width, upper.kind);
    const int64_t c = interval_count(usable, lo[i], hi[i]);
    sum += c;
    if (left) {
      empty[i] = c == 0 ? 1 : 0;
      cnt[i] = c == 0 ? 1 : c;
    } else {
      cnt[i] = c;
    }
  }
  if (matched != nullptr) *matched += sum;
}

void interval_expand(const int64_t *off, const int64_t *lo, const uint8_t *empty, const int64_t *rrows, int64_t nl,
                     int64_t nr, int64_t total, int64_t *li, int64_t *ri, void *) {
  if (total == 0) return;
  CYLON_CHECK(total > 0 && nl > 0 && nr >= 0, Code::Invalid,
              "interval: " << total << " pairs of " << nl << " left rows");
  for (int64_t l = 0; l < nl; ++l) {
    const bool filler = empty != nullptr && empty[l] != 0;
    for (int64_t o = off[l]; o < off[l + 1]; ++o) {
      li[o] = l;
      ri[o] = filler ? -1 : rrows[lo[l] + (o - off[l])];
    }
  }
}

}  // namespace cpu
}  // namespace cylon
