// CPU twin of kernels/asof.hip, and the definition of the as-of join's scan (docs/semantics.md
// "As-of join"): one sequential loop over the positions of the merged order that remembers the last
// candidate seen since the partition head.  The tile pairs and carries of the device's three phases
// have no part in it: asof_tile only writes the code bytes, asof_apply walks all positions.
#include <cstring>

#include "asof_common.hpp"
#include "kernels.hpp"

namespace cylon {
namespace cpu {

namespace {

inline uint64_t raw_bits(const ColView &c, int64_t i) {
  uint64_t b = 0;
  std::memcpy(&b, c.data + i * c.width, (size_t)c.width);  // little endian
  return b;
}

void check_on(const ColView &c) {
  const bool isf = c.kind == static_cast<int>(ValueKind::FLOAT);
  const bool w = isf ? (c.width == 4 || c.width == 8) : (c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8);
  CYLON_CHECK(w && c.kind <= static_cast<int>(ValueKind::FLOAT) && c.data != nullptr, Code::Invalid,
              "asof: `on` column of width " << c.width << ", kind " << c.kind);
}

}  // namespace

void asof_tile(const ColView &on, const int64_t *perm, const uint8_t *, int64_t n, int64_t nfirst, bool right_first,
               bool reverse, uint8_t *code, int64_t *, uint8_t *, void *) {
  if (n == 0) return;
  check_on(on);
  CYLON_CHECK(nfirst >= 0 && nfirst <= n, Code::Invalid, "asof: " << nfirst << " first rows of " << n);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t r = perm[reverse ? n - 1 - k : k];
    const bool valid = on.valid == nullptr || on.valid[r] != 0;
    code[k] = asof_code((r < nfirst) == right_first, valid, raw_bits(on, r), on.width, on.kind);
  }
}

void asof_apply(const int64_t *perm, const uint8_t *restarts, const uint8_t *code, int64_t n, int64_t nfirst,
                bool right_first, bool reverse, const int64_t *, int64_t *match, int64_t *matched, void *) {
  const int64_t lbase = right_first ? nfirst : 0, rbase = right_first ? 0 : nfirst;
  int64_t last = -1, cnt = 0;  // the last candidate's row in the concatenation
  for (int64_t k = 0; k < n; ++k) {
    if (restarts[k] & 1) last = -1;  // a new partition
    const int64_t r = perm[reverse ? n - 1 - k : k];
    if (code[k] & kAsofRight) {
      if (code[k] & kAsofUsable) last = r;
      continue;
    }
    const bool hit = (code[k] & kAsofUsable) && last >= 0;
    match[r - lbase] = hit ? last - rbase : -1;
    cnt += hit ? 1 : 0;
  }
  if (matched != nullptr) *matched += cnt;
}

void asof_pick(const ColView &left_on, const ColView &right_on, int64_t nl, const int64_t *back, const int64_t *fwd,
               bool has_tolerance, int64_t tolerance_i, double tolerance_f, int64_t *match, int64_t *matched, void *) {
  if (nl == 0) return;
  check_on(left_on);
  CYLON_CHECK(right_on.data != nullptr && right_on.width == left_on.width && right_on.kind == left_on.kind,
              Code::Invalid, "asof: `on` columns of different types");
  const AsofPick p{left_on.width, left_on.kind, has_tolerance ? 1 : 0, tolerance_i, tolerance_f};
  int64_t cnt = 0;
  for (int64_t i = 0; i < nl; ++i) {
    const int64_t b = back[i], f = fwd != nullptr ? fwd[i] : -1;
    const uint64_t x = (b >= 0 || f >= 0) ? raw_bits(left_on, i) : 0;
    const uint64_t yb = b >= 0 ? raw_bits(right_on, b) : 0;
    const uint64_t yf = f >= 0 ? raw_bits(right_on, f) : 0;
    const int64_t m = asof_pick_one(p, x, b, yb, f, yf);
    match[i] = m;
    cnt += m >= 0 ? 1 : 0;
  }
  if (matched != nullptr) *matched += cnt;
}

}  // namespace cpu
}  // namespace cylon
