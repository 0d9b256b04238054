// CPU twin of kernels/strmatch.hip, and the definition of the string predicates on CPU contexts
// (docs/semantics.md "String predicates"): one plain loop over the rows that calls the shared cell
// matchers of strmatch_common.hpp.  The tiles and the long-row path of the device have no part in
// it.  A null row gives 0 and its bytes are never read.
#include "kernels.hpp"
#include "strmatch_common.hpp"

namespace cylon {
namespace cpu {

using namespace strmatch;

namespace {
inline bool live(const ColView &c, int64_t i) { return c.valid == nullptr || c.valid[i] != 0; }
}  // namespace

int64_t string_tile_bytes() { return kStrTileBytes; }  // the device's tile; nothing is staged here

void str_compare(const ColView &a, const ColView &b, int b_scalar, int op, int64_t n, uint8_t *out, void *) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t j = b_scalar ? 0 : i;
    if (!live(a, i) || !live(b, j)) {
      out[i] = 0;
      continue;
    }
    const int64_t ab = a.offsets[i], bb = b.offsets[j];
    out[i] = sm_cmp_result(sm_compare(a.data + ab, a.offsets[i + 1] - ab, b.data + bb, b.offsets[j + 1] - bb), op);
  }
}

void str_match(const ColView &a, int kind, const uint8_t *pat, int64_t plen, int utf8, int64_t n, uint8_t *out,
               void *) {
  CYLON_CHECK(plen >= 0 && plen <= kStrMaxPatternBytes, Code::Invalid,
              "string match: a pattern of " << plen << " bytes (at most " << kStrMaxPatternBytes << ")");
  CYLON_CHECK(kind >= STR_STARTS_WITH && kind <= STR_EQUALS, Code::Invalid, "string match: kind " << kind);
  for (int64_t i = 0; i < n; ++i) {
    if (!live(a, i)) {
      out[i] = 0;
      continue;
    }
    const int64_t b = a.offsets[i], len = a.offsets[i + 1] - b;
    const uint8_t *s = a.data + b;
    bool r;
    switch (kind) {
      case STR_STARTS_WITH: r = sm_starts_with(s, len, pat, plen, utf8); break;
      case STR_ENDS_WITH: r = sm_ends_with(s, len, pat, plen, utf8); break;
      case STR_CONTAINS: r = sm_contains(s, len, pat, plen, utf8); break;
      case STR_LIKE: r = sm_like(s, len, pat, pat + plen, (int)plen, utf8); break;
      default: r = sm_equals(s, len, pat, plen); break;
    }
    out[i] = r ? 1 : 0;
  }
}

void str_length(const ColView &a, int unit, int64_t n, int64_t *out, void *) {
  for (int64_t i = 0; i < n; ++i) {
    if (!live(a, i)) {
      out[i] = 0;
      continue;
    }
    const int64_t b = a.offsets[i], len = a.offsets[i + 1] - b;
    out[i] = unit == STR_LEN_BYTES ? len : sm_count_chars(a.data + b, len);
  }
}

}  // namespace cpu
}  // namespace cylon
