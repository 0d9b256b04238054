// CPU twin of kernels/strxform.hip, and the definition of the string transforms on CPU contexts
// (docs/semantics.md "String transforms"): one plain loop over the rows that calls the shared cell
// functions of strxform_common.hpp.  The tiles and the long-row path of the device have no part in
// it.  A row that is not live has length 0 and its bytes are never read.
#include "kernels.hpp"
#include "strxform_common.hpp"

namespace cylon {
namespace cpu {

using namespace strxform;

namespace {

inline bool live(const ColView &a, const ColView &b, const StrXform &x, int64_t i) {
  return (a.valid == nullptr || a.valid[i] != 0) && (x.fn != SX_CONCAT || b.valid == nullptr || b.valid[i] != 0);
}

void check_xform(const StrXform &x) {
  CYLON_CHECK(x.fn >= SX_SLICE && x.fn <= SX_REPLACE, Code::Invalid, "string transform: function " << x.fn);
  CYLON_CHECK(x.len1 >= 0 && x.len2 >= 0 && x.len1 <= kStrMaxPatternBytes && x.len2 <= kStrMaxPatternBytes,
              Code::Invalid, "string transform: a literal of more than " << kStrMaxPatternBytes << " bytes");
  CYLON_CHECK(x.fn != SX_REPLACE || x.len1 > 0, Code::Invalid, "string replace: the pattern is empty");
}

}  // namespace

void strx_lengths(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                  int64_t *lens, void *) {
  check_xform(x);
  for (int64_t i = 0; i < n; ++i) {
    if (!live(a, b, x, i)) {
      lens[i] = 0;
      continue;
    }
    const int64_t ra = x.a_bcast ? 0 : i;
    const int64_t ab = a.offsets[ra], la = a.offsets[ra + 1] - ab;
    if (x.fn == SX_CONCAT) {
      const int64_t rb = x.b_bcast ? 0 : i;
      lens[i] = la + x.len1 + (b.offsets[rb + 1] - b.offsets[rb]);
    } else {
      lens[i] = sx_cell_len(x, a.data + ab, la, lit);
    }
  }
}

void strx_write(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                const int64_t *out_off, uint8_t *out, uint32_t *flag, void *) {
  check_xform(x);
  uint8_t high = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!live(a, b, x, i)) continue;
    const int64_t ra = x.a_bcast ? 0 : i;
    const int64_t ab = a.offsets[ra], la = a.offsets[ra + 1] - ab;
    const uint8_t *sa = a.data + ab;
    uint8_t *d = out + out_off[i];
    if (x.fn == SX_CONCAT) {
      const int64_t rb = x.b_bcast ? 0 : i;
      const int64_t bb = b.offsets[rb], lb = b.offsets[rb + 1] - bb;
      for (int64_t k = 0; k < la; ++k) d[k] = sa[k];
      for (int64_t k = 0; k < x.len1; ++k) d[la + k] = lit[k];
      for (int64_t k = 0; k < lb; ++k) d[la + x.len1 + k] = b.data[bb + k];
    } else {
      if (x.fn == SX_CASE)
        for (int64_t k = 0; k < la; ++k) high |= sa[k];
      sx_cell_write(x, sa, la, lit, d);
    }
  }
  if (flag != nullptr && (high & 0x80u)) *flag = 1;
}

void strx_case_flat(const ColView &a, int upper, int64_t n, int64_t total, int64_t *out_off, uint8_t *out,
                    uint32_t *flag, void *) {
  const int64_t base = a.offsets[0];
  for (int64_t i = 0; i <= n; ++i) out_off[i] = a.offsets[i] - base;
  uint8_t high = 0;
  for (int64_t k = 0; k < total; ++k) {
    const uint8_t c = a.data[base + k];
    high |= c;
    out[k] = sx_case(c, upper);
  }
  if (high & 0x80u) *flag = 1;
}

}  // namespace cpu
}  // namespace cylon
