// CPU twin of kernels/frame_moments.hip, and the behaviour of the framed VAR / STD on CPU contexts
// (docs/semantics.md "Framed aggregates", VAR / STD).  The state, its merge, the pyramid's layout, the
// ROWS frame and the query are the shared rules of frame_moments_common.hpp; what differs is the walk:
// the pyramid's levels are built by one loop each and the positions are visited in order.
#include <cstring>

#include "frame_moments_common.hpp"
#include "kernels.hpp"

namespace cylon {
namespace cpu {

namespace {

void check_rows(int64_t n) {
  CYLON_CHECK(n < (int64_t(1) << 32), Code::Invalid, "moment frame: " << n << " rows");  // counts and lo / hi are 32-bit
}

void check_value(const ColView &c) {
  const bool is_float = c.kind == static_cast<int>(ValueKind::FLOAT);
  CYLON_CHECK(c.kind <= static_cast<int>(ValueKind::FLOAT) &&
                  (c.width == 4 || c.width == 8 || (!is_float && (c.width == 1 || c.width == 2))),
              Code::Invalid, "moment frame: value column of width " << c.width << ", kind " << c.kind);
}

}  // namespace

void frame_moments_pyramid(const ColView &col, int64_t n, const uint64_t *dense, const uint8_t *dense_valid,
                           uint64_t *P, uint64_t *S, uint64_t *E, void *) {
  if (n <= kFrRadix) return;
  check_rows(n);
  check_value(col);
  const FmPyramid src{FmPlanes{}, FmPlanes{}, FmPlanes{}, dense, dense_valid, col.width, col.kind};
  const FmMutPlanes p = fm_planes(P, fm_ps_slots(n)), s = fm_planes(S, fm_ps_slots(n)), ep = fm_planes(E, fm_e_slots(n));
  const FmPlanes in = fm_planes(static_cast<const uint64_t *>(E), fm_e_slots(n));
  int64_t nl = n, ps = 0, e = 0, ein = 0;  // ein: this level's offset in E, e: the next level's
  for (bool level0 = true; nl > kFrRadix; level0 = false) {
    for (int64_t b = 0; b < fr_up(nl); ++b) {
      const int64_t j0 = b * kFrRadix;
      const int cnt = j0 + kFrRadix <= nl ? kFrRadix : (int)(nl - j0);
      FmState ent[kFrRadix];
      for (int k = 0; k < kFrRadix; ++k)
        ent[k] = k >= cnt ? fm_identity() : level0 ? fm_level0(src, j0 + k) : fm_load(in, ein + j0 + k);
      FmState acc = fm_identity();
      for (int k = 0; k < kFrRadix; ++k) {
        acc = fm_merge(acc, ent[k]);
        fm_store(p, ps + j0 + k, acc);
      }
      fm_store(ep, e + b, acc);
      acc = fm_identity();
      for (int k = kFrRadix - 1; k >= 0; --k) {
        acc = fm_merge(ent[k], acc);
        fm_store(s, ps + j0 + k, acc);
      }
    }
    ps += fr_cap(nl);
    nl = fr_up(nl);
    ein = e;
    e += fr_cap(nl);
  }
}

void frame_moments_apply(const ColView &col, const int64_t *perm, int64_t n, bool std_dev, int64_t ddof,
                         int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo,
                         const uint32_t *hi, const int64_t *phead, const int64_t *rtail, int64_t preceding,
                         int64_t following, const uint64_t *P, const uint64_t *S, const uint64_t *E, uint8_t *out,
                         uint8_t *out_valid, void *) {
  if (n == 0) return;
  check_rows(n);
  check_value(col);
  CYLON_CHECK(ddof >= 0, Code::Invalid, "moment frame: ddof " << ddof);
  CYLON_CHECK(min_periods >= 1, Code::Invalid, "moment frame: min_periods " << min_periods);
  CYLON_CHECK(perm != nullptr && dense != nullptr, Code::Invalid, "moment frame: apply inputs");
  const bool range = lo != nullptr || hi != nullptr;
  CYLON_CHECK(range ? (lo != nullptr && hi != nullptr)
                    : (phead != nullptr && rtail != nullptr && preceding >= 0 && following >= 0),
              Code::Invalid, "moment frame: frame bounds");
  CYLON_CHECK(n <= kFrRadix || (P != nullptr && S != nullptr && E != nullptr), Code::Invalid,
              "moment frame: pyramid");
  CYLON_CHECK(out != nullptr && out_valid != nullptr, Code::Invalid, "moment frame: output");
  const FmPyramid pyr{fm_planes(P, fm_ps_slots(n)), fm_planes(S, fm_ps_slots(n)), fm_planes(E, fm_e_slots(n)),
                      dense,                        dense_valid,                  col.width,
                      col.kind};
  for (int64_t i = 0; i < n; ++i) {
    int64_t l, h;
    if (range) {
      l = lo[i];
      h = hi[i];
    } else {
      fm_rows_frame(i, n, phead[i], n - 1 - rtail[n - 1 - i], preceding, following, &l, &h);
    }
    const int64_t r = perm[i];
    const double v = fm_result(fm_query(pyr, n, l, h), std_dev, ddof, min_periods, &out_valid[r]);
    std::memcpy(out + r * 8, &v, 8);
  }
}

}  // namespace cpu
}  // namespace cylon
