// CPU twin of kernels/window_nav.hip, and the definition of the navigation and distribution window
// functions (docs/semantics.md "Navigation and distribution functions"): every function is one
// sequential loop over the sorted positions.  The tile pairs and carries of the device's three phases
// have no part in it: window_fill_tile does nothing, window_fill_apply walks all positions.
#include <cstring>

#include "kernels.hpp"

namespace cylon {
namespace cpu {

namespace {

enum : int { NAV_FIRST = 0, NAV_LAST = 1, NAV_NTH = 2, NAV_FIRST_LIVE = 3, NAV_LAST_LIVE = 4 };
enum : int { NAV_NTILE = 0, NAV_PERCENT_RANK = 1, NAV_CUME_DIST = 2 };

inline bool plain_width(int w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// the value mode's buffers, or none of them
void check_value(const ColView &col, const uint64_t *dense, const uint8_t *out, const uint8_t *out_valid) {
  if (out == nullptr) return;
  CYLON_CHECK(plain_width(col.width), Code::Invalid, "window: value mode on a column of width " << col.width);
  CYLON_CHECK(out_valid != nullptr && dense != nullptr, Code::Invalid, "window: value mode output");
}

inline void store_bits(uint8_t *out, int64_t r, int w, uint64_t v) {
  std::memcpy(out + r * w, &v, (size_t)w);  // little endian
}

}  // namespace

void window_fill_tile(const uint8_t *restarts, int64_t n, bool, const uint8_t *dense_valid, int64_t *, uint8_t *,
                      void *) {
  if (n == 0) return;
  CYLON_CHECK(restarts != nullptr && dense_valid != nullptr, Code::Invalid, "window: fill scan inputs");
}

void window_fill_apply(const ColView &col, const int64_t *perm, const uint8_t *restarts, int64_t n, bool reverse,
                       int64_t limit, const uint64_t *dense, const uint8_t *dense_valid, const int64_t *,
                       uint8_t *out, uint8_t *out_valid, int64_t *src, int64_t *pos, void *) {
  if (n == 0) return;
  CYLON_CHECK(limit >= 0, Code::Invalid, "window: fill limit " << limit);
  CYLON_CHECK(out != nullptr || src != nullptr || pos != nullptr, Code::Invalid, "window: fill without an output");
  CYLON_CHECK(out == nullptr || src == nullptr, Code::Invalid, "window: fill in value mode and source mode at once");
  CYLON_CHECK(perm != nullptr && restarts != nullptr && dense_valid != nullptr, Code::Invalid,
              "window: fill scan inputs");
  check_value(col, dense, out, out_valid);
  int64_t last = -1;  // the scan position of the partition's latest non-null value
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = reverse ? n - 1 - k : k;
    if (restarts[k] & 1) last = -1;
    if (dense_valid[i] != 0) last = k;
    const bool has = last >= 0 && (limit == 0 || k - last <= limit);
    const int64_t j = has ? (reverse ? n - 1 - last : last) : -1;
    const int64_t r = perm[i];
    if (out != nullptr) {
      store_bits(out, r, col.width, dense[has ? j : i]);
      out_valid[r] = has ? 1 : 0;
    }
    if (src != nullptr) src[r] = has ? perm[j] : -1;
    if (pos != nullptr) pos[i] = j;
  }
}

void window_nav_pick(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail,
                     const int64_t *fillpos, int64_t n, int form, int64_t k, const uint64_t *dense,
                     const uint8_t *dense_valid, uint8_t *out, uint8_t *out_valid, int64_t *src, void *) {
  if (n == 0) return;
  CYLON_CHECK(form >= NAV_FIRST && form <= NAV_LAST_LIVE, Code::Invalid, "window: navigation form " << form);
  CYLON_CHECK(perm != nullptr && (out != nullptr || src != nullptr), Code::Invalid, "window: navigation outputs");
  CYLON_CHECK(phead != nullptr || form == NAV_LAST || form == NAV_LAST_LIVE, Code::Invalid, "window: partition heads");
  CYLON_CHECK(rtail != nullptr || form == NAV_FIRST || form == NAV_FIRST_LIVE, Code::Invalid, "window: reversed tails");
  CYLON_CHECK(fillpos != nullptr || form < NAV_FIRST_LIVE, Code::Invalid, "window: fill positions");
  CYLON_CHECK(form != NAV_NTH || k >= 1, Code::Invalid, "window: nth_value of row " << k);
  check_value(col, dense, out, out_valid);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t hd = phead != nullptr ? phead[i] : 0;
    const int64_t tl = rtail != nullptr ? n - 1 - rtail[n - 1 - i] : 0;
    int64_t j;
    switch (form) {
      case NAV_FIRST: j = hd; break;
      case NAV_LAST: j = tl; break;
      case NAV_NTH: j = k - 1 <= tl - hd ? hd + k - 1 : -1; break;
      case NAV_FIRST_LIVE: j = fillpos[hd]; break;
      default: j = fillpos[tl]; break;
    }
    const int64_t r = perm[i];
    if (out != nullptr) {
      store_bits(out, r, col.width, j >= 0 ? dense[j] : 0);
      out_valid[r] = j >= 0 ? (dense_valid != nullptr ? dense_valid[j] != 0 : 1) : 0;
    }
    if (src != nullptr) src[r] = j >= 0 ? perm[j] : -1;
  }
}

void window_rev_peer_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *) {
  for (int64_t k = 0; k < n; ++k) rflags[k] = k == 0 ? (uint8_t)3 : (uint8_t)(flags[n - k] & 3);
}

void window_rank_heads(const uint8_t *flags, int64_t n, const int64_t *, int64_t *phead, int64_t *qhead, void *) {
  int64_t p = 0, q = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (flags[i] & 1) p = i;
    if (flags[i] & 2) q = i;
    if (phead != nullptr) phead[i] = p;
    if (qhead != nullptr) qhead[i] = q;
  }
}

void window_dist_apply(const int64_t *perm, const int64_t *phead, const int64_t *rtail, const int64_t *qhead,
                       const int64_t *rqhead, int64_t n, int func, int64_t k, uint8_t *out, void *) {
  if (n == 0) return;
  CYLON_CHECK(func >= NAV_NTILE && func <= NAV_CUME_DIST, Code::Invalid, "window: distribution function " << func);
  CYLON_CHECK(perm != nullptr && phead != nullptr && rtail != nullptr && out != nullptr, Code::Invalid,
              "window: distribution inputs");
  CYLON_CHECK(func != NAV_NTILE || k >= 1, Code::Invalid, "window: ntile of " << k << " buckets");
  CYLON_CHECK(func != NAV_PERCENT_RANK || qhead != nullptr, Code::Invalid, "window: peer heads");
  CYLON_CHECK(func != NAV_CUME_DIST || rqhead != nullptr, Code::Invalid, "window: peer tails");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t hd = phead[i], tl = n - 1 - rtail[n - 1 - i];
    const int64_t s = tl - hd + 1, r = i - hd;
    const int64_t row = perm[i];
    if (func == NAV_NTILE) {
      const int64_t q = s / k, m = s % k, big = m * (q + 1);
      const int64_t b = r < big ? r / (q + 1) + 1 : m + (r - big) / (q > 0 ? q : 1) + 1;
      std::memcpy(out + row * 8, &b, 8);
    } else {
      double v;
      if (func == NAV_PERCENT_RANK) {
        v = s == 1 ? 0.0 : (double)(qhead[i] - hd) / (double)(s - 1);
      } else {
        const int64_t pt = n - 1 - rqhead[n - 1 - i];
        v = (double)(pt - hd + 1) / (double)s;
      }
      std::memcpy(out + row * 8, &v, 8);
    }
  }
}

}  // namespace cpu
}  // namespace cylon
