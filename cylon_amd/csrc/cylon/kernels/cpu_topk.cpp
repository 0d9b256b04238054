// CPU twin of kernels/topk.hip: the same scan / start / hist / pick / collect primitives over the same
// state words and the same image (order_image.hpp), in plain loops.  The lists come out in row order.
#include <cstring>

#include "kernels.hpp"
#include "order_image.hpp"

namespace cylon {
namespace cpu {

namespace {

constexpr int kTKDigitBits = 11;
constexpr int kTKBins = 1 << kTKDigitBits;

// kernels/topk.hip TKState
enum : int { PIMG = 0, ILO, IHI, PROW, RLO, RHI, KREM, SURE, BUCKET, NONNULL, OR_, AND_, CUR_SURE, CUR_CAND, ERROR_,
             WORDS = 16 };

inline uint64_t raw_bits(const ColView &c, int64_t i) {
  uint64_t b = 0;
  std::memcpy(&b, c.data + i * c.width, (size_t)c.width);  // little endian
  return b;
}

inline bool live(const ColView &c, int64_t i) { return c.valid == nullptr || c.valid[i] != 0; }

inline uint64_t image(const ColView &c, int64_t i, bool desc) {
  return sort_key_image(raw_bits(c, i), c.width, c.kind, desc);
}

}  // namespace

int topk_digit_bits() { return kTKDigitBits; }
int64_t topk_state_words() { return WORDS; }
int64_t topk_workspace() { return WORDS + kTKBins; }

void topk_scan(const ColView &col, int64_t n, bool desc, int64_t *ws, void *) {
  std::memset(ws, 0, sizeof(int64_t) * (size_t)(WORDS + kTKBins));
  uint64_t o = 0, a = ~0ull;
  int64_t cnt = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!live(col, i)) continue;
    const uint64_t k = image(col, i, desc);
    o |= k;
    a &= k;
    ++cnt;
  }
  ws[OR_] = (int64_t)o;
  ws[AND_] = (int64_t)a;
  ws[NONNULL] = cnt;
}

void topk_start(int64_t *ws, int64_t k, int ihi, int rhi, void *) {
  ws[PIMG] = 0;
  ws[ILO] = ws[IHI] = ihi;
  ws[PROW] = 0;
  ws[RLO] = ws[RHI] = rhi;
  ws[KREM] = k;
  ws[SURE] = 0;
  ws[BUCKET] = ws[NONNULL];
}

void topk_hist(const ColView &col, int64_t n, bool desc, int64_t *ws, int src, int db, void *) {
  CYLON_CHECK(db >= 1 && db <= kTKDigitBits, Code::Invalid, "top-k select: digit of " << db << " bits");
  const int ilo = (int)ws[ILO], ihi = (int)ws[IHI], rlo = (int)ws[RLO], rhi = (int)ws[RHI];
  const uint64_t pimg = (uint64_t)ws[PIMG], prow = (uint64_t)ws[PROW];
  const int top = src ? rlo : ilo;
  int64_t *h = ws + WORDS;
  for (int64_t i = 0; i < n; ++i) {
    if (!live(col, i)) continue;
    const uint64_t k = image(col, i, desc);
    if (bit_field(k, ilo, ihi) != pimg || bit_field((uint64_t)i, rlo, rhi) != prow) continue;
    ++h[bit_field(src ? (uint64_t)i : k, top - db, top)];
  }
}

void topk_pick(int64_t *ws, int src, int db, void *) {
  int64_t *h = ws + WORDS;
  const int64_t krem = ws[KREM];
  int64_t cum = 0;
  int b = 0;
  while (b < kTKBins && cum + h[b] < krem) cum += h[b++];
  if (b >= kTKBins || krem <= 0) {
    ws[ERROR_] = 2;
  } else {
    ws[SURE] += cum;
    ws[KREM] = krem - cum;
    ws[BUCKET] = h[b];
    if (src) {
      ws[PROW] = (int64_t)(((uint64_t)ws[PROW] << db) | (uint64_t)b);
      ws[RLO] -= db;
    } else {
      ws[PIMG] = (int64_t)(((uint64_t)ws[PIMG] << db) | (uint64_t)b);
      ws[ILO] -= db;
    }
  }
  std::memset(h, 0, sizeof(int64_t) * kTKBins);
}

void topk_collect(const ColView &col, int64_t n, bool desc, int64_t *ws, uint64_t *sure_img, int64_t *sure_row,
                  int64_t sure_cap, uint64_t *cand_img, int64_t *cand_row, int64_t cand_cap, void *) {
  const int ilo = (int)ws[ILO], ihi = (int)ws[IHI], rlo = (int)ws[RLO], rhi = (int)ws[RHI];
  const uint64_t pimg = (uint64_t)ws[PIMG], prow = (uint64_t)ws[PROW];
  for (int64_t i = 0; i < n; ++i) {
    if (!live(col, i)) continue;
    const uint64_t k = image(col, i, desc);
    const uint64_t fi = bit_field(k, ilo, ihi), fr = bit_field((uint64_t)i, rlo, rhi);
    const bool sure = fi < pimg || (fi == pimg && fr < prow);
    const bool cand = fi == pimg && fr == prow;
    if (!sure && !cand) continue;
    int64_t &cur = ws[sure ? CUR_SURE : CUR_CAND];
    const int64_t pos = cur++;
    if (pos >= (sure ? sure_cap : cand_cap)) {  // never past a buffer
      ws[ERROR_] = 1;
      continue;
    }
    (sure ? sure_img : cand_img)[pos] = k;
    (sure ? sure_row : cand_row)[pos] = i;
  }
}

}  // namespace cpu
}  // namespace cylon
