// CPU twin of kernels/window.hip, and the definition of the window functions (docs/semantics.md
// "Window functions"): every function is one sequential loop over the sorted positions.  The tile
// pairs and carries of the device's three phases have no part in it: window_tile only gathers the
// values into sorted order, window_carry does nothing, the apply functions walk all positions.
#include <cstring>

#include "kernels.hpp"
#include "order_image.hpp"

namespace cylon {
namespace cpu {

namespace {

constexpr int64_t kWinTile = 2048;        // reported for symmetry with the device; nothing here is tiled
constexpr int64_t kWinCarryTiles = 2048;

enum : int { WF_SUM_I = 0, WF_SUM_F = 1, WF_MIN = 2, WF_MAX = 3, WF_COUNT = 4, WF_RANK = 5 };

inline bool plain_width(int w) { return w == 1 || w == 2 || w == 4 || w == 8; }

inline uint64_t raw_bits(const ColView &c, int64_t i) {
  uint64_t b = 0;
  if (plain_width(c.width)) std::memcpy(&b, c.data + i * c.width, (size_t)c.width);  // little endian
  return b;
}

inline int64_t sign_extend(uint64_t b, int w) {
  switch (w) {
    case 1: return (int8_t)b;
    case 2: return (int16_t)b;
    case 4: return (int32_t)b;
    default: return (int64_t)b;
  }
}

inline double as_f64(uint64_t b, int w) {
  if (w == 8) {
    double d;
    std::memcpy(&d, &b, 8);
    return d;
  }
  const uint32_t u = (uint32_t)b;
  float f;
  std::memcpy(&f, &u, 4);
  return (double)f;
}

void check_value(const ColView &c, int func) {
  CYLON_CHECK(func >= WF_SUM_I && func <= WF_COUNT, Code::Invalid, "window: value function " << func);
  if (func == WF_COUNT) return;
  CYLON_CHECK(plain_width(c.width) && c.kind <= static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "window: value column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_F || (c.kind == static_cast<int>(ValueKind::FLOAT) && c.width >= 4), Code::Invalid,
              "window: float sum of a column of width " << c.width << ", kind " << c.kind);
  CYLON_CHECK(func != WF_SUM_I || c.kind != static_cast<int>(ValueKind::FLOAT), Code::Invalid,
              "window: integer sum of a float column");
}

}  // namespace

int64_t window_tile_rows() { return kWinTile; }
int64_t window_carry_tiles() { return kWinCarryTiles; }

void window_flags(const uint8_t *part, const uint8_t *peer, int64_t n, uint8_t *flags, void *) {
  for (int64_t i = 0; i < n; ++i) {
    const bool ph = part[i] != 0, qh = peer != nullptr ? peer[i] != 0 : ph;
    flags[i] = (uint8_t)((ph ? 1 : 0) | (qh ? 2 : 0));
  }
}

void window_tile(const ColView &col, const int64_t *perm, const uint8_t *, int64_t n, int func, uint64_t *dense,
                 uint8_t *dense_valid, bool gather, int64_t *, uint8_t *, void *) {
  check_value(col, func);
  if (!gather) return;
  CYLON_CHECK(col.valid == nullptr || dense_valid != nullptr, Code::Invalid,
              "window: nullable column without a dense validity buffer");
  for (int64_t i = 0; i < n; ++i) {
    dense[i] = raw_bits(col, perm[i]);
    if (dense_valid != nullptr) dense_valid[i] = col.valid == nullptr || col.valid[perm[i]] != 0;
  }
}

void window_carry(const int64_t *, const uint8_t *, int64_t, int, int, int64_t step, int64_t *, void *) {
  CYLON_CHECK(step <= kWinCarryTiles, Code::Invalid, "window: carry step of " << step << " tiles");
}

void window_apply(const ColView &col, const int64_t *perm, const uint8_t *flags, int64_t n, int func,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *, uint8_t *out,
                  uint8_t *out_valid, void *) {
  check_value(col, func);
  const int w = col.width, kind = col.kind;
  uint64_t acc = 0;  // integer sum (mod 2^64), count, or the extreme image seen so far
  double facc = 0;
  bool seen = false;  // a non-null value of this partition has been met
  for (int64_t i = 0; i < n; ++i) {
    if (flags[i] & 1) {  // a new partition
      acc = 0;
      facc = 0;
      seen = false;
    }
    const bool live = dense_valid == nullptr || dense_valid[i] != 0;
    if (live) {
      const uint64_t b = dense[i];
      switch (func) {
        case WF_SUM_I:
          acc += kind == static_cast<int>(ValueKind::SIGNED_INT) ? (uint64_t)sign_extend(b, w) : b;
          break;
        case WF_SUM_F: facc += as_f64(b, w); break;
        case WF_MIN: {
          const uint64_t im = order_image(b, w, kind);
          if (!seen || im < acc) acc = im;
          break;
        }
        case WF_MAX: {
          const uint64_t im = order_image(b, w, kind);
          if (!seen || im > acc) acc = im;
          break;
        }
        default: acc += 1; break;
      }
      seen = true;
    }
    const int64_t r = perm[i];
    if (func == WF_MIN || func == WF_MAX) {
      const uint64_t v = order_unimage(acc, w, kind);  // a null row's bytes are unspecified
      std::memcpy(out + r * w, &v, (size_t)w);
    } else if (func == WF_SUM_F) {
      std::memcpy(out + r * 8, &facc, 8);
    } else {
      std::memcpy(out + r * 8, &acc, 8);
    }
    if (out_valid != nullptr) out_valid[r] = live;
  }
}

void window_rank_tile(const uint8_t *, int64_t, int64_t *, uint8_t *, void *) {}

void window_rank_apply(const int64_t *perm, const uint8_t *flags, int64_t n, const int64_t *, int64_t *row_number,
                       int64_t *rank, int64_t *dense_rank, int64_t *phead, void *) {
  int64_t p = 0, q = 0, d = 0;  // last partition head, last peer head, peer heads of this partition
  for (int64_t i = 0; i < n; ++i) {
    if (flags[i] & 1) {
      p = i;
      d = 0;
    }
    if (flags[i] & 2) {
      q = i;
      ++d;
    }
    const int64_t r = perm[i];
    if (row_number != nullptr) row_number[r] = i - p + 1;
    if (rank != nullptr) rank[r] = q - p + 1;
    if (dense_rank != nullptr) dense_rank[r] = d;
    if (phead != nullptr) phead[i] = p;
  }
}

void window_shift(const int64_t *perm, const int64_t *phead, int64_t n, int64_t delta, int64_t *src, void *) {
  CYLON_CHECK(delta >= -n && delta <= n, Code::Invalid, "window: shift of " << delta << " over " << n << " rows");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t j = i + delta;
    src[perm[i]] = (j >= 0 && j < n && phead[j] == phead[i]) ? perm[j] : -1;
  }
}

}  // namespace cpu
}  // namespace cylon
