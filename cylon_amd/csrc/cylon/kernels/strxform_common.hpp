// String transforms of one cell, shared by the HIP kernels (strxform.hip) and their CPU twin
// (cpu_strxform.cpp): the kept byte range of a slice and of a strip, the output length and the
// writer of a literal replace, and the ASCII case map of one byte (docs/semantics.md "String
// transforms").  No function here reads a byte outside [s, s + n) of the cell it is given, and
// none writes outside [dst, dst + the length it reports).
#pragma once
#include <cstdint>

#include "../common.hpp"
#include "strmatch_common.hpp"

namespace cylon {
namespace strxform {

using strmatch::kStrMaxPatternBytes;
using strmatch::sm_is_cont;

enum StrXformFn : int { SX_SLICE = 0, SX_STRIP = 1, SX_CASE = 2, SX_CONCAT = 3, SX_REPLACE = 4 };
enum StrStripSide : int { SX_LEFT = 1, SX_RIGHT = 2, SX_BOTH = 3 };

// What the kernels take besides the columns.  The literal buffer `lit` (device memory) holds
//   SX_STRIP:   the byte set as a 256-bit bitmap (32 bytes; bit b of byte b / 8)
//   SX_CONCAT:  the separator (len1 bytes)
//   SX_REPLACE: the pattern (len1 bytes), then the replacement (len2 bytes)
struct StrXform {
  int32_t fn = 0;
  int32_t utf8 = 0;           // SX_SLICE: the indices count code points (a STRING column)
  int32_t has_stop = 0;       // SX_SLICE: stop is given (else: the end of the cell)
  int32_t side = SX_BOTH;     // SX_STRIP: a StrStripSide
  int32_t upper = 0;          // SX_CASE
  int32_t a_bcast = 0, b_bcast = 0;  // SX_CONCAT: the operand is row 0 of a one-row column
  int32_t len1 = 0, len2 = 0;
  int64_t start = 0, stop = 0;  // SX_SLICE
  int64_t max_repl = -1;        // SX_REPLACE: < 0 = every match
};

constexpr int kStrSetBytes = 32;

CYLON_HD bool sx_in_set(const uint8_t *set, uint8_t b) { return (set[b >> 3] >> (b & 7)) & 1u; }

// a unit of a STRING cell begins at byte 0 and at every later byte that is no continuation byte
// (the positions strmatch's sm_boundary accepts); of a BINARY cell, at every byte
CYLON_HD bool sx_unit_start(const uint8_t *s, int64_t i) { return i == 0 || !sm_is_cont(s[i]); }

CYLON_HD int64_t sx_count_units(const uint8_t *s, int64_t n) {
  int64_t c = 0;
  for (int64_t i = 0; i < n; ++i) c += sx_unit_start(s, i) ? 1 : 0;
  return c;
}

// Python's [start:stop] over nu units, step 1: the kept unit range [*ub, *ue), clamped at both ends
CYLON_HD void sx_slice_units(int64_t nu, int64_t start, int64_t stop, int has_stop, int64_t *ub, int64_t *ue) {
  int64_t b = start < 0 ? start + nu : start;
  int64_t e = !has_stop ? nu : (stop < 0 ? stop + nu : stop);
  b = b < 0 ? 0 : (b > nu ? nu : b);
  e = e < 0 ? 0 : (e > nu ? nu : e);
  if (e < b) e = b;
  *ub = b;
  *ue = e;
}

// the byte at which unit k of a STRING cell begins; n when the cell has no more than k units
CYLON_HD int64_t sx_unit_pos(const uint8_t *s, int64_t n, int64_t k) {
  int64_t i = 0;
  for (; i < n; ++i) {
    if (sx_unit_start(s, i)) {
      if (k == 0) return i;
      --k;
    }
  }
  return n;
}

// the kept byte range [*b, *e) of a slice
CYLON_HD void sx_slice_range(const uint8_t *s, int64_t n, const StrXform &x, int64_t *b, int64_t *e) {
  if (!x.utf8) {
    sx_slice_units(n, x.start, x.stop, x.has_stop, b, e);
    return;
  }
  // the units are counted only when an index counts from the end
  const bool from_end = x.start < 0 || (x.has_stop && x.stop < 0);
  int64_t ub, ue;
  if (from_end) {
    sx_slice_units(sx_count_units(s, n), x.start, x.stop, x.has_stop, &ub, &ue);
  } else {
    ub = x.start;
    ue = x.has_stop ? (x.stop < ub ? ub : x.stop) : -1;
  }
  *b = sx_unit_pos(s, n, ub);
  *e = ue < 0 ? n : (ue == ub ? *b : sx_unit_pos(s, n, ue));
}

// the kept byte range [*b, *e) of a strip: leading (SX_LEFT) and / or trailing (SX_RIGHT) bytes of
// the set go
CYLON_HD void sx_strip_range(const uint8_t *s, int64_t n, const uint8_t *set, int side, int64_t *b, int64_t *e) {
  int64_t lo = 0, hi = n;
  if (side & SX_LEFT)
    while (lo < hi && sx_in_set(set, s[lo])) ++lo;
  if (side & SX_RIGHT)
    while (hi > lo && sx_in_set(set, s[hi - 1])) --hi;
  *b = lo;
  *e = hi;
}

CYLON_HD uint8_t sx_case(uint8_t b, int upper) {
  if (upper) return (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
  return (b >= 'A' && b <= 'Z') ? (uint8_t)(b + 32) : b;
}

// sx_case of the four bytes of a word at once: bit 7 of a byte of m is set iff the byte is a letter
// of the case that changes (no carry leaves a byte: 0x7f + 0x3f < 0x100)
CYLON_HD uint32_t sx_case_word(uint32_t w, int upper) {
  const uint32_t x = w & 0x7f7f7f7fu;
  const uint32_t ge = x + (upper ? 0x1f1f1f1fu : 0x3f3f3f3fu);  // >= 'a' / 'A'
  const uint32_t gt = x + (upper ? 0x05050505u : 0x25252525u);  // > 'z' / 'Z'
  const uint32_t m = ge & ~gt & ~w & 0x80808080u;
  return w ^ (m >> 2);
}

// leftmost, non-overlapping occurrences of the literal p (np > 0), at most max_repl (< 0: all)
CYLON_HD int64_t sx_replace_count(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, int64_t max_repl) {
  int64_t c = 0;
  for (int64_t i = 0; i + np <= n && (max_repl < 0 || c < max_repl);) {
    if (strmatch::sm_bytes_equal(s + i, p, np)) {
      ++c;
      i += np;
    } else {
      ++i;
    }
  }
  return c;
}

CYLON_HD int64_t sx_replace_len(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, int64_t nr,
                                int64_t max_repl) {
  return n + sx_replace_count(s, n, p, np, max_repl) * (nr - np);
}

// writes sx_replace_len(...) bytes at dst and returns that length
CYLON_HD int64_t sx_replace_write(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, const uint8_t *r,
                                  int64_t nr, int64_t max_repl, uint8_t *dst) {
  int64_t c = 0, i = 0, o = 0;
  while (i < n) {
    if (i + np <= n && (max_repl < 0 || c < max_repl) && strmatch::sm_bytes_equal(s + i, p, np)) {
      for (int64_t k = 0; k < nr; ++k) dst[o++] = r[k];
      ++c;
      i += np;
    } else {
      dst[o++] = s[i++];
    }
  }
  return o;
}

// SX_SLICE / SX_STRIP / SX_CASE / SX_REPLACE of one live cell: the output length ...
CYLON_HD int64_t sx_cell_len(const StrXform &x, const uint8_t *s, int64_t n, const uint8_t *lit) {
  int64_t b, e;
  switch (x.fn) {
    case SX_SLICE: sx_slice_range(s, n, x, &b, &e); return e - b;
    case SX_STRIP: sx_strip_range(s, n, lit, x.side, &b, &e); return e - b;
    case SX_REPLACE: return sx_replace_len(s, n, lit, x.len1, x.len2, x.max_repl);
    default: return n;
  }
}

// ... and its bytes at dst
CYLON_HD void sx_cell_write(const StrXform &x, const uint8_t *s, int64_t n, const uint8_t *lit, uint8_t *dst) {
  int64_t b = 0, e = n;
  switch (x.fn) {
    case SX_SLICE: sx_slice_range(s, n, x, &b, &e); break;
    case SX_STRIP: sx_strip_range(s, n, lit, x.side, &b, &e); break;
    case SX_REPLACE: sx_replace_write(s, n, lit, x.len1, lit + x.len1, x.len2, x.max_repl, dst); return;
    case SX_CASE:
      for (int64_t i = 0; i < n; ++i) dst[i] = sx_case(s[i], x.upper);
      return;
    default: break;
  }
  for (int64_t i = b; i < e; ++i) dst[i - b] = s[i];
}

}  // namespace strxform
}  // namespace cylon
