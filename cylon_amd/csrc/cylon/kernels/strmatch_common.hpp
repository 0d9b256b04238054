// String predicates of one cell, shared by the HIP kernels (strmatch.hip) and their CPU twins
// (cpu_strings.cpp): comparison, prefix, suffix, substring, code-point count and SQL LIKE over a
// byte pointer and a length (docs/semantics.md "String predicates").  No function here reads a
// byte outside [s, s + n) of the cell it is given.
#pragma once
#include <cstdint>

#include "../common.hpp"

namespace cylon {
namespace strmatch {

// longest literal pattern / compiled LIKE pattern the native entry points take (bytes / tokens)
constexpr int kStrMaxPatternBytes = 1024;
// string_tile_bytes(): the largest byte span of a block's 256 consecutive rows that the device
// stages in LDS (strmatch.hip, whose header gives the sizing); the CPU twin stages nothing
constexpr int kStrTileBytes = 16384;

enum StrCmpOp : int { STR_EQ = 0, STR_NE = 1, STR_LT = 2, STR_LE = 3, STR_GT = 4, STR_GE = 5 };
// STR_EQUALS is what a LIKE pattern without a wildcard compiles to; it is not a public kind
enum StrMatchKind : int { STR_STARTS_WITH = 0, STR_ENDS_WITH = 1, STR_CONTAINS = 2, STR_LIKE = 3, STR_EQUALS = 4 };
enum StrLenUnit : int { STR_LEN_BYTES = 0, STR_LEN_CHARS = 1 };

// compiled LIKE pattern: ntok tokens, kind[i] one of these, lit[i] the byte of a TOK_LIT
enum StrTok : uint8_t { TOK_LIT = 0, TOK_ONE = 1, TOK_ANY = 2 };

struct StrPattern {
  int32_t ntok = 0;
  uint8_t kind[kStrMaxPatternBytes];
  uint8_t lit[kStrMaxPatternBytes];
};

CYLON_HD bool sm_is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// a position where a unit of a STRING cell may begin or end: the cell's ends and every byte that
// is no continuation byte.  utf8 == 0 (BINARY): every position.
CYLON_HD bool sm_boundary(const uint8_t *s, int64_t n, int64_t i, int utf8) {
  return !utf8 || i <= 0 || i >= n || !sm_is_cont(s[i]);
}

// <0, 0, >0: unsigned bytes, lexicographic, a proper prefix is smaller
CYLON_HD int sm_compare(const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb) {
  const int64_t m = na < nb ? na : nb;
  for (int64_t i = 0; i < m; ++i) {
    const int d = (int)a[i] - (int)b[i];
    if (d != 0) return d;
  }
  return na < nb ? -1 : (na > nb ? 1 : 0);
}

CYLON_HD bool sm_cmp_result(int c, int op) {
  switch (op) {
    case STR_EQ: return c == 0;
    case STR_NE: return c != 0;
    case STR_LT: return c < 0;
    case STR_LE: return c <= 0;
    case STR_GT: return c > 0;
    default: return c >= 0;
  }
}

CYLON_HD bool sm_bytes_equal(const uint8_t *s, const uint8_t *p, int64_t np) {
  for (int64_t i = 0; i < np; ++i)
    if (s[i] != p[i]) return false;
  return true;
}

// utf8 != 0 (a LIKE pattern over a STRING cell): the match must begin and end at unit boundaries
CYLON_HD bool sm_starts_with(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, int utf8) {
  return np <= n && sm_bytes_equal(s, p, np) && sm_boundary(s, n, np, utf8);
}

CYLON_HD bool sm_ends_with(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, int utf8) {
  return np <= n && sm_bytes_equal(s + (n - np), p, np) && sm_boundary(s, n, n - np, utf8);
}

CYLON_HD bool sm_equals(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np) {
  return np == n && sm_bytes_equal(s, p, np);
}

// does p occur at position i of the cell (i + np <= n is the caller's)
CYLON_HD bool sm_match_at(const uint8_t *s, int64_t n, int64_t i, const uint8_t *p, int64_t np, int utf8) {
  return sm_bytes_equal(s + i, p, np) && sm_boundary(s, n, i, utf8) && sm_boundary(s, n, i + np, utf8);
}

CYLON_HD bool sm_contains(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np, int utf8) {
  for (int64_t i = 0; i + np <= n; ++i)
    if (sm_match_at(s, n, i, p, np, utf8)) return true;
  return false;
}

// code points: the bytes that are no continuation bytes
CYLON_HD int64_t sm_count_chars(const uint8_t *s, int64_t n) {
  int64_t c = 0;
  for (int64_t i = 0; i < n; ++i) c += sm_is_cont(s[i]) ? 0 : 1;
  return c;
}

// the end of the unit that begins at i < n
CYLON_HD int64_t sm_unit_end(const uint8_t *s, int64_t n, int64_t i, int utf8) {
  ++i;
  if (utf8)
    while (i < n && sm_is_cont(s[i])) ++i;
  return i;
}

// SQL LIKE anchored at both ends: the iterative two-pointer glob match.  It remembers the last
// TOK_ANY and, on a mismatch, resumes one unit later; a wildcard may begin only at a unit boundary.
CYLON_HD bool sm_like(const uint8_t *s, int64_t n, const uint8_t *kind, const uint8_t *lit, int ntok, int utf8) {
  int64_t i = 0, star_i = 0;
  int p = 0, star_p = -1;
  for (;;) {
    if (p < ntok) {
      const uint8_t k = kind[p];
      if (k == TOK_ANY) {
        if (sm_boundary(s, n, i, utf8)) {
          star_p = p++;
          star_i = i;
          continue;
        }
      } else if (i < n) {
        if (k == TOK_LIT) {
          if (s[i] == lit[p]) {
            ++i;
            ++p;
            continue;
          }
        } else if (sm_boundary(s, n, i, utf8)) {
          i = sm_unit_end(s, n, i, utf8);
          ++p;
          continue;
        }
      }
    } else if (i == n) {
      return true;
    }
    if (star_p < 0 || star_i >= n) return false;
    star_i = sm_unit_end(s, n, star_i, utf8);
    i = star_i;
    p = star_p + 1;
  }
}

}  // namespace strmatch
}  // namespace cylon
