// What kernels/frame_range.hip and its CPU twin (cpu_frame_range.cpp) share, so that they agree by
// construction (docs/semantics.md "Framed aggregates", RANGE): the search key of an order value, the
// bound of a frame in key space, the operators, the pyramid's geometry and the query that reads an
// aggregate off it.
//
// Keys.  A number's key is a 64-bit image whose unsigned order is the column's sort order: integers
// (and temporal values) as value - INT64_MIN resp. the value itself, floats as the order image of the
// value widened to float64 (-0.0 == +0.0); a descending column takes the complement.  NaN and null
// keys are 0 with class 1 resp. 2, so (class, key) never decreases along a partition.
//   integer keys   the key is the value up to a shift, so key -/+ distance, saturating at 0 / 2^64 - 1,
//                  is the bound as a mathematical integer: nothing wraps
//   float keys     the bound is one float64 operation on the value; inf - inf (NaN) is replaced by
//                  the value itself, which leaves a +-inf row its peers
// A NaN or null row's frame is its class: both bounds are (class, 0).
//
// Pyramid of n level-0 entries.  Level l has n_l entries, n_0 = n, n_(l+1) = ceil(n_l / 8); a level with
// more than 8 entries stores P and S in fr_cap(n_l) slots each (the levels back to back), every level
// above 0 its entries E (likewise back to back, level 1 first).  The last level has at most 8 entries
// and is only ever combined serially.
#pragma once
#include <cstdint>

#include "../types.hpp"
#include "order_image.hpp"

namespace cylon {

constexpr int kFrRadix = 8;     // entries per pyramid block
constexpr int kFrShift = 3;     // log2(kFrRadix)
constexpr int kFrHalo = 1024;   // keys staged on either side of a bounds tile (a multiple of 8)

enum : int { FR_NUMBER = 0, FR_NAN = 1, FR_NULL = 2 };        // key classes
enum : int { FR_UNBOUNDED = 0, FR_INT = 1, FR_FLOAT = 2 };    // a side's offset
enum : int { FR_SUM_I = 0, FR_SUM_F = 1, FR_MIN = 2, FR_MAX = 3, FR_COUNT = 4 };  // = window.hip WinFunc

struct FrFrame {  // one (preceding, following) of a call
  int pre_mode, fol_mode;
  uint64_t pre_i, fol_i;
  double pre_f, fol_f;
  int float_keys, desc;
};

CYLON_HD double fr_bits_f64(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, 8);
  return d;
}

CYLON_HD uint64_t fr_f64_bits(double d) {
  uint64_t b;
  __builtin_memcpy(&b, &d, 8);
  return b;
}

CYLON_HD double fr_widen_float(uint64_t bits, int w) {
  if (w == 8) return fr_bits_f64(bits);
  const uint32_t u = (uint32_t)bits;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return (double)f;
}

CYLON_HD int64_t fr_sign_extend(uint64_t b, int w) {
  return w == 1 ? (int64_t)(int8_t)b : w == 2 ? (int64_t)(int16_t)b : w == 4 ? (int64_t)(int32_t)b : (int64_t)b;
}

// ---------------------------------------------------------------------------
// keys and bounds
// ---------------------------------------------------------------------------
// w: 1, 2, 4, 8 (floats 4, 8); kind: SIGNED_INT, UNSIGNED_INT or FLOAT
CYLON_HD void fr_key(uint64_t bits, bool live, int w, int kind, bool desc, uint64_t *key, uint8_t *cls) {
  *key = 0;
  if (!live) {
    *cls = FR_NULL;
    return;
  }
  uint64_t u;
  if (kind == static_cast<int>(ValueKind::FLOAT)) {
    const double d = fr_widen_float(bits, w);
    if (d != d) {
      *cls = FR_NAN;
      return;
    }
    u = order_image(fr_f64_bits(d), 8, kind);
  } else if (kind == static_cast<int>(ValueKind::SIGNED_INT)) {
    u = (uint64_t)fr_sign_extend(bits, w) ^ (1ull << 63);
  } else {
    u = w == 8 ? bits : (bits & ((1ull << (8 * w)) - 1));
  }
  *cls = FR_NUMBER;
  *key = desc ? ~u : u;
}

// The key bound of a number's frame on its `upper` (following) or lower (preceding) side; mode is
// FR_INT or FR_FLOAT.  Never above the key on the lower side nor below it on the upper side.
CYLON_HD uint64_t fr_bound(uint64_t key, bool upper, const FrFrame &fr) {
  if (!fr.float_keys) {
    const uint64_t d = upper ? fr.fol_i : fr.pre_i;
    if (upper) return key + d < key ? ~0ull : key + d;
    return key < d ? 0ull : key - d;
  }
  const int kind = static_cast<int>(ValueKind::FLOAT);
  const double v = fr_bits_f64(order_unimage(fr.desc ? ~key : key, 8, kind));
  const double d = upper ? fr.fol_f : fr.pre_f;
  // towards smaller keys the value falls in an ascending column and rises in a descending one
  double t = (upper == (fr.desc != 0)) ? v - d : v + d;
  if (t != t) t = v;  // inf - inf
  const uint64_t img = order_image(fr_f64_bits(t), 8, kind);
  return fr.desc ? ~img : img;
}

// (c1, k1) >= (c2, k2)
CYLON_HD bool fr_ge(uint8_t c1, uint64_t k1, uint8_t c2, uint64_t k2) { return c1 > c2 || (c1 == c2 && k1 >= k2); }

// ---------------------------------------------------------------------------
// operators: func is a constant in the device templates
// ---------------------------------------------------------------------------
CYLON_HD uint64_t fr_identity(int func) { return func == FR_MIN ? ~0ull : 0ull; }

CYLON_HD uint64_t fr_op(int func, uint64_t x, uint64_t y) {
  if (func == FR_SUM_F) return fr_f64_bits(fr_bits_f64(x) + fr_bits_f64(y));
  if (func == FR_MIN) return x < y ? x : y;
  if (func == FR_MAX) return x > y ? x : y;
  return x + y;
}

// raw column bits -> a level-0 entry; a null value is the operator's identity
CYLON_HD uint64_t fr_entry0(int func, uint64_t bits, bool live, int w, int kind) {
  if (!live) return fr_identity(func);
  if (func == FR_COUNT) return 1;
  if (func == FR_SUM_I)
    return kind == static_cast<int>(ValueKind::SIGNED_INT) ? (uint64_t)fr_sign_extend(bits, w) : bits;
  if (func == FR_SUM_F) return fr_f64_bits(fr_widen_float(bits, w));
  return order_image(bits, w, kind);
}

// ---------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------
CYLON_HD int64_t fr_cap(int64_t n) { return (n + kFrRadix - 1) & ~(int64_t)(kFrRadix - 1); }
CYLON_HD int64_t fr_up(int64_t n) { return (n + kFrRadix - 1) >> kFrShift; }

// words of P (and of S): the levels with more than one block
CYLON_HD int64_t fr_ps_slots(int64_t n) {
  int64_t s = 0;
  for (; n > kFrRadix; n = fr_up(n)) s += fr_cap(n);
  return s;
}

// words of E: every level above 0
CYLON_HD int64_t fr_e_slots(int64_t n) {
  int64_t s = 0;
  while (n > kFrRadix) {
    n = fr_up(n);
    s += fr_cap(n);
  }
  return s;
}

// ---------------------------------------------------------------------------
// the query
// ---------------------------------------------------------------------------
struct FrPyramid {
  const uint64_t *P, *S, *E;
  // level 0: the dense column
  const uint64_t *dense;
  const uint8_t *dvalid;  // nullptr: no nulls
  int w, kind;
};

CYLON_HD uint64_t fr_level0(int func, const FrPyramid &p, int64_t j) {
  return fr_entry0(func, p.dense[j], p.dvalid == nullptr || p.dvalid[j] != 0, p.w, p.kind);
}

// entries lo .. hi (0 <= lo <= hi < n) of level 0 combined, left to right, each exactly once: per level
// S[lo] and P[hi] while the two lie in different blocks, then the blocks strictly between them one
// level up; a run inside one block is combined entry by entry
CYLON_HD uint64_t fr_query(int func, const FrPyramid &p, int64_t n, int64_t lo, int64_t hi) {
  uint64_t left = fr_identity(func), right = fr_identity(func), mid = fr_identity(func);
  int64_t nl = n, ps = 0, e = 0;  // this level's entries, its offset in P / S, and (above level 0) in E
  bool level0 = true;
  for (;;) {
    if ((lo >> kFrShift) == (hi >> kFrShift)) {
      for (int64_t j = lo; j <= hi; ++j) mid = fr_op(func, mid, level0 ? fr_level0(func, p, j) : p.E[e + j]);
      break;
    }
    left = fr_op(func, left, p.S[ps + lo]);
    right = fr_op(func, p.P[ps + hi], right);
    lo = (lo >> kFrShift) + 1;
    hi = (hi >> kFrShift) - 1;
    if (lo > hi) break;
    ps += fr_cap(nl);
    if (!level0) e += fr_cap(nl);
    nl = fr_up(nl);
    level0 = false;
  }
  return fr_op(func, fr_op(func, left, mid), right);
}

// one block of level `l`: in[0 .. cnt) are its entries (cnt <= 8); P and S get 8 slots each
CYLON_HD uint64_t fr_block(int func, const uint64_t *in, int cnt, uint64_t *P, uint64_t *S) {
  uint64_t acc = fr_identity(func);
  for (int k = 0; k < kFrRadix; ++k) {
    if (k < cnt) acc = fr_op(func, acc, in[k]);
    P[k] = acc;
  }
  const uint64_t total = acc;
  acc = fr_identity(func);
  for (int k = kFrRadix - 1; k >= 0; --k) {
    if (k < cnt) acc = fr_op(func, in[k], acc);
    S[k] = acc;
  }
  return total;
}

}  // namespace cylon
