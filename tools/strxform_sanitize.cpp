// Host sanitizer check of the CPU twin of the string transforms (kernels/cpu_strxform.cpp) and of the
// shared cell functions (kernels/strxform_common.hpp): slice, strip, case, concat and replace over
// columns whose bytes, offsets and validity live in exactly-sized heap buffers -- the inputs and, sized
// by the lengths pass, the outputs -- against brute-force versions written here.  The shapes are the
// adversarial ones of the GPU tests: a pattern that would match only by reading into the next row or
// past the buffer's end, matches at the very end of a row, overlapping matches, empty rows, null rows
// over garbage that would match / strip / change case, multi-byte and malformed UTF-8, offsets that do
// not begin at 0.  Any read or write past a buffer is an AddressSanitizer report.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/strxform_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_strxform.cpp -o strxform_sanitize
//   ./strxform_sanitize          # prints "strxform_sanitize: ok", exit status 0
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cylon/kernels/kernels.hpp"
#include "cylon/kernels/strxform_common.hpp"
#include "cylon/types.hpp"

namespace {

using namespace cylon;
using namespace cylon::strxform;
using Cell = std::string;

int failures = 0;

void expect(bool ok, const char *what, const std::string &detail) {
  if (ok) return;
  if (++failures <= 20) std::fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

// a column in heap buffers of exactly the needed size (no slack for an over-read to hide in); `skip`
// leading rows belong to the buffers but not to the column, so that its offsets begin past 0
struct Col {
  std::unique_ptr<uint8_t[]> bytes, valid;
  std::unique_ptr<int64_t[]> offs;
  int64_t n = 0;
  ColView view{};
};

Col make_col(const std::vector<Cell> &rows, const std::vector<bool> &null, size_t skip = 0) {
  Col c;
  c.n = (int64_t)(rows.size() - skip);
  size_t total = 0;
  for (auto &r : rows) total += r.size();
  if (total) c.bytes.reset(new uint8_t[total]);
  c.offs.reset(new int64_t[rows.size() + 1]);
  size_t pos = 0;
  for (size_t i = 0; i < rows.size(); ++i) {
    c.offs[i] = (int64_t)pos;
    if (!rows[i].empty()) std::memcpy(c.bytes.get() + pos, rows[i].data(), rows[i].size());
    pos += rows[i].size();
  }
  c.offs[rows.size()] = (int64_t)pos;
  bool any = false;
  for (bool b : null) any |= b;
  if (any) {
    c.valid.reset(new uint8_t[rows.size()]);
    for (size_t i = 0; i < rows.size(); ++i) c.valid[i] = null[i] ? 0 : 1;
  }
  c.view.data = c.bytes.get();
  c.view.offsets = c.offs.get() + skip;
  c.view.valid = any ? c.valid.get() + skip : nullptr;
  c.view.kind = static_cast<int>(ValueKind::VAR_BYTES);
  return c;
}

// ---- brute force -------------------------------------------------------------------------------
bool cont(unsigned char b) { return b >= 0x80 && b <= 0xBF; }

std::vector<Cell> units(const Cell &s, bool utf8) {
  std::vector<Cell> u;
  for (size_t i = 0; i < s.size(); ++i) {
    if (utf8 && !u.empty() && cont((unsigned char)s[i])) u.back().push_back(s[i]);
    else u.emplace_back(1, s[i]);
  }
  return u;
}

Cell brute_slice(const Cell &s, long start, long stop, bool has_stop, bool utf8) {
  const std::vector<Cell> u = units(s, utf8);
  const long n = (long)u.size();
  long b = start < 0 ? start + n : start, e = !has_stop ? n : (stop < 0 ? stop + n : stop);
  b = b < 0 ? 0 : (b > n ? n : b);
  e = e < 0 ? 0 : (e > n ? n : e);
  Cell out;
  for (long i = b; i < e; ++i) out += u[(size_t)i];
  return out;
}

Cell brute_strip(Cell s, int side, const Cell &set) {
  if (side & SX_LEFT)
    while (!s.empty() && set.find(s.front()) != Cell::npos) s.erase(s.begin());
  if (side & SX_RIGHT)
    while (!s.empty() && set.find(s.back()) != Cell::npos) s.pop_back();
  return s;
}

Cell brute_case(Cell s, bool upper) {
  for (auto &ch : s) {
    if (upper && ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
    else if (!upper && ch >= 'A' && ch <= 'Z') ch = (char)(ch - 'A' + 'a');
  }
  return s;
}

Cell brute_replace(const Cell &s, const Cell &p, const Cell &r, long max_repl) {
  Cell out;
  size_t pos = 0;
  long c = 0;
  for (;;) {
    const size_t hit = (max_repl < 0 || c < max_repl) ? s.find(p, pos) : Cell::npos;
    if (hit == Cell::npos) break;
    out.append(s, pos, hit - pos);
    out += r;
    pos = hit + p.size();
    ++c;
  }
  out.append(s, pos, Cell::npos);
  return out;
}

// ---- the engine's side: lengths, the scan, an output buffer of exactly the total, the write ----
struct Out {
  std::vector<Cell> rows;
  bool flag = false;
};

Out run(const Col &a, const Col *b, const StrXform &x, const Cell &lit, int64_t n) {
  std::unique_ptr<uint8_t[]> dlit;
  if (!lit.empty()) {
    dlit.reset(new uint8_t[lit.size()]);
    std::memcpy(dlit.get(), lit.data(), lit.size());
  }
  std::unique_ptr<int64_t[]> lens(new int64_t[n ? n : 1]), offs(new int64_t[n + 1]);
  const ColView bv = b ? b->view : ColView{};
  cpu::strx_lengths(a.view, bv, x, dlit.get(), n, lens.get(), nullptr);
  offs[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    expect(lens[i] >= 0, "length", "negative");
    offs[i + 1] = offs[i] + lens[i];
  }
  std::unique_ptr<uint8_t[]> bytes;
  if (offs[n]) bytes.reset(new uint8_t[offs[n]]);
  uint32_t flag = 0;
  cpu::strx_write(a.view, bv, x, dlit.get(), n, offs.get(), bytes.get(), x.fn == SX_CASE ? &flag : nullptr, nullptr);
  Out o;
  o.flag = flag != 0;
  for (int64_t i = 0; i < n; ++i)
    o.rows.emplace_back(reinterpret_cast<const char *>(bytes.get()) + offs[i], (size_t)lens[i]);
  return o;
}

void check_rows(const Out &got, const std::vector<Cell> &want, const char *what, const std::string &detail) {
  expect(got.rows.size() == want.size(), what, detail + ": row count");
  for (size_t i = 0; i < want.size() && i < got.rows.size(); ++i)
    expect(got.rows[i] == want[i], what, detail + " row " + std::to_string(i) + " got '" + got.rows[i] + "' want '" +
                                             want[i] + "'");
}

Cell bitmap_of(const Cell &set) {
  Cell bm(kStrSetBytes, '\0');
  for (unsigned char c : set) bm[c >> 3] = (char)((unsigned char)bm[c >> 3] | (1u << (c & 7)));
  return bm;
}

void run_all(const std::vector<Cell> &all_rows, const std::vector<bool> &all_null, size_t skip = 0) {
  const Col c = make_col(all_rows, all_null, skip);
  const std::vector<Cell> rows(all_rows.begin() + (long)skip, all_rows.end());
  const std::vector<bool> null(all_null.begin() + (long)skip, all_null.end());
  const int64_t n = c.n;
  auto map = [&](auto fn) {
    std::vector<Cell> w;
    for (size_t i = 0; i < rows.size(); ++i) w.push_back(null[i] ? Cell() : fn(rows[i]));
    return w;
  };
  // slice
  const long idx[] = {0, 1, 2, 3, 5, 100, -1, -2, -3, -5, -100};
  for (int utf8 = 0; utf8 < 2; ++utf8)
    for (long start : idx)
      for (int has_stop = 0; has_stop < 2; ++has_stop)
        for (long stop : idx) {
          if (!has_stop && stop != 0) continue;
          StrXform x;
          x.fn = SX_SLICE, x.utf8 = utf8, x.start = start, x.stop = stop, x.has_stop = has_stop;
          check_rows(run(c, nullptr, x, Cell(), n), map([&](const Cell &s) {
                       return brute_slice(s, start, stop, has_stop != 0, utf8 != 0);
                     }), "slice", std::to_string(start) + ":" + (has_stop ? std::to_string(stop) : "") +
                                      (utf8 ? " utf8" : " bytes"));
        }
  // strip
  for (const Cell &set : {Cell(" \t\n\v\f\r"), Cell("ab"), Cell("a"), Cell("\x80\xFF", 2), Cell()})
    for (int side = SX_LEFT; side <= SX_BOTH; ++side) {
      StrXform x;
      x.fn = SX_STRIP, x.side = side;
      check_rows(run(c, nullptr, x, bitmap_of(set), n), map([&](const Cell &s) { return brute_strip(s, side, set); }),
                 "strip", "side " + std::to_string(side) + " set '" + set + "'");
    }
  // case, and the non-ASCII flag
  bool high = false;
  for (size_t i = 0; i < rows.size(); ++i)
    if (!null[i])
      for (unsigned char ch : rows[i]) high |= ch >= 0x80;
  for (int upper = 0; upper < 2; ++upper) {
    StrXform x;
    x.fn = SX_CASE, x.upper = upper;
    const Out got = run(c, nullptr, x, Cell(), n);
    check_rows(got, map([&](const Cell &s) { return brute_case(s, upper != 0); }), "case", upper ? "upper" : "lower");
    expect(got.flag == high, "case", "non-ASCII flag");
    bool any_null = false;
    for (bool b : null) any_null |= b;
    if (!any_null) {  // the flat form: no validity
      std::unique_ptr<int64_t[]> offs(new int64_t[n + 1]);
      const int64_t total = c.view.offsets[n] - c.view.offsets[0];
      std::unique_ptr<uint8_t[]> bytes;
      if (total) bytes.reset(new uint8_t[total]);
      uint32_t flag = 0;
      ColView v = c.view;
      v.valid = nullptr;
      cpu::strx_case_flat(v, upper, n, total, offs.get(), bytes.get(), &flag, nullptr);
      Out flat;
      for (int64_t i = 0; i < n; ++i)
        flat.rows.emplace_back(reinterpret_cast<const char *>(bytes.get()) + offs[i], (size_t)(offs[i + 1] - offs[i]));
      expect(offs[0] == 0 && (flag != 0) == high, "case flat", "offsets[0] / flag");
      check_rows(flat, map([&](const Cell &s) { return brute_case(s, upper != 0); }), "case flat", upper ? "upper" : "lower");
    }
  }
  // replace
  for (const Cell &p : {Cell("a"), Cell("ab"), Cell("aa"), Cell("abab"), Cell("bc"), Cell("\xC3\xA9"), Cell("\x80", 1)})
    for (const Cell &r : {Cell(), Cell("x"), Cell("ab"), Cell("abcabc"), Cell("aaaa")})
      for (long max_repl : {-1L, 0L, 1L, 2L}) {
        StrXform x;
        x.fn = SX_REPLACE, x.len1 = (int32_t)p.size(), x.len2 = (int32_t)r.size(), x.max_repl = max_repl;
        check_rows(run(c, nullptr, x, p + r, n), map([&](const Cell &s) { return brute_replace(s, p, r, max_repl); }),
                   "replace", "'" + p + "' -> '" + r + "' max " + std::to_string(max_repl));
      }
  // concat: with the rows rotated by one, and with a one-row scalar on either side
  std::vector<Cell> rot(rows.begin() + (rows.empty() ? 0 : 1), rows.end());
  std::vector<bool> rnull(null.begin() + (rows.empty() ? 0 : 1), null.end());
  if (!rows.empty()) rot.push_back(rows[0]), rnull.push_back(null[0]);
  const Col b = make_col(rot, rnull);
  for (const Cell &sep : {Cell(), Cell("--")}) {
    StrXform x;
    x.fn = SX_CONCAT, x.len1 = (int32_t)sep.size();
    std::vector<Cell> want;
    for (size_t i = 0; i < rows.size(); ++i) want.push_back(null[i] || rnull[i] ? Cell() : rows[i] + sep + rot[i]);
    check_rows(run(c, &b, x, sep, n), want, "concat", "columns, sep '" + sep + "'");
    if (n > 1) {
      const Col one = make_col({"<->"}, {false});
      x.b_bcast = 1;
      check_rows(run(c, &one, x, sep, n), map([&](const Cell &s) { return s + sep + "<->"; }), "concat", "scalar right");
      x.b_bcast = 0, x.a_bcast = 1;
      // the broadcast operand carries no validity; the column's (now b's) decides
      std::vector<Cell> w;
      for (size_t i = 0; i < rows.size(); ++i) w.push_back(null[i] ? Cell() : "<->" + sep + rows[i]);
      check_rows(run(one, &c, x, sep, n), w, "concat", "scalar left");
    }
  }
}

}  // namespace

int main() {
  // the case map of a word against the case map of a byte, every byte value in every lane
  for (int upper = 0; upper < 2; ++upper)
    for (uint32_t b = 0; b < 256; ++b)
      for (int lane = 0; lane < 4; ++lane) {
        const uint32_t others = 0x61417a5au;  // a A z Z around it
        const uint32_t w = (others & ~(0xffu << (8 * lane))) | (b << (8 * lane));
        uint32_t want = 0;
        for (int k = 0; k < 4; ++k) want |= (uint32_t)sx_case((uint8_t)(w >> (8 * k)), upper) << (8 * k);
        expect(sx_case_word(w, upper) == want, "case word", std::to_string(b));
      }
  // the fixed adversarial shapes
  run_all({}, {});
  run_all({"ab", "cd"}, {false, false});
  run_all({"", "", ""}, {false, false, false});
  run_all({" ab "}, {true});  // one null row over garbage
  run_all({"abab", " ab", "abc ", "", "xab", "b", "AbC", "aaa", "ababab"},
          {true, false, true, false, false, true, false, false, false});
  run_all({"\xC3\xA9", "\xE6\x97\xA5\xE6\x9C\xAC", "a\xC3\xA9\xF0\x9D\x84\x9E", "\x80", "a\x80", "a\x80" "b", "\xE6\x97",
           "\xFF\xFE", "\x80\x80" "a", " \xC3\xA9 "},
          std::vector<bool>(10, false));
  run_all({" abAB ", "ab", " ab", "ab ", "", "a"}, {false, false, true, false, false, false}, 2);  // offsets[0] != 0
  {  // a long row whose only match is its last bytes, followed by a row that would complete a pattern
    Cell big(3000, 'x');
    big += "a";
    run_all({"b", big, "b", Cell(64, 'a'), "a", Cell(300, ' ')}, std::vector<bool>(6, false));
  }
  // random cells over letters, blanks, a 2-byte code point and a stray continuation byte; every 7th row
  // null over garbage
  std::mt19937 rng(17);
  for (int round = 0; round < 25; ++round) {
    std::vector<Cell> rows;
    std::vector<bool> null;
    const int n = 1 + (int)(rng() % 40);
    for (int i = 0; i < n; ++i) {
      Cell s;
      const int len = (int)(rng() % 13);
      for (int k = 0; k < len; ++k) {
        const unsigned r = rng() % 10;
        if (r == 9) s += "\xC3\xA9";
        else if (r == 8) s.push_back((char)0x80);
        else s.push_back("abcAB  \t"[r]);
      }
      rows.push_back(s);
      null.push_back(rng() % 7 == 0);
    }
    run_all(rows, null, round % 3 == 0 ? 1 : 0);
  }
  if (failures) {
    std::fprintf(stderr, "strxform_sanitize: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("strxform_sanitize: ok\n");
  return 0;
}
