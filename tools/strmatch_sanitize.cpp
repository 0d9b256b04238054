// Host sanitizer check of the CPU twin of the string predicates (kernels/cpu_strings.cpp) and of the
// shared cell matchers (kernels/strmatch_common.hpp): comparison, starts_with / ends_with / contains,
// LIKE and length over columns whose bytes, offsets and validity live in exactly-sized heap buffers,
// against brute-force matchers written here.  The shapes are the adversarial ones of the GPU tests:
// a needle that would match only by reading into the next row or past the buffer's end, needles at the
// very end of a row, empty rows, null rows over matching garbage, multi-byte and malformed UTF-8.
// Any read past a row's buffer is an AddressSanitizer report.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/strmatch_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_strings.cpp -o strmatch_sanitize
//   ./strmatch_sanitize          # prints "strmatch_sanitize: ok", exit status 0
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cylon/kernels/kernels.hpp"
#include "cylon/kernels/strmatch_common.hpp"
#include "cylon/types.hpp"

namespace {

using namespace cylon;
using namespace cylon::strmatch;
using Cell = std::string;

int failures = 0;

void expect(bool ok, const char *what, const std::string &detail) {
  if (ok) return;
  if (++failures <= 20) std::fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

// a column in heap buffers of exactly the needed size (no slack for an over-read to hide in)
struct Col {
  std::unique_ptr<uint8_t[]> bytes, valid;
  std::unique_ptr<int64_t[]> offs;
  int64_t n = 0;
  ColView view{};
};

// null[i]: row i is null, its bytes (kept, as garbage) must never be read
Col make_col(const std::vector<Cell> &rows, const std::vector<bool> &null) {
  Col c;
  c.n = (int64_t)rows.size();
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
  c.view.offsets = c.offs.get();
  c.view.valid = c.valid.get();
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

struct Tok {
  int kind;  // 0 literal unit, 1 one, 2 any
  Cell lit;
};

std::vector<Tok> tokens(const Cell &p, char esc, bool utf8) {
  std::vector<Tok> t;
  Cell run;
  auto flush = [&] {
    for (auto &u : units(run, utf8)) t.push_back({0, u});
    run.clear();
  };
  for (size_t i = 0; i < p.size(); ++i) {
    if (p[i] == esc) {
      run.push_back(p[++i]);
    } else if (p[i] == '%' || p[i] == '_') {
      flush();
      t.push_back({p[i] == '%' ? 2 : 1, Cell()});
    } else {
      run.push_back(p[i]);
    }
  }
  flush();
  return t;
}

bool like_rec(const std::vector<Cell> &u, size_t ui, const std::vector<Tok> &t, size_t ti) {
  if (ti == t.size()) return ui == u.size();
  if (t[ti].kind == 2) {
    for (size_t k = ui; k <= u.size(); ++k)
      if (like_rec(u, k, t, ti + 1)) return true;
    return false;
  }
  if (ui >= u.size()) return false;
  if (t[ti].kind == 0 && u[ui] != t[ti].lit) return false;
  return like_rec(u, ui + 1, t, ti + 1);
}

bool brute_match(const Cell &s, int kind, const Cell &p, bool utf8) {
  switch (kind) {
    case STR_STARTS_WITH: return s.size() >= p.size() && s.compare(0, p.size(), p) == 0;
    case STR_ENDS_WITH: return s.size() >= p.size() && s.compare(s.size() - p.size(), p.size(), p) == 0;
    case STR_CONTAINS: return s.find(p) != Cell::npos;
    default: return like_rec(units(s, utf8), 0, tokens(p, '\\', utf8), 0);
  }
}

int brute_cmp(const Cell &a, const Cell &b) {
  const size_t m = a.size() < b.size() ? a.size() : b.size();
  for (size_t i = 0; i < m; ++i)
    if (a[i] != b[i]) return (unsigned char)a[i] < (unsigned char)b[i] ? -1 : 1;
  return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

// ---- the engine's side: what ops/strings.cpp does with a LIKE pattern, without the classification ----
std::vector<uint8_t> compile(const Cell &p, int *ntok) {
  std::vector<uint8_t> kind, lit;
  for (size_t i = 0; i < p.size(); ++i) {
    uint8_t k = TOK_LIT, l = (uint8_t)p[i];
    if (p[i] == '\\') l = (uint8_t)p[++i];
    else if (p[i] == '%') k = TOK_ANY;
    else if (p[i] == '_') k = TOK_ONE;
    if (k == TOK_ANY && !kind.empty() && kind.back() == TOK_ANY) continue;
    kind.push_back(k);
    lit.push_back(k == TOK_LIT ? l : 0);
  }
  *ntok = (int)kind.size();
  kind.insert(kind.end(), lit.begin(), lit.end());
  return kind;
}

void run_match(const std::vector<Cell> &rows, const std::vector<bool> &null, int kind, const Cell &p, bool utf8) {
  Col c = make_col(rows, null);
  std::unique_ptr<uint8_t[]> out(new uint8_t[rows.size() ? rows.size() : 1]);
  std::unique_ptr<uint8_t[]> pat;
  int64_t plen = (int64_t)p.size();
  if (kind == STR_LIKE) {
    int nt = 0;
    std::vector<uint8_t> buf = compile(p, &nt);
    if (!buf.empty()) {
      pat.reset(new uint8_t[buf.size()]);
      std::memcpy(pat.get(), buf.data(), buf.size());
    }
    plen = nt;
  } else if (plen) {
    pat.reset(new uint8_t[p.size()]);
    std::memcpy(pat.get(), p.data(), p.size());
  }
  const int u = kind == STR_LIKE && utf8 ? 1 : 0;
  cpu::str_match(c.view, kind, pat.get(), plen, u, c.n, out.get(), nullptr);
  for (size_t i = 0; i < rows.size(); ++i) {
    const bool want = !null[i] && brute_match(rows[i], kind, p, utf8);
    expect(out[i] == (want ? 1 : 0), "match", "kind " + std::to_string(kind) + " pattern '" + p + "' row " +
                                                  std::to_string(i) + " '" + rows[i] + "'");
  }
}

void run_all(const std::vector<Cell> &rows, const std::vector<bool> &null, const std::vector<Cell> &needles,
             const std::vector<Cell> &likes) {
  for (auto &p : needles)
    for (int kind : {STR_STARTS_WITH, STR_ENDS_WITH, STR_CONTAINS}) run_match(rows, null, kind, p, false);
  for (auto &p : likes)
    for (bool utf8 : {true, false}) run_match(rows, null, STR_LIKE, p, utf8);
  // lengths
  Col c = make_col(rows, null);
  std::unique_ptr<int64_t[]> len(new int64_t[rows.size() ? rows.size() : 1]);
  for (int unit : {STR_LEN_BYTES, STR_LEN_CHARS}) {
    cpu::str_length(c.view, unit, c.n, len.get(), nullptr);
    for (size_t i = 0; i < rows.size(); ++i) {
      int64_t want = 0;
      if (!null[i]) want = unit == STR_LEN_BYTES ? (int64_t)rows[i].size() : (int64_t)units(rows[i], true).size();
      // a cell that begins with continuation bytes: they are one unit but no code point
      if (!null[i] && unit == STR_LEN_CHARS && !rows[i].empty() && cont((unsigned char)rows[i][0])) --want;
      expect(len[i] == want, "length", "row " + std::to_string(i));
    }
  }
  // comparison: with the rows rotated by one, and with each needle as a one-row scalar column
  std::vector<Cell> rot(rows.begin() + (rows.empty() ? 0 : 1), rows.end());
  std::vector<bool> rnull(null.begin() + (rows.empty() ? 0 : 1), null.end());
  if (!rows.empty()) rot.push_back(rows[0]), rnull.push_back(null[0]);
  Col b = make_col(rot, rnull);
  std::unique_ptr<uint8_t[]> out(new uint8_t[rows.size() ? rows.size() : 1]);
  for (int op = STR_EQ; op <= STR_GE; ++op) {
    cpu::str_compare(c.view, b.view, 0, op, c.n, out.get(), nullptr);
    for (size_t i = 0; i < rows.size(); ++i) {
      const bool want = !null[i] && !rnull[i] && sm_cmp_result(brute_cmp(rows[i], rot[i]), op);
      expect(out[i] == (want ? 1 : 0), "compare", "op " + std::to_string(op) + " row " + std::to_string(i));
    }
    for (auto &p : needles) {
      Col s = make_col({p}, {false});
      cpu::str_compare(c.view, s.view, 1, op, c.n, out.get(), nullptr);
      for (size_t i = 0; i < rows.size(); ++i) {
        const bool want = !null[i] && sm_cmp_result(brute_cmp(rows[i], p), op);
        expect(out[i] == (want ? 1 : 0), "compare scalar", "op " + std::to_string(op) + " row " + std::to_string(i));
      }
    }
  }
}

}  // namespace

int main() {
  const std::vector<Cell> needles = {"", "a", "b", "ab", "bc", "abc", "cab", Cell(65, 'a'), "\xC3\xA9", "\x80", "\xFF"};
  const std::vector<Cell> likes = {"", "%", "%%", "_", "__", "_%_", "a%b%c", "%__", "a%", "%b", "%ab%", "a\\%b", "a\\_b",
                                   "a\\\\b", "%a_", "_%b", "%\xC3\xA9", "\xC3_", "%\x80", "__%__", "%c%ab", "a%%b"};
  // the fixed adversarial shapes
  run_all({}, {}, needles, likes);
  run_all({"ab", "cd"}, {false, false}, {"bc", "abc", "bcd", "d", "cd"}, {"%bc%", "ab_", "%cd", "_bcd", "ab%c%"});
  run_all({"", "", ""}, {false, false, false}, needles, likes);
  run_all({"ab"}, {true}, needles, likes);  // one null row over matching garbage
  run_all({"abab", "ab", "abc", "", "xab", "b"}, {true, false, true, false, false, true}, needles, likes);
  run_all({"\xC3\xA9", "\xE6\x97\xA5\xE6\x9C\xAC", "a\xC3\xA9\xF0\x9D\x84\x9E", "\x80", "a\x80", "a\x80" "b", "\xE6\x97",
           "\xFF\xFE", "\x80\x80" "a"},
          std::vector<bool>(9, false), needles, likes);
  {  // a long row whose only match is its last bytes, followed by a row that would complete a needle
    Cell big(3000, 'x');
    big += "ab";
    run_all({"c", big, "c", Cell(64, 'a'), "a"}, std::vector<bool>(5, false), needles, likes);
  }
  // random cells over a 3-letter alphabet plus a 2-byte code point, every 7th row null over garbage
  std::mt19937 rng(16);
  for (int round = 0; round < 40; ++round) {
    std::vector<Cell> rows;
    std::vector<bool> null;
    const int n = 1 + (int)(rng() % 60);
    for (int i = 0; i < n; ++i) {
      Cell s;
      const int len = (int)(rng() % 13);
      for (int k = 0; k < len; ++k) {
        const unsigned r = rng() % 8;
        if (r == 7) s += "\xC3\xA9";
        else if (r == 6) s.push_back((char)0x80);
        else s.push_back("abc"[r % 3]);
      }
      rows.push_back(s);
      null.push_back(rng() % 7 == 0);
    }
    run_all(rows, null, {"", "a", "ab", "bc", "abc", "\xC3\xA9"},
            {"%", "_", "a%", "%b", "%ab%", "a%b%c", "_%_", "%__", "a_c", "%a_b%", "_b%", "%\xC3\xA9_"});
  }
  if (failures) {
    std::fprintf(stderr, "strmatch_sanitize: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("strmatch_sanitize: ok\n");
  return 0;
}
