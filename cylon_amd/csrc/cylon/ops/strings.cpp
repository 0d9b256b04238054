// K15 string predicates (docs/semantics.md "String predicates"; kernels/strmatch.hip and its CPU
// twin kernels/cpu_strings.cpp): comparison of a string / binary column with a scalar or a column,
// starts_with / ends_with / contains / LIKE with a literal pattern, byte and code-point length.
// Every argument check runs before any launch; the LIKE pattern is compiled here, on the host, and
// uploaded as a small device buffer.
// Reference: pycylon compute (python/pycylon/pycylon/data/compute.pyx) compares string columns with
// Arrow's host kernels.
#include <cstring>

#include "../kernels/strmatch_common.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

using namespace strmatch;

namespace {

bool is_text(const Column &c) { return c.type.type == Type::STRING || c.type.type == Type::BINARY; }

// pattern -> tokens: '%' any run, '_' one unit, the escape makes the next character literal;
// consecutive '%' are one
void compile_like(const std::string &pattern, char escape, StrPattern *out) {
  int n = 0;
  for (size_t i = 0; i < pattern.size(); ++i) {
    const char ch = pattern[i];
    uint8_t kind = TOK_LIT, lit = (uint8_t)ch;
    if (ch == escape) {
      CYLON_CHECK(i + 1 < pattern.size(), Code::Invalid, "like: the pattern ends in a lone escape character");
      lit = (uint8_t)pattern[++i];
    } else if (ch == '%') {
      if (n > 0 && out->kind[n - 1] == TOK_ANY) continue;
      kind = TOK_ANY;
    } else if (ch == '_') {
      kind = TOK_ONE;
    }
    out->kind[n] = kind;
    out->lit[n] = kind == TOK_LIT ? lit : 0;
    ++n;
  }
  out->ntok = n;
}

at::Tensor upload(const Exec &ex, const uint8_t *bytes, int64_t n) {
  at::Tensor h = at::empty({n}, at::TensorOptions().dtype(at::kByte));
  if (n) std::memcpy(h.data_ptr(), bytes, (size_t)n);
  return ex.gpu ? h.to(ex.device) : h;
}

}  // namespace

Column StringCompare(const Column &a, const Column &b, int op) {
  CYLON_CHECK(is_text(a), Code::TypeError, "string compare: column " << a.name << " is not a string / binary column");
  CYLON_CHECK(is_text(b) && b.type.type == a.type.type, Code::TypeError,
              "string compare: the other column must have the type of " << a.name);
  CYLON_CHECK(op >= STR_EQ && op <= STR_GE, Code::Invalid, "string compare: operator " << op);
  const int64_t n = a.length;
  CYLON_CHECK(b.length == n || b.length == 1, Code::Invalid,
              "string compare: other has " << b.length << " rows, want " << n << " or 1");
  CYLON_CHECK(b.device() == a.device(), Code::Invalid, "string compare: columns on different devices");
  Exec ex(a.device());
  const bool scalar = b.length == 1;
  at::Tensor out = ex.empty_u8(n);
  at::Tensor valid;
  if (a.nullable() || b.nullable()) {
    if (!b.nullable()) {
      valid = a.validity;
    } else if (scalar) {
      // a null scalar: every row is null, and the scalar's bytes are not read
      if (b.validity[0].item<uint8_t>() == 0) return Column(a.name, DataType(Type::BOOL), n, out.zero_(),
                                                            at::Tensor(), ex.zeros_u8(n));
      valid = a.nullable() ? a.validity : at::ones({n}, ex.opts(at::kByte));
    } else {
      valid = a.nullable() ? at::bitwise_and(a.validity, b.validity) : b.validity;
    }
  }
  ColView bv = b.view();
  if (scalar) bv.valid = nullptr;  // checked above
  KCALL(ex, str_compare, a.view(), bv, scalar ? 1 : 0, op, n, ptr<uint8_t>(out));
  return Column(a.name, DataType(Type::BOOL), n, out, at::Tensor(), valid);
}

Column StringMatch(const Column &a, int kind, const std::string &pattern, char escape) {
  CYLON_CHECK(is_text(a), Code::TypeError, "string match: column " << a.name << " is not a string / binary column");
  CYLON_CHECK(kind >= STR_STARTS_WITH && kind <= STR_LIKE, Code::Invalid, "string match: kind " << kind);
  CYLON_CHECK((int64_t)pattern.size() <= kStrMaxPatternBytes, Code::Invalid,
              "string match: a pattern of " << pattern.size() << " bytes (at most " << kStrMaxPatternBytes << ")");
  int utf8 = 0;
  std::string buf = pattern;  // what the kernel reads
  int64_t plen = (int64_t)pattern.size();
  if (kind == STR_LIKE) {
    StrPattern pat;
    compile_like(pattern, escape, &pat);
    utf8 = a.type.type == Type::STRING ? 1 : 0;
    // classify: a pattern of one of these shapes runs on the simpler kernel
    const int nt = pat.ntok;
    int wild = 0;
    for (int i = 0; i < nt; ++i) wild += pat.kind[i] != TOK_LIT;
    const bool any_first = nt > 0 && pat.kind[0] == TOK_ANY, any_last = nt > 0 && pat.kind[nt - 1] == TOK_ANY;
    int lo = 0, hi = nt;
    if (wild == 0) {
      kind = STR_EQUALS;
    } else if (wild == 1 && any_last) {
      kind = STR_STARTS_WITH, hi = nt - 1;
    } else if (wild == 1 && any_first) {
      kind = STR_ENDS_WITH, lo = 1;
    } else if (wild == 2 && any_first && any_last) {
      kind = STR_CONTAINS, lo = 1, hi = nt - 1;
    }
    if (kind == STR_LIKE) {
      buf.assign(reinterpret_cast<const char *>(pat.kind), (size_t)nt);
      buf.append(reinterpret_cast<const char *>(pat.lit), (size_t)nt);
      plen = nt;
    } else {
      buf.assign(reinterpret_cast<const char *>(pat.lit) + lo, (size_t)(hi - lo));
      plen = hi - lo;
    }
  }
  Exec ex(a.device());
  const int64_t n = a.length;
  at::Tensor out = ex.empty_u8(n);
  at::Tensor dpat = upload(ex, reinterpret_cast<const uint8_t *>(buf.data()), (int64_t)buf.size());
  KCALL(ex, str_match, a.view(), kind, ptr<uint8_t>(dpat), plen, utf8, n, ptr<uint8_t>(out));
  return Column(a.name, DataType(Type::BOOL), n, out, at::Tensor(), a.validity);
}

Column StringLength(const Column &a, int unit) {
  CYLON_CHECK(is_text(a), Code::TypeError, "string length: column " << a.name << " is not a string / binary column");
  CYLON_CHECK(unit == STR_LEN_BYTES || unit == STR_LEN_CHARS, Code::Invalid, "string length: unit " << unit);
  CYLON_CHECK(unit == STR_LEN_BYTES || a.type.type == Type::STRING, Code::TypeError,
              "string length: a binary column has no code points (column " << a.name << ")");
  Exec ex(a.device());
  const int64_t n = a.length;
  at::Tensor out = ex.empty_i64(n);
  KCALL(ex, str_length, a.view(), unit, n, ptr<int64_t>(out));
  return Column(a.name, DataType(Type::INT64), n, out, at::Tensor(), a.validity);
}

int64_t StringTileBytes() { return hip::string_tile_bytes(); }

}  // namespace ops
}  // namespace cylon
