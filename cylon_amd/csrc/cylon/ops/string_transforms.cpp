// K15 string transforms (docs/semantics.md "String transforms"; kernels/strxform.hip and its CPU twin
// kernels/cpu_strxform.cpp): slice, strip, ASCII case, element-wise concat and literal replace of a
// string / binary column.  Each is a lengths pass, the exclusive scan, one read of the total and a
// write pass, as CastIntegerToString and SelectVar are built.  Every argument check runs before any
// launch; the literals travel as one small device buffer.
// Reference: pycylon has no string transforms (its callers go through pandas on the host).
#include <cstring>

#include "../kernels/strxform_common.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

using namespace strxform;

namespace {

bool is_text(const Column &c) { return c.type.type == Type::STRING || c.type.type == Type::BINARY; }

void check_text(const Column &a, const char *what) {
  CYLON_CHECK(is_text(a), Code::TypeError, what << ": column " << a.name << " is not a string / binary column");
}

void check_literal(const std::string &s, const char *what) {
  CYLON_CHECK((int64_t)s.size() <= kStrMaxPatternBytes, Code::Invalid,
              what << ": a literal of " << s.size() << " bytes (at most " << kStrMaxPatternBytes << ")");
}

at::Tensor upload(const Exec &ex, const std::string &bytes) {
  at::Tensor h = at::empty({(int64_t)bytes.size()}, at::TensorOptions().dtype(at::kByte));
  if (!bytes.empty()) std::memcpy(h.data_ptr(), bytes.data(), bytes.size());
  return ex.gpu ? h.to(ex.device) : h;
}

// a column of n rows of length 0: no row (n == 0), or every row null (valid = zeros)
Column empty_rows(const Exec &ex, const Column &like, int64_t n, const at::Tensor &valid) {
  return Column(like.name, like.type, n, ex.empty_bytes(0), at::zeros({n + 1}, ex.opts(at::kLong)), valid);
}

// lengths -> scan -> total -> write; flag: the device word of SX_CASE (or undefined)
Column transform(const Exec &ex, const Column &like, const ColView &av, const ColView &bv, const StrXform &x,
                 const std::string &lit, int64_t n, const at::Tensor &valid, const at::Tensor &flag = at::Tensor()) {
  if (n == 0) return empty_rows(ex, like, 0, valid);
  at::Tensor dlit = upload(ex, lit);
  at::Tensor lens = ex.empty_i64(n);
  KCALL(ex, strx_lengths, av, bv, x, ptr<uint8_t>(dlit), n, ptr<int64_t>(lens));
  at::Tensor offs = exclusive_scan(ex, lens);
  at::Tensor bytes = ex.empty_bytes(read_i64(offs, n));
  KCALL(ex, strx_write, av, bv, x, ptr<uint8_t>(dlit), n, ptr<int64_t>(offs), ptr<uint8_t>(bytes),
        flag.defined() ? reinterpret_cast<uint32_t *>(flag.data_ptr()) : nullptr);
  return Column(like.name, like.type, n, bytes, offs, valid);
}

}  // namespace

Column StringSlice(const Column &a, int64_t start, const std::optional<int64_t> &stop) {
  check_text(a, "string slice");
  StrXform x;
  x.fn = SX_SLICE;
  x.utf8 = a.type.type == Type::STRING ? 1 : 0;
  x.start = start;
  x.has_stop = stop ? 1 : 0;
  x.stop = stop ? *stop : 0;
  Exec ex(a.device());
  return transform(ex, a, a.view(), ColView{}, x, std::string(), a.length, a.validity);
}

Column StringStrip(const Column &a, int side, const std::optional<std::string> &chars) {
  check_text(a, "string strip");
  CYLON_CHECK(side >= SX_LEFT && side <= SX_BOTH, Code::Invalid, "string strip: side " << side);
  const std::string set = chars ? *chars : std::string(" \t\n\v\f\r");
  std::string bitmap(kStrSetBytes, '\0');
  for (unsigned char c : set) {
    CYLON_CHECK(c < 0x80 || a.type.type == Type::BINARY, Code::Invalid,
                "string strip: the characters to strip from a string column must be ASCII");
    bitmap[c >> 3] = (char)((unsigned char)bitmap[c >> 3] | (1u << (c & 7)));
  }
  StrXform x;
  x.fn = SX_STRIP;
  x.side = side;
  Exec ex(a.device());
  return transform(ex, a, a.view(), ColView{}, x, bitmap, a.length, a.validity);
}

std::pair<Column, bool> StringCase(const Column &a, bool upper) {
  check_text(a, "string case");
  StrXform x;
  x.fn = SX_CASE;
  x.upper = upper ? 1 : 0;
  Exec ex(a.device());
  const int64_t n = a.length;
  if (n == 0) return {empty_rows(ex, a, 0, a.validity), false};
  at::Tensor flag = at::zeros({1}, ex.opts(at::kInt));
  Column out;
  if (a.nullable()) {
    out = transform(ex, a, a.view(), ColView{}, x, std::string(), n, a.validity, flag);
  } else {
    const std::vector<int64_t> ends = to_host_vec(at::stack({a.offsets[0], a.offsets[n]}));
    const int64_t total = ends[1] - ends[0];
    at::Tensor offs = ex.empty_i64(n + 1), bytes = ex.empty_bytes(total);
    KCALL(ex, strx_case_flat, a.view(), x.upper, n, total, ptr<int64_t>(offs), ptr<uint8_t>(bytes),
          reinterpret_cast<uint32_t *>(flag.data_ptr()));
    out = Column(a.name, a.type, n, bytes, offs, at::Tensor());
  }
  return {out, flag.item<int32_t>() != 0};
}

Column StringConcat(const Column &a, const Column &b, const std::string &sep) {
  check_text(a, "string concat");
  CYLON_CHECK(is_text(b) && b.type.type == a.type.type, Code::TypeError,
              "string concat: the other column must have the type of " << a.name);
  check_literal(sep, "string concat");
  CYLON_CHECK(a.length == b.length || a.length == 1 || b.length == 1, Code::Invalid,
              "string concat: columns of " << a.length << " and " << b.length << " rows (want equal, or one row)");
  CYLON_CHECK(b.device() == a.device(), Code::Invalid, "string concat: columns on different devices");
  Exec ex(a.device());
  StrXform x;
  x.fn = SX_CONCAT;
  x.len1 = (int32_t)sep.size();
  x.a_bcast = a.length == 1 && b.length != 1;
  x.b_bcast = b.length == 1 && a.length != 1;
  const int64_t n = x.a_bcast ? b.length : a.length;
  ColView av = a.view(), bv = b.view();
  at::Tensor valid;
  if (x.a_bcast || x.b_bcast) {
    const Column &one = x.a_bcast ? a : b, &col = x.a_bcast ? b : a;
    if (one.nullable()) {
      // a null scalar: every row is null, and the scalar's bytes are not read
      if (one.validity[0].item<uint8_t>() == 0) return empty_rows(ex, a, n, ex.zeros_u8(n));
      valid = col.nullable() ? col.validity : at::ones({n}, ex.opts(at::kByte));
    } else {
      valid = col.validity;
    }
    (x.a_bcast ? av : bv).valid = nullptr;  // checked above
  } else if (a.nullable() || b.nullable()) {
    valid = !b.nullable() ? a.validity : (a.nullable() ? at::bitwise_and(a.validity, b.validity) : b.validity);
  }
  return transform(ex, a, av, bv, x, sep, n, valid);
}

Column StringReplace(const Column &a, const std::string &pat, const std::string &repl, int64_t max_replacements) {
  check_text(a, "string replace");
  CYLON_CHECK(!pat.empty(), Code::Invalid, "string replace: the pattern is empty");
  check_literal(pat, "string replace");
  check_literal(repl, "string replace");
  StrXform x;
  x.fn = SX_REPLACE;
  x.len1 = (int32_t)pat.size();
  x.len2 = (int32_t)repl.size();
  x.max_repl = max_replacements < 0 ? -1 : max_replacements;
  Exec ex(a.device());
  return transform(ex, a, a.view(), ColView{}, x, pat + repl, a.length, a.validity);
}

}  // namespace ops
}  // namespace cylon
