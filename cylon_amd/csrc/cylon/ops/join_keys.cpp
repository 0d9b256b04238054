// Keys of the LDS radix join (RadixKeys, join_internal.hpp) and the join of any large device
// table pair through it: string keys and payload as word columns, composite keys, proxies and the
// rebuild of the output columns, verification of hashed keys.
#include "cylon/knobs.hpp"
#include <algorithm>
#include <limits>
#include <optional>

#include "join_internal.hpp"
#include "../trace.hpp"

namespace cylon {
namespace ops {

// Fixed-length strings / binaries (every row L <= 64 bytes, no nulls) travel through the radix join
// as ceil(L / 8) int64 word columns -- moved by the partition passes and the write kernel like any
// payload -- instead of a row number and a gather by it afterwards (random reads at ~50 G accesses/s:
// a 200M x 200M join on 16-byte string keys spent 26 of its 62 ms gathering, profiles/r05).
static int64_t fixed_var_len(const Exec &ex, const Column &c) {  // L, or -1
  if (c.nullable() || !(c.type.type == Type::STRING || c.type.type == Type::BINARY) || c.length == 0) return -1;
  at::Tensor mm = ex.empty_i64(2);
  hip::var_len_minmax(ptr<int64_t>(c.offsets), c.length, ptr<int64_t>(mm), ex.stream);
  at::Tensor h = mm.cpu();
  const int64_t lo = h[0].item<int64_t>(), hi = h[1].item<int64_t>();
  return lo == hi && lo > 0 && lo <= 64 ? lo : -1;
}

// words 0..W-1 (inv: words 1..W-1, *hash = the invertible word key that stands in for word 0)
static std::vector<at::Tensor> var_to_words(const Exec &ex, const Column &c, int64_t L, at::Tensor *hash = nullptr,
                                            bool inv = false) {
  const int64_t n = c.length, W = (L + 7) / 8;
  if (hash) *hash = ex.empty_i64(n);
  const int64_t o0 = c.offsets.slice(0, 0, 1).cpu().item<int64_t>();
  std::vector<at::Tensor> out;
  std::vector<int64_t *> wp;
  if (inv) wp.push_back(nullptr);
  for (int64_t j = inv ? 1 : 0; j < W; ++j) {
    out.push_back(ex.empty_i64(n));
    wp.push_back(ptr<int64_t>(out.back()));
  }
  hip::bytes_to_words(ptr<uint8_t>(c.data) + o0, n, (int)L, wp.data(), ex.stream,
                      hash ? reinterpret_cast<uint64_t *>(ptr<int64_t>(*hash)) : nullptr, inv);
  return out;
}

// {min, max} row length of a non-null string / binary column, or {-1, -1}
static std::pair<int64_t, int64_t> var_len_range(const Exec &ex, const Column &c) {
  if (c.nullable() || !(c.type.type == Type::STRING || c.type.type == Type::BINARY)) return {-1, -1};
  if (c.length == 0) return {0, 0};
  at::Tensor mm = ex.empty_i64(2);
  hip::var_len_minmax(ptr<int64_t>(c.offsets), c.length, ptr<int64_t>(mm), ex.stream);
  const std::vector<int64_t> h = to_host_vec(mm);
  return {h[0], h[1]};
}

// a variable-length column (rows <= 8 W bytes) as W zero-padded words: *key = the padded word key
// (word 0's stand-in), *lens = the row lengths; returns words 1..W-1.  One read of the bytes.
static std::vector<at::Tensor> var_to_padded(const Exec &ex, const Column &c, int W, at::Tensor *key,
                                             at::Tensor *lens, unsigned int *nul = nullptr) {
  const int64_t n = c.length;
  *key = ex.empty_i64(n);
  if (lens) *lens = ex.empty_i64(n);
  std::vector<at::Tensor> out;
  std::vector<int64_t *> wp{nullptr};
  for (int j = 1; j < W; ++j) {
    out.push_back(ex.empty_i64(n));
    wp.push_back(ptr<int64_t>(out.back()));
  }
  hip::var_to_words(ptr<uint8_t>(c.data), ptr<int64_t>(c.offsets), n, W, wp.data(),
                    reinterpret_cast<uint64_t *>(ptr<int64_t>(*key)), lens ? ptr<int64_t>(*lens) : nullptr, nullptr,
                    ex.stream, lens == nullptr, nul);
  return out;
}

// wc = {padded word key, words 1..W-1[, lengths]} of m rows -> a string / binary column (rows whose
// key column is null -- an outer join's absent side -- become null, zero bytes).  Text mode (no
// length column): the lengths come from the words.
static Column padded_to_var(const Exec &ex, const std::string &name, const DataType &type,
                            const std::vector<Column> &wc, int W, bool text) {
  const Column &kc = wc[0];
  const int64_t m = kc.length;
  at::Tensor lens;
  if (text) {
    lens = ex.empty_i64(std::max<int64_t>(m, 1)).slice(0, 0, m);
    std::vector<const int64_t *> wp;
    for (int j = 0; j < W; ++j) wp.push_back(ptr<int64_t>(wc[(size_t)j].data));
    hip::padded_text_lens(wp.data(), reinterpret_cast<const uint64_t *>(wp[0]), m, W, ptr<int64_t>(lens), ex.stream);
  } else {
    lens = wc[(size_t)W].data.slice(0, 0, m);
  }
  if (kc.nullable()) lens = at::where(kc.validity.slice(0, 0, m).to(at::kBool), lens, at::zeros({1}, lens.options()));
  // offsets = the device exclusive scan of the lengths (offs[m] = total): no zero fill + ATen cumsum
  at::Tensor offs = m ? exclusive_scan(ex, lens.contiguous()) : at::zeros({1}, ex.opts(at::kLong));
  const int64_t nbytes = m ? read_i64(offs, m) : 0;
  at::Tensor bytes = ex.empty_bytes(std::max<int64_t>(1, nbytes));
  std::vector<const int64_t *> wp;
  for (int j = 0; j < W; ++j) wp.push_back(ptr<int64_t>(wc[(size_t)j].data));
  hip::words_to_var(wp.data(), reinterpret_cast<const uint64_t *>(wp[0]), ptr<int64_t>(lens),
                    ptr<int64_t>(offs), m, W, ptr<uint8_t>(bytes), ex.stream, text);
  return Column(name, type, m, bytes.slice(0, 0, nbytes), offs, kc.validity);
}

// wc = the word columns 0..W-1 (inv: wc[0] = the invertible word key, wc[1..] = words 1..W-1)
static Column words_to_var(const Exec &ex, const std::string &name, const DataType &type,
                           const std::vector<Column> &wc, int64_t L, bool inv = false) {
  const int64_t m = wc[0].length;
  std::vector<const int64_t *> wp;
  for (const auto &c : wc) wp.push_back(ptr<int64_t>(c.data));
  at::Tensor bytes = ex.empty_bytes(std::max<int64_t>(1, m * L));
  hip::words_to_bytes(wp.data(), m, (int)L, ptr<uint8_t>(bytes), ex.stream,
                      inv ? reinterpret_cast<const uint64_t *>(wp[0]) : nullptr);
  at::Tensor offs = at::arange(0, (m + 1) * L, L, ex.opts(at::kLong));
  // (a null row of an outer join keeps L zero bytes under its null: Arrow allows any length there)
  return Column(name, type, m, bytes.slice(0, 0, m * L), offs, wc[0].validity);
}

bool int_key(const Column &c) {
  return simple_key(c) && (c.type.kind() == ValueKind::SIGNED_INT ||
                           (c.type.kind() == ValueKind::UNSIGNED_INT && c.type.width() < 8));
}

// an integer key column that may hold nulls (fixed width <= 8, dense storage): packable into an exact
// composite with one field value reserved for null, so nulls match nulls (docs/semantics.md)
bool nullable_int_key(const Column &c) {
  return c.nullable() && !c.is_var() && c.type.kind() != ValueKind::FIXED_BYTES && c.type.width() <= 8 &&
         c.data.element_size() == c.type.width() &&
         (c.type.kind() == ValueKind::SIGNED_INT || (c.type.kind() == ValueKind::UNSIGNED_INT && c.type.width() < 8));
}

RadixKeys radix_keys(const Exec &ex, const TablePtr &left, const TablePtr &right, const JoinConfig &cfg, bool words_ok) {
  const auto &lc = cfg.GetLeftColumnIdx();
  const auto &rc = cfg.GetRightColumnIdx();
  RadixKeys k;
  if (lc.size() == 1) {
    const Column &a = left->column(lc[0]), &b = right->column(rc[0]);
    if (simple_key(a) && simple_key(b) && a.type == b.type) {
      k.l = encode_keys(ex, left, lc, true).keys;
      k.r = encode_keys(ex, right, rc, true).keys;
      k.ok = true;
      return k;
    }
  }
  bool packable = lc.size() <= (size_t)kMaxCompositeKeys;
  // non-null string / binary / fixed-size binary key columns join through the verified row hash
  // (their bytes travel as gathered var-width columns; reference arrow_partition_kernels.cpp:243-305)
  auto hashed_ok = [](const Column &c) {
    return !c.nullable() && (c.is_var() || c.type.kind() == ValueKind::FIXED_BYTES);
  };
  for (size_t i = 0; i < lc.size(); ++i) {
    const Column &a = left->column(lc[i]), &b = right->column(rc[i]);
    if (!(a.type == b.type)) return k;
    const bool na = nullable_int_key(a), nb = nullable_int_key(b);
    if ((!simple_key(a) && !na && !hashed_ok(a)) || (!simple_key(b) && !nb && !hashed_ok(b))) return k;
    k.nulls = k.nulls || na || nb;
    packable = packable && (int_key(a) || na) && (int_key(b) || nb);
    if (hashed_ok(a)) trace::add_counter("join.radix.var_key", 1);
  }
  if (k.nulls && !packable) return k;  // nullable keys only as an exact composite
  k.ok = true;
  if (packable) {
    // per-key span over both relations (signed / byte storage: min / max of the column itself,
    // wider unsigned storage through its 64-bit image)
    auto span_of = [&](const Column &c, const TablePtr &t, int col) -> at::Tensor {
      if (c.data.numel() == 0)
        return at::tensor({std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()},
                          ex.opts(at::kLong));
      if (c.nullable()) {  // over the valid rows only (all null: an empty span)
        at::Tensor x = ex.empty_i64(t->Rows());
        hip::key64_from_column(c.view(), t->Rows(), ptr<int64_t>(x), ex.stream);
        const at::Tensor valid = c.validity.slice(0, 0, t->Rows()).ne(0);
        return at::stack({at::where(valid, x, std::numeric_limits<int64_t>::max()).min(),
                          at::where(valid, x, std::numeric_limits<int64_t>::min()).max()});
      }
      const bool direct = c.type.kind() == ValueKind::SIGNED_INT || c.type.width() == 1;
      at::Tensor x = direct ? c.data : encode_keys(ex, t, {col}, true).keys;
      auto m2 = at::aminmax(x);
      return at::stack({std::get<0>(m2).to(at::kLong), std::get<1>(m2).to(at::kLong)});
    };
    std::vector<at::Tensor> mm;
    for (size_t i = 0; i < lc.size(); ++i) {
      mm.push_back(span_of(left->column(lc[i]), left, lc[i]));
      mm.push_back(span_of(right->column(rc[i]), right, rc[i]));
    }
    const std::vector<int64_t> h = to_host_vec(at::cat(mm));
    const size_t nk = lc.size();
    k.lo.resize(nk);
    k.bits.resize(nk);
    k.shift.resize(nk);
    k.ncode.assign(nk, -1);
    int total = 0;
    for (size_t i = 0; i < nk; ++i) {
      k.lo[i] = std::min(h[4 * i], h[4 * i + 2]);
      const int64_t hi = std::max(h[4 * i + 1], h[4 * i + 3]);
      if (hi < k.lo[i]) k.lo[i] = 0;  // no valid key on either side
      uint64_t span = hi >= k.lo[i] ? (uint64_t)hi - (uint64_t)k.lo[i] : 0;
      if (left->column(lc[i]).nullable() || right->column(rc[i]).nullable()) {
        if (span >= (uint64_t)std::numeric_limits<int64_t>::max()) return k.ok = false, k;  // no free field value
        k.ncode[i] = (int64_t)span + 1;  // one past the largest valid field
        span += 1;
      }
      int b = 0;
      while (b < 64 && (span >> b) != 0) ++b;
      k.bits[i] = b;
      total += b;
    }
    if (total > 63 && k.nulls) return k.ok = false, k;  // nullable keys only as an exact composite
    if (total <= 63) {  // exact: key i occupies its own bit range (the last key the lowest bits)
      for (size_t i = nk, sh = 0; i-- > 0;) {
        k.shift[i] = (int)sh;
        sh += k.bits[i];
      }
      auto pack = [&](const TablePtr &t, const std::vector<int> &cols) {
        std::vector<ColView> v = views(t, cols);
        at::Tensor out = ex.empty_i64(t->Rows());
        KCALL(ex, composite_key_pack, v.data(), (int)nk, k.lo.data(), k.shift.data(), t->Rows(), ptr<int64_t>(out),
              k.nulls ? k.ncode.data() : nullptr);
        return out;
      };
      k.l = pack(left, lc);
      k.r = pack(right, rc);
      k.composite = true;
      trace::add_counter("join.radix.composite_key", 1);
      return k;
    }
  }
  k.verify = true;
  if (words_ok && lc.size() == 1 && left->device().is_cuda()) {
    // one fixed-length string key per side: its invertible word key (the join key, standing in for
    // word 0) and words 1..W-1 come out of one read of the bytes (the proxies below carry them)
    const int64_t L = fixed_var_len(ex, left->column(lc[0]));
    if (L > 0 && fixed_var_len(ex, right->column(rc[0])) == L) {
      k.wlen = L;
      k.lwords = var_to_words(ex, left->column(lc[0]), L, &k.l, true);
      k.rwords = var_to_words(ex, right->column(rc[0]), L, &k.r, true);
      trace::add_counter("join.radix.hashed_key", 1);
      return k;
    }
    // variable-length rows of <= 64 bytes: zero-padded words + the length (the padded word key seeds
    // its chain with the row's length, so equal keys + equal words 1..W-1 + equal lengths <=> equal
    // strings), no row-number gather of the key bytes after the join
    const Column &a = left->column(lc[0]), &b = right->column(rc[0]);
    if (a.is_var() && b.is_var() && knobs::Flag("RJ_VAR_WORDS", true)) {
      const auto ra = var_len_range(ex, a), rb = var_len_range(ex, b);
      const int64_t hi = std::max(ra.second, rb.second);
      if (ra.first >= 0 && rb.first >= 0 && hi <= 64) {
        k.vw = (int)std::max<int64_t>(1, (hi + 7) / 8);
        // text mode first (no zero byte in any row: the padding encodes the length, no length
        // column travels); a zero byte on either side redoes both sides with lengths
        at::Tensor nul = at::zeros({1}, ex.opts(at::kInt));
        unsigned int *np = reinterpret_cast<unsigned int *>(nul.data_ptr<int>());
        k.lwords = var_to_padded(ex, a, k.vw, &k.l, nullptr, np);
        k.rwords = var_to_padded(ex, b, k.vw, &k.r, nullptr, np);
        k.vtext = nul.item<int>() == 0;
        if (!k.vtext) {
          k.lwords = var_to_padded(ex, a, k.vw, &k.l, &k.llen);
          k.rwords = var_to_padded(ex, b, k.vw, &k.r, &k.rlen);
        }
        trace::add_counter(k.vtext ? "join.radix.var_word_key_text" : "join.radix.var_word_key", 1);
        return k;
      }
    }
  }
  k.l = encode_keys(ex, left, lc, false).keys;  // row hash of the key columns
  k.r = encode_keys(ex, right, rc, false).keys;
  trace::add_counter("join.radix.hashed_key", 1);
  return k;
}

// Rows of a hashed-key radix join whose key columns differ (64-bit key-hash collisions), as a bool
// mask, or an undefined tensor when there are none.  Rows where both sides are present only (outer
// rows carry one null side); row-wise equality of every key type (strings / binary byte-wise) by
// the rows_equal kernel.
static at::Tensor key_mismatches(const TablePtr &out, const JoinConfig &cfg, int nleft) {
  const auto &lc = cfg.GetLeftColumnIdx();
  const auto &rc = cfg.GetRightColumnIdx();
  const int64_t m = out->Rows();
  if (m == 0) return at::Tensor();
  Exec ex(out->device());
  std::vector<int> lcols(lc.begin(), lc.end()), rcols;
  for (int c : rc) rcols.push_back(nleft + c);
  std::vector<ColView> lv = views(out, lcols), rv = views(out, rcols);
  at::Tensor idx = at::arange(m, ex.opts(at::kLong));
  at::Tensor eq = ex.empty_u8(m);
  KCALL(ex, rows_equal, lv.data(), rv.data(), (int)lv.size(), ptr<int64_t>(idx), ptr<int64_t>(idx), m,
        ptr<uint8_t>(eq));
  at::Tensor bad = eq.eq(0);
  for (size_t i = 0; i < lc.size(); ++i) {  // compare where both sides hold a row
    const Column &a = out->column(lc[i]), &b = out->column(nleft + rc[i]);
    if (a.nullable()) bad.logical_and_(a.validity.slice(0, 0, m));
    if (b.nullable()) bad.logical_and_(b.validity.slice(0, 0, m));
  }
  return bad.any().item<bool>() ? bad : at::Tensor();
}

// A collision pairs rows whose keys differ: an inner join drops those rows; any other join type
// redoes the join on the exact path (nullptr), since a falsely matched row may owe an unmatched one.
static TablePtr drop_false_matches(const TablePtr &out, const JoinConfig &cfg, int nleft) {
  at::Tensor bad = key_mismatches(out, cfg, nleft);
  if (!bad.defined()) return out;
  const int64_t n = bad.sum().item<int64_t>();
  if (cfg.GetType() != JoinType::INNER) {
    trace::add_counter("join.radix.hash_collision_fallback", n);
    return nullptr;
  }
  trace::add_counter("join.radix.hash_collision_dropped", n);
  return FilterByMask(out, bad.logical_not());
}

// LDS radix join of any large device join (every type, one or several keys, var-width payload
// columns); nullptr when ineligible or when the kernels report an overflow / collision.  Tables
// with string / binary / list columns join their fixed-width columns plus a row-number column,
// and the var-width columns are gathered by those row numbers afterwards (two-pass offsets +
// bytes gather, row -1 -> null).  Exact composite keys (no sink): the proxy tables carry the
// composite in place of the key columns, so the passes and the write kernel move one 8-byte key
// (as in the one-key join), and composite_key_unpack rebuilds the key columns of the output.
TablePtr radix_join_any(const Exec &ex, const TablePtr &left, const TablePtr &right, const JoinConfig &cfg,
                        JoinSink *sink) {
  std::optional<trace::Phase> keys_phase;
  keys_phase.emplace("join.radix.keys", ex.device);  // key encoding + proxies (ends before the join)
  RadixKeys k = radix_keys(ex, left, right, cfg, sink == nullptr);  // (a sink takes no var-width keys)
  if (!k.ok) return nullptr;
  auto var_col = [](const Column &c) { return c.is_var() || c.type.kind() == ValueKind::FIXED_BYTES; };
  auto has_var = [&](const TablePtr &t) {
    for (const auto &c : t->columns())
      if (var_col(c)) return true;
    return false;
  };
  const bool lvar = has_var(left), rvar = has_var(right);
  // a chunked distributed join writes into its sink: fixed-width tables on exact keys only
  if ((lvar || rvar || k.verify) && sink) return nullptr;
  const bool ckey = k.composite && !sink;
  const auto &lc = cfg.GetLeftColumnIdx();
  const auto &rc = cfg.GetRightColumnIdx();
  // proxy of a side: [composite key] + its fixed-width non-key columns + the word columns of its
  // fixed-length strings [+ the row number, when other var-width columns are gathered by it];
  // pos[c] = proxy column of the side's column c (-1: rebuilt from the key or gathered);
  // wlen[c] = L of a column carried as words (from proxy column pos[c]), else -1
  static const std::string kRow = "__cylon_row", kKey = "__cylon_key";
  // vwid[c] = W of a variable-length key carried as W padded words + its length column
  auto proxy = [&](const TablePtr &t, bool &var, const std::vector<int> &keys, const at::Tensor &img,
                   std::vector<int> &pos, std::vector<int64_t> &wlen, std::vector<int> &vwid,
                   const std::vector<at::Tensor> &kwords, const at::Tensor &klens) {
    pos.assign(t->Columns(), -1);
    wlen.assign(t->Columns(), -1);
    vwid.assign(t->Columns(), 0);
    std::vector<Column> cols;
    if (ckey) cols.emplace_back(kKey, DataType(Type::INT64), t->Rows(), img);
    var = false;
    for (int c = 0; c < t->Columns(); ++c) {
      const Column &col = t->column(c);
      if (ckey && std::find(keys.begin(), keys.end(), c) != keys.end()) continue;
      if (var_col(col)) {
        if (k.vw > 0 && c == keys[0]) {  // padded word key, words 1..W-1, length (radix_keys)
          vwid[c] = k.vw;
          pos[c] = (int)cols.size();
          cols.emplace_back("__cylon_wk" + std::to_string(c), DataType(Type::INT64), t->Rows(), img);
          for (size_t j = 0; j < kwords.size(); ++j)
            cols.emplace_back("__cylon_w" + std::to_string(c) + "_" + std::to_string(j + 1), DataType(Type::INT64),
                              t->Rows(), kwords[j]);
          if (!k.vtext) cols.emplace_back("__cylon_wl" + std::to_string(c), DataType(Type::INT64), t->Rows(), klens);
          continue;
        }
        const bool kw = k.wlen > 0 && c == keys[0];  // the key's word key + words from radix_keys
        const int64_t L = kw ? k.wlen : fixed_var_len(ex, col);
        if (L < 0) {
          var = true;
          continue;
        }
        wlen[c] = L;
        pos[c] = (int)cols.size();
        // the key's word key is the join key itself (no pass moves it twice), then words 1..W-1
        if (kw) cols.emplace_back("__cylon_wk" + std::to_string(c), DataType(Type::INT64), t->Rows(), img);
        std::vector<at::Tensor> w = kw ? kwords : var_to_words(ex, col, L);
        for (size_t j = 0; j < w.size(); ++j)
          cols.emplace_back("__cylon_w" + std::to_string(c) + "_" + std::to_string(j + (kw ? 1 : 0)),
                            DataType(Type::INT64), t->Rows(), w[j]);
        continue;
      }
      pos[c] = (int)cols.size();
      cols.push_back(col);
    }
    if (var) cols.emplace_back(kRow, DataType(Type::INT64), t->Rows(), at::arange(t->Rows(), ex.opts(at::kLong)));
    return Table::Make(t->GetContext(), std::move(cols));
  };
  std::vector<int> lpos, rpos, lvw, rvw;
  std::vector<int64_t> lwlen, rwlen;
  const bool lpx = lvar || ckey, rpx = rvar || ckey;
  bool lgather = false, rgather = false;  // var-width columns gathered by row number after the join
  TablePtr lp = lpx ? proxy(left, lgather, lc, k.l, lpos, lwlen, lvw, k.lwords, k.llen) : left;
  TablePtr rp = rpx ? proxy(right, rgather, rc, k.r, rpos, rwlen, rvw, k.rwords, k.rlen) : right;
  if (lpx || rpx) {
    int64_t nw = 0;
    for (int64_t L : lwlen) nw += L > 0;
    for (int64_t L : rwlen) nw += L > 0;
    for (int W : lvw) nw += W > 0;
    for (int W : rvw) nw += W > 0;
    if (nw) trace::add_counter("join.radix.word_columns", nw);
  }
  if (!radix_eligible(lp) || !radix_eligible(rp)) return nullptr;
  keys_phase.reset();
  const int mchunks = sink ? 1 : radix_join_chunks(ex, lp, rp, k.l, k.r, cfg.GetType());
  TablePtr out = mchunks > 1 ? radix_join_chunked(ex, lp, rp, k.l, k.r, cfg, mchunks, k.verify)
                             : radix_join(ex, lp, rp, std::move(k.l), std::move(k.r), cfg, sink, k.verify);
  if (!out) return nullptr;
  if (k.verify && !lvar && !rvar) return drop_false_matches(out, cfg, left->Columns());
  if (!lpx && !rpx) return out;
  CYLON_PHASE("join.radix.rebuild", ex.device);  // word / proxy columns back to the output columns
  const JoinType jt = cfg.GetType();
  // Inner join on one fixed-length string key per side (same type and length, no nulls): the key
  // words are verified equal row by row below, so the right output key column is the left one's
  // bytes and offsets (one words -> bytes conversion; CYLON_RJ_SHARE_KEY=0 converts both).
  const bool share_skey = jt == JoinType::INNER && k.verify && lc.size() == 1 && lpx && rpx &&
                          ((lwlen[lc[0]] > 0 && lwlen[lc[0]] == rwlen[rc[0]]) || (lvw[lc[0]] > 0 && lvw[lc[0]] == rvw[rc[0]])) &&
                          left->column(lc[0]).type == right->column(rc[0]).type &&
                          !left->column(lc[0]).nullable() && !right->column(rc[0]).nullable() &&
                          knobs::Flag("RJ_SHARE_KEY", true);
  auto side = [&](const TablePtr &orig, bool px, bool var, const std::vector<int> &pos, const std::vector<int64_t> &wlen,
                  const std::vector<int> &vwid, const std::vector<int> &keys, int first, int np, bool may_null,
                  const std::string &prefix, int skip_col) {
    std::vector<Column> cols(orig->Columns());
    if (!px) {
      for (int c = 0; c < orig->Columns(); ++c) cols[c] = out->column(first + c);
      return cols;
    }
    for (int c = 0; c < orig->Columns(); ++c) {
      if (pos[c] < 0 || c == skip_col) continue;
      if (vwid[c] > 0) {  // a variable-length string from its padded words + length
        std::vector<Column> wc;
        for (int j = 0; j < vwid[c] + (k.vtext ? 0 : 1); ++j) wc.push_back(out->column(first + pos[c] + j));
        cols[c] = padded_to_var(ex, prefix + orig->column(c).name, orig->column(c).type, wc, vwid[c], k.vtext);
        continue;
      }
      if (wlen[c] > 0) {  // a fixed-length string from its word columns
        const int64_t L = wlen[c];
        std::vector<Column> wc;
        for (int64_t j = 0; j < (L + 7) / 8; ++j) wc.push_back(out->column(first + pos[c] + (int)j));
        cols[c] = words_to_var(ex, prefix + orig->column(c).name, orig->column(c).type, wc, L,
                               k.wlen > 0 && c == keys[0]);
      } else {
        cols[c] = out->column(first + pos[c]);
      }
    }
    if (ckey) {  // the key columns from the composite (its validity: the side's presence)
      const Column &img = out->column(first);
      std::vector<MutColView> mv;
      for (size_t i = 0; i < keys.size(); ++i) {
        const Column &kc = orig->column(keys[i]);
        Column o = make_fixed_column(prefix + kc.name, kc.type, img.length, ex.device, false);
        o.validity = img.validity;
        MutColView v;
        if (k.ncode[i] >= 0) {  // nulls come back where the field holds the null code (own validity)
          o.validity = img.validity.defined() ? img.validity.clone() : at::ones({img.length}, ex.opts(at::kByte));
          v.valid = img.length ? o.validity.data_ptr<uint8_t>() : nullptr;
        }
        v.data = reinterpret_cast<uint8_t *>(ptr<uint8_t>(o.data.view(at::kByte)));
        v.width = kc.type.width();
        v.kind = static_cast<int>(kc.type.kind());
        mv.push_back(v);
        cols[keys[i]] = std::move(o);
      }
      KCALL(ex, composite_key_unpack, ptr<int64_t>(img.data), img.length, (int)keys.size(), k.lo.data(),
            k.shift.data(), k.bits.data(), mv.data(), k.nulls ? k.ncode.data() : nullptr);
      trace::add_counter("join.radix.composite_unpacked", (int64_t)keys.size());
    }
    if (!var) return cols;
    const Column &rid = out->column(first + np - 1);
    at::Tensor idx = rid.nullable() ? at::where(rid.validity.to(at::kBool), rid.data, at::full({1}, -1, rid.data.options()))
                                    : rid.data;
    std::vector<Column> vcols;
    std::vector<int> vpos;
    for (int c = 0; c < orig->Columns(); ++c)
      if (var_col(orig->column(c))) {
        vcols.push_back(orig->column(c));
        vpos.push_back(c);
      }
    TablePtr g = GatherNullable(Table::Make(orig->GetContext(), vcols), idx.contiguous(), may_null);
    for (size_t j = 0; j < vpos.size(); ++j) cols[vpos[j]] = g->column((int)j).with_name(prefix + g->column((int)j).name);
    return cols;
  };
  std::vector<Column> all = side(left, lpx, lgather, lpos, lwlen, lvw, lc, 0, lp->Columns(), left_may_null(jt),
                                cfg.GetLeftTablePrefix(), -1);
  std::vector<Column> rcols = side(right, rpx, rgather, rpos, rwlen, rvw, rc, lp->Columns(), rp->Columns(),
                                   right_may_null(jt), cfg.GetRightTablePrefix(), share_skey ? rc[0] : -1);
  if (share_skey) {
    rcols[rc[0]] = all[lc[0]].with_name(cfg.GetRightTablePrefix() + right->column(rc[0]).name);
    trace::add_counter("join.radix.shared_key_column", 1);
  }
  for (auto &c : rcols) all.push_back(std::move(c));
  TablePtr res = Table::Make(left->GetContext(), std::move(all));
  if (lgather || rgather) trace::add_counter("join.radix.var_gather", 1);
  if (!k.verify) return res;
  // keys that are all fixed-length strings: compare their word columns (8 bytes per compare)
  bool words = lpx && rpx;
  for (size_t i = 0; words && i < lc.size(); ++i)
    words = (lwlen[lc[i]] > 0 && lwlen[lc[i]] == rwlen[rc[i]]) || (lvw[lc[i]] > 0 && lvw[lc[i]] == rvw[rc[i]]);
  if (!words) return drop_false_matches(res, cfg, left->Columns());
  const int64_t m = out->Rows();
  if (m == 0) return res;
  std::vector<const int64_t *> aw, bw;
  const int rfirst = lp->Columns();
  // (a word-key column: the key words 1..W-1 -- equal word keys were matched, so word 0 is equal too;
  // a padded word key: words 1..W-1 and the length, which seeds the key's chain)
  for (size_t i = 0; i < lc.size(); ++i) {
    const int64_t nwc = lvw[lc[i]] > 0 ? lvw[lc[i]] + (k.vtext ? 0 : 1) : (lwlen[lc[i]] + 7) / 8;
    for (int64_t j = (k.wlen > 0 || k.vw > 0) ? 1 : 0; j < nwc; ++j) {
      aw.push_back(ptr<int64_t>(out->column(lpos[lc[i]] + (int)j).data));
      bw.push_back(ptr<int64_t>(out->column(rfirst + rpos[rc[i]] + (int)j).data));
    }
  }
  if (aw.empty()) return res;  // an L <= 8 word key is the string itself: no false matches
  if (aw.size() > 8) return drop_false_matches(res, cfg, left->Columns());
  const Column &lw = out->column(lpos[lc[0]]), &rw = out->column(rfirst + rpos[rc[0]]);
  at::Tensor badb = ex.empty_u8(m);  // both sides present and some key word differs
  at::Tensor nbadd = ex.empty_i64(1);
  hip::words_mismatch(aw.data(), bw.data(), (int)aw.size(), lw.nullable() ? ptr<uint8_t>(lw.validity) : nullptr,
                      rw.nullable() ? ptr<uint8_t>(rw.validity) : nullptr, m, ptr<uint8_t>(badb), ptr<int64_t>(nbadd),
                      ex.stream);
  const int64_t nbad = nbadd.item<int64_t>();
  if (nbad == 0) return res;
  at::Tensor bad = badb.to(at::kBool);
  if (jt != JoinType::INNER) {
    trace::add_counter("join.radix.hash_collision_fallback", nbad);
    return nullptr;
  }
  trace::add_counter("join.radix.hash_collision_dropped", nbad);
  return FilterByMask(res, bad.logical_not());
}

}  // namespace ops
}  // namespace cylon
