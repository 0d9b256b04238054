// Join (L3 local + L4 distributed).
//
// Reference: cpp/src/cylon/join/join.cpp:29-100 (JoinTables dispatch),
// hash_join.cpp:188-346, sort_join.cpp:576-722, join_utils.cpp:126-181
// (build_final_table: left columns ++ right columns, prefixed names, index -1
// -> null), table.cpp:428-502 (Join / DistributedJoin).
//
// Device plan for one local join:
//   1. key encoding: a single non-null fixed-width key column is used as-is
//      (int64 zero-copy, narrower types sign/zero-extended); otherwise a 64-bit
//      row hash over the key columns + a rows_equal confirmation pass.
//   2. hash: build the smaller side into the open-addressing multimap, probe
//      the other side (count, scan, write).
//      sort: radix-sort (key, row) of both sides and expand equal ranges
//      (sort_join.cpp).
//   3. outer completion: matched flags (mark_indices) + compaction of the
//      unmatched rows of the preserved side(s), appended with -1 partners.
//   4. materialisation: one fused gather launch per side (K4).
#include "cylon/knobs.hpp"
#include <algorithm>
#include <optional>
#include <array>
#include <cmath>
#include <cstdlib>
#include <limits>

#include "join_internal.hpp"
#include "../trace.hpp"

namespace cylon {
namespace ops {

// defined in sort_join.cpp
std::pair<at::Tensor, at::Tensor> SortJoinPairs(const Exec &ex, const at::Tensor &lkeys, const at::Tensor &rkeys);

static int64_t next_pow2(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

bool simple_key(const Column &c) {
  return !c.nullable() && !c.is_var() && c.type.kind() != ValueKind::FIXED_BYTES && c.type.width() <= 8;
}

KeyEncoding encode_keys(const Exec &ex, const TablePtr &t, const std::vector<int> &cols, bool exact_ok) {
  const int64_t n = t->Rows();
  if (exact_ok) {
    const Column &c = t->column(cols[0]);
    if (c.type.width() == 8 && c.type.kind() == ValueKind::SIGNED_INT) return {c.data.view(at::kLong), true};
    at::Tensor k = ex.empty_i64(n);
    KCALL(ex, key64_from_column, c.view(), n, ptr<int64_t>(k));
    return {k, true};
  }
  std::vector<ColView> v = views(t, cols);
  at::Tensor k = ex.empty_i64(n);
  KCALL(ex, row_hash64, v.data(), (int)v.size(), n, reinterpret_cast<uint64_t *>(ptr<int64_t>(k)));
  return {k, false};
}

// Build sides at least this large use the atomic-free sorted build (random
// 64-bit CAS into a table far beyond the caches runs at the memory-side atomic
// rate: 213 ms for 1B keys, profiles/); probe sides this large use the
// single-pass probe.
static constexpr int64_t kSortedBuildRows = int64_t(1) << 20;
static constexpr int64_t kEmitProbeRows = int64_t(1) << 22;

// inner-join index pairs on int64 keys via the K5 hash table (build = smaller side)
// Global-table hash join (the path of joins the LDS radix join does not take).  Clustering-free
// directory: the build keys are sorted once, and the open-addressing table holds each DISTINCT key
// once with its head index h; key k's build rows are perm[hstart[h], hstart[h + 1]).  A hot key is
// one slot, so no probe ever walks through its duplicates (a row-per-slot linear-probing multimap
// puts a hot key's duplicates into every nearby key's probe path: primary clustering that grows
// with the hot run's length).  Probes find <= 1 directory entry; the (probe, head) pairs are then
// expanded into (probe, build row) pairs in probe-row order.  Reference: the unordered_multimap of
// join/hash_join.cpp:255-298.
std::pair<at::Tensor, at::Tensor> hash_join_pairs(const Exec &ex, const at::Tensor &lk, const at::Tensor &rk) {
  const bool build_left = lk.numel() < rk.numel();
  const at::Tensor &bk0 = build_left ? lk : rk;
  const at::Tensor &pk = build_left ? rk : lk;
  const int64_t nb0 = bk0.numel(), np = pk.numel();
  at::Tensor sk, perm, hstart;
  bool distinct = false;
  {
    CYLON_PHASE("join.build.directory", ex.device);
    auto sr = at::sort(bk0);
    sk = std::get<0>(sr);
    perm = std::get<1>(sr);
    at::Tensor head = at::ones({nb0}, ex.opts(at::kBool));
    if (nb0 > 1) head.slice(0, 1, nb0).copy_(sk.slice(0, 1, nb0) != sk.slice(0, 0, nb0 - 1));
    // distinct build keys (the common case): the sorted keys ARE the directory and
    // every head is its own row -- no compaction, and the expansion below is one gather
    distinct = nb0 == 0 || head.all().item<bool>();
    if (!distinct) {
      at::Tensor hpos = head.nonzero().flatten();
      sk = sk.index_select(0, hpos);  // distinct keys, ascending
      hstart = at::cat({hpos, at::full({1}, nb0, ex.opts(at::kLong))});
    }
  }
  const at::Tensor &bk = sk;
  const int64_t nb = bk.numel();
  const int64_t cap = next_pow2(std::max<int64_t>(2 * nb, 64));
  const int shift = 64 - __builtin_ctzll((unsigned long long)cap);
  at::Tensor table;
  HashTableRef t{nullptr, cap, shift};
  if (ex.gpu && nb >= kSortedBuildRows) {
    CYLON_PHASE("join.build.sorted", ex.device);
    // atomic-free build: radix sort (key,row) by slot, prefix-max placement, sequential stores
    at::Tensor ka = ex.empty_i64(nb), va = ex.empty_i64(nb), kb = ex.empty_i64(nb), vb = ex.empty_i64(nb);
    at::Tensor mp = ex.empty_i64(1);
    at::Tensor ws = ex.empty_i64(KSIZE(ex, hash_build_sorted_workspace, nb));
    const int which = KCALL(ex, hash_build_sorted, ptr<int64_t>(bk), nb, shift, ptr<int64_t>(ws),
                            reinterpret_cast<uint64_t *>(ptr<int64_t>(ka)), ptr<int64_t>(va),
                            reinterpret_cast<uint64_t *>(ptr<int64_t>(kb)), ptr<int64_t>(vb), ptr<int64_t>(mp));
    ws = at::Tensor();
    const int64_t maxpos = read_i64(mp, 0) + nb - 1;
    t.tsize = std::max<int64_t>(cap, maxpos + 2);
    table = at::empty({t.tsize * 2}, ex.opts(at::kLong));  // HashSlot = 2 x int64
    t.slots = reinterpret_cast<HashSlot *>(table.data_ptr());
    KCALL(ex, hash_table_init, t.slots, t.tsize);
    const at::Tensor &sk2 = which ? kb : ka;
    const at::Tensor &sr2 = which ? vb : va;
    const at::Tensor &pm = which ? ka : kb;
    KCALL(ex, hash_table_place, reinterpret_cast<const uint64_t *>(ptr<int64_t>(sk2)), ptr<int64_t>(sr2),
          ptr<int64_t>(pm), nb, t);
  } else {
    table = at::empty({cap * 2}, ex.opts(at::kLong));
    t.slots = reinterpret_cast<HashSlot *>(table.data_ptr());
    KCALL(ex, hash_table_init, t.slots, cap);
    KCALL(ex, hash_build, ptr<int64_t>(bk), nb, t);
  }
  // (probe row, head) pairs: at most one per probe row
  at::Tensor po, ho;
  if (ex.gpu && np >= kEmitProbeRows) {
    CYLON_PHASE("join.probe.emit", ex.device);
    const int64_t capacity = np + 4096;
    po = ex.empty_i64(capacity);
    ho = ex.empty_i64(capacity);
    at::Tensor cnt = ex.empty_i64(1);
    KCALL(ex, hash_probe_emit, ptr<int64_t>(pk), np, t, capacity, ptr<int64_t>(cnt), ptr<int64_t>(po),
          ptr<int64_t>(ho));
    const int64_t m = read_i64(cnt, 0);
    CYLON_CHECK(m <= np, Code::ExecutionError, "directory probe: " << m << " matches for " << np << " probe rows");
    po = po.slice(0, 0, m);
    ho = ho.slice(0, 0, m);
  } else {
    CYLON_PHASE("join.probe.twopass", ex.device);
    at::Tensor counts = ex.empty_i64(np);
    KCALL(ex, hash_probe_count, ptr<int64_t>(pk), np, t, ptr<int64_t>(counts));
    at::Tensor offs = exclusive_scan(ex, counts);
    counts = at::Tensor();
    const int64_t m = read_i64(offs, np);
    po = ex.empty_i64(m);
    ho = ex.empty_i64(m);
    KCALL(ex, hash_probe_write, ptr<int64_t>(pk), np, t, ptr<int64_t>(offs), ptr<int64_t>(po), ptr<int64_t>(ho));
  }
  table = at::Tensor();
  at::Tensor bo;
  {
    CYLON_PHASE("join.probe.expand", ex.device);
    if (distinct) return build_left ? std::make_pair(perm.index_select(0, ho), po)
                                    : std::make_pair(po, perm.index_select(0, ho));
    at::Tensor first = hstart.index_select(0, ho);
    at::Tensor cnt = hstart.index_select(0, ho + 1) - first;
    const int64_t m = po.numel() ? cnt.sum().item<int64_t>() : 0;
    if (m != po.numel()) {  // some key has duplicates: repeat each pair over its key's rows
      at::Tensor excl = cnt.cumsum(0) - cnt;
      po = po.repeat_interleave(cnt, 0, m);
      at::Tensor pos = (first - excl).repeat_interleave(cnt, 0, m) + at::arange(m, ex.opts(at::kLong));
      bo = perm.index_select(0, pos);
    } else {
      bo = perm.index_select(0, first);
    }
  }
  return build_left ? std::make_pair(bo, po) : std::make_pair(po, bo);
}

std::pair<at::Tensor, at::Tensor> JoinIndices(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg) {
  if (is_semi(cfg.GetType())) return semi_join_indices(left, right, cfg);
  return join_impl(left, right, cfg, false, nullptr, nullptr);
}

void check_join_keys(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg) {
  const auto &lc = cfg.GetLeftColumnIdx();
  const auto &rc = cfg.GetRightColumnIdx();
  CYLON_CHECK(lc.size() == rc.size(), Code::Invalid, "left/right key counts differ");
  CYLON_CHECK(left->device() == right->device(), Code::Invalid, "join inputs on different devices");
  for (size_t i = 0; i < lc.size(); ++i) {
    const auto &a = left->column(lc[i]).type;
    const auto &b = right->column(rc[i]).type;
    const bool both_int = a.kind() != ValueKind::FLOAT && b.kind() != ValueKind::FLOAT && a.width() <= 8 &&
                          b.width() <= 8 && !a.is_variable_width() && !b.is_variable_width() &&
                          a.kind() != ValueKind::FIXED_BYTES && b.kind() != ValueKind::FIXED_BYTES;
    CYLON_CHECK(a == b || both_int, Code::TypeError,
                "join key types differ: " << a.ToString() << " vs " << b.ToString());
  }
}

std::pair<at::Tensor, at::Tensor> join_impl(TablePtr left, TablePtr right, const JoinConfig &cfg, bool allow_reorder,
                                            TablePtr *lout, TablePtr *rout) {
  const auto &lc = cfg.GetLeftColumnIdx();
  const auto &rc = cfg.GetRightColumnIdx();
  check_join_keys(left, right, cfg);
  Exec ex(left->device());
  const bool exact = lc.size() == 1 && simple_key(left->column(lc[0])) && simple_key(right->column(rc[0])) &&
                     left->column(lc[0]).type == right->column(rc[0]).type;
  KeyEncoding lk = encode_keys(ex, left, lc, exact);
  KeyEncoding rk = encode_keys(ex, right, rc, exact);
  (void)allow_reorder;  // hook for input reordering strategies (none profitable so far, see docs)
  if (lout) *lout = left;
  if (rout) *rout = right;

  std::pair<at::Tensor, at::Tensor> pr;
  if (cfg.GetAlgorithm() == JoinAlgorithm::SORT)
    pr = SortJoinPairs(ex, lk.keys, rk.keys);
  else
    pr = hash_join_pairs(ex, lk.keys, rk.keys);
  at::Tensor li = pr.first, ri = pr.second;

  if (!exact && li.numel() > 0) {  // confirm hash candidates
    std::vector<ColView> lv = views(left, lc), rv = views(right, rc);
    at::Tensor eq = ex.empty_u8(li.numel());
    KCALL(ex, rows_equal, lv.data(), rv.data(), (int)lv.size(), ptr<int64_t>(li), ptr<int64_t>(ri), li.numel(),
          ptr<uint8_t>(eq));
    at::Tensor keep = MaskToIndices(eq);
    if (keep.numel() != li.numel()) {
      li = li.index_select(0, keep);
      ri = ri.index_select(0, keep);
    }
  }

  const JoinType jt = cfg.GetType();
  std::vector<at::Tensor> lparts{li}, rparts{ri};
  if (jt == JoinType::LEFT || jt == JoinType::FULL_OUTER) {
    at::Tensor matched = ex.zeros_u8(left->Rows());
    KCALL(ex, mark_indices, ptr<int64_t>(li), li.numel(), ptr<uint8_t>(matched));
    at::Tensor um = MaskToIndices(matched, true);
    lparts.push_back(um);
    rparts.push_back(at::full({um.numel()}, -1, ex.opts(at::kLong)));
  }
  if (jt == JoinType::RIGHT || jt == JoinType::FULL_OUTER) {
    at::Tensor matched = ex.zeros_u8(right->Rows());
    KCALL(ex, mark_indices, ptr<int64_t>(ri), ri.numel(), ptr<uint8_t>(matched));
    at::Tensor um = MaskToIndices(matched, true);
    rparts.push_back(um);
    lparts.push_back(at::full({um.numel()}, -1, ex.opts(at::kLong)));
  }
  if (lparts.size() > 1) {
    li = at::cat(lparts);
    ri = at::cat(rparts);
  }
  return {li, ri};
}

// K7 sort-merge join on row-sorted tables (device, large inner joins on one exact
// integer key, algorithm = SORT).  Both relations are first sorted by the key with
// the row-moving LSD passes of ops::Sort (every column moves with the key, constant
// key bits skipped), so the merge's index pairs are monotone in both tables and
// the final gathers stream through HBM instead of touching it at random (the
// pair-sort + gather form spends most of its time in those random gathers).  The
// output comes out ordered by key, as the reference's sort join does.
static TablePtr sorted_merge_join(const Exec &ex, const TablePtr &left, const TablePtr &right,
                                  const JoinConfig &cfg) {
  const int lc = cfg.GetLeftColumnIdx()[0], rc = cfg.GetRightColumnIdx()[0];
  TablePtr ls, rs;
  {
    CYLON_PHASE("join.sortmerge.sort", ex.device);
    ls = Sort(left, {lc}, {true});
    rs = Sort(right, {rc}, {true});
  }
  // merge_join_* compare keys as uint64: the sign-flipped image of a signed key is
  // ordered like the key itself
  auto image = [&](const TablePtr &t, int c) {
    KeyEncoding k = encode_keys(ex, t, {c}, true);
    return t->column(c).type.kind() == ValueKind::SIGNED_INT
               ? at::bitwise_xor(k.keys, at::full({1}, std::numeric_limits<int64_t>::min(), k.keys.options()))
               : k.keys;
  };
  at::Tensor lk = image(ls, lc), rk = image(rs, rc);
  const int64_t nl = ls->Rows(), nr = rs->Rows();
  at::Tensor li, ri;
  {
    CYLON_PHASE("join.sortmerge.merge", ex.device);
    at::Tensor lo = ex.empty_i64(nl), counts = ex.empty_i64(nl);
    KCALL(ex, merge_join_count, reinterpret_cast<const uint64_t *>(ptr<int64_t>(lk)), nl,
          reinterpret_cast<const uint64_t *>(ptr<int64_t>(rk)), nr, ptr<int64_t>(lo), ptr<int64_t>(counts));
    at::Tensor offs = exclusive_scan(ex, counts);
    const int64_t m = read_i64(offs, nl);
    at::Tensor lperm = ex.empty_i64(nl), rperm = ex.empty_i64(nr);
    KCALL(ex, iota, ptr<int64_t>(lperm), nl, 0);
    KCALL(ex, iota, ptr<int64_t>(rperm), nr, 0);
    li = ex.empty_i64(m);
    ri = ex.empty_i64(m);
    KCALL(ex, merge_join_write, ptr<int64_t>(lperm), nl, ptr<int64_t>(rperm), ptr<int64_t>(lo), ptr<int64_t>(offs),
          ptr<int64_t>(li), ptr<int64_t>(ri));
  }
  CYLON_PHASE("join.sortmerge.materialize", ex.device);
  TablePtr lo = GatherNullable(ls, li, false);
  TablePtr ro = GatherNullable(rs, ri, false);
  std::vector<Column> cols;
  for (const auto &c : lo->columns()) cols.push_back(c.with_name(cfg.GetLeftTablePrefix() + c.name));
  for (const auto &c : ro->columns()) cols.push_back(c.with_name(cfg.GetRightTablePrefix() + c.name));
  trace::add_counter("join.sortmerge.rows_out", li.numel());
  return Table::Make(left->GetContext(), std::move(cols));
}

// K7 range join (device, inner, one signed integer key, algorithm = SORT): both
// relations are radix-partitioned into key ranges in key order (RangeSpec), each
// partition holding 2^rshift consecutive key values (rshift <= 12), and each
// partition is joined in LDS by exact key offset, emitting its rows in key order
// (radix_join.hip k_rg_*).  Same passes as the hash radix join, no full sort.
// Returns nullptr when the keys are too sparse for 12-bit partitions or a
// partition overflows (skew): the caller then runs sorted_merge_join.
static bool range_join_enabled() {
  return knobs::Flag("RANGE_JOIN", true);  // test knob: 0 = sort-merge path only
}

static TablePtr range_join(const Exec &ex, const TablePtr &left, const TablePtr &right, const JoinConfig &cfg) {
  const int lc = cfg.GetLeftColumnIdx()[0], rc = cfg.GetRightColumnIdx()[0];
  if (left->column(lc).type.kind() != ValueKind::SIGNED_INT) return nullptr;
  const int64_t nl = left->Rows(), nr = right->Rows();
  KeyEncoding lk = encode_keys(ex, left, {lc}, true), rk = encode_keys(ex, right, {rc}, true);
  at::Tensor mm = at::stack({lk.keys.min(), lk.keys.max(), rk.keys.min(), rk.keys.max()}).to(at::kCPU);
  const int64_t *h = mm.data_ptr<int64_t>();
  const int64_t kmin = std::min(h[0], h[2]), kmax = std::max(h[1], h[3]);
  const uint64_t span = (uint64_t)kmax - (uint64_t)kmin;  // signed range as an unsigned count
  int span_bits = 0;
  while (span_bits < 64 && (span >> span_bits) != 0) ++span_bits;
  // ~half the LDS capacity per side and partition on average: far below the cap for uniform keys
  const int64_t target = hip::range_join_max_rows() / 2;
  int bits = 0;
  while ((std::max(nl, nr) >> bits) > target) ++bits;
  // sparse keys: up to 16x more (smaller) partitions than the row count asks for keep
  // each partition's key range within the 4096 exact-offset buckets
  const int maxs = hip::range_join_max_shift();
  if (span_bits - bits > maxs && span_bits - maxs <= bits + 4) bits = span_bits - maxs;
  const int rshift = std::max(0, span_bits - bits);
  if (rshift > maxs) {
    trace::add_counter("join.range.sparse_fallback", 1);
    return nullptr;
  }
  const int pbits = span_bits - rshift;
  RangeSpec spec;
  spec.flip = uint64_t(1) << 63;  // signed -> order-preserving unsigned image
  spec.mn = (uint64_t)kmin ^ spec.flip;
  spec.rshift = rshift;
  const int64_t nparts = int64_t(1) << pbits;
  RadixSide L, R;
  {
    CYLON_PHASE("join.range.partition", ex.device);
    L = radix_partition(ex, left, lk.keys, pbits, &spec);
    R = radix_partition(ex, right, rk.keys, pbits, &spec);
  }
  at::Tensor counts = ex.empty_i64(nparts);
  at::Tensor overflow = at::empty({1}, ex.opts(at::kInt));
  {
    CYLON_PHASE("join.range.count", ex.device);
    hip::range_join_count(ptr<int64_t>(L.keys), ptr<int64_t>(L.offs), ptr<int64_t>(R.keys), ptr<int64_t>(R.offs),
                          nparts, spec.flip, spec.mn, rshift, ptr<int64_t>(counts), overflow.data_ptr<int>(),
                          ex.stream);
  }
  if (overflow.item<int>() != 0) {
    trace::add_counter("join.range.overflow_fallback", 1);
    return nullptr;
  }
  at::Tensor out_offs = exclusive_scan(ex, counts);
  const int64_t m = read_i64(out_offs, nparts);
  CYLON_PHASE("join.range.write", ex.device);
  std::vector<Column> lcols, rcols;
  for (const auto &col : left->columns())
    lcols.push_back(make_fixed_column(cfg.GetLeftTablePrefix() + col.name, col.type, m, ex.device, col.nullable()));
  for (const auto &col : right->columns())
    rcols.push_back(make_fixed_column(cfg.GetRightTablePrefix() + col.name, col.type, m, ex.device, col.nullable()));
  if (m > 0) {
    std::vector<at::Tensor> lwords, rwords;
    for (size_t i = 0; i < L.vwords.size(); ++i) lwords.push_back(ex.empty_i64(m));
    for (size_t i = 0; i < R.vwords.size(); ++i) rwords.push_back(ex.empty_i64(m));
    RadixCols a = radix_cols(left, &L, &lcols, 0, &lwords), b = radix_cols(right, &R, &rcols, 0, &rwords);
    for (auto &q : a.in)
      if (!q) q = reinterpret_cast<const uint8_t *>(L.keys.data_ptr());
    for (auto &q : b.in)
      if (!q) q = reinterpret_cast<const uint8_t *>(R.keys.data_ptr());
    hip::range_join_write(ptr<int64_t>(L.keys), ptr<int64_t>(L.offs), ptr<int64_t>(R.keys), ptr<int64_t>(R.offs),
                          nparts, spec.flip, spec.mn, rshift, ptr<int64_t>(out_offs), a.in.data(), a.out.data(),
                          a.w.data(), (int)a.in.size(), b.in.data(), b.out.data(), b.w.data(), (int)b.in.size(),
                          ex.stream);
    unpack_validity_words(ex, left, L, lwords, lcols, 0, m);
    unpack_validity_words(ex, right, R, rwords, rcols, 0, m);
  }
  trace::add_counter("join.range.rows_out", m);
  for (auto &c : rcols) lcols.push_back(std::move(c));
  return Table::Make(left->GetContext(), std::move(lcols));
}

// Local join.  With a sink (chunked distributed join) the radix path writes into
// the sink and nullptr is returned; other paths return their table.
static TablePtr join_local(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg, JoinSink *sink) {
  if (is_semi(cfg.GetType())) return semi_join_local(left, right, cfg);
  const bool big = left->device().is_cuda() && std::min(left->Rows(), right->Rows()) >= radix_join_min_rows();
  const JoinType jt = cfg.GetType();
  if (big && jt == JoinType::INNER && cfg.GetAlgorithm() == JoinAlgorithm::SORT &&
      cfg.GetLeftColumnIdx().size() == 1 && radix_eligible(left) && radix_eligible(right)) {
    const Column &a = left->column(cfg.GetLeftColumnIdx()[0]);
    const Column &b = right->column(cfg.GetRightColumnIdx()[0]);
    if (simple_key(a) && simple_key(b) && a.type == b.type && a.type.kind() != ValueKind::FLOAT) {
      Exec ex(left->device());
      if (range_join_enabled())
        if (TablePtr out = range_join(ex, left, right, cfg)) return out;
      return sorted_merge_join(ex, left, right, cfg);
    }
  }
  // the LDS radix hash join: hash joins of every type, and sort-algorithm outer / multi-key
  // joins (their output order is unspecified, docs/semantics.md)
  if (big && (cfg.GetAlgorithm() == JoinAlgorithm::HASH || jt != JoinType::INNER ||
              cfg.GetLeftColumnIdx().size() > 1)) {
    Exec ex(left->device());
    if (TablePtr out = radix_join_any(ex, left, right, cfg, sink)) return sink ? nullptr : out;
  }
  TablePtr l = left, r = right;
  auto idx = join_impl(left, right, cfg, true, &l, &r);
  const bool lnull = left_may_null(jt);
  const bool rnull = right_may_null(jt);
  CYLON_PHASE("join.materialize", l->device());
  TablePtr lo = GatherNullable(l, idx.first, lnull);
  TablePtr ro = GatherNullable(r, idx.second, rnull);
  std::vector<Column> cols;
  cols.reserve(lo->Columns() + ro->Columns());
  for (const auto &c : lo->columns()) cols.push_back(c.with_name(cfg.GetLeftTablePrefix() + c.name));
  for (const auto &c : ro->columns()) cols.push_back(c.with_name(cfg.GetRightTablePrefix() + c.name));
  return Table::Make(left->GetContext(), std::move(cols));
}

TablePtr Join(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg) {
  return join_local(left, right, cfg, nullptr);
}

TablePtr DistributedJoin(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg) {
  auto ctx = left->GetContext();
  if (!ctx->ShuffleRequired()) return Join(left, right, cfg);
  if (is_semi(cfg.GetType())) {
    // only the right side's key columns travel; equal keys land in the same hash chunk, so the
    // per-chunk semi / anti joins are exact and their outputs concatenate
    const auto &rc = cfg.GetRightColumnIdx();
    std::vector<int> rkeys(rc.size());
    for (size_t i = 0; i < rc.size(); ++i) rkeys[i] = (int)i;
    const JoinConfig kcfg(cfg.GetType(), cfg.GetLeftColumnIdx(), rkeys, cfg.GetAlgorithm(), cfg.GetLeftTablePrefix(),
                          cfg.GetRightTablePrefix());
    std::vector<TablePtr> parts;
    ShufflePairPlanned(left, cfg.GetLeftColumnIdx(), Project(right, rc), rkeys,
                       [&](int, int, const TablePtr &l, const TablePtr &r) { parts.push_back(Join(l, r, kcfg)); });
    return parts.size() == 1 ? parts[0] : Merge(parts);
  }
  JoinSink sink;
  TablePtr whole;
  ShufflePairPlanned(left, cfg.GetLeftColumnIdx(), right, cfg.GetRightColumnIdx(),
                     [&](int, int K, const TablePtr &l, const TablePtr &r) {
                       if (K == 1) {  // unchunked: the shuffled pair is joined as a whole
                         whole = Join(l, r, cfg);
                         return;
                       }
                       sink.chunks_total = K;
                       if (TablePtr t = join_local(l, r, cfg, &sink)) sink.tables.push_back(t);
                       ++sink.chunks_done;
                     });
  return whole ? whole : sink.finish(ctx);
}

}  // namespace ops
}  // namespace cylon
