// ---------------------------------------------------------------------------
// K5 LDS radix join (radix_join.hip): partition both sides, all columns, into
// LDS-sized buckets and join bucket pairs inside one workgroup each, emitting
// the output columns directly.  Used on the GPU for large inner joins on one
// exact key where every column is fixed width <= 8 bytes.
// ---------------------------------------------------------------------------
#include "cylon/knobs.hpp"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>

#include "join_internal.hpp"
#include "radix_sizing.hpp"
#include "../trace.hpp"

namespace cylon {
namespace ops {

int64_t radix_join_min_rows() {
  return knobs::Int("RADIX_JOIN_MIN_ROWS", int64_t(1) << 22);
}

bool radix_eligible(const TablePtr &t) {
  int slots = 1;
  for (const auto &c : t->columns()) {
    const int w = c.type.width();
    if (c.is_var() || c.type.kind() == ValueKind::FIXED_BYTES || !(w == 1 || w == 2 || w == 4 || w == 8) ||
        c.data.element_size() != w)
      return false;
    slots += 1 + (c.nullable() ? 1 : 0);
  }
  return slots <= kMaxFusedCols;
}

// partitioned key array (int64, or uint32 offsets when narrowed) as the kernels' pointer
static const int64_t *kptr(const at::Tensor &k) { return reinterpret_cast<const int64_t *>(k.data_ptr()); }

// rows of each partition / its first row in the partitioned arrays (slot mode: p * slot)
static at::Tensor part_counts(const RadixSide &s, int64_t nparts) {
  return s.slot ? s.offs.slice(0, 0, nparts) : s.offs.slice(0, 1, nparts + 1) - s.offs.slice(0, 0, nparts);
}
static at::Tensor part_starts(const RadixSide &s, int64_t nparts) {
  return s.slot ? at::arange(nparts, s.offs.options()) * s.slot : s.offs.slice(0, 0, nparts);
}

// the partition / write kernels move validity packed when every data column is 8 bytes wide
// (the all-8-byte kernel variants; byte runs of 1-byte validity columns cost 2x)
static bool packs_validity(const TablePtr &t) {
  bool any = false;
  for (const auto &c : t->columns()) {
    if (c.type.width() != 8) return false;
    any |= c.nullable();
  }
  return any;
}

RadixSide radix_partition(const Exec &ex, const TablePtr &t, const at::Tensor &keys, int bits, const RangeSpec *range,
                          int64_t slot, const hip::NarrowKeys *nk) {
  std::vector<at::Tensor> cur{keys};
  std::vector<int> widths{8};
  std::vector<int> dslot(t->Columns(), -1), vslot(t->Columns(), -1);
  for (int c = 0; c < t->Columns(); ++c) {
    const Column &col = t->column(c);
    if (col.type.width() == 8 && col.data.data_ptr() == keys.data_ptr()) {
      dslot[c] = 0;  // the key column itself
    } else {
      dslot[c] = (int)cur.size();
      cur.push_back(col.data);
      widths.push_back(col.type.width());
    }
    if (col.nullable()) {
      vslot[c] = (int)cur.size();
      cur.push_back(col.validity);
      widths.push_back(1);
    }
  }
  at::Tensor offs;
  const size_t nslots = cur.size();
  std::vector<int> packed;
  // hash partitions: the LDS join ignores row order inside a partition, so the first LSD pass
  // ranks with LDS atomics (later passes must keep its order)
  RadixSide s;
  std::vector<at::Tensor> sl;
  if (slot > 0 && !range)
    sl = RadixPartitionSlotted(ex, cur, widths, bits, slot, &offs, &s.overflow,
                               packs_validity(t) ? &packed : nullptr, nk);
  if (!sl.empty()) {
    cur = std::move(sl);
    s.slot = slot;
  } else {
    cur = RadixPartition(ex, std::move(cur), widths, bits, &offs, range, packs_validity(t) ? &packed : nullptr,
                         range != nullptr, nk);
  }
  s.keys = cur[0];
  s.offs = offs;
  for (size_t w = nslots; w < cur.size(); ++w) s.vwords.push_back(cur[w]);
  for (int c = 0; c < t->Columns(); ++c) {
    s.data.push_back(cur[dslot[c]]);
    const bool pk = vslot[c] >= 0 && !s.vwords.empty();
    s.valid.push_back(vslot[c] >= 0 && !pk ? cur[vslot[c]] : at::Tensor());
    int pos = -1;
    if (pk)
      for (size_t j = 0; j < packed.size(); ++j)
        if (packed[j] == vslot[c]) pos = (int)j;
    s.vpos.push_back(pos);
    s.is_key.push_back(dslot[c] == 0);
  }
  return s;
}

RadixCols radix_cols(const TablePtr &t, const RadixSide *s, const std::vector<Column> *outs, int64_t out_off,
                     const std::vector<at::Tensor> *word_outs) {
  RadixCols rc;
  const bool packed = s ? !s->vwords.empty() : packs_validity(t);
  int nnull = 0;
  for (int c = 0; c < t->Columns(); ++c) {
    const Column &col = t->column(c);
    rc.in.push_back(s && !s->is_key[c] ? reinterpret_cast<const uint8_t *>(s->data[c].data_ptr())
                                       : (s ? nullptr : reinterpret_cast<const uint8_t *>(1)));
    rc.out.push_back(outs ? reinterpret_cast<uint8_t *>((*outs)[c].data.data_ptr()) + out_off * col.type.width()
                          : nullptr);
    rc.w.push_back(col.type.width());
    if (col.nullable() && packed) {
      ++nnull;
    } else if (col.nullable()) {
      rc.in.push_back(s ? s->valid[c].data_ptr<uint8_t>() : reinterpret_cast<const uint8_t *>(1));
      rc.out.push_back(outs ? (*outs)[c].validity.data_ptr<uint8_t>() + out_off : nullptr);
      rc.w.push_back(1);
    }
  }
  if (packed) {  // the packed validity words, 8 bytes per row (outputs: temporary words)
    const int nw = (nnull + 7) / 8;
    for (int w = 0; w < nw; ++w) {
      rc.in.push_back(s ? reinterpret_cast<const uint8_t *>(s->vwords[w].data_ptr()) : reinterpret_cast<const uint8_t *>(1));
      rc.out.push_back(word_outs ? reinterpret_cast<uint8_t *>((*word_outs)[w].data_ptr()) : nullptr);
      rc.w.push_back(8);
    }
  }
  return rc;
}

void unpack_validity_words(const Exec &ex, const TablePtr &t, const RadixSide &s, const std::vector<at::Tensor> &words,
                           std::vector<Column> &outs, int64_t out_off, int64_t m) {
  if (s.vwords.empty() || m == 0) return;
  std::vector<uint8_t *> dst;
  for (int c = 0; c < t->Columns(); ++c)
    if (s.vpos[c] >= 0) dst.push_back(outs[c].validity.data_ptr<uint8_t>() + out_off);
  std::vector<const uint64_t *> wp;
  for (const auto &w : words) wp.push_back(reinterpret_cast<const uint64_t *>(w.data_ptr()));
  hip::unpack_byte_columns(wp.data(), (int)dst.size(), m, dst.data(), ex.stream);
}

int outer_mode(JoinType jt, bool build_left) {
  const bool lp = jt == JoinType::LEFT || jt == JoinType::FULL_OUTER;
  const bool rp = jt == JoinType::RIGHT || jt == JoinType::FULL_OUTER;
  return ((build_left ? rp : lp) ? 1 : 0) | ((build_left ? lp : rp) ? 2 : 0);
}

// validity of the output columns of a side that can be null: the side's presence bytes, AND the
// column's own validity where the input column was nullable.  Without a sink the columns of a
// non-nullable input share the presence bytes as their validity (no per-column copy: a 1B-row
// FULL OUTER join would otherwise hold 8 more bytes per output row); a sink's columns own theirs.
static void apply_presence(std::vector<Column> &cols, const TablePtr &in, const at::Tensor &pres, int64_t off,
                           int64_t m, bool share) {
  at::Tensor p = pres.slice(0, 0, m);
  for (int c = 0; c < in->Columns(); ++c) {
    if (share && !in->column(c).nullable()) {
      cols[c].validity = p;
      continue;
    }
    at::Tensor v = cols[c].validity.slice(0, off, off + m);
    if (in->column(c).nullable()) v.mul_(p);
    else v.copy_(p);
  }
}

std::vector<int> key_columns(const TablePtr &t, const at::Tensor &k) {
  std::vector<int> cols;
  for (int c = 0; c < t->Columns(); ++c)
    if (t->column(c).data.defined() && t->column(c).data.data_ptr() == k.data_ptr()) cols.push_back(c);
  return cols;
}

static bool int64_column(const Column &c) {
  return c.type.width() == 8 && (c.type.kind() == ValueKind::SIGNED_INT || c.type.kind() == ValueKind::UNSIGNED_INT);
}

int radix_extra_bits(int bits) {
  const int64_t xb = knobs::Int("RJ_EXTRA_BITS", 0);  // test knob: finer partitions
  return xb ? std::min(bits + (int)std::max<int64_t>(0, xb), 2 * 10) : bits;
}

// ---------------------------------------------------------------------------
// The plan: every size of one radix join.
// ---------------------------------------------------------------------------
void RadixJoinPlan::set_bits(int b) {
  bits = b;
  nparts = int64_t(1) << bits;
  slot_l = bits < 11 ? 0 : sizing::slot_rows((double)nl / (double)nparts);
  slot_r = bits < 11 ? 0 : sizing::slot_rows((double)nr / (double)nparts);
  pch = std::max<int64_t>(int64_t(1) << 15, 8 * (((build_left ? nr : nl) + nparts - 1) / nparts));
  bmean = ((build_left ? nl : nr) + nparts - 1) / nparts;
}

// test knob CYLON_RJ_SPLIT_ROWS: split partitions below the LDS capacity
static int64_t split_rows_of(int64_t cap) {
  return std::max<int64_t>(8, std::min<int64_t>(cap, knobs::Int("RJ_SPLIT_ROWS", cap)));
}

RadixJoinPlan RadixJoinPlan::without_narrowing() const {
  RadixJoinPlan p = *this;
  p.narrow = false;
  p.split_rows = split_rows_of(p.cap8);
  return p;
}

RadixJoinPlan plan_radix_join(const TablePtr &left, const TablePtr &right, const std::vector<bool> &build_is_key,
                              bool narrow, JoinType jt, int pre_bits) {
  RadixJoinPlan p;
  p.nl = left->Rows();
  p.nr = right->Rows();
  p.build_left = p.nl < p.nr;
  p.oj = outer_mode(jt, p.build_left);
  // LDS capacity from the build side's staged row width (key column counted once)
  const TablePtr &bt = p.build_left ? left : right;
  p.shape = radix_cols(bt, nullptr, nullptr);
  for (int c = 0, q = 0; c < bt->Columns(); ++c, ++q) {
    if (build_is_key[(size_t)c]) p.shape.in[q] = nullptr;
    if (bt->column(c).nullable() && !packs_validity(bt)) ++q;  // packed validity words sit after the columns
  }
  auto capacity = [&](int key_bytes) {
    return hip::radix_join_capacity(p.shape.w.data(), p.shape.in.data(), (int)p.shape.w.size(), (p.oj & 2) != 0,
                                    key_bytes);
  };
  p.cap4 = capacity(4);
  p.cap8 = capacity(8);
  p.narrow = narrow;
  p.split_rows = split_rows_of(p.cap());
  const int64_t nb = std::min(p.nl, p.nr);
  if (pre_bits >= 0) {
    p.set_bits(pre_bits);
    return p;
  }
  p.set_bits(radix_extra_bits(sizing::partition_bits(nb, p.cap())));
  if (p.narrow && p.bits == 0) {  // one partition: no pass runs, so nothing would narrow the keys
    p = p.without_narrowing();
    p.set_bits(radix_extra_bits(sizing::partition_bits(nb, p.cap())));
  }
  return p;
}

// ---------------------------------------------------------------------------
// The phases of radix_join (in its order) and what each hands on.
// ---------------------------------------------------------------------------
// the call's arguments, as every phase sees them
struct RadixJoinIn {
  const Exec &ex;
  const TablePtr &left, &right;
  const JoinConfig &cfg;
  JoinSink *sink;
  const PrePartition *pre;  // (tables: schema only, partitions in pre)
};

// Narrowed keys (kernel_decls.inc NarrowKeys): when each side's join key is its own int64 column,
// the partitions carry it as a uint32 offset from base = (left key 0) - 2^31 -- 4 B/row less in
// every pass write, the second pass's reads and the join kernel's reads (the headline's 1B x 1B
// join: 16 of 128 bytes moved per row and side).  A key outside [base, base + 2^32) is detected
// by the first pass, and the join repartitions without narrowing.
struct Narrowing {
  at::Tensor bad;       // int32 device flag: a key left the range
  at::Tensor base_src;  // the base's source (left key 0), its own copy: a released input's key column goes away
  hip::NarrowKeys nk;
};

struct SkewMasks {
  at::Tensor bcnt, pcnt, heavy, mid, sums;  // sums: [heavy partitions, mid partitions] (device)
  int64_t cap = 0;
};

static SkewMasks skew_masks(const RadixJoinPlan &plan, const RadixSide &Bs, const RadixSide &Ps) {
  SkewMasks k;
  k.cap = plan.cap();
  const int64_t nparts = plan.nparts, np_rows = plan.build_left ? plan.nr : plan.nl;
  k.bcnt = part_counts(Bs, nparts);
  k.pcnt = part_counts(Ps, nparts);
  k.heavy = at::logical_or(k.bcnt > plan.split_rows, k.pcnt > 2 * plan.pch);
  // hot-ish partitions (far above the mean, not split) are counted exactly instead of sampled: a
  // sample that misses them under-estimates the output and costs a second write (skip = 2)
  k.mid = at::logical_and(k.heavy.logical_not(),
                          at::logical_or(k.pcnt > 4 * (np_rows + nparts - 1) / nparts + 1024, k.bcnt > 4 * plan.bmean + 1024));
  k.sums = at::stack({k.heavy.sum(), k.mid.sum()});
  return k;
}

// what the partition phase hands on
struct Partitioned {
  RadixSide L, R;
  bool released = false;  // an input is gone: no fallback can run, the remaining failure exits raise
  SkewMasks sk;           // computed with the partition flags' read when no side was repartitioned
  bool widened = false;   // a key left the narrowed range: repartitioned on 8-byte keys (generic write kernel)
};

// (a released input can no longer feed a fallback: the remaining failure exits raise instead)
static bool fail(bool released, const char *why) {
  CYLON_CHECK(!released, Code::ExecutionError,
              "radix join with a released (retain = false) input could not complete: " << why);
  return false;
}

// A side with a hot partition would overflow a slot and repartition exactly after both slot
// passes (1B x 1B with 16 build keys x 200k duplicates: +48 ms): a histogram of ~1M sampled keys
// (every stride-th) finds a partition far above the mean first, and that side starts exact.
static void drop_slots_of_skewed_sides(const RadixJoinIn &in, const RadixJoinPlan &plan, const at::Tensor &lk,
                                       const at::Tensor &rk, const hip::NarrowKeys *nkp, int64_t &sl, int64_t &sr) {
  const Exec &ex = in.ex;
  auto sample = [&](const at::Tensor &k, int64_t rows, at::Tensor &h, int64_t &stride) {
    stride = std::max<int64_t>(1, rows >> 20);
    h = at::empty({plan.nparts}, ex.opts(at::kInt));
    hip::radix_part_sample(ptr<int64_t>(k), rows, plan.bits, stride, reinterpret_cast<uint32_t *>(h.data_ptr<int>()),
                           nkp, ex.stream);
  };
  at::Tensor hl, hr;
  int64_t stl = 1, str = 1;
  sample(lk, plan.nl, hl, stl);
  sample(rk, plan.nr, hr, str);
  at::Tensor mx = at::stack({hl.max(), hr.max()}).cpu();
  auto hot = [&](int64_t m, int64_t rows, int64_t stride) {
    const double mean = (double)((rows + stride - 1) / stride) / (double)plan.nparts;
    return (double)m > 4.0 * mean + 32.0;
  };
  if (sl && hot(mx[0].item<int>(), plan.nl, stl)) sl = 0;
  if (sr && hot(mx[1].item<int>(), plan.nr, str)) sr = 0;
  if (!sl || !sr) trace::add_counter("join.radix.sampled_skew_sides", (sl ? 0 : 1) + (sr ? 0 : 1));
}

// Phase 2: both sides' partitions.  Releases retain = false inputs, repartitions a side whose slot
// overflowed exactly and both sides on 8-byte keys when a key left the narrowed range (plan changes).
static Partitioned partition_sides(const RadixJoinIn &in, RadixJoinPlan &plan, at::Tensor &lk, at::Tensor &rk,
                                   const Narrowing &nw) {
  const Exec &ex = in.ex;
  const TablePtr &left = in.left, &right = in.right;
  const int bits = plan.bits;
  Partitioned out;
  RadixSide &L = out.L, &R = out.R;
  // retain = false (reference table.cpp:150-154): an input is released as soon as nothing can need
  // it again -- its own passes fit their slots and no key of either side leaves the narrowed range
  // (else it would be repartitioned from the input) -- so its buffers are free before the other
  // side's passes and the output allocation (1B x 1B: ~64 GB lower peak).  Only the sink-less join
  // on partitions that can always complete releases (no global-table fallback needs the input later).
  const bool rel_l = !left->IsRetain() && !in.sink, rel_r = !right->IsRetain() && !in.sink;
  const bool narrow = plan.narrow;
  at::Tensor r_outside;  // narrowed keys: right keys outside [base, base + 2^32) (checked before releasing left)
  if (rel_l && narrow) {
    auto mm = at::aminmax(rk);
    const at::Tensor base = nw.base_src - (int64_t(1) << 31);
    r_outside = at::logical_or(std::get<0>(mm) < base, (std::get<1>(mm) - base) > (int64_t)0xffffffffll).to(at::kInt);
  }
  // (one host read: the side's slot overflow flag, the narrowing flag so far, the right keys' range)
  auto release_if_done = [&](const TablePtr &t, at::Tensor &key, const RadixSide &s, const at::Tensor *outside) {
    at::Tensor z = at::zeros({1}, ex.opts(at::kInt));
    std::vector<at::Tensor> flags{s.slot ? s.overflow.slice(0, 0, 1) : z, narrow ? nw.bad : z};
    if (outside) flags.push_back(outside->defined() ? outside->reshape({1}) : z);
    if (at::cat(flags).sum().item<int>() != 0) return;
    t->ReleaseIfNotRetained();
    key = at::Tensor();
    trace::add_counter("join.radix.released_inputs", 1);
    out.released = true;
  };
  CYLON_PHASE("join.radix.partition", ex.device);
  const hip::NarrowKeys *nkp = narrow ? &nw.nk : nullptr;
  // test knob CYLON_RJ_SLOT=0: exact passes only
  const bool slot_on = knobs::Flag("RJ_SLOT", true);
  int64_t sl = slot_on ? plan.slot_l : 0, sr = slot_on ? plan.slot_r : 0;
  if ((sl || sr) && std::max(plan.nl, plan.nr) >= (int64_t(1) << 24) && (!in.sink || in.sink->sample_skew))
    drop_slots_of_skewed_sides(in, plan, lk, rk, nkp, sl, sr);
  L = radix_partition(ex, left, lk, bits, nullptr, sl, nkp);
  if (rel_l) release_if_done(left, lk, L, &r_outside);
  R = radix_partition(ex, right, rk, bits, nullptr, sr, nkp);
  if (rel_r) release_if_done(right, rk, R, nullptr);
  if (!(L.slot || R.slot || narrow)) return out;
  // a side whose partition outgrew a slot is partitioned exactly
  at::Tensor z = at::zeros({}, ex.opts(at::kInt));
  // the skew masks of the partitions as they stand ride in the same copy (used when no side is
  // repartitioned below: one host sync instead of two)
  out.sk = skew_masks(plan, plan.build_left ? L : R, plan.build_left ? R : L);
  at::Tensor f = at::cat({at::stack({L.slot ? L.overflow[0] : z, R.slot ? R.overflow[0] : z,
                                     narrow ? nw.bad[0] : z}).to(at::kLong),
                          out.sk.sums}).cpu();
  bool redo = f[2].item<int64_t>() != 0;
  if (redo) {  // a key outside the uint32 offset range: both sides as int64 keys
    trace::add_counter("join.radix.narrow_fallback", 1);
    plan = plan.without_narrowing();
    nkp = nullptr;
    out.widened = true;
    L = radix_partition(ex, left, lk, bits, nullptr, slot_on ? plan.slot_l : 0);
    R = radix_partition(ex, right, rk, bits, nullptr, slot_on ? plan.slot_r : 0);
    if (L.slot || R.slot)
      f = at::stack({L.slot ? L.overflow[0] : z, R.slot ? R.overflow[0] : z, z}).to(at::kLong).cpu();
  }
  if (f[0].item<int64_t>()) {
    trace::add_counter("join.radix.slot_overflow", 1);
    L = radix_partition(ex, left, lk, bits, nullptr, 0, nkp);
    redo = true;
  }
  if (f[1].item<int64_t>()) {
    trace::add_counter("join.radix.slot_overflow", 1);
    R = radix_partition(ex, right, rk, bits, nullptr, 0, nkp);
    redo = true;
  }
  if (redo) out.sk = SkewMasks();
  else out.sk.sums = f.slice(0, 3, 5);  // (host copy of the sums)
  trace::add_counter("join.radix.slot_sides", (L.slot ? 1 : 0) + (R.slot ? 1 : 0));
  if (plan.narrow) trace::add_counter("join.radix.narrow_keys", 1);
  return out;
}

// what the skew phase hands on: the split partitions as work items, the hot-ish ones as count items
// (the tensors own what the RJSplits point at)
struct SplitWork {
  int64_t nheavy = 0, nmid = 0, nitems = 0, nemits = 0;
  int64_t emit_bound = 0;  // deferred unmatched rows the emission items can add at most
  at::Tensor skip, skip_sample, items_d, emits_d, gprobe, gbuild, mid_items;
  hip::RJSplit main, emit;
};

// the work items of the heavy partitions: info = per partition {probe first row, probe rows, build
// first row, build rows} (host), kRJItemWords per item
static void split_items(const RadixJoinPlan &plan, const int64_t *h, int64_t nheavy, std::vector<int64_t> &items,
                        std::vector<int64_t> &emits, int64_t &emit_bound) {
  const int oj = plan.oj;
  const int64_t split_rows = plan.split_rows, pch = plan.pch;
  std::vector<std::array<int64_t, hip::kRJItemWords>> work;
  for (int64_t i = 0; i < nheavy; ++i) {
    const int64_t lb0 = h[4 * i], nl0 = h[4 * i + 1], rb0 = h[4 * i + 2], nr0 = h[4 * i + 3];
    const int64_t nbc = std::max<int64_t>(1, (nr0 + split_rows - 1) / split_rows);
    const int64_t npc = nl0 > 2 * pch ? (nl0 + pch - 1) / pch : 1;
    // a side split into several items learns "unmatched" only from all of them: deferred
    const bool pdef = (oj & 1) && nbc > 1, bdef = (oj & 2) && npc > 1;
    const int64_t fl = (pdef ? hip::kRJItemPDefer : 0) | (bdef ? hip::kRJItemBDefer : 0);
    for (int64_t bc = 0; bc < nbc; ++bc)
      for (int64_t pc = 0; pc < npc; ++pc) {
        const int64_t b0 = nr0 * bc / nbc, b1 = nr0 * (bc + 1) / nbc, p0 = nl0 * pc / npc, p1 = nl0 * (pc + 1) / npc;
        if (b1 > b0 || p1 > p0) work.push_back({lb0 + p0, p1 - p0, rb0 + b0, b1 - b0, fl});
      }
    if (pdef) {
      for (int64_t pc = 0; pc < npc; ++pc)
        emits.insert(emits.end(), {lb0 + nl0 * pc / npc, nl0 * (pc + 1) / npc - nl0 * pc / npc, 0, 0,
                                   (int64_t)hip::kRJItemPEmit});
      emit_bound += nl0;
    }
    if (bdef) {
      for (int64_t bc = 0; bc < nbc; ++bc)
        emits.insert(emits.end(), {0, 0, rb0 + nr0 * bc / nbc, nr0 * (bc + 1) / nbc - nr0 * bc / nbc,
                                   (int64_t)hip::kRJItemBEmit});
      emit_bound += nr0;
    }
  }
  // heaviest items first: they lead the write kernel's grid-stride order
  std::stable_sort(work.begin(), work.end(), [](const auto &a, const auto &b) {
    return a[1] * std::max<int64_t>(1, a[3]) > b[1] * std::max<int64_t>(1, b[3]);
  });
  for (const auto &w : work) items.insert(items.end(), w.begin(), w.end());
  trace::add_counter("join.radix.split_partitions", nheavy);
  trace::add_counter("join.radix.split_items", (int64_t)work.size());
}

// Phase 3: skew masks (unless they came with the partition flags) and split items.  false: a
// prepartitioned side's slot overflowed (flagged in pre, nothing written).
static bool split_skewed(const RadixJoinIn &in, const RadixJoinPlan &plan, const RadixSide &B, const RadixSide &P,
                         SkewMasks &sk, SplitWork &w) {
  const Exec &ex = in.ex;
  const PrePartition *pre = in.pre;
  const int64_t nparts = plan.nparts;
  if (!sk.heavy.defined() || sk.cap != plan.cap()) sk = skew_masks(plan, B, P);
  w.skip = sk.heavy.to(at::kByte);
  w.skip_sample = at::logical_or(sk.heavy, sk.mid).to(at::kByte);
  // {probe first row, probe rows, build first row, build rows} of the masked partitions
  auto spans = [&](const at::Tensor &mask) -> std::vector<at::Tensor> {
    at::Tensor idx = mask.nonzero().flatten();
    return {part_starts(P, nparts).index_select(0, idx), sk.pcnt.index_select(0, idx),
            part_starts(B, nparts).index_select(0, idx), sk.bcnt.index_select(0, idx)};
  };
  at::Tensor hm;
  if (pre) {  // the prepartitioned sides' slot overflow flags in the same copy
    hm = at::cat({sk.sums.to(at::kLong), pre->L.overflow.to(at::kLong), pre->R.overflow.to(at::kLong)}).cpu();
    pre->overflow_l = hm[2].item<int64_t>() != 0;
    pre->overflow_r = hm[3].item<int64_t>() != 0;
    if (pre->overflow_l || pre->overflow_r) {
      pre->overflowed = true;
      return false;
    }
  } else {
    hm = sk.sums.is_cuda() ? sk.sums.cpu() : sk.sums;
  }
  const int64_t nheavy = w.nheavy = hm[0].item<int64_t>(), nmid = w.nmid = hm[1].item<int64_t>();
  std::vector<int64_t> items, emits;  // kRJItemWords per item
  if (nheavy > 0) {
    at::Tensor info = at::stack(spans(sk.heavy), 1).cpu().contiguous();
    split_items(plan, info.data_ptr<int64_t>(), nheavy, items, emits, w.emit_bound);
  }
  const int64_t nitems = w.nitems = (int64_t)items.size() / hip::kRJItemWords;
  const int64_t nemits = w.nemits = (int64_t)emits.size() / hip::kRJItemWords;
  w.items_d = nitems ? at::tensor(items, at::TensorOptions().dtype(at::kLong)).to(ex.device) : at::Tensor();
  w.emits_d = nemits ? at::tensor(emits, at::TensorOptions().dtype(at::kLong)).to(ex.device) : at::Tensor();
  at::Tensor &gprobe = w.gprobe, &gbuild = w.gbuild;  // matched flags of the deferred sides (per partitioned row)
  for (int64_t i = 0; i < nitems; ++i) {
    const int64_t f = items[i * hip::kRJItemWords + 4];
    if ((f & hip::kRJItemPDefer) && !gprobe.defined()) gprobe = at::zeros({std::max<int64_t>(1, P.keys.numel())}, ex.opts(at::kByte));
    if ((f & hip::kRJItemBDefer) && !gbuild.defined()) gbuild = at::zeros({std::max<int64_t>(1, B.keys.numel())}, ex.opts(at::kByte));
  }
  w.main.skip = nheavy ? w.skip.data_ptr<uint8_t>() : nullptr;
  if (nmid > 0) {  // count-only items of the skip = 2 partitions
    std::vector<at::Tensor> cols = spans(sk.mid);
    cols.push_back(at::zeros({nmid}, ex.opts(at::kLong)));
    w.mid_items = at::stack(cols, 1).contiguous();
    trace::add_counter("join.radix.exact_counted_partitions", nmid);
  }
  w.main.items = nitems ? ptr<int64_t>(w.items_d) : nullptr;
  w.main.nitems = nitems;
  w.main.gprobe = gprobe.defined() ? gprobe.data_ptr<uint8_t>() : nullptr;
  w.main.gbuild = gbuild.defined() ? gbuild.data_ptr<uint8_t>() : nullptr;
  w.emit = w.main;
  w.emit.skip = nullptr;
  w.emit.items = nemits ? ptr<int64_t>(w.emits_d) : nullptr;
  w.emit.nitems = nemits;
  return true;
}

// what the join kernels' launches of one join share
struct JoinLaunch {
  const Exec &ex;
  const RadixJoinPlan &plan;
  const RadixSide &P, &B;
  const int64_t *nbase;  // the narrowed-key base (nullptr: 8-byte keys)
  at::Tensor overflow;   // int32 device flags of the count / write kernels
};

// what the count phase hands on (the size) and the write phase after it (the columns of the output --
// the sink's, at row `off`, with one -- and the temporaries the finish needs)
struct JoinOutput {
  int64_t stride = 1;  // 1: exact offsets (out_offs, m rows); else cursor mode into `alloc` rows
  int64_t m = 0, alloc = 0, off = 0;
  at::Tensor out_offs;
  std::vector<Column> lcols, rcols;
  std::vector<at::Tensor> lwords, rwords;  // packed validity words as written
  at::Tensor ppres, bpres;                 // presence bytes of the probe / build side (outer joins)
};

// Phase 4: the output size.  Exact mode: a count kernel over every partition, a scan, then the write
// kernel at the scanned offsets.  Fused mode (default): the count kernel runs on every
// 32nd partition only, the output is allocated for the extrapolated size + 2 % (partitions
// are hash-uniform: the estimate's standard error is ~0.03 % at 1B rows), and the write
// kernel counts each partition's matches itself and claims its output rows with one
// atomic.  A claim past the allocation makes the kernel report the exact total instead,
// and the write runs again into an exact allocation (skewed keys); the row order differs
// between runs either way (docs/semantics.md).
// test / A-B knobs: CYLON_RJ_EXACT_COUNT=1 (count kernel over every partition),
// CYLON_RJ_FUSED_MIN_PARTS (default 4096), CYLON_RJ_ESTIMATE_SCALE (scales the estimate: < 1
// forces the exact rerun)
static bool count_output(const JoinLaunch &jl, const SplitWork &w, bool released, JoinOutput &o) {
  const Exec &ex = jl.ex;
  const RadixSide &P = jl.P, &B = jl.B;
  const int64_t nparts = jl.plan.nparts, nheavy = w.nheavy, nmid = w.nmid, nitems = w.nitems;
  const bool exact_count = knobs::Flag("RJ_EXACT_COUNT", false);
  const int64_t fused_min = knobs::Int("RJ_FUSED_MIN_PARTS", 4096);
  const char *es = knobs::Get("RJ_ESTIMATE_SCALE");
  const double est_scale = es ? std::atof(es) : 1.0;
  int64_t &stride = o.stride, &m = o.m, &alloc = o.alloc;
  stride = exact_count || nparts < fused_min ? 1 : std::min<int64_t>(32, std::max<int64_t>(1, nparts / 64));
  at::Tensor counts;
  const at::Tensor &overflow = jl.overflow;
  CYLON_PHASE("join.radix.count", ex.device);
  // one count launch: np partitions at stride st (np = 0: the split's items), into n counts
  auto launch = [&](int64_t np, int64_t st, const hip::RJSplit &sp, int64_t n) {
    at::Tensor c = ex.empty_i64(n);
    hip::radix_join_count(kptr(P.keys), ptr<int64_t>(P.offs), kptr(B.keys), ptr<int64_t>(B.offs), np, jl.plan.cap(),
                          ptr<int64_t>(c), overflow.data_ptr<int>(), ex.stream, st, jl.plan.oj, P.slot, B.slot, &sp,
                          jl.nbase);
    return c;
  };
  // the partition count skips split partitions (items are counted below); the sampled count also
  // the hot-ish ones (counted exactly below)
  auto count = [&](int64_t st) {
    hip::RJSplit skip_only;
    skip_only.skip = st > 1 && nmid ? w.skip_sample.data_ptr<uint8_t>() : w.main.skip;
    counts = launch(nparts, st, skip_only, (nparts + st - 1) / st);
  };
  count(stride);
  // the ranking guard of the stable (second and later) partition passes: its device flag travels
  // in the same copy as the count results (one host sync instead of two)
  const at::Tensor oflag = at::from_blob(hip::rp_order_flag(), {1}, ex.opts(at::kInt)).to(at::kLong);
  auto order_violation = [&](int64_t flag) {
    if (!flag) return false;
    hip::rp_note_order_violation(ex.stream);
    trace::add_counter("join.radix.order_violation_fallback", 1);
    return true;
  };
  int64_t ssum = 0, sover = 0;  // the sample's total and overflow flag (one read for both uses)
  if (stride > 1) {
    // Skew check of the sample: extrapolating a hot key's partition 32x would over-allocate
    // (ADVICE r03), so a sample whose largest partition output is far above its mean is
    // counted exactly instead.
    at::Tensor st = at::stack({counts.sum(), counts.max(), overflow.to(at::kLong)[0], oflag[0]}).cpu();
    if (order_violation(st[3].item<int64_t>())) return fail(released, "order violation");
    ssum = st[0].item<int64_t>();
    sover = st[2].item<int64_t>();
    const int64_t smax = st[1].item<int64_t>();
    const int64_t nsample = counts.numel();
    if (sover == 0 && smax > 16 * (ssum / std::max<int64_t>(1, nsample)) + 65536) {
      trace::add_counter("join.radix.skewed_sample_exact_count", 1);
      stride = 1;
      count(1);
    }
  }
  if (stride == 1) {
    o.out_offs = exclusive_scan(ex, counts);
    at::Tensor tail = at::cat({o.out_offs.slice(0, nparts, nparts + 1), overflow.to(at::kLong), oflag}).cpu();
    if (order_violation(tail[2].item<int64_t>())) return fail(released, "order violation");
    m = tail[0].item<int64_t>();
    if (tail[1].item<int64_t>() != 0) {
      trace::add_counter("join.radix.overflow_fallback", 1);
      return fail(released, "overflow");
    }
    alloc = m;
  } else {
    if (sover != 0) {  // a sampled partition already overflows the LDS (or is misplaced)
      trace::add_counter("join.radix.overflow_fallback", 1);
      return fail(released, "overflow");
    }
    const double est = (double)ssum * (double)nparts / (double)counts.numel();
    // skewed inputs (split or exactly counted partitions exist): the sampled rest still holds
    // moderately hot keys, so its estimate gets 10 % slack instead of 2 % (memory, not a rewrite)
    const double slack = nheavy + nmid > 0 ? 1.10 : 1.02;
    alloc = (int64_t)(est * slack * est_scale) + (est_scale < 1.0 ? 0 : 65536);
    trace::add_counter("join.radix.estimated_rows", (int64_t)est);
  }
  if (nmid > 0 && stride > 1) {  // the partitions left out of the sample, counted exactly
    hip::RJSplit only;
    only.items = ptr<int64_t>(w.mid_items);
    only.nitems = nmid;
    alloc += launch(0, 1, only, nmid).sum().item<int64_t>();
  }
  if (nitems > 0) {  // split items: counted exactly (their deferred rows bounded), cursor mode
    hip::RJSplit only = w.main;
    only.skip = nullptr;
    const int64_t exact_items = launch(0, 1, only, nitems).sum().item<int64_t>();
    alloc = (stride == 1 ? m : alloc) + exact_items + w.emit_bound;
    stride = 2;  // (cursor mode below)
    o.out_offs = at::Tensor();
  }
  return true;
}

// Inner joins keyed on one integer column per side (the partitioned key itself, same type, no
// nulls): the two key values of every output row are equal, so the build side's output key
// column is the probe side's -- one buffer behind both (columns are immutable): 8 B/row less
// written and allocated (1B x 1B: 8 GB).  A/B knob: CYLON_RJ_SHARE_KEY=0.
struct SharedKey {
  bool on = false;
  int kl = -1, kr = -1;  // the sides' key columns
};

static void allocate_output(const RadixJoinIn &in, const RadixJoinPlan &plan, const Partitioned &pt,
                            const SharedKey &share, int64_t rows, JoinOutput &o) {
  const Exec &ex = in.ex;
  const int nlc = in.left->Columns();
  o.lcols.clear();
  o.rcols.clear();
  if (in.sink) {
    std::vector<Column> proto;  // (the proto's validity only says whether the column is nullable)
    auto add = [&](const TablePtr &t, const std::string &prefix, bool may_null) {
      for (const auto &col : t->columns())
        proto.emplace_back(prefix + col.name, col.type, 0, col.data, at::Tensor(),
                           col.nullable() || may_null ? col.data : at::Tensor());
    };
    add(in.left, in.cfg.GetLeftTablePrefix(), left_may_null(in.cfg.GetType()));
    add(in.right, in.cfg.GetRightTablePrefix(), right_may_null(in.cfg.GetType()));
    o.off = in.sink->reserve(ex, rows, proto);
    o.lcols.assign(in.sink->cols.begin(), in.sink->cols.begin() + nlc);
    o.rcols.assign(in.sink->cols.begin() + nlc, in.sink->cols.end());
  } else {  // (null-side validity: apply_presence; the build side's shared key column is not written)
    auto add = [&](const TablePtr &t, const std::string &prefix, int shared_col, std::vector<Column> &cols) {
      for (int c = 0; c < t->Columns(); ++c)
        cols.push_back(make_fixed_column(prefix + t->column(c).name, t->column(c).type, c == shared_col ? 0 : rows,
                                         ex.device, t->column(c).nullable()));
    };
    add(in.left, in.cfg.GetLeftTablePrefix(), share.on && plan.build_left ? share.kl : -1, o.lcols);
    add(in.right, in.cfg.GetRightTablePrefix(), share.on && !plan.build_left ? share.kr : -1, o.rcols);
  }
  auto word_outs = [&](const RadixSide &sd) {
    std::vector<at::Tensor> w;
    for (size_t i = 0; i < sd.vwords.size(); ++i) w.push_back(ex.empty_i64(std::max<int64_t>(rows, 1)));
    return w;
  };
  o.lwords = word_outs(pt.L);
  o.rwords = word_outs(pt.R);
  if (plan.oj & 2) o.ppres = ex.empty_u8(std::max<int64_t>(rows, 1));
  if (plan.oj & 1) o.bpres = ex.empty_u8(std::max<int64_t>(rows, 1));
}

// the write kernel over the partitions and split items, then the emission items; offs: exact
// offsets, else the rows are claimed from *cursor (at most `rows`)
static void write_output(const RadixJoinIn &in, const JoinLaunch &jl, const Partitioned &pt, const SharedKey &share,
                         const SplitWork &w, JoinOutput &o, int64_t rows, const int64_t *offs, int64_t *cursor) {
  const RadixJoinPlan &plan = jl.plan;
  const RadixSide &P = jl.P, &B = jl.B;
  const bool build_left = plan.build_left;
  RadixCols lc = radix_cols(in.left, &pt.L, &o.lcols, o.off, &o.lwords);
  RadixCols rc = radix_cols(in.right, &pt.R, &o.rcols, o.off, &o.rwords);
  RadixCols &pc = build_left ? rc : lc, &bc = build_left ? lc : rc;
  if (share.on) {  // the build key column's entry (after any unpacked validity entries before it)
    const TablePtr &bt = build_left ? in.left : in.right;
    const int bkc = build_left ? share.kl : share.kr;
    int q = 0;
    for (int c = 0; c < bkc; ++c) q += 1 + (bt->column(c).nullable() && B.vwords.empty());
    bc.in.erase(bc.in.begin() + q);
    bc.out.erase(bc.out.begin() + q);
    bc.w.erase(bc.w.begin() + q);
  }
  // probe-side columns are streamed from HBM; the key column (in == nullptr) is written from
  // the probe key the kernel already holds
  int pkey = -1;
  for (size_t q = 0; q < pc.in.size(); ++q)
    if (!pc.in[q]) {
      pc.in[q] = reinterpret_cast<const uint8_t *>(P.keys.data_ptr());
      if (pkey < 0) pkey = (int)q;
    }
  auto launch = [&](int64_t np, const int64_t *out_offs, const hip::RJSplit &sp) {
    const bool exact =
        hip::radix_join_write(kptr(P.keys), ptr<int64_t>(P.offs), kptr(B.keys), ptr<int64_t>(B.offs), np, plan.cap(),
                          out_offs, pc.in.data(), pc.out.data(), pc.w.data(), (int)pc.in.size(), bc.in.data(),
                          bc.out.data(), bc.w.data(), (int)bc.in.size(), jl.ex.stream, cursor, rows,
                          jl.overflow.data_ptr<int>(), pkey, plan.oj,
                          o.ppres.defined() ? o.ppres.data_ptr<uint8_t>() : nullptr,
                          o.bpres.defined() ? o.bpres.data_ptr<uint8_t>() : nullptr, P.slot, B.slot, &sp, jl.nbase,
                          !pt.widened);
    if (exact) trace::add_counter("join.radix.write_exact", 1);
  };
  launch(plan.nparts, offs, w.main);
  if (w.nemits > 0) launch(0, nullptr, w.emit);  // the deferred sides' unmatched rows, after every item recorded its matches
}

// Phase 5: allocate and write; in cursor mode the write reports a short estimate and runs again
// into an exact allocation.  false: a build partition beyond the LDS capacity (the sink is rewound).
static bool allocate_and_write(const RadixJoinIn &in, const JoinLaunch &jl, const Partitioned &pt,
                               const SharedKey &share, const SplitWork &w, JoinOutput &o) {
  const Exec &ex = in.ex;
  JoinSink *sink = in.sink;
  const at::Tensor &overflow = jl.overflow;
  int64_t &m = o.m;
  if (o.stride == 1) {
    allocate_output(in, jl.plan, pt, share, m, o);
    if (m > 0) write_output(in, jl, pt, share, w, o, m, ptr<int64_t>(o.out_offs), nullptr);
    return true;
  }
  at::Tensor cursor = at::zeros({1}, ex.opts(at::kLong));
  overflow.zero_();
  allocate_output(in, jl.plan, pt, share, o.alloc, o);
  write_output(in, jl, pt, share, w, o, o.alloc, nullptr, ptr<int64_t>(cursor));
  at::Tensor res = at::cat({cursor, overflow.to(at::kLong)}).cpu();
  m = res[0].item<int64_t>();
  const int64_t flags = res[1].item<int64_t>();
  if (flags & 1) {  // a build partition beyond the LDS capacity: global-table join instead
    if (sink) sink->size = o.off;
    trace::add_counter("join.radix.overflow_fallback", 1);
    return fail(pt.released, "overflow");
  }
  if (flags & 2) {  // the estimate was short: write again into an exact allocation
    trace::add_counter("join.radix.estimate_rerun", 1);
    if (sink) sink->size = o.off;
    cursor.zero_();
    overflow.zero_();
    if (w.gprobe.defined()) w.gprobe.zero_();
    if (w.gbuild.defined()) w.gbuild.zero_();
    allocate_output(in, jl.plan, pt, share, m, o);
    write_output(in, jl, pt, share, w, o, m, nullptr, ptr<int64_t>(cursor));
    CYLON_CHECK(at::cat({cursor, overflow.to(at::kLong)}).cpu().equal(at::tensor({m, (int64_t)0})),
                Code::ExecutionError, "radix join: exact rerun did not match its own count");
  } else if (sink) {
    sink->size = o.off + m;  // give back the estimate's slack
  }
  if (!sink) {
    for (auto &c : o.lcols)
      if (c.length > 0) c = c.slice(0, m);
    for (auto &c : o.rcols)
      if (c.length > 0) c = c.slice(0, m);
  }
  return true;
}

// Phase 6: the shared key column, the packed validity and the null side's validity; the table
static TablePtr finish_columns(const RadixJoinIn &in, const RadixJoinPlan &plan, const Partitioned &pt,
                               const SharedKey &share, JoinOutput &o) {
  const TablePtr &left = in.left, &right = in.right;
  std::vector<Column> &lcols = o.lcols, &rcols = o.rcols;
  const int64_t m = o.m, off = o.off;
  if (share.on) {
    Column &dst = plan.build_left ? lcols[share.kl] : rcols[share.kr];
    const Column &src = plan.build_left ? rcols[share.kr] : lcols[share.kl];
    dst.data = src.data;
    dst.length = src.length;
    trace::add_counter("join.radix.shared_key_column", 1);
  }
  if (m > 0) {
    unpack_validity_words(in.ex, left, pt.L, o.lwords, lcols, off, m);
    unpack_validity_words(in.ex, right, pt.R, o.rwords, rcols, off, m);
  }
  {  // outer joins: the null side's validity from the presence bytes
    const JoinType jt = in.cfg.GetType();
    const at::Tensor &lpres = plan.build_left ? o.bpres : o.ppres, &rpres = plan.build_left ? o.ppres : o.bpres;
    if (left_may_null(jt)) apply_presence(lcols, left, lpres, off, m, in.sink == nullptr);
    if (right_may_null(jt)) apply_presence(rcols, right, rpres, off, m, in.sink == nullptr);
  }
  trace::add_counter("join.radix.rows_out", m);
  if (plan.oj) trace::add_counter("join.radix.outer", plan.oj);
  if (in.sink) return Table::Make(left->GetContext(), in.sink->cols);
  for (auto &c : rcols) lcols.push_back(std::move(c));
  return Table::Make(left->GetContext(), std::move(lcols));
}

// Returns nullptr when a build partition overflows the LDS capacity (heavy key
// skew / duplicates); the caller then runs the global-table join.  With a sink the
// rows are written into the sink's columns and the sink's table is returned.
// Every column of both tables is fixed width (radix_eligible); lk / rk are the int64 join keys
// (a key column itself, or the composite image of several key columns).  All four join types:
// the kernels emit unmatched rows of the preserved side(s) with presence bytes (outer_mode).
//
// The phases, the failure exits (nullptr, or a raise once an input is released) that can still
// occur AFTER each, and whether an input may already be gone by then:
//   1. plan                 -- every exit below; no input released.
//   2. partition both sides -- a retain = false input of a sink-less join is released here: left
//      right after its own passes (before the right side's), right after its own, each only when its
//      slots held and no key seen so far left the narrowed range (the right keys' range is checked
//      before left goes).  The narrow and slot-overflow retries come after both and read the inputs.
//      After it: prepartitioned slot overflow (3), order violation and LDS overflow (4), LDS
//      overflow found by the write (5).  From here on an input may be gone: those exits raise.
//   3. skew masks and split items -- exits of 4 and 5 remain.
//   4. count                -- the write's LDS overflow (5, cursor mode only) remains.
//   5. allocate and write   -- none; the estimate rerun is not an exit.
//   6. finish columns       -- none.
TablePtr radix_join(const Exec &ex, const TablePtr &left, const TablePtr &right, at::Tensor lk, at::Tensor rk,
                    const JoinConfig &cfg, JoinSink *sink, bool hashed_key) {
  const RadixJoinIn in{ex, left, right, cfg, sink, sink ? sink->pre : nullptr};
  const PrePartition *pre = in.pre;
  const int64_t nl = left->Rows(), nr = right->Rows();
  const bool build_left = nl < nr;
  // ---- 1. plan
  const std::vector<int> lkeys = pre ? std::vector<int>() : key_columns(left, lk);
  const std::vector<int> rkeys = pre ? std::vector<int>() : key_columns(right, rk);
  // narrowing needs the key to be exactly ONE int64 column of its side (a key buffer the table holds
  // twice is not narrowed)
  auto own_key_column = [](const TablePtr &t, const std::vector<int> &keys) {
    return std::count_if(keys.begin(), keys.end(), [&](int c) { return int64_column(t->column(c)); }) == 1;
  };
  // (a hashed key -- the invertible string word key a proxy carries as a column -- never fits 32 bits)
  const bool want_narrow = pre != nullptr || (!hashed_key && nl > 0 && nr > 0 && lk.scalar_type() == at::kLong &&
                                              rk.scalar_type() == at::kLong && own_key_column(left, lkeys) &&
                                              own_key_column(right, rkeys));
  Narrowing nw;
  if (want_narrow) {
    nw.bad = at::zeros({1}, ex.opts(at::kInt));
    nw.base_src = pre ? pre->base_src : lk.slice(0, 0, 1).clone();
  }
  // the build side's columns that are the key array itself (every 8-byte column on the key's buffer)
  const TablePtr &bt = build_left ? left : right;
  std::vector<bool> build_is_key(bt->Columns(), false);
  if (pre) build_is_key = (build_left ? pre->L : pre->R).is_key;
  else
    for (int c : build_left ? lkeys : rkeys) build_is_key[(size_t)c] = bt->column(c).type.width() == 8;
  RadixJoinPlan plan = plan_radix_join(left, right, build_is_key, want_narrow, cfg.GetType(), pre ? pre->bits : -1);
  if (plan.narrow) {
    nw.nk.base_src = ptr<int64_t>(nw.base_src);
    nw.nk.bad = reinterpret_cast<unsigned int *>(nw.bad.data_ptr<int>());
  }
  // the shared output key: as above and non-null (only a table that holds the key's buffer a second
  // time under a validity mask tells the two conditions apart; kept as it was), same type on both sides
  auto share_col = [](const TablePtr &t, const std::vector<int> &keys) {
    int idx = -1, hits = 0;
    for (int c : keys)
      if (int64_column(t->column(c)) && !t->column(c).nullable()) idx = c, ++hits;
    return hits == 1 ? idx : -1;
  };
  SharedKey share;
  share.kl = share_col(left, lkeys);
  share.kr = share_col(right, rkeys);
  share.on = plan.oj == 0 && !sink && share.kl >= 0 && share.kr >= 0 &&
             left->column(share.kl).type == right->column(share.kr).type && knobs::Flag("RJ_SHARE_KEY", true);
  // ---- 2. partition both sides
  Partitioned pt;
  if (pre) {
    pt.L = pre->L;
    pt.R = pre->R;
  } else {
    pt = partition_sides(in, plan, lk, rk, nw);
  }
  const RadixSide &B = build_left ? pt.L : pt.R, &P = build_left ? pt.R : pt.L;
  // ---- 3. skew masks and split items
  SplitWork work;
  if (!split_skewed(in, plan, B, P, pt.sk, work)) return nullptr;
  // ---- 4. count
  const JoinLaunch jl{ex, plan, P, B, plan.narrow ? ptr<int64_t>(nw.base_src) : nullptr,
                      at::empty({1}, ex.opts(at::kInt))};
  JoinOutput out;
  if (!count_output(jl, work, pt.released, out)) return nullptr;
  // ---- 5. allocate and write, 6. finish columns
  CYLON_PHASE("join.radix.write", ex.device);
  if (!allocate_and_write(in, jl, pt, share, work, out)) return nullptr;
  return finish_columns(in, plan, pt, share, out);
}

}  // namespace ops
}  // namespace cylon
