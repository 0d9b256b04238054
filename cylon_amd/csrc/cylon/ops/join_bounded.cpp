// ---------------------------------------------------------------------------
// Bounded memory.  radix_join's working set -- both sides' partitioned copies (the
// second pass's slots) plus the first pass's transient copy of one side -- and its output are sized
// against the device headroom (free HBM + the caching allocator's cached blocks; config
// "memory_budget_mb" caps it).  When they do not fit, the join runs in C key-hash chunks: rows whose
// multiplicative key hash falls in chunk c are gathered from both sides, partitioned and joined into
// ONE output sink allocated for the whole result, so the peak is inputs + output + ~1/C of the
// working set (plus the chunk copies) instead of inputs + output + the whole working set.  The
// output size is estimated from an exactly joined 1/1024 key-hash sample when it matters.
// Reference: the retain=false release of shuffled inputs, table.cpp:150-155.
// ---------------------------------------------------------------------------
#include "cylon/knobs.hpp"
#include <algorithm>
#include <cmath>

#include "join_internal.hpp"
#include "radix_sizing.hpp"
#include "../trace.hpp"

namespace cylon {
namespace ops {

static int64_t radix_row_bytes(const TablePtr &t) {
  int64_t b = 0;
  for (const auto &c : t->columns()) b += c.type.width() + (c.nullable() ? 1 : 0);
  return std::max<int64_t>(b, 8);
}

static at::Tensor key_chunk_ids(const at::Tensor &k, int64_t C) {  // independent of fmix64 / fmix32 bits
  at::Tensor h = k * (int64_t)0x9E3779B97F4A7C15ull;
  return at::bitwise_and(at::bitwise_right_shift(h, 32), 0x7fffffff).remainder(C);
}

int radix_join_chunks(const Exec &ex, const TablePtr &l, const TablePtr &r, const at::Tensor &lk, const at::Tensor &rk,
                      JoinType jt) {
  if (!ex.gpu) return 1;
  const int64_t head = l->GetContext()->DeviceHeadroom();
  if (head <= 0) return 1;
  const int64_t nl = l->Rows(), nr = r->Rows();
  const int64_t bl = radix_row_bytes(l) * nl, br = radix_row_bytes(r) * nr;
  const int64_t work = (int64_t)(1.17 * (double)(bl + br)) + (int64_t)(1.03 * (double)std::max(bl, br));
  const int64_t out_row = radix_row_bytes(l) + radix_row_bytes(r);
  const double budget = 0.92 * (double)head;
  // one output row per row of the larger side, with room to spare (plus every preserved row of an
  // outer join): no estimate needed
  const int64_t outer_rows = (jt == JoinType::LEFT || jt == JoinType::FULL_OUTER ? nl : 0) +
                             (jt == JoinType::RIGHT || jt == JoinType::FULL_OUTER ? nr : 0);
  if ((double)work + (1.5 * (double)std::max(nl, nr) + (double)outer_rows) * (double)out_row <= budget) return 1;
  int64_t est = 0;
  {  // exact join of a 1/1024 hash sample of both key sets, scaled up
    at::Tensor sl = at::bitwise_and(at::bitwise_right_shift(lk * (int64_t)0x632BE59BD9B4E019ll, 40), 1023).eq(0);
    at::Tensor sr = at::bitwise_and(at::bitwise_right_shift(rk * (int64_t)0x632BE59BD9B4E019ll, 40), 1023).eq(0);
    auto pr = hash_join_pairs(ex, lk.masked_select(sl), rk.masked_select(sr));
    est = (int64_t)(1.1 * 1024.0 * (double)pr.first.numel()) + 65536;
  }
  // the sample counts matched pairs only: an outer join also emits its preserved side's unmatched
  // rows -- up to all of them (a low-match join), so they are added in full
  est += outer_rows;
  const double out_bytes = (double)est * (double)out_row;
  if ((double)work + out_bytes <= budget) return 1;
  const double room = budget - out_bytes;
  const int C = room <= 0 ? 64 : (int)std::min<double>(64.0, std::ceil((double)(work + bl + br) / room));
  trace::add_counter("join.radix.memory_chunks", C);
  trace::add_counter("join.radix.estimated_output_rows", est);
  return std::max(C, 2);
}

// (column, its validity bytes?) of every buffer of t that moves with the key in a row-moving pass:
// each column's data but the key column's own, and each nullable column's validity
using MovingBuffer = std::pair<int, bool>;
static std::vector<MovingBuffer> moving_buffers(const TablePtr &t, int key_col) {
  std::vector<MovingBuffer> ent;
  for (int c = 0; c < t->Columns(); ++c) {
    if (c != key_col) ent.push_back({c, false});
    if (t->column(c).nullable()) ent.push_back({c, true});
  }
  return ent;
}

// Column groups: a pass moves the key plus <= 3 other buffers, and the group's input buffers
// are released before the next group's pass, so the side's copy reuses its own input's memory
// (peak: the inputs + one group's copies, not the inputs + a whole second copy).  With several
// groups the passes rank stably (exact tile offsets, stable in-tile order): every group's rows
// land where the first group's did, the later passes rewriting the same keys in place.
// pass(g, e0, e1, stable) moves ent[e0, e1); returns the number of groups.
template <class Pass>
static size_t for_column_groups(const TablePtr &t, const std::vector<MovingBuffer> &ent, Pass pass) {
  constexpr size_t kGroup = 3;
  const size_t ngroups = std::max<size_t>(1, (ent.size() + kGroup - 1) / kGroup);
  const bool stable = ngroups > 1;
  for (size_t g = 0; g < ngroups; ++g) {
    const size_t e0 = ent.size() * g / ngroups, e1 = ent.size() * (g + 1) / ngroups;
    pass(g, e0, e1, stable);
    if (stable)
      for (size_t e = e0; e < e1; ++e) t->ReleaseBufferIfNotRetained(ent[e].first, ent[e].second);
  }
  return ngroups;
}

// Bounded memory with retain = false and an int64 key column per side: the chunk pass IS the join's
// first radix pass -- every column moved once by the HIGH db1 bits of the narrowed partition hash
// (exact, so each first-level bucket is a contiguous row range; column groups with stable passes as
// in the chunk-major path, releasing each group's input buffers) -- and chunk c is a range of
// consecutive first-level buckets.  Per chunk only the slot second pass runs (radix_slot_segment_pass
// over its buckets) and radix_join joins the prepartitioned chunk into the sink (JoinSink::pre):
// the rows cross HBM in two passes, as in the unbounded join, instead of three (chunk-major pass +
// the chunk's own two passes).  nullptr when not applicable (the caller takes the chunk-major path).
static TablePtr radix_join_first_pass_chunks(const Exec &ex, const TablePtr &l, const TablePtr &r, const at::Tensor &lk,
                                             const at::Tensor &rk, int lkc, int rkc, const JoinConfig &cfg, int C,
                                             bool hashed_key) {
  if (l->IsRetain() || r->IsRetain() || hashed_key || lkc < 0 || rkc < 0 || lk.scalar_type() != at::kLong ||
      rk.scalar_type() != at::kLong || !knobs::Flag("RJ_FIRST_PASS_CHUNKS", true))
    return nullptr;
  // (nullable columns take the chunk-major path: radix_join sizes the LDS rows for packed validity
  // words, which these partitions do not carry)
  for (const TablePtr &t : {l, r})
    for (const auto &c : t->columns())
      if (c.is_var() || c.type.width() > 8 || c.nullable()) return nullptr;
  const int64_t nl = l->Rows(), nr = r->Rows();
  if (nl < (int64_t(1) << 20) || nr < (int64_t(1) << 20)) return nullptr;
  // the narrowed-key range, checked before anything is released: [base, base + 2^32), base = (left
  // key 0) - 2^31, as in radix_join
  const at::Tensor base_src = lk.slice(0, 0, 1).clone();
  {
    auto ml = at::aminmax(lk), mr = at::aminmax(rk);
    const at::Tensor h = at::stack({std::get<0>(ml), std::get<1>(ml), std::get<0>(mr), std::get<1>(mr), base_src[0]}).cpu();
    const int64_t base = h[4].item<int64_t>() - (int64_t(1) << 31);
    for (int i = 0; i < 4; ++i) {
      const int64_t v = h[i].item<int64_t>();
      if (v < base || (uint64_t)(v - base) > 0xffffffffull) return nullptr;
    }
  }
  // the whole join's sizes as radix_join plans them on narrowed keys.  The key is the ONE column this
  // path found on the key's buffer (lkc / rkc): a second column on the same buffer moves as data
  // here, where radix_join would treat it as the key too and not narrow at all.
  const bool build_left = nl < nr;
  std::vector<bool> build_is_key((build_left ? l : r)->Columns(), false);
  build_is_key[(size_t)(build_left ? lkc : rkc)] = true;
  const RadixJoinPlan plan = plan_radix_join(l, r, build_is_key, /*narrow=*/true, cfg.GetType());
  const int bits = plan.bits;
  const int db1 = sizing::digit_split(bits).db1, db2 = sizing::digit_split(bits).db2;
  if (bits < 11 || db1 > 10) return nullptr;
  int cbits = 1;  // chunks: twice what the retained-input budget asks for, as the chunk-major path
  while ((1 << cbits) < 2 * C) ++cbits;
  cbits = std::min(cbits, db1);
  const int gbits = db1 - cbits;  // first-level buckets per chunk: 2^gbits
  if ((1 << gbits) > 4096) return nullptr;
  at::Tensor narrow_bad = at::zeros({1}, ex.opts(at::kInt));
  hip::NarrowKeys nk;
  nk.base_src = ptr<int64_t>(base_src);
  nk.bad = reinterpret_cast<unsigned int *>(narrow_bad.data_ptr<int>());
  // ---- first pass of each side, column group by column group
  struct First {
    at::Tensor keys;                     // uint32 offsets, first-level bucket order
    std::vector<at::Tensor> data, valid;  // per column (data of the key column: undefined)
    std::vector<int64_t> boff;            // 2^db1 + 1 bucket starts
    at::Tensor boff_dev;                  // the same on the device
    int64_t n = 0;
  };
  auto first_pass = [&](const TablePtr &t, const at::Tensor &k, int kc) {
    First f;
    f.n = t->Rows();
    f.data.resize((size_t)t->Columns());
    f.valid.resize((size_t)t->Columns());
    const std::vector<MovingBuffer> ent = moving_buffers(t, kc);
    f.keys = at::empty({f.n}, ex.opts(at::kInt));
    at::Tensor ws = ex.empty_i64(hip::radix_rows_pass_workspace(f.n, db1));
    for_column_groups(t, ent, [&](size_t, size_t e0, size_t e1, bool stable) {
      std::vector<const uint8_t *> in{reinterpret_cast<const uint8_t *>(k.data_ptr())};
      std::vector<uint8_t *> out{reinterpret_cast<uint8_t *>(f.keys.data_ptr())};
      std::vector<int> widths{8};
      for (size_t e = e0; e < e1; ++e) {
        const Column &col = t->column(ent[e].first);
        const at::Tensor &src = ent[e].second ? col.validity : col.data;
        at::Tensor dst = at::empty_like(src);
        in.push_back(reinterpret_cast<const uint8_t *>(src.data_ptr()));
        out.push_back(reinterpret_cast<uint8_t *>(dst.data_ptr()));
        widths.push_back(ent[e].second ? 1 : col.type.width());
        (ent[e].second ? f.valid : f.data)[(size_t)ent[e].first] = dst;
      }
      hip::radix_rows_pass(reinterpret_cast<const int64_t *>(k.data_ptr()), f.n, bits, db2, db1, in.data(), out.data(),
                           widths.data(), (int)in.size(), ptr<int64_t>(ws), ex.stream, stable, nullptr, 0, &nk);
    });
    at::Tensor offs = ex.empty_i64((int64_t(1) << db1) + 1);
    hip::radix_part_offsets32(reinterpret_cast<const uint32_t *>(f.keys.data_ptr()), f.n, db1, ptr<int64_t>(offs),
                              ex.stream);
    f.boff = to_host_vec(offs);
    f.boff_dev = offs;
    return f;
  };
  First fl = first_pass(l, lk, lkc);
  l->ReleaseIfNotRetained();
  First fr = first_pass(r, rk, rkc);
  r->ReleaseIfNotRetained();
  trace::add_counter("join.radix.released_inputs", 2);
  trace::add_counter("join.radix.first_pass_chunks", int64_t(1) << cbits);
  CYLON_CHECK(narrow_bad.item<int>() == 0, Code::ExecutionError, "first-pass chunks: a key left the narrowed range");
  // schema tables of a chunk (names, types, nullability; the data lives in the partitions)
  auto schema = [&](const TablePtr &t, int64_t rows) {
    std::vector<Column> cols;
    for (const auto &c : t->columns())
      cols.emplace_back(c.name, c.type, rows, at::empty({0}, c.data.options()), at::Tensor(),
                        c.nullable() ? at::empty({0}, ex.opts(at::kByte)) : at::Tensor());
    return Table::Make(t->GetContext(), std::move(cols));
  };
  // second pass of one side's chunk [b0, b1) of first-level buckets -> its RadixSide
  auto second_pass = [&](const TablePtr &t, const First &f, int kc, int64_t b0, int64_t b1, int64_t slot) {
    const int64_t r0 = f.boff[(size_t)b0], r1 = f.boff[(size_t)b1], n = r1 - r0;
    const int nseg = (int)(b1 - b0);
    const int64_t nslots = int64_t(nseg) << db2;
    RadixSide s;
    std::vector<const uint8_t *> in{reinterpret_cast<const uint8_t *>(ptr<int32_t>(f.keys) + r0)};
    std::vector<int> widths{4};
    const std::vector<MovingBuffer> ent = moving_buffers(t, kc);
    for (const auto &e : ent) {
      const at::Tensor &src = e.second ? f.valid[(size_t)e.first] : f.data[(size_t)e.first];
      const int w = e.second ? 1 : t->column(e.first).type.width();
      in.push_back(reinterpret_cast<const uint8_t *>(src.data_ptr()) + r0 * w);
      widths.push_back(w);
    }
    s.data.assign((size_t)t->Columns(), at::Tensor());
    s.valid.assign((size_t)t->Columns(), at::Tensor());
    s.is_key.assign((size_t)t->Columns(), false);
    s.vpos.assign((size_t)t->Columns(), -1);
    if (n == 0) {  // (an empty chunk side: empty partitions)
      s.keys = at::empty({0}, ex.opts(at::kInt));
      s.offs = at::zeros({nslots}, ex.opts(at::kLong));
      s.slot = 1;
      s.overflow = at::zeros({1}, ex.opts(at::kInt));
      for (int c = 0; c < t->Columns(); ++c) {
        s.is_key[(size_t)c] = c == kc;
        s.data[(size_t)c] = c == kc ? s.keys : at::empty({0}, t->column(c).data.options());
        if (t->column(c).nullable()) s.valid[(size_t)c] = at::empty({0}, ex.opts(at::kByte));
      }
      return s;
    }
    const at::Tensor bb = (f.boff_dev.slice(0, b0, b1) - r0).to(at::kInt);  // (device: no host copy per chunk)
    const int64_t rows = nslots * slot + hip::radix_slot_tile_rows();
    std::vector<at::Tensor> fin;
    std::vector<uint8_t *> out;
    fin.push_back(at::empty({rows}, ex.opts(at::kInt)));
    out.push_back(reinterpret_cast<uint8_t *>(fin.back().data_ptr()));
    for (const auto &e : ent) {
      const at::Tensor &src = e.second ? f.valid[(size_t)e.first] : f.data[(size_t)e.first];
      fin.push_back(at::empty({rows}, src.options()));
      out.push_back(reinterpret_cast<uint8_t *>(fin.back().data_ptr()));
    }
    int fbits = 0;
    while ((1 << fbits) < nseg) ++fbits;
    at::Tensor ws = ex.empty_i64(hip::radix_slot_workspace(std::max(1, fbits), db2));
    s.offs = ex.empty_i64(nslots);
    s.overflow = at::zeros({1}, ex.opts(at::kInt));
    hip::NarrowKeys nk2 = nk;
    nk2.kin4 = 1;
    hip::radix_slot_segment_pass(reinterpret_cast<const uint32_t *>(ptr<int32_t>(f.keys) + r0), n, bits, db2, in.data(),
                                 out.data(), widths.data(), (int)in.size(),
                                 reinterpret_cast<const uint32_t *>(bb.data_ptr<int>()), nseg, slot, ptr<int64_t>(ws),
                                 ptr<int64_t>(s.offs), reinterpret_cast<unsigned int *>(s.overflow.data_ptr<int>()),
                                 ex.stream, &nk2);
    s.slot = slot;
    s.keys = fin[0];
    for (int c = 0; c < t->Columns(); ++c) {
      s.is_key[(size_t)c] = c == kc;
      if (c == kc) s.data[(size_t)c] = s.keys;
    }
    for (size_t j = 0; j < ent.size(); ++j) (ent[j].second ? s.valid : s.data)[(size_t)ent[j].first] = fin[1 + j];
    return s;
  };
  JoinSink sink;
  sink.chunks_total = 1 << cbits;
  sink.sample_skew = false;
  const int64_t ls = plan.slot_l, rs = plan.slot_r;
  for (int64_t c = 0; c < (int64_t(1) << cbits); ++c) {
    const int64_t b0 = c << gbits, b1 = (c + 1) << gbits;
    PrePartition pp;
    pp.bits = gbits + db2;
    pp.base_src = base_src;
    int64_t lslot = ls, rslot = rs;
    const TablePtr ls_t = schema(l, fl.boff[(size_t)b1] - fl.boff[(size_t)b0]);
    const TablePtr rs_t = schema(r, fr.boff[(size_t)b1] - fr.boff[(size_t)b0]);
    for (int attempt = 0;; ++attempt) {
      pp.L = second_pass(l, fl, lkc, b0, b1, lslot);
      pp.R = second_pass(r, fr, rkc, b0, b1, rslot);
      pp.overflowed = false;
      sink.pre = &pp;
      const bool done = radix_join(ex, ls_t, rs_t, pp.L.keys, pp.R.keys, cfg, &sink) != nullptr;
      sink.pre = nullptr;
      if (done) break;
      CYLON_CHECK(pp.overflowed && attempt == 0, Code::ExecutionError,
                  "radix join of a first-pass chunk of released (retain = false) inputs did not complete");
      // a partition beyond its slot (skewed keys; radix_join saw the flags and wrote nothing): the
      // overflowing side again with slots as large as the chunk's largest first-level bucket (which
      // bounds every partition of the chunk)
      trace::add_counter("join.radix.slot_overflow", 1);
      auto widest = [&](const First &f) {
        int64_t m = 0;
        for (int64_t b = b0; b < b1; ++b) m = std::max(m, f.boff[(size_t)b + 1] - f.boff[(size_t)b]);
        return (m + 7) & ~int64_t(7);
      };
      if (pp.overflow_l) lslot = std::max<int64_t>(lslot, widest(fl));
      if (pp.overflow_r) rslot = std::max<int64_t>(rslot, widest(fr));
    }
    ++sink.chunks_done;
  }
  return sink.finish(l->GetContext());
}

// the column of t that is the key tensor's buffer (the first, when a table holds the buffer twice:
// the bounded-memory passes move any other as data), -1: the key is no column of t
static int chunk_key_column(const TablePtr &t, const at::Tensor &k) {
  const std::vector<int> cols = key_columns(t, k);
  return cols.empty() ? -1 : cols[0];
}

TablePtr radix_join_chunked(const Exec &ex, const TablePtr &l, const TablePtr &r, const at::Tensor &lk,
                            const at::Tensor &rk, const JoinConfig &cfg, int C, bool hashed_key) {
  const int lkc = chunk_key_column(l, lk), rkc = chunk_key_column(r, rk);
  if (TablePtr t = radix_join_first_pass_chunks(ex, l, r, lk, rk, lkc, rkc, cfg, C, hashed_key)) return t;
  // retain = false on both inputs: one chunk-major pass per side (radix.cpp RadixChunkPartition: every
  // column, chunk = the LOW bits of fmix64(key)) whose input is released right after it, so each chunk
  // is a contiguous slice and the inputs are read once -- instead of a chunk-id filter + row gather
  // per chunk, whose gathers touch nearly every cache line of the inputs C times
  if (!l->IsRetain() && !r->IsRetain() && C <= 1024) {
    int cbits = 1;  // (twice the chunks the retained-input budget asks for: the copies and the output
    while ((1 << cbits) < 2 * C) ++cbits;  // hold ~inputs + output, so each chunk's working set must be small)
    const int64_t C2 = int64_t(1) << cbits;
    // (column groups: for_column_groups)
    auto chunk_major = [&](const TablePtr &t, const at::Tensor &k, int kc, at::Tensor &kout, std::vector<int64_t> &offs) {
      const std::vector<MovingBuffer> ent = moving_buffers(t, kc);
      std::vector<at::Tensor> dout(t->Columns()), vout(t->Columns());
      at::Tensor o;
      const size_t ngroups = for_column_groups(t, ent, [&](size_t g, size_t e0, size_t e1, bool stable) {
        std::vector<at::Tensor> sub{k};
        std::vector<int> widths{8};
        for (size_t e = e0; e < e1; ++e) {
          const Column &col = t->column(ent[e].first);
          sub.push_back(ent[e].second ? col.validity : col.data);
          widths.push_back(ent[e].second ? 1 : col.type.width());
        }
        std::vector<at::Tensor> res =
            RadixChunkPartition(ex, std::move(sub), widths, cbits, g == 0 ? &o : nullptr, g == 0 ? nullptr : &kout, stable);
        if (g == 0) kout = res[0];
        for (size_t e = e0; e < e1; ++e) (ent[e].second ? vout : dout)[(size_t)ent[e].first] = res[1 + e - e0];
      });
      offs = to_host_vec(o);
      std::vector<Column> cols;
      for (int c = 0; c < t->Columns(); ++c) {
        const Column &col = t->column(c);
        at::Tensor d = c == kc ? kout : dout[(size_t)c];
        if (c == kc && d.scalar_type() != col.data.scalar_type()) d = d.view(col.data.scalar_type());
        cols.emplace_back(col.name, col.type, kout.numel(), d, at::Tensor(), vout[(size_t)c]);
      }
      TablePtr res = Table::Make(t->GetContext(), std::move(cols));
      t->ReleaseIfNotRetained();
      trace::add_counter("join.radix.released_inputs", 1);
      if (ngroups > 1) trace::add_counter("join.radix.chunk_pass_groups", (int64_t)ngroups);
      return res;
    };
    at::Tensor lkp, rkp;
    std::vector<int64_t> lo, ro;
    TablePtr lp = chunk_major(l, lk, lkc, lkp, lo);
    TablePtr rp = chunk_major(r, rk, rkc, rkp, ro);
    trace::add_counter("join.radix.chunk_pass", 2);
    JoinSink sink;
    sink.chunks_total = (int)C2;
    sink.sample_skew = false;
    auto slice_tab = [&](const TablePtr &t, int64_t a, int64_t b) {
      std::vector<Column> cols;
      for (const auto &c : t->columns()) cols.push_back(c.slice(a, b - a));
      return Table::Make(t->GetContext(), std::move(cols));
    };
    for (int64_t c = 0; c < C2; ++c) {
      TablePtr lc = slice_tab(lp, lo[c], lo[c + 1]), rc = slice_tab(rp, ro[c], ro[c + 1]);
      const at::Tensor lkc_t = lkc >= 0 ? lc->column(lkc).data.view(at::kLong) : lkp.slice(0, lo[c], lo[c + 1]);
      const at::Tensor rkc_t = rkc >= 0 ? rc->column(rkc).data.view(at::kLong) : rkp.slice(0, ro[c], ro[c + 1]);
      CYLON_CHECK(radix_join(ex, lc, rc, lkc_t, rkc_t, cfg, &sink, hashed_key), Code::ExecutionError,
                  "radix join of a chunk of released (retain = false) inputs did not complete");
      ++sink.chunks_done;
    }
    return sink.finish(l->GetContext());
  }
  const at::Tensor cl = key_chunk_ids(lk, C), cr = key_chunk_ids(rk, C);
  JoinSink sink;
  sink.chunks_total = C;
  for (int c = 0; c < C; ++c) {
    at::Tensor il = cl.eq(c).nonzero().flatten(), ir = cr.eq(c).nonzero().flatten();
    TablePtr lc = Gather(l, il), rc = Gather(r, ir);
    const at::Tensor lkc_t = lkc >= 0 ? lc->column(lkc).data : lk.index_select(0, il);
    const at::Tensor rkc_t = rkc >= 0 ? rc->column(rkc).data : rk.index_select(0, ir);
    il = at::Tensor();
    ir = at::Tensor();
    if (!radix_join(ex, lc, rc, lkc_t, rkc_t, cfg, &sink, hashed_key)) return nullptr;
    ++sink.chunks_done;
  }
  return sink.finish(l->GetContext());
}

}  // namespace ops
}  // namespace cylon
