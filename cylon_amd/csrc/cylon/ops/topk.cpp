// Top-k row selection (ORDER BY cols LIMIT k; docs/semantics.md "Top-k"): exactly the rows, and
// the row order, of Slice(GatherNullable(t, SortIndices(t, cols, ascending)), 0, min(k, rows)).
//
// One fixed-width numeric order column takes the radix select of kernels/topk.hip: the key column is
// read a few times, no row is moved, and the payload columns are touched by one gather of k rows.
// Everything else (several order columns, string / binary / fixed-bytes keys, a large k, a small
// table) is that definition itself, through the stable index sort.
//
// Context config keys (not CYLON_* knobs), defaults from the measured crossovers (docs/design.md §3.3,
// profiles/r07/topk.txt):
//   topk_select_min_rows  fewest rows for the select path                         (default 2^23)
//   topk_candidates       stop refining once the threshold bucket is this small   (default 2^16)
//   topk_max_k            largest k for the select path                           (default 2^22)
//   topk_rows_per_k       ... and k <= rows / this: the k rows are sorted and gathered at about 60
//                         times the per-row cost of the row-moving sort           (default 64)
#include <algorithm>
#include <cstdlib>

#include "../trace.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

namespace {

int64_t config_i64(const std::shared_ptr<CylonContext> &ctx, const char *key, int64_t def) {
  const std::string v = ctx->GetConfig(key, "");
  if (v.empty()) return def;
  char *end = nullptr;
  const long long x = std::strtoll(v.c_str(), &end, 10);
  CYLON_CHECK(end != v.c_str() && *end == '\0' && x >= 0, Code::Invalid, "config " << key << " = '" << v << "'");
  return (int64_t)x;
}

int ceil8(int bits) { return std::max(8, (bits + 7) / 8 * 8); }

// (image, row) pairs in ascending (image, row) order: a sort by the row, then a stable one by the image
std::pair<at::Tensor, at::Tensor> sort_image_row(const Exec &ex, at::Tensor img, at::Tensor row, int img_bits,
                                                 int row_bits) {
  if (img.numel() <= 1) return {img, row};
  auto by_row = RadixSortPairs(ex, std::move(row), std::move(img), ceil8(row_bits));  // keys = rows
  return RadixSortPairs(ex, std::move(by_row.second), std::move(by_row.first), ceil8(img_bits));
}

TablePtr topk_by_sort(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &asc, int64_t k) {
  trace::add_counter("topk.sort_fallback", 1);
  at::Tensor idx = SortIndices(t, cols, asc);
  return GatherNullable(t, idx.slice(0, 0, std::min(k, t->Rows())), false);
}

bool select_key(const Column &c) {
  if (c.is_var() || !c.type.is_numeric()) return false;
  const int w = c.type.width();
  return (w == 1 || w == 2 || w == 4 || w == 8) && c.data.defined() && c.data.is_contiguous() &&
         c.data.numel() * (int64_t)c.data.element_size() == c.length * w;
}

struct SelectState {
  int64_t krem, sure, bucket, nonnull, cur_sure, cur_cand, error;
  int ilo, rlo;
  uint64_t bits_or, bits_and;
};

SelectState read_state(const Exec &ex, const at::Tensor &ws) {
  const std::vector<int64_t> h = to_host_vec(ws.slice(0, 0, (ex.gpu ? hip::topk_state_words() : cpu::topk_state_words())));
  SelectState s;
  s.ilo = (int)h[1];
  s.rlo = (int)h[4];
  s.krem = h[6];
  s.sure = h[7];
  s.bucket = h[8];
  s.nonnull = h[9];
  s.bits_or = (uint64_t)h[10];
  s.bits_and = (uint64_t)h[11];
  s.cur_sure = h[12];
  s.cur_cand = h[13];
  s.error = h[14];
  return s;
}

// the first k rows of the stable sort by column col, k < rows: their row numbers, in order
at::Tensor select_rows(const TablePtr &t, int col, bool asc, int64_t k, int64_t candidates) {
  Exec ex(t->device());
  CYLON_PHASE("topk.select", ex.device);
  const Column &kc = t->column(col);
  const ColView kv = kc.view();
  const int64_t n = t->Rows();
  const bool desc = !asc;
  const int D = (ex.gpu ? hip::topk_digit_bits() : cpu::topk_digit_bits());
  at::Tensor ws = ex.empty_i64((ex.gpu ? hip::topk_workspace() : cpu::topk_workspace()));
  int64_t key_reads = 1, passes = 0;
  KCALL(ex, topk_scan, kv, n, desc, ptr<int64_t>(ws));
  SelectState st = read_state(ex, ws);
  const int64_t take = std::min(k, st.nonnull);
  at::Tensor rows = ex.empty_i64(0);
  if (take > 0) {
    // passes run over the image bits that vary, from the highest down; bits outside [ifloor, ihi)
    // are the same in every non-null row
    const uint64_t diff = st.bits_or ^ st.bits_and;
    const int ihi = diff ? 64 - __builtin_clzll(diff) : 0, ifloor = diff ? __builtin_ctzll(diff) : 0;
    const int rbits = n > 1 ? 64 - __builtin_clzll((uint64_t)(n - 1)) : 0;
    KCALL(ex, topk_start, ptr<int64_t>(ws), take, ihi, rbits);
    st.bucket = st.nonnull;
    st.ilo = ihi;
    st.rlo = rbits;
    st.krem = take;
    st.sure = 0;
    // image bits exhausted: every row of the bucket is an exact tie, and the row number decides
    while (st.bucket > candidates && (st.ilo > ifloor || st.rlo > 0)) {
      const int src = st.ilo > ifloor ? 0 : 1;
      const int db = std::min(D, src ? st.rlo : st.ilo - ifloor);
      KCALL(ex, topk_hist, kv, n, desc, ptr<int64_t>(ws), src, db);
      KCALL(ex, topk_pick, ptr<int64_t>(ws), src, db);
      st = read_state(ex, ws);
      CYLON_CHECK(st.error == 0, Code::ExecutionError, "top-k select: histogram short of k (" << st.error << ")");
      ++passes;
      ++key_reads;
    }
    at::Tensor simg = ex.empty_i64(st.sure), srow = ex.empty_i64(st.sure);
    at::Tensor cimg = ex.empty_i64(st.bucket), crow = ex.empty_i64(st.bucket);
    KCALL(ex, topk_collect, kv, n, desc, ptr<int64_t>(ws), reinterpret_cast<uint64_t *>(ptr<int64_t>(simg)),
          ptr<int64_t>(srow), st.sure, reinterpret_cast<uint64_t *>(ptr<int64_t>(cimg)), ptr<int64_t>(crow), st.bucket);
    ++key_reads;
    const SelectState end = read_state(ex, ws);
    CYLON_CHECK(end.error == 0 && end.cur_sure == st.sure && end.cur_cand == st.bucket, Code::ExecutionError,
                "top-k select: collected " << end.cur_sure << " + " << end.cur_cand << " rows, expected " << st.sure
                                           << " + " << st.bucket);
    auto cand = sort_image_row(ex, cimg, crow, ihi, rbits);
    at::Tensor aimg = cand.first.slice(0, 0, st.krem), arow = cand.second.slice(0, 0, st.krem);
    if (st.sure > 0) {
      aimg = at::cat({simg, aimg});
      arow = at::cat({srow, arow});
    } else {
      aimg = aimg.contiguous();
      arow = arow.contiguous();
    }
    rows = sort_image_row(ex, aimg, arow, ihi, rbits).second;
  }
  if (take < k) {  // fewer than k non-null keys: nulls follow in row order
    at::Tensor nulls = MaskToIndices(kc.validity, true).slice(0, 0, k - take);
    rows = at::cat({rows, nulls});
    trace::add_counter("topk.null_fill", 1);
  }
  trace::add_counter("topk.select", 1);
  trace::add_counter("topk.passes", passes);
  trace::add_counter("topk.key_reads", key_reads);
  return rows;
}

}  // namespace

TablePtr TopK(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending, int64_t k) {
  CYLON_CHECK(k >= 0, Code::Invalid, "top-k needs k >= 0, got " << k);
  CYLON_CHECK(!cols.empty(), Code::Invalid, "top-k needs at least one order column");
  const std::vector<bool> asc = ascending.empty() ? std::vector<bool>{true} : ascending;
  CYLON_CHECK(asc.size() == cols.size() || asc.size() == 1, Code::Invalid, "ascending flags must match order columns");
  for (int c : cols) CYLON_CHECK(c >= 0 && c < t->Columns(), Code::Invalid, "top-k order column " << c);
  const int64_t n = t->Rows();
  if (k == 0 || n == 0) return Slice(t, 0, 0);
  auto ctx = t->GetContext();
  const bool eligible = cols.size() == 1 && k < n && select_key(t->column(cols[0])) &&
                        n >= config_i64(ctx, "topk_select_min_rows", int64_t(1) << 23) &&
                        k <= config_i64(ctx, "topk_max_k", int64_t(1) << 22) &&
                        k <= n / std::max<int64_t>(1, config_i64(ctx, "topk_rows_per_k", 64));
  if (!eligible) return topk_by_sort(t, cols, asc, k);
  const int64_t candidates = std::max<int64_t>(1, config_i64(ctx, "topk_candidates", int64_t(1) << 16));
  return GatherNullable(t, select_rows(t, cols[0], asc[0], k, candidates), false);
}

TablePtr DistributedTopK(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending,
                         int64_t k) {
  CYLON_CHECK(k >= 0, Code::Invalid, "top-k needs k >= 0, got " << k);
  auto ctx = t->GetContext();
  const int W = ctx->GetWorldSize();
  if (W <= 1) return TopK(t, cols, ascending, k);
  // at most k rows per rank travel to rank 0; they arrive rank-major, so rank 0's stable top-k breaks
  // global ties by (rank, local row number)
  TablePtr local = TopK(t, cols, ascending, k);
  std::vector<int64_t> counts(W, 0);
  counts[0] = local->Rows();
  TablePtr recv = AllToAllTable(local, counts);
  if (ctx->GetRank() != 0) return recv->Rows() == 0 ? recv : Slice(recv, 0, 0);
  return TopK(recv, cols, ascending, k);
}

}  // namespace ops
}  // namespace cylon
