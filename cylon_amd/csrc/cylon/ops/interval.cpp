// Interval join (docs/semantics.md "Interval join"): every pair of a left row and a right row of its
// `by` group whose `on` value lies between the left row's `lower` and `upper`, ordered by left row,
// then right `on`, then right row.
//
// Only key rows are sorted, once, by the stable index sort: nr + 2 nl rows (by .., value) with value =
// on for a right row (R), lower for a left row's L-copy and upper for its U-copy.  Because the sort
// is stable the concatenation order decides how equal keys interleave, which is all `closed` changes:
//   BOTH      L ++ R ++ U   right rows equal to lower come after the L-copy, those equal to upper
//                           before the U-copy: both counted in
//   LEFT      L ++ U ++ R   a right row equal to upper comes after the U-copy: excluded
//   RIGHT     R ++ L ++ U   a right row equal to lower comes before the L-copy: excluded
//   NEITHER   U ++ R ++ L   both excluded
// The side of a sorted position is the range its perm entry falls in.  The rank pass
// (kernels/interval.hip interval_rank) counts the right rows before every position: lo[l] at the
// L-copy, hi[l] at the U-copy, and rrows = the right rows in sorted order.  `by` is the major sort key
// and null / NaN `on` values sort to the end of their group, so the rows of other groups and a group's
// unusable right rows lie outside [lo, hi) of every left row whose bounds are usable; interval_counts
// zeroes the others.  off = exclusive_scan(cnt), its last entry is read back once to size the output,
// and interval_expand writes the pairs: one block per tile of output rows, whatever the counts.
// Payload columns are neither sorted nor copied before the final gathers.  The GPU context always
// takes the kernels: there is no other device path.
#include "../trace.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

namespace {

// the as-of join's `on` types
bool on_type(const DataType &t) {
  switch (t.type) {
    case Type::UINT8:
    case Type::INT8:
    case Type::UINT16:
    case Type::INT16:
    case Type::UINT32:
    case Type::INT32:
    case Type::UINT64:
    case Type::INT64:
    case Type::FLOAT:
    case Type::DOUBLE:
    case Type::DATE32:
    case Type::DATE64:
    case Type::TIMESTAMP:
    case Type::TIME32:
    case Type::TIME64:
    case Type::DURATION: return true;
    default: return false;
  }
}

void check(const TablePtr &left, const TablePtr &right, int lower, int upper, int on, const std::vector<int> &left_by,
           const std::vector<int> &right_by, const IntervalOptions &o) {
  CYLON_CHECK(lower >= 0 && lower < left->Columns(), Code::Invalid, "interval join: `lower` column " << lower);
  CYLON_CHECK(upper >= 0 && upper < left->Columns(), Code::Invalid, "interval join: `upper` column " << upper);
  CYLON_CHECK(on >= 0 && on < right->Columns(), Code::Invalid, "interval join: `on` column " << on);
  CYLON_CHECK(left_by.size() == right_by.size(), Code::Invalid,
              "interval join: " << left_by.size() << " left and " << right_by.size() << " right `by` columns");
  CYLON_CHECK(left_by.size() + 1 <= (size_t)kMaxFusedCols, Code::Invalid,
              "interval join: more than " << kMaxFusedCols - 1 << " `by` columns");
  for (size_t i = 0; i < left_by.size(); ++i) {
    CYLON_CHECK(left_by[i] >= 0 && left_by[i] < left->Columns(), Code::Invalid,
                "interval join: left `by` column " << left_by[i]);
    CYLON_CHECK(right_by[i] >= 0 && right_by[i] < right->Columns(), Code::Invalid,
                "interval join: right `by` column " << right_by[i]);
    const DataType &lt = left->column(left_by[i]).type, &rt = right->column(right_by[i]).type;
    CYLON_CHECK(lt == rt, Code::Invalid,
                "interval join: `by` columns of types " << lt.ToString() << " and " << rt.ToString());
  }
  const DataType &lt = left->column(lower).type, &ut = left->column(upper).type, &rt = right->column(on).type;
  CYLON_CHECK(on_type(lt), Code::Invalid,
              "interval join: `lower`, `upper` and `on` must be integer, float32 / float64 or temporal columns, got "
                  << lt.ToString());
  CYLON_CHECK(lt == ut && lt == rt, Code::Invalid,
              "interval join: `lower`, `upper` and `on` of types " << lt.ToString() << ", " << ut.ToString() << " and "
                                                                  << rt.ToString());
  CYLON_CHECK(o.closed >= INTERVAL_BOTH && o.closed <= INTERVAL_NEITHER, Code::Invalid,
              "interval join: closed " << o.closed);
  CYLON_CHECK(o.how == INTERVAL_INNER || o.how == INTERVAL_LEFT_OUTER, Code::Invalid, "interval join: how " << o.how);
}

TablePtr key_rows(const TablePtr &t, const std::vector<int> &by, int value) {
  std::vector<int> cols = by;
  cols.push_back(value);
  return Project(t, cols);
}

// the rank pass's outputs: right rows sorted before each left row's L-copy / U-copy, and the right side in sorted order
struct Ranks {
  at::Tensor lo, hi, rrows;
};

Ranks rank(const Exec &ex, const TablePtr &left, const TablePtr &right, int lower, int upper, int on,
           const std::vector<int> &left_by, const std::vector<int> &right_by, int closed, int64_t step) {
  const int64_t nl = left->Rows(), nr = right->Rows(), n = nr + 2 * nl;
  const TablePtr L = key_rows(left, left_by, lower), U = key_rows(left, left_by, upper), R = key_rows(right, right_by, on);
  // the three blocks in concatenation order; each starts where the one before it ends
  std::vector<TablePtr> blocks;
  switch (closed) {
    case INTERVAL_BOTH: blocks = {L, R, U}; break;
    case INTERVAL_LEFT: blocks = {L, U, R}; break;
    case INTERVAL_RIGHT: blocks = {R, L, U}; break;
    default: blocks = {U, R, L}; break;
  }
  int64_t lbase = 0, rbase = 0, ubase = 0, at = 0;
  for (const TablePtr &b : blocks) {
    (b == L ? lbase : b == R ? rbase : ubase) = at;
    at += b->Rows();
  }
  TablePtr keys = Merge(blocks);
  blocks.clear();
  std::vector<int> all(keys->Columns());
  for (size_t c = 0; c < all.size(); ++c) all[c] = (int)c;
  at::Tensor perm = SortIndices(keys, all, std::vector<bool>(all.size(), true)).contiguous();
  if (reinterpret_cast<uintptr_t>(perm.data_ptr()) % 16 != 0) perm = perm.clone();  // the rank pass's 16-byte loads
  keys.reset();
  Ranks r{ex.empty_i64(nl), ex.empty_i64(nl), ex.empty_i64(nr)};
  at::Tensor ws = ex.empty_i64(KSIZE(ex, interval_rank_workspace, n));
  KCALL(ex, interval_rank, ptr<int64_t>(perm), nl, nr, lbase, rbase, ubase, step, ptr<int64_t>(ws), ptr<int64_t>(r.lo),
        ptr<int64_t>(r.hi), ptr<int64_t>(r.rrows));
  const int64_t T = KSIZE(ex, window_tile_rows);
  trace::add_counter("interval.sort", 1);
  trace::add_counter("interval.rank_tiles", (n + T - 1) / T);
  return r;
}

int64_t carry_step(const Exec &ex, int64_t carry_step_tiles) {
  const int64_t max_step = KSIZE(ex, window_carry_tiles);
  CYLON_CHECK(carry_step_tiles <= max_step, Code::Invalid,
              "interval join: carry step of " << carry_step_tiles << " tiles");
  return carry_step_tiles > 0 ? carry_step_tiles : max_step;
}

TablePtr assemble(const TablePtr &left, const TablePtr &right, const std::pair<at::Tensor, at::Tensor> &idx,
                  const IntervalOptions &o) {
  const TablePtr lo = Gather(left, idx.first);
  const TablePtr ro = GatherNullable(right, idx.second, o.how == INTERVAL_LEFT_OUTER);
  std::vector<Column> cols;
  cols.reserve(lo->Columns() + ro->Columns());
  for (const auto &c : lo->columns()) cols.push_back(c.with_name(o.left_prefix + c.name));
  for (const auto &c : ro->columns()) cols.push_back(c.with_name(o.right_prefix + c.name));
  return Table::Make(left->GetContext(), std::move(cols));
}

}  // namespace

at::Tensor IntervalJoinCounts(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper,
                              int right_on, const std::vector<int> &left_by, const std::vector<int> &right_by,
                              const IntervalOptions &options, int64_t carry_step_tiles) {
  check(left, right, left_lower, left_upper, right_on, left_by, right_by, options);
  CYLON_CHECK(left->device() == right->device(), Code::Invalid, "interval join: tables on different devices");
  Exec ex(left->device());
  const int64_t step = carry_step(ex, carry_step_tiles);
  const int64_t nl = left->Rows(), nr = right->Rows();
  if (nl == 0 || nr == 0) return at::zeros({nl}, ex.opts(at::kLong));
  CYLON_PHASE("interval", ex.device);
  const Ranks r = rank(ex, left, right, left_lower, left_upper, right_on, left_by, right_by, options.closed, step);
  at::Tensor cnt = ex.empty_i64(nl);
  KCALL(ex, interval_counts, left->column(left_lower).view(), left->column(left_upper).view(), ptr<int64_t>(r.lo),
        ptr<int64_t>(r.hi), nl, false, ptr<int64_t>(cnt), static_cast<uint8_t *>(nullptr),
        static_cast<int64_t *>(nullptr));
  return cnt;
}

std::pair<at::Tensor, at::Tensor> IntervalJoinIndices(const TablePtr &left, const TablePtr &right, int left_lower,
                                                      int left_upper, int right_on, const std::vector<int> &left_by,
                                                      const std::vector<int> &right_by,
                                                      const IntervalOptions &options, int64_t carry_step_tiles) {
  check(left, right, left_lower, left_upper, right_on, left_by, right_by, options);
  CYLON_CHECK(left->device() == right->device(), Code::Invalid, "interval join: tables on different devices");
  Exec ex(left->device());
  const int64_t step = carry_step(ex, carry_step_tiles);
  const int64_t nl = left->Rows(), nr = right->Rows();
  const bool outer = options.how == INTERVAL_LEFT_OUTER;
  if (nl == 0 || nr == 0) {  // no pairs: nothing, or one filler per left row
    if (!outer) return {ex.empty_i64(0), ex.empty_i64(0)};
    return {at::arange(nl, ex.opts(at::kLong)), at::full({nl}, -1, ex.opts(at::kLong))};
  }
  CYLON_PHASE("interval", ex.device);
  const Ranks r = rank(ex, left, right, left_lower, left_upper, right_on, left_by, right_by, options.closed, step);
  at::Tensor cnt = ex.empty_i64(nl), empty = outer ? ex.empty_u8(nl) : at::Tensor();
  at::Tensor counter = at::zeros({1}, ex.opts(at::kLong));
  KCALL(ex, interval_counts, left->column(left_lower).view(), left->column(left_upper).view(), ptr<int64_t>(r.lo),
        ptr<int64_t>(r.hi), nl, outer, ptr<int64_t>(cnt), outer ? ptr<uint8_t>(empty) : nullptr,
        ptr<int64_t>(counter));
  const at::Tensor off = exclusive_scan(ex, cnt);
  cnt = at::Tensor();
  const int64_t total = read_i64(off, nl);  // the one read-back: it sizes the output
  CYLON_CHECK(total >= 0 && total < (int64_t(1) << 62), Code::CapacityError,
              "interval join: the output would have " << total << " rows");
  at::Tensor li = ex.empty_i64(total), ri = ex.empty_i64(total);
  KCALL(ex, interval_expand, ptr<int64_t>(off), ptr<int64_t>(r.lo), outer ? ptr<uint8_t>(empty) : nullptr,
        ptr<int64_t>(r.rrows), nl, nr, total, ptr<int64_t>(li), ptr<int64_t>(ri));
  const int64_t T = KSIZE(ex, interval_tile_rows);
  trace::add_counter("interval.pairs", total);
  trace::add_counter("interval.matched", read_i64(counter, 0));
  trace::add_counter("interval.tiles", (total + T - 1) / T);
  return {li, ri};
}

TablePtr IntervalJoin(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper, int right_on,
                      const std::vector<int> &left_by, const std::vector<int> &right_by,
                      const IntervalOptions &options, int64_t carry_step_tiles) {
  return assemble(left, right,
                  IntervalJoinIndices(left, right, left_lower, left_upper, right_on, left_by, right_by, options,
                                      carry_step_tiles),
                  options);
}

TablePtr DistributedIntervalJoin(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper,
                                 int right_on, const std::vector<int> &left_by, const std::vector<int> &right_by,
                                 const IntervalOptions &options) {
  if (left->GetContext()->GetWorldSize() <= 1)
    return IntervalJoin(left, right, left_lower, left_upper, right_on, left_by, right_by, options);
  CYLON_CHECK(!left_by.empty(), Code::Invalid,
              "a distributed interval join needs a `by` column (a global order of the intervals is not supported)");
  check(left, right, left_lower, left_upper, right_on, left_by, right_by, options);  // every rank fails before the exchange, or none
  const auto sh = ShufflePair(left, left_by, right, right_by);
  return IntervalJoin(sh.first, sh.second, left_lower, left_upper, right_on, left_by, right_by, options);
}

}  // namespace ops
}  // namespace cylon
