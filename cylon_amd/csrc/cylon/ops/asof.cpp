// As-of join (docs/semantics.md "As-of join"): left's columns in left's row order, plus right's
// columns gathered from the nearest right row of the same group at or before (BACKWARD), at or after
// (FORWARD) or on either side (NEAREST) of the left row's `on` value.
//
// Only the key columns (by .. ++ on) of the two sides are concatenated and sorted, once, by the stable
// index sort; payload columns are never copied or sorted.  The side of a sorted row is perm[i] <
// nfirst, and because the sort is stable the concatenation order decides how equal (by, on) keys of
// the two sides interleave -- which is all that allow_exact_matches changes:
//   BACKWARD, exact      right ++ left, scanned in sort order     equal right rows come first: included
//   BACKWARD, no exact   left ++ right, scanned in sort order     equal right rows come after: excluded
//   FORWARD, exact       left ++ right, scanned in reverse        the last right seen is the lowest equal row
//   FORWARD, no exact    right ++ left, scanned in reverse        equal right rows are excluded
//   NEAREST, exact       right ++ left, both scans of one sort    an equal right row wins at distance 0
//                                                                 backwards, so forwards may exclude it
//   NEAREST, no exact    BACKWARD and FORWARD without exact matches: two sorts
// A scan is the segmented running maximum of kernels/asof.hip (asof_tile / window_carry / asof_apply)
// restarted at the partition heads (segment_heads over the by columns); it writes match[left row]
// directly.  asof_pick then makes the NEAREST choice and applies the tolerance; it is skipped when
// neither is asked for.  The matched rows are counted on the device by the last launch and read back
// once.  The GPU context always takes the kernels: there is no other device path.
#include "../trace.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

namespace {

constexpr int kMax = 3;  // kernels/window.hip WinFunc: the carry scan of a running maximum

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

void check(const TablePtr &left, const TablePtr &right, int left_on, int right_on, const std::vector<int> &left_by,
           const std::vector<int> &right_by, const AsofOptions &o) {
  CYLON_CHECK(left_on >= 0 && left_on < left->Columns(), Code::Invalid, "asof join: left `on` column " << left_on);
  CYLON_CHECK(right_on >= 0 && right_on < right->Columns(), Code::Invalid,
              "asof join: right `on` column " << right_on);
  CYLON_CHECK(left_by.size() == right_by.size(), Code::Invalid,
              "asof join: " << left_by.size() << " left and " << right_by.size() << " right `by` columns");
  CYLON_CHECK(left_by.size() + 1 <= (size_t)kMaxFusedCols, Code::Invalid,
              "asof join: more than " << kMaxFusedCols - 1 << " `by` columns");
  for (size_t i = 0; i < left_by.size(); ++i) {
    CYLON_CHECK(left_by[i] >= 0 && left_by[i] < left->Columns(), Code::Invalid,
                "asof join: left `by` column " << left_by[i]);
    CYLON_CHECK(right_by[i] >= 0 && right_by[i] < right->Columns(), Code::Invalid,
                "asof join: right `by` column " << right_by[i]);
    const DataType &lt = left->column(left_by[i]).type, &rt = right->column(right_by[i]).type;
    CYLON_CHECK(lt == rt, Code::Invalid,
                "asof join: `by` columns of types " << lt.ToString() << " and " << rt.ToString());
  }
  const DataType &lt = left->column(left_on).type, &rt = right->column(right_on).type;
  CYLON_CHECK(on_type(lt), Code::Invalid,
              "asof join: `on` must be an integer, float32 / float64 or temporal column, got " << lt.ToString());
  CYLON_CHECK(lt == rt, Code::Invalid, "asof join: `on` columns of types " << lt.ToString() << " and " << rt.ToString());
  CYLON_CHECK(o.direction >= ASOF_BACKWARD && o.direction <= ASOF_NEAREST, Code::Invalid,
              "asof join: direction " << o.direction);
  if (o.has_tolerance) {
    const bool isf = lt.kind() == ValueKind::FLOAT;
    CYLON_CHECK(o.tolerance_is_float == isf, Code::Invalid,
                "asof join: " << (isf ? "a float `on` takes a float tolerance" : "an integer or temporal `on` takes an integer tolerance"));
    CYLON_CHECK(isf ? o.tolerance_f >= 0 : o.tolerance_i >= 0, Code::Invalid, "asof join: tolerance < 0");  // NaN too
  }
}

// the merged order of the two sides' key rows for one concatenation order
struct Order {
  TablePtr keys;  // by .. ++ on of the first side, then of the second
  at::Tensor perm, heads, rheads;
  int64_t n = 0, nfirst = 0;
  bool right_first = false;
};

Order make_order(const Exec &ex, const TablePtr &lk, const TablePtr &rk, bool right_first) {
  Order o;
  o.right_first = right_first;
  o.keys = right_first ? Merge({rk, lk}) : Merge({lk, rk});
  o.n = o.keys->Rows();
  o.nfirst = right_first ? rk->Rows() : lk->Rows();
  std::vector<int> all(o.keys->Columns()), by(o.keys->Columns() - 1);
  for (size_t c = 0; c < all.size(); ++c) all[c] = (int)c;
  for (size_t c = 0; c < by.size(); ++c) by[c] = (int)c;
  o.perm = SortIndices(o.keys, all, std::vector<bool>(all.size(), true)).contiguous();
  if (reinterpret_cast<uintptr_t>(o.perm.data_ptr()) % 16 != 0) o.perm = o.perm.clone();  // the scans' 16-byte loads
  o.heads = ex.empty_u8(o.n);
  const std::vector<ColView> bv = views(o.keys, by);
  KCALL(ex, segment_heads, bv.data(), (int)bv.size(), ptr<int64_t>(o.perm), o.n, ptr<uint8_t>(o.heads));
  return o;
}

// match[left row] = the last candidate of its partition before it in scan order
at::Tensor scan(const Exec &ex, Order &o, bool reverse, int64_t nl, int64_t step, int64_t *matched) {
  const int64_t T = KSIZE(ex, window_tile_rows), ntiles = (o.n + T - 1) / T;
  if (reverse && !o.rheads.defined()) {
    o.rheads = ex.empty_u8(o.n);
    KCALL(ex, window_rev_flags, ptr<uint8_t>(o.heads), o.n, ptr<uint8_t>(o.rheads));
  }
  const uint8_t *restarts = ptr<uint8_t>(reverse ? o.rheads : o.heads);
  at::Tensor code = ex.empty_u8(o.n), match = ex.empty_i64(nl);
  at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles), carry = ex.empty_i64(ntiles);
  const ColView on = o.keys->column(o.keys->Columns() - 1).view();
  KCALL(ex, asof_tile, on, ptr<int64_t>(o.perm), restarts, o.n, o.nfirst, o.right_first, reverse, ptr<uint8_t>(code),
        ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
  KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 1, kMax, step, ptr<int64_t>(carry));
  KCALL(ex, asof_apply, ptr<int64_t>(o.perm), restarts, ptr<uint8_t>(code), o.n, o.nfirst, o.right_first, reverse,
        ptr<int64_t>(carry), ptr<int64_t>(match), matched);
  return match;
}

TablePtr key_rows(const TablePtr &t, const std::vector<int> &by, int on) {
  std::vector<int> cols = by;
  cols.push_back(on);
  return Project(t, cols);
}

TablePtr assemble(const TablePtr &left, const TablePtr &right, const at::Tensor &match, const AsofOptions &o) {
  TablePtr ro = GatherNullable(right, match, true);
  std::vector<Column> cols;
  cols.reserve(left->Columns() + ro->Columns());
  for (const auto &c : left->columns()) cols.push_back(c.with_name(o.left_prefix + c.name));
  for (const auto &c : ro->columns()) cols.push_back(c.with_name(o.right_prefix + c.name));
  return Table::Make(left->GetContext(), std::move(cols));
}

}  // namespace

at::Tensor AsofJoinIndices(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                           const std::vector<int> &left_by, const std::vector<int> &right_by, const AsofOptions &options,
                           int64_t carry_step_tiles) {
  check(left, right, left_on, right_on, left_by, right_by, options);
  CYLON_CHECK(left->device() == right->device(), Code::Invalid, "asof join: tables on different devices");
  Exec ex(left->device());
  const int64_t max_step = KSIZE(ex, window_carry_tiles);
  CYLON_CHECK(carry_step_tiles <= max_step, Code::Invalid, "asof join: carry step of " << carry_step_tiles << " tiles");
  const int64_t step = carry_step_tiles > 0 ? carry_step_tiles : max_step;
  const int64_t nl = left->Rows(), nr = right->Rows();
  if (nl == 0 || nr == 0) return at::full({nl}, -1, ex.opts(at::kLong));
  CYLON_PHASE("asof", ex.device);

  const TablePtr lk = key_rows(left, left_by, left_on), rk = key_rows(right, right_by, right_on);
  const bool exact = options.allow_exact_matches;
  const bool nearest = options.direction == ASOF_NEAREST;
  const bool pick = nearest || options.has_tolerance;
  at::Tensor counter = at::zeros({1}, ex.opts(at::kLong));
  int64_t *matched = ptr<int64_t>(counter);
  int64_t *scan_count = pick ? nullptr : matched;

  at::Tensor back, fwd;
  int64_t sorts = 1, scans = 0, tiles = 0;
  const int64_t T = KSIZE(ex, window_tile_rows), ntiles = (nl + nr + T - 1) / T;
  {
    // the backward scan wants equal right rows first iff they match; the forward one, reversed, the opposite
    const bool want_back = options.direction != ASOF_FORWARD, want_fwd = options.direction != ASOF_BACKWARD;
    const bool back_rf = exact, fwd_rf = nearest ? true : !exact;
    Order o = make_order(ex, lk, rk, want_back ? back_rf : fwd_rf);
    if (want_back) {
      back = scan(ex, o, false, nl, step, scan_count);
      ++scans;
    }
    if (want_fwd) {
      if (o.right_first != fwd_rf) {
        o = Order();  // release the first order before the second sort
        o = make_order(ex, lk, rk, fwd_rf);
        ++sorts;
      }
      fwd = scan(ex, o, true, nl, step, scan_count);
      ++scans;
    }
    tiles = scans * ntiles;
  }

  at::Tensor match = back.defined() ? back : fwd;
  if (pick) {
    const at::Tensor &one = back.defined() ? back : fwd;  // a one-directional join picks in place
    KCALL(ex, asof_pick, left->column(left_on).view(), right->column(right_on).view(), nl, ptr<int64_t>(one),
          nearest ? ptr<int64_t>(fwd) : nullptr, options.has_tolerance, options.tolerance_i, options.tolerance_f,
          ptr<int64_t>(match), matched);
  }
  trace::add_counter("asof.sort", sorts);
  trace::add_counter("asof.scan", scans);
  trace::add_counter("asof.tiles", tiles);
  trace::add_counter("asof.matched", read_i64(counter, 0));
  return match;
}

TablePtr AsofJoin(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                  const std::vector<int> &left_by, const std::vector<int> &right_by, const AsofOptions &options,
                  int64_t carry_step_tiles) {
  return assemble(left, right,
                  AsofJoinIndices(left, right, left_on, right_on, left_by, right_by, options, carry_step_tiles), options);
}

TablePtr DistributedAsofJoin(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                             const std::vector<int> &left_by, const std::vector<int> &right_by,
                             const AsofOptions &options) {
  if (left->GetContext()->GetWorldSize() <= 1) return AsofJoin(left, right, left_on, right_on, left_by, right_by, options);
  CYLON_CHECK(!left_by.empty(), Code::Invalid,
              "a distributed asof join needs a `by` column (a global as-of order is not supported)");
  check(left, right, left_on, right_on, left_by, right_by, options);  // every rank fails before the exchange, or none
  const auto sh = ShufflePair(left, left_by, right, right_by);
  return AsofJoin(sh.first, sh.second, left_on, right_on, left_by, right_by, options);
}

}  // namespace ops
}  // namespace cylon
