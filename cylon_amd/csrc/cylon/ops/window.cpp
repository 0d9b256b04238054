// Window functions (docs/semantics.md "Window functions"): t's columns unchanged, in t's row order,
// plus one column per spec computed along perm = SortIndices(t, partition_cols ++ order_cols).
//
// One sort, one flag byte per sorted position (segment_heads over the partition columns and over all
// key columns, merged by window_flags), then per spec a three-phase segmented scan of
// kernels/window.hip (window_tile / window_carry / window_apply).  The three ranking functions and the
// partition heads that LAG / LEAD need come out of one scan of the flags; specs on the same value
// column share its values gathered into sorted order.  The scans write straight to out[perm[i]], so
// nothing is sorted back.  The GPU context always takes the kernels: there is no other device path.
//
// A ROLLING spec (a bounded ROWS frame) shares the sort, the flags, the gathered values and the
// partition heads; the partition tails come from the same rank scan run over the reversed flags.  A
// frame of at most window_frame_lds_rows() rows is one launch of kernels/rolling.hip (rolling_lds);
// a wider one scans forwards and over the reversed order (rolling_tile / window_carry /
// rolling_scan) and combines the two (rolling_combine).
//
// A RANGE spec (a frame over the one order column's values) shares all of that too.  The order column
// is gathered like a value column and turned into search keys once per call; every distinct
// (preceding, following) gets one bounds search (lo / hi per sorted position), every (column, operator)
// one scan pyramid, and a spec is then one query launch of kernels/frame_range.hip.
//
// The navigation and distribution functions (kernels/window_nav.hip) share all of that as well.  FFILL /
// BFILL and the IGNORE NULLS forms of FIRST / LAST_VALUE scan "the last non-null position" over the
// dense validity bytes, once per (column, direction) whatever the number of specs; a column without a
// validity array is answered without a scan.  FIRST / LAST / NTH_VALUE are one element-wise launch over
// phead / rtail, the distribution functions one over phead, rtail and the peer heads / tails that the
// two rank scans carry anyway.  Columns of width 1, 2, 4 or 8 are written straight from the dense
// values (value mode); every other type goes through a source-row array and GatherColumn.
//
// A VAR / STD spec over a ROWS or a RANGE frame (kernels/frame_moments.hip) shares all of that again.  Every
// value column gets one moment pyramid of (count, mean, M2) states per call, whatever the number of specs,
// their frame kinds, offsets, ddof or min_periods; a RANGE spec reuses the bounds search of its
// (preceding, following), a ROWS spec computes its bounds from phead / rtail in the query launch.
#include <algorithm>
#include <map>
#include <set>
#include <tuple>

#include "../kernels/frame_moments_common.hpp"
#include "../kernels/frame_range_common.hpp"

#include "../trace.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

namespace {

// kernels/window.hip WinFunc
constexpr int kSumI = 0, kSumF = 1, kMin = 2, kMax = 3, kCount = 4, kRank = 5;

const char *func_name(WindowFunc f) {
  switch (f) {
    case WIN_ROW_NUMBER: return "row_number";
    case WIN_RANK: return "rank";
    case WIN_DENSE_RANK: return "dense_rank";
    case WIN_CUMCOUNT: return "cumcount";
    case WIN_CUMSUM: return "cumsum";
    case WIN_CUMMIN: return "cummin";
    case WIN_CUMMAX: return "cummax";
    case WIN_LAG: return "lag";
    case WIN_LEAD: return "lead";
    case WIN_ROLLING_COUNT: return "rolling_count";
    case WIN_ROLLING_SUM: return "rolling_sum";
    case WIN_ROLLING_MEAN: return "rolling_mean";
    case WIN_ROLLING_MIN: return "rolling_min";
    case WIN_ROLLING_MAX: return "rolling_max";
    case WIN_RANGE_COUNT: return "range_count";
    case WIN_RANGE_SUM: return "range_sum";
    case WIN_RANGE_MEAN: return "range_mean";
    case WIN_RANGE_MIN: return "range_min";
    case WIN_RANGE_MAX: return "range_max";
    case WIN_FIRST_VALUE: return "first_value";
    case WIN_LAST_VALUE: return "last_value";
    case WIN_NTH_VALUE: return "nth_value";
    case WIN_FFILL: return "ffill";
    case WIN_BFILL: return "bfill";
    case WIN_NTILE: return "ntile";
    case WIN_PERCENT_RANK: return "percent_rank";
    case WIN_CUME_DIST: return "cume_dist";
    case WIN_ROLLING_VAR: return "rolling_var";
    case WIN_ROLLING_STD: return "rolling_std";
    case WIN_RANGE_VAR: return "range_var";
    case WIN_RANGE_STD: return "range_std";
  }
  CYLON_THROW(Code::Invalid, "window function " << static_cast<int>(f));
}

bool is_ranking(WindowFunc f) { return f == WIN_ROW_NUMBER || f == WIN_RANK || f == WIN_DENSE_RANK; }
bool is_shift(WindowFunc f) { return f == WIN_LAG || f == WIN_LEAD; }
bool is_rolling(WindowFunc f) { return f >= WIN_ROLLING_COUNT && f <= WIN_ROLLING_MAX; }
bool is_range(WindowFunc f) { return f >= WIN_RANGE_COUNT && f <= WIN_RANGE_MAX; }
// VAR / STD over a ROWS resp. a RANGE frame
bool is_moment_rolling(WindowFunc f) { return f == WIN_ROLLING_VAR || f == WIN_ROLLING_STD; }
bool is_moment_range(WindowFunc f) { return f == WIN_RANGE_VAR || f == WIN_RANGE_STD; }
bool is_moment(WindowFunc f) { return is_moment_rolling(f) || is_moment_range(f); }
bool is_framed(WindowFunc f) { return is_rolling(f) || is_range(f) || is_moment(f); }
bool is_pick(WindowFunc f) { return f >= WIN_FIRST_VALUE && f <= WIN_NTH_VALUE; }
bool is_fill(WindowFunc f) { return f == WIN_FFILL || f == WIN_BFILL; }
bool is_dist(WindowFunc f) { return f >= WIN_NTILE && f <= WIN_CUME_DIST; }
bool no_column(WindowFunc f) { return is_ranking(f) || is_dist(f); }
// what a navigation or distribution function reads of the two rank scans
bool nav_needs_phead(WindowFunc f) { return f == WIN_FIRST_VALUE || f == WIN_NTH_VALUE || is_dist(f); }
bool nav_needs_rtail(WindowFunc f) { return f == WIN_LAST_VALUE || f == WIN_NTH_VALUE || is_dist(f); }
// the ROLLING function whose result rules a RANGE function shares
WindowFunc rolling_twin(WindowFunc f) {
  return is_range(f) ? static_cast<WindowFunc>(f - WIN_RANGE_COUNT + WIN_ROLLING_COUNT) : f;
}

// the order column of a RANGE frame: an integer of any width, a temporal type, float32 or float64
bool range_order_type(const Column &c) {
  switch (c.type.type) {
    case Type::UINT8: case Type::INT8: case Type::UINT16: case Type::INT16: case Type::UINT32: case Type::INT32:
    case Type::UINT64: case Type::INT64: case Type::FLOAT: case Type::DOUBLE: case Type::DATE32: case Type::DATE64:
    case Type::TIMESTAMP: case Type::TIME32: case Type::TIME64: case Type::DURATION: return !c.is_var();
    default: return false;
  }
}

// a column whose cells the navigation kernels copy themselves (value mode)
bool nav_value_mode(const Column &c) {
  if (c.is_var()) return false;
  const int w = c.type.width();
  return w == 1 || w == 2 || w == 4 || w == 8;
}

bool scan_value(const Column &c) {
  if (c.is_var() || !c.type.is_numeric()) return false;
  const int w = c.type.width();
  return w == 1 || w == 2 || w == 4 || w == 8;
}

// the result type of CUMSUM = the group-by's SUM
Type sum_type(const Column &c) {
  if (c.type.kind() == ValueKind::FLOAT) return Type::DOUBLE;
  return c.type.kind() == ValueKind::UNSIGNED_INT ? Type::UINT64 : Type::INT64;
}

// the kernel function and the output type of a value spec
std::pair<int, DataType> value_plan(const WindowSpec &s, const Column &c) {
  switch (rolling_twin(s.func)) {
    case WIN_CUMCOUNT:
    case WIN_ROLLING_COUNT: return {kCount, DataType(Type::INT64)};
    case WIN_ROLLING_MEAN: return {c.type.kind() == ValueKind::FLOAT ? kSumF : kSumI, DataType(Type::DOUBLE)};
    case WIN_ROLLING_VAR:
    case WIN_ROLLING_STD:
    case WIN_RANGE_VAR:
    case WIN_RANGE_STD: return {kCount, DataType(Type::DOUBLE)};  // the moment kernels take no function
    case WIN_ROLLING_SUM:
    case WIN_CUMSUM: return {c.type.kind() == ValueKind::FLOAT ? kSumF : kSumI, DataType(sum_type(c))};
    case WIN_ROLLING_MIN:
    case WIN_CUMMIN: return {kMin, c.type};
    default: return {kMax, c.type};
  }
}

struct Checked {
  std::vector<bool> asc;           // one per order column
  std::vector<std::string> names;  // one per spec
};

Checked check(const TablePtr &t, const std::vector<int> &part, const std::vector<int> &order,
              const std::vector<bool> &ascending, const std::vector<WindowSpec> &specs) {
  for (int c : part) CYLON_CHECK(c >= 0 && c < t->Columns(), Code::Invalid, "window partition column " << c);
  for (int c : order) CYLON_CHECK(c >= 0 && c < t->Columns(), Code::Invalid, "window order column " << c);
  CYLON_CHECK(part.size() + order.size() <= (size_t)kMaxFusedCols, Code::Invalid,
              "window: more than " << kMaxFusedCols << " partition and order columns");
  Checked ck;
  CYLON_CHECK(ascending.empty() || ascending.size() == 1 || ascending.size() == order.size(), Code::Invalid,
              "ascending flags must match the order columns");
  for (size_t i = 0; i < order.size(); ++i)
    ck.asc.push_back(ascending.empty() ? true : ascending[ascending.size() == 1 ? 0 : i]);
  std::set<std::string> taken;
  for (const auto &c : t->columns()) taken.insert(c.name);
  for (const auto &s : specs) {
    const char *fn = func_name(s.func);
    std::string name = s.name;
    if (no_column(s.func)) {
      if (name.empty()) name = fn;
      if (s.func == WIN_NTILE) CYLON_CHECK(s.arg >= 1, Code::Invalid, "window ntile of " << s.arg << " buckets");
    } else {
      CYLON_CHECK(s.col >= 0 && s.col < t->Columns(), Code::Invalid, "window " << fn << " of column " << s.col);
      const Column &c = t->column(s.col);
      if (name.empty()) name = std::string(fn) + "_" + c.name;
      if (s.func == WIN_CUMSUM || s.func == WIN_CUMMIN || s.func == WIN_CUMMAX)
        CYLON_CHECK(scan_value(c) && !(s.func == WIN_CUMSUM && c.type.type == Type::HALF_FLOAT), Code::Invalid,
                    "window " << fn << " needs a fixed-width numeric column, got " << c.type.ToString());
      if (is_shift(s.func)) CYLON_CHECK(s.arg >= 0, Code::Invalid, "window " << fn << " offset " << s.arg << " < 0");
      if (s.func == WIN_NTH_VALUE) {
        CYLON_CHECK(s.arg >= 1, Code::Invalid, "window nth_value of row " << s.arg << " < 1");
        CYLON_CHECK(!s.ignore_nulls, Code::Invalid, "window nth_value does not take ignore_nulls");
      }
      if (is_fill(s.func)) CYLON_CHECK(s.limit >= 0, Code::Invalid, "window " << fn << " limit " << s.limit << " < 0");
      if (is_framed(s.func)) {
        const WindowFunc rf = rolling_twin(s.func);
        CYLON_CHECK(t->Rows() < (int64_t(1) << 32), Code::Invalid,
                    "window " << fn << " over " << t->Rows() << " rows: framed functions take fewer than 2^32");
        const bool sum = rf == WIN_ROLLING_SUM || rf == WIN_ROLLING_MEAN || is_moment(s.func);
        CYLON_CHECK(rf == WIN_ROLLING_COUNT || (scan_value(c) && !(sum && c.type.type == Type::HALF_FLOAT)),
                    Code::Invalid, "window " << fn << " needs a fixed-width numeric column, got " << c.type.ToString());
        CYLON_CHECK(s.preceding >= 0 && s.following >= 0, Code::Invalid,
                    "window " << fn << " frame of " << s.preceding << " preceding, " << s.following << " following");
        CYLON_CHECK(rf == WIN_ROLLING_COUNT || s.min_periods >= 1, Code::Invalid,
                    "window " << fn << " min_periods " << s.min_periods << " < 1");
        CYLON_CHECK(!is_moment(s.func) || s.ddof >= 0, Code::Invalid, "window " << fn << " ddof " << s.ddof << " < 0");
      }
      if (is_range(s.func) || is_moment_range(s.func)) {
        CYLON_CHECK(order.size() == 1, Code::Invalid,
                    "window " << fn << " needs exactly one order column, got " << order.size());
        const Column &oc = t->column(order[0]);
        CYLON_CHECK(range_order_type(oc), Code::Invalid,
                    "window " << fn << " needs an integer, temporal, float32 or float64 order column, got "
                              << oc.type.ToString());
        if (s.offset_is_float) {
          CYLON_CHECK(oc.type.kind() == ValueKind::FLOAT, Code::Invalid,
                      "window " << fn << ": a float offset on the " << oc.type.ToString() << " order column");
          // written so that a NaN fails
          CYLON_CHECK((s.preceding == kWindowUnbounded || s.preceding_f >= 0) &&
                          (s.following == kWindowUnbounded || s.following_f >= 0),
                      Code::Invalid,
                      "window " << fn << " frame of " << s.preceding_f << " preceding, " << s.following_f
                                << " following");
        }
      }
    }
    CYLON_CHECK(taken.insert(name).second, Code::Invalid, "window output column '" << name << "' already exists");
    ck.names.push_back(name);
  }
  return ck;
}

Column int64_column(const std::string &name, const at::Tensor &v) {
  return Column(name, DataType(Type::INT64), v.numel(), v);
}

// A running aggregate is null where its row's value is; a framed one where the frame holds fewer than
// min_periods values, which a frame of a column without nulls can only do for min_periods > 1.  A
// navigation function's output is always nullable (NTH_VALUE past the partition's end), except the
// fill of a column without nulls, which is the column itself; a distribution function's never is.
bool nullable_result(const WindowSpec &s, const Column &c) {
  if (is_pick(s.func) || is_moment(s.func)) return true;  // VAR / STD: null where m - ddof <= 0
  if (is_fill(s.func)) return c.nullable();
  if (s.func == WIN_CUMCOUNT || s.func == WIN_ROLLING_COUNT || s.func == WIN_RANGE_COUNT) return false;
  return c.nullable() || (is_framed(s.func) && s.min_periods > 1);
}

// the new columns of an empty table
TablePtr empty_result(const TablePtr &t, const std::vector<WindowSpec> &specs, const Checked &ck) {
  Exec ex(t->device());
  std::vector<Column> out = t->columns();
  for (size_t i = 0; i < specs.size(); ++i) {
    const WindowSpec &s = specs[i];
    if (is_ranking(s.func) || s.func == WIN_NTILE) {
      out.push_back(int64_column(ck.names[i], ex.empty_i64(0)));
    } else if (is_dist(s.func)) {
      out.push_back(make_fixed_column(ck.names[i], DataType(Type::DOUBLE), 0, ex.device, false));
    } else if (is_shift(s.func) || is_pick(s.func) || is_fill(s.func)) {
      out.push_back(GatherColumn(t->column(s.col), ex.empty_i64(0)).with_name(ck.names[i]));
    } else {
      const Column &c = t->column(s.col);
      out.push_back(make_fixed_column(ck.names[i], value_plan(s, c).second, 0, ex.device, nullable_result(s, c)));
    }
  }
  return Table::Make(t->GetContext(), std::move(out));
}

int64_t *opt_ptr(const at::Tensor &t) { return t.defined() ? ptr<int64_t>(t) : nullptr; }

struct Dense {  // a value column gathered into sorted order
  at::Tensor bits, valid;
};

}  // namespace

TablePtr Window(const TablePtr &t, const std::vector<int> &partition_cols, const std::vector<int> &order_cols,
                const std::vector<bool> &ascending, const std::vector<WindowSpec> &specs, int64_t carry_step_tiles) {
  const Checked ck = check(t, partition_cols, order_cols, ascending, specs);
  if (specs.empty()) return t;
  const int64_t n = t->Rows();
  if (n == 0) return empty_result(t, specs, ck);
  Exec ex(t->device());
  CYLON_PHASE("window", ex.device);
  const int64_t max_step = KSIZE(ex, window_carry_tiles);
  CYLON_CHECK(carry_step_tiles <= max_step, Code::Invalid, "window: carry step of " << carry_step_tiles << " tiles");
  const int64_t step = carry_step_tiles > 0 ? carry_step_tiles : max_step;

  // the defining order
  std::vector<int> keys = partition_cols;
  keys.insert(keys.end(), order_cols.begin(), order_cols.end());
  std::vector<bool> dirs(partition_cols.size(), true);
  dirs.insert(dirs.end(), ck.asc.begin(), ck.asc.end());
  at::Tensor perm = ex.empty_i64(n);
  if (keys.empty()) {
    KCALL(ex, iota, ptr<int64_t>(perm), n, 0);
  } else {
    perm = SortIndices(t, keys, dirs).contiguous();
    if (reinterpret_cast<uintptr_t>(perm.data_ptr()) % 16 != 0) perm = perm.clone();  // the scans' 16-byte loads
  }
  trace::add_counter("window.sort", keys.empty() ? 0 : 1);

  // bit 0: partition head, bit 1: peer head
  at::Tensor flags = ex.empty_u8(n), peer;
  {
    const std::vector<ColView> pv = views(t, partition_cols);
    KCALL(ex, segment_heads, pv.data(), (int)pv.size(), ptr<int64_t>(perm), n, ptr<uint8_t>(flags));
    if (!order_cols.empty()) {
      const std::vector<ColView> kv = views(t, keys);
      peer = ex.empty_u8(n);
      KCALL(ex, segment_heads, kv.data(), (int)kv.size(), ptr<int64_t>(perm), n, ptr<uint8_t>(peer));
    }
    KCALL(ex, window_flags, ptr<uint8_t>(flags), peer.defined() ? ptr<uint8_t>(peer) : nullptr, n, ptr<uint8_t>(flags));
    peer = at::Tensor();
  }

  const int64_t T = KSIZE(ex, window_tile_rows);
  const int64_t ntiles = (n + T - 1) / T;
  int64_t scans = 0;

  // ranking functions and LAG / LEAD: one scan of the flags
  at::Tensor row_number, rank, dense_rank, phead, qhead, rqhead;
  bool framed = false, nav = false, nav_rtail = false, nav_rflags = false, percent_rank = false, cume_dist = false;
  for (const auto &s : specs) {
    if (is_pick(s.func) || is_fill(s.func) || is_dist(s.func)) nav = true;
    if (nav_needs_phead(s.func) && !phead.defined()) phead = ex.empty_i64(n);
    if (nav_needs_rtail(s.func)) nav_rtail = true;
    // the reversed fill scan restarts at the reversed flags
    if (s.func == WIN_BFILL || (s.func == WIN_FIRST_VALUE && s.ignore_nulls)) nav_rflags = true;
    if (s.func == WIN_PERCENT_RANK) percent_rank = true;
    if (s.func == WIN_CUME_DIST) cume_dist = true;
    if (s.func == WIN_ROW_NUMBER && !row_number.defined()) row_number = ex.empty_i64(n);
    if (s.func == WIN_RANK && !rank.defined()) rank = ex.empty_i64(n);
    if (s.func == WIN_DENSE_RANK && !dense_rank.defined()) dense_rank = ex.empty_i64(n);
    if ((is_shift(s.func) || is_framed(s.func)) && !phead.defined()) phead = ex.empty_i64(n);
    if (is_framed(s.func)) framed = true;
  }
  if (row_number.defined() || rank.defined() || dense_rank.defined() || phead.defined()) {
    at::Tensor tagg = ex.empty_i64(3 * ntiles), tflag = ex.empty_u8(ntiles), carry = ex.empty_i64(3 * ntiles);
    KCALL(ex, window_rank_tile, ptr<uint8_t>(flags), n, ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
    KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 3, kRank, step, ptr<int64_t>(carry));
    KCALL(ex, window_rank_apply, ptr<int64_t>(perm), ptr<uint8_t>(flags), n, ptr<int64_t>(carry),
          opt_ptr(row_number), opt_ptr(rank), opt_ptr(dense_rank), opt_ptr(phead));
    if (percent_rank) {  // RANK - 1 = the head of the row's peers - phead
      qhead = ex.empty_i64(n);
      KCALL(ex, window_rank_heads, ptr<uint8_t>(flags), n, ptr<int64_t>(carry), nullptr, ptr<int64_t>(qhead));
    }
    ++scans;
  }

  // framed specs, and the functions that look at the partition's end: the partition tails, as the
  // heads of the reversed order.  CUME_DIST marks the peer tails in the same flags, and the scan's q word
  // is then the last peer of every position.
  at::Tensor rflags, rtail;
  if (framed || nav_rtail || nav_rflags) {
    rflags = ex.empty_u8(n);
    if (cume_dist) KCALL(ex, window_rev_peer_flags, ptr<uint8_t>(flags), n, ptr<uint8_t>(rflags));
    else KCALL(ex, window_rev_flags, ptr<uint8_t>(flags), n, ptr<uint8_t>(rflags));
  }
  if (framed || nav_rtail) {
    rtail = ex.empty_i64(n);
    at::Tensor tagg = ex.empty_i64(3 * ntiles), tflag = ex.empty_u8(ntiles), carry = ex.empty_i64(3 * ntiles);
    KCALL(ex, window_rank_tile, ptr<uint8_t>(rflags), n, ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
    KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 3, kRank, step, ptr<int64_t>(carry));
    KCALL(ex, window_rank_apply, ptr<int64_t>(perm), ptr<uint8_t>(rflags), n, ptr<int64_t>(carry), nullptr, nullptr,
          nullptr, ptr<int64_t>(rtail));
    if (cume_dist) {
      rqhead = ex.empty_i64(n);
      KCALL(ex, window_rank_heads, ptr<uint8_t>(rflags), n, ptr<int64_t>(carry), nullptr, ptr<int64_t>(rqhead));
    }
    ++scans;
  }
  const int64_t lds_rows = KSIZE(ex, window_frame_lds_rows);
  int64_t frames_lds = 0, frames_wide = 0;

  std::map<int, Dense> dense;  // by value column
  // the dense values of a column, gathered by its first user (window_tile's tile pairs are not used
  // by the framed functions: COUNT suits every column)
  auto dense_of = [&](int col) -> const Dense & {
    auto it = dense.find(col);
    if (it != dense.end()) return it->second;
    const Column &c = t->column(col);
    Dense d;
    d.bits = ex.empty_i64(n);
    if (c.nullable()) d.valid = ex.empty_u8(n);
    at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles);
    KCALL(ex, window_tile, c.view(), ptr<int64_t>(perm), ptr<uint8_t>(flags), n, kCount,
          reinterpret_cast<uint64_t *>(ptr<int64_t>(d.bits)), d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr, true,
          ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
    return dense.emplace(col, d).first->second;
  };
  auto u64 = [](const at::Tensor &x) { return reinterpret_cast<uint64_t *>(ptr<int64_t>(x)); };
  auto u32 = [](const at::Tensor &x) { return reinterpret_cast<uint32_t *>(ptr<int64_t>(x)); };

  // RANGE frames: the order column's search keys once, the bounds once per (preceding, following),
  // a pyramid once per (column, operator)
  struct Bounds {
    at::Tensor lo, hi;  // n uint32 each
  };
  struct Pyramid {
    at::Tensor P, S, E;
  };
  at::Tensor rkeys, rcls;
  bool rfloat = false;
  std::map<std::tuple<int, uint64_t, int, uint64_t>, Bounds> range_bounds;
  std::map<std::pair<int, int>, Pyramid> pyramids;  // by (value column, kernel function)
  std::map<int, Pyramid> moment_pyramids;           // by value column
  int64_t range_specs = 0, moment_specs = 0;
  auto bounds_of = [&](const WindowSpec &s) -> const Bounds & {
    if (!rkeys.defined()) {
      const Column &oc = t->column(order_cols[0]);
      rfloat = oc.type.kind() == ValueKind::FLOAT;
      const Dense &d = dense_of(order_cols[0]);
      rkeys = ex.empty_i64(n);
      rcls = ex.empty_u8(n);
      KCALL(ex, frame_range_keys, oc.view(), u64(d.bits), d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr, n,
            !ck.asc[0], u64(rkeys), ptr<uint8_t>(rcls));
    }
    // a side: unbounded, an integer distance (integer keys) or a float64 one (float keys)
    auto side = [&](int64_t i, double f, int *mode, uint64_t *ui, double *df) {
      *ui = 0;
      *df = 0;
      if (i == kWindowUnbounded) {
        *mode = FR_UNBOUNDED;
      } else if (rfloat) {
        *mode = FR_FLOAT;
        *df = s.offset_is_float ? f : (double)i;
      } else {
        *mode = FR_INT;
        *ui = (uint64_t)i;
      }
    };
    int pm, fm;
    uint64_t pi, fi;
    double pf, ff;
    side(s.preceding, s.preceding_f, &pm, &pi, &pf);
    side(s.following, s.following_f, &fm, &fi, &ff);
    const auto key = std::make_tuple(pm, rfloat ? fr_f64_bits(pf) : pi, fm, rfloat ? fr_f64_bits(ff) : fi);
    auto it = range_bounds.find(key);
    if (it != range_bounds.end()) return it->second;
    Bounds b{ex.empty_i64((n + 1) / 2), ex.empty_i64((n + 1) / 2)};
    KCALL(ex, frame_range_bounds, u64(rkeys), ptr<uint8_t>(rcls), ptr<int64_t>(phead), ptr<int64_t>(rtail), n, rfloat,
          !ck.asc[0], pm, pi, pf, fm, fi, ff, u32(b.lo), u32(b.hi));
    return range_bounds.emplace(key, b).first->second;
  };
  auto pyramid_of = [&](int col, int func) -> const Pyramid & {
    auto it = pyramids.find({col, func});
    if (it != pyramids.end()) return it->second;
    const Dense &d = dense_of(col);
    Pyramid p{ex.empty_i64(fr_ps_slots(n)), ex.empty_i64(fr_ps_slots(n)), ex.empty_i64(fr_e_slots(n))};
    KCALL(ex, frame_range_pyramid, t->column(col).view(), n, func, u64(d.bits),
          d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr, u64(p.P), u64(p.S), u64(p.E));
    return pyramids.emplace(std::make_pair(col, func), p).first->second;
  };

  auto moment_pyramid_of = [&](int col) -> const Pyramid & {
    auto it = moment_pyramids.find(col);
    if (it != moment_pyramids.end()) return it->second;
    const Dense &d = dense_of(col);
    Pyramid p{ex.empty_i64(fm_words(fm_ps_slots(n))), ex.empty_i64(fm_words(fm_ps_slots(n))),
              ex.empty_i64(fm_words(fm_e_slots(n)))};
    KCALL(ex, frame_moments_pyramid, t->column(col).view(), n, u64(d.bits),
          d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr, u64(p.P), u64(p.S), u64(p.E));
    return moment_pyramids.emplace(col, p).first->second;
  };

  // fills: the tile pass and the carries once per (column, direction); pos = the fill position of
  // every sorted position, which only the IGNORE NULLS forms ask for
  struct Fill {
    at::Tensor carry, pos;
  };
  std::map<std::pair<int, bool>, Fill> fills;
  int64_t nav_gather = 0, nav_skipped = 0;
  auto fill_of = [&](int col, bool rev) -> Fill & {
    auto it = fills.find({col, rev});
    if (it != fills.end()) return it->second;
    const Dense &d = dense_of(col);
    Fill f;
    f.carry = ex.empty_i64(ntiles);
    at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles);
    KCALL(ex, window_fill_tile, rev ? ptr<uint8_t>(rflags) : ptr<uint8_t>(flags), n, rev, ptr<uint8_t>(d.valid),
          ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
    KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 1, kMax, step, ptr<int64_t>(f.carry));
    ++scans;
    return fills.emplace(std::make_pair(col, rev), f).first->second;
  };

  std::vector<Column> out = t->columns();
  for (size_t i = 0; i < specs.size(); ++i) {
    const WindowSpec &s = specs[i];
    const std::string &name = ck.names[i];
    if (is_ranking(s.func)) {
      out.push_back(int64_column(name, s.func == WIN_ROW_NUMBER ? row_number : s.func == WIN_RANK ? rank : dense_rank));
      continue;
    }
    if (is_dist(s.func)) {
      Column col = make_fixed_column(name, DataType(s.func == WIN_NTILE ? Type::INT64 : Type::DOUBLE), n, ex.device,
                                     false);
      KCALL(ex, window_dist_apply, ptr<int64_t>(perm), ptr<int64_t>(phead), ptr<int64_t>(rtail), opt_ptr(qhead),
            opt_ptr(rqhead), n, s.func - WIN_NTILE, s.arg, reinterpret_cast<uint8_t *>(col.data.data_ptr()));
      out.push_back(std::move(col));
      continue;
    }
    const Column &c = t->column(s.col);
    if (is_fill(s.func) || is_pick(s.func)) {
      if (is_fill(s.func) && !c.nullable()) {  // nothing to fill: the column itself, no scan
        out.push_back(c.with_name(name));
        ++nav_skipped;
        continue;
      }
      const bool value = nav_value_mode(c);
      const bool rev = s.func == WIN_BFILL || s.func == WIN_FIRST_VALUE;
      // the IGNORE NULLS forms of a column without nulls are the plain ones
      const bool scan = is_fill(s.func) || (s.ignore_nulls && c.nullable());
      const ColView cv = c.view();
      Column col;
      at::Tensor src;
      if (value) col = make_fixed_column(name, c.type, n, ex.device, true);
      else src = ex.empty_i64(n);
      uint8_t *o = value ? reinterpret_cast<uint8_t *>(col.data.data_ptr()) : nullptr;
      uint8_t *ov = value ? col.validity.data_ptr<uint8_t>() : nullptr;
      const Dense *d = (value || scan) ? &dense_of(s.col) : nullptr;
      const uint64_t *bits = d != nullptr ? u64(d->bits) : nullptr;
      const uint8_t *valid = d != nullptr && d->valid.defined() ? ptr<uint8_t>(d->valid) : nullptr;
      const uint8_t *restarts = !scan ? nullptr : rev ? ptr<uint8_t>(rflags) : ptr<uint8_t>(flags);
      Fill *f = scan ? &fill_of(s.col, rev) : nullptr;
      if (is_fill(s.func)) {
        KCALL(ex, window_fill_apply, cv, ptr<int64_t>(perm), restarts, n, rev, s.limit, bits, valid,
              ptr<int64_t>(f->carry), o, ov, opt_ptr(src), nullptr);
      } else {
        if (f != nullptr && !f->pos.defined()) {
          f->pos = ex.empty_i64(n);
          KCALL(ex, window_fill_apply, cv, ptr<int64_t>(perm), restarts, n, rev, 0, bits, valid,
                ptr<int64_t>(f->carry), nullptr, nullptr, nullptr, ptr<int64_t>(f->pos));
        }
        const int form = s.func == WIN_NTH_VALUE ? 2 : (s.func == WIN_FIRST_VALUE ? 0 : 1) + (f != nullptr ? 3 : 0);
        KCALL(ex, window_nav_pick, cv, ptr<int64_t>(perm), opt_ptr(phead), opt_ptr(rtail),
              f != nullptr ? ptr<int64_t>(f->pos) : nullptr, n, form, s.arg, bits, valid, o, ov, opt_ptr(src));
      }
      if (value) {
        out.push_back(std::move(col));
      } else {
        out.push_back(GatherColumn(c, src).with_name(name));
        ++nav_gather;
      }
      continue;
    }
    if (is_shift(s.func)) {
      const int64_t off = std::min(s.arg, n);  // n rows away is outside every partition
      at::Tensor src = ex.empty_i64(n);
      KCALL(ex, window_shift, ptr<int64_t>(perm), ptr<int64_t>(phead), n, s.func == WIN_LAG ? -off : off,
            ptr<int64_t>(src));
      out.push_back(GatherColumn(c, src).with_name(name));
      continue;
    }
    if (is_moment(s.func)) {
      const Bounds *b = is_moment_range(s.func) ? &bounds_of(s) : nullptr;
      const Dense &d = dense_of(s.col);
      const Pyramid &mp = moment_pyramid_of(s.col);
      Column col = make_fixed_column(name, DataType(Type::DOUBLE), n, ex.device, true);
      KCALL(ex, frame_moments_apply, c.view(), ptr<int64_t>(perm), n,
            s.func == WIN_ROLLING_STD || s.func == WIN_RANGE_STD, (int64_t)s.ddof, s.min_periods, u64(d.bits),
            d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr, b != nullptr ? u32(b->lo) : nullptr,
            b != nullptr ? u32(b->hi) : nullptr, ptr<int64_t>(phead), ptr<int64_t>(rtail), s.preceding, s.following,
            u64(mp.P), u64(mp.S), u64(mp.E), reinterpret_cast<uint8_t *>(col.data.data_ptr()),
            col.validity.data_ptr<uint8_t>());
      ++moment_specs;
      ++scans;
      out.push_back(std::move(col));
      continue;
    }
    const auto plan = value_plan(s, c);
    const bool nullable_out = nullable_result(s, c);
    if (is_range(s.func)) {
      const Bounds &b = bounds_of(s);
      const Dense &d = dense_of(s.col);
      const bool nulls = d.valid.defined();
      // COUNT of a column without nulls is hi - lo + 1; with nulls the count pyramid also gives every
      // other function its m
      static const Pyramid none;
      const Pyramid &cnt = nulls ? pyramid_of(s.col, kCount) : none;
      const Pyramid &val = plan.first == kCount ? cnt : pyramid_of(s.col, plan.first);
      Column col = make_fixed_column(name, plan.second, n, ex.device, nullable_out);
      KCALL(ex, frame_range_apply, c.view(), ptr<int64_t>(perm), n, plan.first, s.func == WIN_RANGE_MEAN,
            s.func == WIN_RANGE_COUNT ? 0 : s.min_periods, u64(d.bits), nulls ? ptr<uint8_t>(d.valid) : nullptr,
            u32(b.lo), u32(b.hi), val.P.defined() ? u64(val.P) : nullptr, val.S.defined() ? u64(val.S) : nullptr,
            val.E.defined() ? u64(val.E) : nullptr, cnt.P.defined() ? u64(cnt.P) : nullptr,
            cnt.S.defined() ? u64(cnt.S) : nullptr, cnt.E.defined() ? u64(cnt.E) : nullptr,
            reinterpret_cast<uint8_t *>(col.data.data_ptr()),
            nullable_out ? col.validity.data_ptr<uint8_t>() : nullptr);
      ++range_specs;
      ++scans;
      out.push_back(std::move(col));
      continue;
    }
    auto it = dense.find(s.col);
    const bool gather = it == dense.end();
    if (gather) {
      Dense d;
      d.bits = ex.empty_i64(n);
      if (c.nullable()) d.valid = ex.empty_u8(n);
      it = dense.emplace(s.col, d).first;
    }
    const Dense &d = it->second;
    Column col = make_fixed_column(name, plan.second, n, ex.device, nullable_out);
    at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles), carry = ex.empty_i64(ntiles);
    uint64_t *bits = reinterpret_cast<uint64_t *>(ptr<int64_t>(d.bits));
    uint8_t *valid = d.valid.defined() ? ptr<uint8_t>(d.valid) : nullptr;
    const ColView cv = c.view();
    if (is_rolling(s.func)) {
      // the dense values first (window_tile's tile pairs are not used: COUNT suits every column)
      if (gather)
        KCALL(ex, window_tile, cv, ptr<int64_t>(perm), ptr<uint8_t>(flags), n, kCount, bits, valid, true,
              ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
      const int64_t pre = std::min(s.preceding, n), fol = std::min(s.following, n);  // n rows: unbounded
      const int64_t w = pre + fol + 1;
      const bool mean = s.func == WIN_ROLLING_MEAN;
      const int64_t minp = s.func == WIN_ROLLING_COUNT ? 0 : s.min_periods;  // COUNT ignores it
      uint8_t *o = reinterpret_cast<uint8_t *>(col.data.data_ptr());
      uint8_t *ov = nullable_out ? col.validity.data_ptr<uint8_t>() : nullptr;
      if (w <= lds_rows) {
        KCALL(ex, rolling_lds, cv, ptr<int64_t>(perm), ptr<uint8_t>(flags), ptr<int64_t>(phead), ptr<int64_t>(rtail), n,
              plan.first, mean, pre, fol, minp, bits, valid, o, ov);
        ++frames_lds;
      } else {
        at::Tensor scan[2] = {ex.empty_i64(n), ex.empty_i64(n)};
        at::Tensor cnt[2] = {ex.empty_i64((n + 1) / 2), ex.empty_i64((n + 1) / 2)};  // n uint32
        at::Tensor tcnt = ex.empty_i64(ntiles), ccnt = ex.empty_i64(ntiles);
        for (int rev = 0; rev < 2; ++rev) {
          const uint8_t *restarts = rev ? ptr<uint8_t>(rflags) : ptr<uint8_t>(flags);
          KCALL(ex, rolling_tile, cv, restarts, n, plan.first, w, rev != 0, bits, valid, ptr<int64_t>(tagg),
                ptr<int64_t>(tcnt), ptr<uint8_t>(tflag));
          KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 1, plan.first, step,
                ptr<int64_t>(carry));
          KCALL(ex, window_carry, ptr<int64_t>(tcnt), ptr<uint8_t>(tflag), ntiles, 1, kCount, step,
                ptr<int64_t>(ccnt));
          KCALL(ex, rolling_scan, cv, restarts, n, plan.first, w, rev != 0, bits, valid, ptr<int64_t>(carry),
                ptr<int64_t>(ccnt), reinterpret_cast<uint64_t *>(ptr<int64_t>(scan[rev])),
                reinterpret_cast<uint32_t *>(ptr<int64_t>(cnt[rev])));
        }
        KCALL(ex, rolling_combine, cv, ptr<int64_t>(perm), ptr<int64_t>(phead), ptr<int64_t>(rtail), n, plan.first, mean,
              pre, fol, minp, reinterpret_cast<uint64_t *>(ptr<int64_t>(scan[0])),
              reinterpret_cast<uint32_t *>(ptr<int64_t>(cnt[0])), reinterpret_cast<uint64_t *>(ptr<int64_t>(scan[1])),
              reinterpret_cast<uint32_t *>(ptr<int64_t>(cnt[1])), o, ov);
        ++frames_wide;
      }
      ++scans;
      out.push_back(std::move(col));
      continue;
    }
    KCALL(ex, window_tile, cv, ptr<int64_t>(perm), ptr<uint8_t>(flags), n, plan.first, bits, valid, gather,
          ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
    KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 1, plan.first, step,
          ptr<int64_t>(carry));
    KCALL(ex, window_apply, cv, ptr<int64_t>(perm), ptr<uint8_t>(flags), n, plan.first, bits, valid,
          ptr<int64_t>(carry), reinterpret_cast<uint8_t *>(col.data.data_ptr()),
          nullable_out ? col.validity.data_ptr<uint8_t>() : nullptr);
    ++scans;
    out.push_back(std::move(col));
  }
  trace::add_counter("window.scan", scans);
  trace::add_counter("window.tiles", scans * ntiles);
  if (nav) {
    trace::add_counter("window.nav.fill", (int64_t)fills.size());
    trace::add_counter("window.nav.gather", nav_gather);
    trace::add_counter("window.nav.skipped", nav_skipped);
  }
  if (frames_lds) trace::add_counter("window.frame.lds", frames_lds);
  if (frames_wide) trace::add_counter("window.frame.wide", frames_wide);
  if (range_specs) {
    trace::add_counter("window.frame.range", range_specs);
    trace::add_counter("window.range.pyramids", (int64_t)pyramids.size());
  }
  // a RANGE VAR / STD spec searches (or shares) bounds too
  if (!range_bounds.empty()) trace::add_counter("window.range.bounds", (int64_t)range_bounds.size());
  if (moment_specs) {
    trace::add_counter("window.frame.moment", moment_specs);
    trace::add_counter("window.moment.pyramids", (int64_t)moment_pyramids.size());
  }
  return Table::Make(t->GetContext(), std::move(out));
}

TablePtr DistributedWindow(const TablePtr &t, const std::vector<int> &partition_cols,
                           const std::vector<int> &order_cols, const std::vector<bool> &ascending,
                           const std::vector<WindowSpec> &specs) {
  if (t->GetContext()->GetWorldSize() <= 1) return Window(t, partition_cols, order_cols, ascending, specs);
  CYLON_CHECK(!partition_cols.empty(), Code::Invalid,
              "a distributed window needs a partition column (a global order is not supported)");
  check(t, partition_cols, order_cols, ascending, specs);  // every rank fails before the exchange, or none
  return Window(Shuffle(t, partition_cols), partition_cols, order_cols, ascending, specs);
}

}  // namespace ops
}  // namespace cylon
