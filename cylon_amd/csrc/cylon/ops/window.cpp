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
// Window() reads top to bottom: check the call, plan what the specs need of the shared scans (from the
// function table of window_internal.hpp), sort and flag, run those scans, then one function per family
// in spec order over the call's WinState, and the trace counters.  The framed families (ROLLING, RANGE,
// VAR / STD) are in window_frames.cpp, the navigation and distribution functions in window_nav.cpp;
// each of those files describes what its specs share.
#include <algorithm>
#include <set>

#include "../trace.hpp"
#include "window_internal.hpp"

namespace cylon {
namespace ops {

namespace {

// the order column of a RANGE frame: an integer of any width, a temporal type, float32 or float64
bool range_order_type(const Column &c) {
  switch (c.type.type) {
    case Type::UINT8: case Type::INT8: case Type::UINT16: case Type::INT16: case Type::UINT32: case Type::INT32:
    case Type::UINT64: case Type::INT64: case Type::FLOAT: case Type::DOUBLE: case Type::DATE32: case Type::DATE64:
    case Type::TIMESTAMP: case Type::TIME32: case Type::TIME64: case Type::DURATION: return !c.is_var();
    default: return false;
  }
}

bool scan_value(const Column &c) { return c.type.is_numeric() && win_word_cells(c); }

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
    const WinFuncInfo &fi = win_info(s.func);
    const WinFamily fam = fi.family;
    const char *fn = fi.name;
    std::string name = s.name;
    if (!fi.column) {
      if (name.empty()) name = fn;
      if (s.func == WIN_NTILE) CYLON_CHECK(s.arg >= 1, Code::Invalid, "window ntile of " << s.arg << " buckets");
    } else {
      CYLON_CHECK(s.col >= 0 && s.col < t->Columns(), Code::Invalid, "window " << fn << " of column " << s.col);
      const Column &c = t->column(s.col);
      const bool sum = fi.kernel == kSum || win_moment(fam);  // float16 values are not summed
      if (name.empty()) name = std::string(fn) + "_" + c.name;
      if (win_framed(fam))
        CYLON_CHECK(t->Rows() < (int64_t(1) << 32), Code::Invalid,
                    "window " << fn << " over " << t->Rows() << " rows: framed functions take fewer than 2^32");
      if (fam == WinFamily::Running || win_framed(fam))  // COUNT reads the validity alone
        CYLON_CHECK(fi.kernel == kCount || (scan_value(c) && !(sum && c.type.type == Type::HALF_FLOAT)),
                    Code::Invalid, "window " << fn << " needs a fixed-width numeric column, got " << c.type.ToString());
      if (fam == WinFamily::Shift)
        CYLON_CHECK(s.arg >= 0, Code::Invalid, "window " << fn << " offset " << s.arg << " < 0");
      if (s.func == WIN_NTH_VALUE) {
        CYLON_CHECK(s.arg >= 1, Code::Invalid, "window nth_value of row " << s.arg << " < 1");
        CYLON_CHECK(!s.ignore_nulls, Code::Invalid, "window nth_value does not take ignore_nulls");
      }
      if (fam == WinFamily::Fill)
        CYLON_CHECK(s.limit >= 0, Code::Invalid, "window " << fn << " limit " << s.limit << " < 0");
      if (win_framed(fam)) {
        CYLON_CHECK(s.preceding >= 0 && s.following >= 0, Code::Invalid,
                    "window " << fn << " frame of " << s.preceding << " preceding, " << s.following << " following");
        CYLON_CHECK(fi.kernel == kCount || s.min_periods >= 1, Code::Invalid,
                    "window " << fn << " min_periods " << s.min_periods << " < 1");
        CYLON_CHECK(!win_moment(fam) || s.ddof >= 0, Code::Invalid, "window " << fn << " ddof " << s.ddof << " < 0");
      }
      if (win_by_value(fam)) {
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

// the new columns of an empty table
TablePtr empty_result(const TablePtr &t, const std::vector<WindowSpec> &specs, const Checked &ck) {
  Exec ex(t->device());
  std::vector<Column> out = t->columns();
  for (size_t i = 0; i < specs.size(); ++i) {
    const WinFuncInfo &fi = win_info(specs[i].func);
    const Column *c = fi.column ? &t->column(specs[i].col) : nullptr;
    out.push_back(fi.result == WinResult::Gathered
                      ? GatherColumn(*c, ex.empty_i64(0)).with_name(ck.names[i])
                      : make_fixed_column(ck.names[i], win_result_type(specs[i], c), 0, ex.device,
                                          win_nullable_result(specs[i], c)));
  }
  return Table::Make(t->GetContext(), std::move(out));
}

// perm = the defining order; flags: bit 0 partition head, bit 1 peer head
void sort_and_flag(WinState &st, const std::vector<int> &partition_cols, const std::vector<int> &order_cols,
                   const std::vector<bool> &asc) {
  const Exec &ex = st.ex;
  const int64_t n = st.n;
  std::vector<int> keys = partition_cols;
  keys.insert(keys.end(), order_cols.begin(), order_cols.end());
  std::vector<bool> dirs(partition_cols.size(), true);
  dirs.insert(dirs.end(), asc.begin(), asc.end());
  st.perm = ex.empty_i64(n);
  if (keys.empty()) {
    KCALL(ex, iota, ptr<int64_t>(st.perm), n, 0);
  } else {
    st.perm = SortIndices(st.t, keys, dirs).contiguous();
    // the scans' 16-byte loads
    if (reinterpret_cast<uintptr_t>(st.perm.data_ptr()) % 16 != 0) st.perm = st.perm.clone();
  }
  trace::add_counter("window.sort", keys.empty() ? 0 : 1);

  st.flags = ex.empty_u8(n);
  at::Tensor peer;
  const std::vector<ColView> pv = views(st.t, partition_cols);
  KCALL(ex, segment_heads, pv.data(), (int)pv.size(), ptr<int64_t>(st.perm), n, ptr<uint8_t>(st.flags));
  if (!order_cols.empty()) {
    const std::vector<ColView> kv = views(st.t, keys);
    peer = ex.empty_u8(n);
    KCALL(ex, segment_heads, kv.data(), (int)kv.size(), ptr<int64_t>(st.perm), n, ptr<uint8_t>(peer));
  }
  KCALL(ex, window_flags, ptr<uint8_t>(st.flags), peer.defined() ? ptr<uint8_t>(peer) : nullptr, n,
        ptr<uint8_t>(st.flags));
}

// One scan of flag bytes: the ranking functions (forward scan only), the head of every position's
// partition, and where `peers` is given the head of every position's peers.
void rank_scan(WinState &st, const at::Tensor &flags, at::Tensor *heads, at::Tensor *peers) {
  const Exec &ex = st.ex;
  const bool forward = heads == &st.phead;
  at::Tensor tagg = ex.empty_i64(3 * st.ntiles), tflag = ex.empty_u8(st.ntiles), carry = ex.empty_i64(3 * st.ntiles);
  KCALL(ex, window_rank_tile, ptr<uint8_t>(flags), st.n, ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
  KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), st.ntiles, 3, kRank, st.step, ptr<int64_t>(carry));
  KCALL(ex, window_rank_apply, ptr<int64_t>(st.perm), ptr<uint8_t>(flags), st.n, ptr<int64_t>(carry),
        forward ? opt_ptr(st.ranks[0]) : nullptr, forward ? opt_ptr(st.ranks[1]) : nullptr,
        forward ? opt_ptr(st.ranks[2]) : nullptr, opt_ptr(*heads));
  if (peers != nullptr) {
    *peers = ex.empty_i64(st.n);
    KCALL(ex, window_rank_heads, ptr<uint8_t>(flags), st.n, ptr<int64_t>(carry), nullptr, ptr<int64_t>(*peers));
  }
  ++st.scans;
}

// CUMCOUNT / CUMSUM / CUMMIN / CUMMAX: one value scan; the first spec on a column gathers its dense
// values in the scan's own tile pass
Column window_running(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const Exec &ex = st.ex;
  const int func = win_kernel(win_info(s.func), c);
  bool gather;
  const WinDense &d = st.dense_of(s.col, &gather);
  Column col = make_fixed_column(name, win_result_type(s, &c), st.n, ex.device, win_nullable_result(s, &c));
  at::Tensor tagg = ex.empty_i64(st.ntiles), tflag = ex.empty_u8(st.ntiles), carry = ex.empty_i64(st.ntiles);
  KCALL(ex, window_tile, c.view(), ptr<int64_t>(st.perm), ptr<uint8_t>(st.flags), st.n, func, d.b(), d.v(), gather,
        ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
  KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), st.ntiles, 1, func, st.step, ptr<int64_t>(carry));
  KCALL(ex, window_apply, c.view(), ptr<int64_t>(st.perm), ptr<uint8_t>(st.flags), st.n, func, d.b(), d.v(),
        ptr<int64_t>(carry), out_data(col), out_valid(col));
  ++st.scans;
  return col;
}

// LAG / LEAD: the source row of every row, then a gather of the column, whatever its type
Column window_shift(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const int64_t off = std::min(s.arg, st.n);  // n rows away is outside every partition
  at::Tensor src = st.ex.empty_i64(st.n);
  KCALL(st.ex, window_shift, ptr<int64_t>(st.perm), ptr<int64_t>(st.phead), st.n, s.func == WIN_LAG ? -off : off,
        ptr<int64_t>(src));
  return GatherColumn(c, src).with_name(name);
}

void add_counters(const WinState &st) {
  trace::add_counter("window.scan", st.scans);
  trace::add_counter("window.tiles", st.scans * st.ntiles);
  if (st.nav) {
    trace::add_counter("window.nav.fill", (int64_t)st.fills.size());
    trace::add_counter("window.nav.gather", st.nav_gather);
    trace::add_counter("window.nav.skipped", st.nav_skipped);
  }
  if (st.frames_lds) trace::add_counter("window.frame.lds", st.frames_lds);
  if (st.frames_wide) trace::add_counter("window.frame.wide", st.frames_wide);
  if (st.range_specs) {
    trace::add_counter("window.frame.range", st.range_specs);
    trace::add_counter("window.range.pyramids", (int64_t)st.pyramids.size());
  }
  // a RANGE VAR / STD spec searches (or shares) bounds too
  if (!st.range_bounds.empty()) trace::add_counter("window.range.bounds", (int64_t)st.range_bounds.size());
  if (st.moment_specs) {
    trace::add_counter("window.frame.moment", st.moment_specs);
    trace::add_counter("window.moment.pyramids", (int64_t)st.moment_pyramids.size());
  }
}

}  // namespace

DataType win_result_type(const WindowSpec &s, const Column *c) {
  switch (win_info(s.func).result) {
    case WinResult::Int64: return DataType(Type::INT64);
    case WinResult::Double: return DataType(Type::DOUBLE);
    case WinResult::Sum:  // the group-by's SUM
      if (c->type.kind() == ValueKind::FLOAT) return DataType(Type::DOUBLE);
      return DataType(c->type.kind() == ValueKind::UNSIGNED_INT ? Type::UINT64 : Type::INT64);
    default: return c->type;
  }
}

// A running aggregate is null where its row's value is; a framed one where the frame holds fewer than
// min_periods values, which a frame of a column without nulls can only do for min_periods > 1.  A
// navigation function's output is always nullable (NTH_VALUE past the partition's end), except the
// fill of a column without nulls, which is the column itself; a distribution function's never is.
bool win_nullable_result(const WindowSpec &s, const Column *c) {
  const WinFuncInfo &fi = win_info(s.func);
  if (!fi.column) return false;
  if (fi.family == WinFamily::Pick || win_moment(fi.family)) return true;  // VAR / STD: null where m - ddof <= 0
  if (fi.family == WinFamily::Fill) return c->nullable();
  if (fi.kernel == kCount) return false;
  return c->nullable() || (win_framed(fi.family) && s.min_periods > 1);
}

const WinDense &WinState::dense_of(int col, bool *gather) {
  auto it = dense.find(col);
  if (gather != nullptr) *gather = it == dense.end();
  if (it != dense.end()) return it->second;
  const Column &c = t->column(col);
  WinDense d;
  d.bits = ex.empty_i64(n);
  if (c.nullable()) d.valid = ex.empty_u8(n);
  if (gather == nullptr) {  // window_tile's tile pairs are not used: COUNT suits every column
    at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles);
    KCALL(ex, window_tile, c.view(), ptr<int64_t>(perm), ptr<uint8_t>(flags), n, kCount, d.b(), d.v(), true,
          ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
  }
  return dense.emplace(col, d).first->second;
}

TablePtr Window(const TablePtr &t, const std::vector<int> &partition_cols, const std::vector<int> &order_cols,
                const std::vector<bool> &ascending, const std::vector<WindowSpec> &specs, int64_t carry_step_tiles) {
  const Checked ck = check(t, partition_cols, order_cols, ascending, specs);
  if (specs.empty()) return t;
  if (t->Rows() == 0) return empty_result(t, specs, ck);
  WinState st(t);
  const Exec &ex = st.ex;
  const int64_t n = st.n;
  CYLON_PHASE("window", ex.device);
  const int64_t max_step = KSIZE(ex, window_carry_tiles);
  CYLON_CHECK(carry_step_tiles <= max_step, Code::Invalid, "window: carry step of " << carry_step_tiles << " tiles");
  st.step = carry_step_tiles > 0 ? carry_step_tiles : max_step;
  st.order_col = order_cols.empty() ? -1 : order_cols[0];
  st.descending = !order_cols.empty() && !ck.asc[0];
  // the plan: what the specs need of the shared scans (kPhead | kRtail | ...).  With IGNORE NULLS,
  // FIRST_VALUE reads the reversed fill scan, which restarts at the reversed flags.
  unsigned need = 0;
  for (const auto &s : specs)
    need |= win_info(s.func).needs | (s.func == WIN_FIRST_VALUE && s.ignore_nulls ? kRflags : 0);

  sort_and_flag(st, partition_cols, order_cols, ck.asc);
  const int64_t T = KSIZE(ex, window_tile_rows);
  st.ntiles = (n + T - 1) / T;

  // ranking functions and the partition heads: one scan of the flags.  PERCENT_RANK's RANK - 1 is the
  // head of the row's peers - phead.
  if (need & kPhead) st.phead = ex.empty_i64(n);
  for (int k = 0; k < 3; ++k)
    if (need & (kRankOut << k)) st.ranks[k] = ex.empty_i64(n);
  if (need & (kPhead | 7 * kRankOut)) rank_scan(st, st.flags, &st.phead, need & kPeerHeads ? &st.qhead : nullptr);

  // framed specs, and the functions that look at the partition's end: the partition tails, as the
  // heads of the reversed order.  CUME_DIST marks the peer tails in the same flags, and the scan's q word
  // is then the last peer of every position.
  if (need & (kRtail | kRflags)) {
    st.rflags = ex.empty_u8(n);
    if (need & kPeerTails) KCALL(ex, window_rev_peer_flags, ptr<uint8_t>(st.flags), n, ptr<uint8_t>(st.rflags));
    else KCALL(ex, window_rev_flags, ptr<uint8_t>(st.flags), n, ptr<uint8_t>(st.rflags));
  }
  if (need & kRtail) {
    st.rtail = ex.empty_i64(n);
    rank_scan(st, st.rflags, &st.rtail, need & kPeerTails ? &st.rqhead : nullptr);
  }

  std::vector<Column> out = t->columns();
  for (size_t i = 0; i < specs.size(); ++i) {
    const WindowSpec &s = specs[i];
    const std::string &name = ck.names[i];
    const WinFuncInfo &fi = win_info(s.func);
    const Column *c = fi.column ? &t->column(s.col) : nullptr;
    switch (fi.family) {
      case WinFamily::Ranking: out.push_back(Column(name, DataType(Type::INT64), n, st.ranks[s.func])); break;
      case WinFamily::Running: out.push_back(window_running(st, s, *c, name)); break;
      case WinFamily::Shift: out.push_back(window_shift(st, s, *c, name)); break;
      case WinFamily::Rolling: out.push_back(window_rolling(st, s, *c, name)); break;
      case WinFamily::Range: out.push_back(window_range(st, s, *c, name)); break;
      case WinFamily::MomentRows:
      case WinFamily::MomentRange: out.push_back(window_moment(st, s, *c, name)); break;
      case WinFamily::Pick:
      case WinFamily::Fill: out.push_back(window_fill_or_pick(st, s, *c, name)); break;
      case WinFamily::Dist: out.push_back(window_dist(st, s, name)); break;
    }
  }
  add_counters(st);
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
