// The navigation and distribution window families (window_internal.hpp, kernels/window_nav.hip).
//
// They share the sort, the flags, the gathered values and the two rank scans of the call.  FFILL /
// BFILL and the IGNORE NULLS forms of FIRST / LAST_VALUE scan "the last non-null position" over the
// dense validity bytes, once per (column, direction) whatever the number of specs; a column without a
// validity array is answered without a scan.  FIRST / LAST / NTH_VALUE are one element-wise launch over
// phead / rtail, the distribution functions one over phead, rtail and the peer heads / tails that the
// two rank scans carry anyway.  Columns of width 1, 2, 4 or 8 are written straight from the dense
// values (value mode); every other type goes through a source-row array and GatherColumn.
#include "window_internal.hpp"

namespace cylon {
namespace ops {

namespace {

// fills: the tile pass and the carries once per (column, direction)
WinFill &fill_of(WinState &st, int col, bool rev) {
  auto it = st.fills.find({col, rev});
  if (it != st.fills.end()) return it->second;
  const Exec &ex = st.ex;
  const WinDense &d = st.dense_of(col);
  WinFill f;
  f.carry = ex.empty_i64(st.ntiles);
  at::Tensor tagg = ex.empty_i64(st.ntiles), tflag = ex.empty_u8(st.ntiles);
  KCALL(ex, window_fill_tile, rev ? ptr<uint8_t>(st.rflags) : ptr<uint8_t>(st.flags), st.n, rev, ptr<uint8_t>(d.valid),
        ptr<int64_t>(tagg), ptr<uint8_t>(tflag));
  KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), st.ntiles, 1, kMax, st.step, ptr<int64_t>(f.carry));
  ++st.scans;
  return st.fills.emplace(std::make_pair(col, rev), f).first->second;
}

}  // namespace

Column window_fill_or_pick(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const Exec &ex = st.ex;
  const int64_t n = st.n;
  const bool fill = win_info(s.func).family == WinFamily::Fill;
  st.nav = true;
  if (fill && !c.nullable()) {  // nothing to fill: the column itself, no scan
    ++st.nav_skipped;
    return c.with_name(name);
  }
  const bool value = win_word_cells(c);  // value mode: the kernels copy the cells themselves
  const bool rev = s.func == WIN_BFILL || s.func == WIN_FIRST_VALUE;
  // the IGNORE NULLS forms of a column without nulls are the plain ones
  const bool scan = fill || (s.ignore_nulls && c.nullable());
  const ColView cv = c.view();
  Column col;
  at::Tensor src;
  if (value) col = make_fixed_column(name, c.type, n, ex.device, true);
  else src = ex.empty_i64(n);
  uint8_t *o = out_data(col), *ov = out_valid(col);  // null in source mode
  const WinDense *d = (value || scan) ? &st.dense_of(s.col) : nullptr;
  const uint64_t *bits = d != nullptr ? d->b() : nullptr;
  const uint8_t *valid = d != nullptr ? d->v() : nullptr;
  const uint8_t *restarts = !scan ? nullptr : rev ? ptr<uint8_t>(st.rflags) : ptr<uint8_t>(st.flags);
  WinFill *f = scan ? &fill_of(st, s.col, rev) : nullptr;
  if (fill) {
    KCALL(ex, window_fill_apply, cv, ptr<int64_t>(st.perm), restarts, n, rev, s.limit, bits, valid,
          ptr<int64_t>(f->carry), o, ov, opt_ptr(src), nullptr);
  } else {
    // pos = the fill position of every sorted position, which only the IGNORE NULLS forms ask for
    if (f != nullptr && !f->pos.defined()) {
      f->pos = ex.empty_i64(n);
      KCALL(ex, window_fill_apply, cv, ptr<int64_t>(st.perm), restarts, n, rev, 0, bits, valid, ptr<int64_t>(f->carry),
            nullptr, nullptr, nullptr, ptr<int64_t>(f->pos));
    }
    const int form = s.func == WIN_NTH_VALUE ? 2 : (s.func == WIN_FIRST_VALUE ? 0 : 1) + (f != nullptr ? 3 : 0);
    KCALL(ex, window_nav_pick, cv, ptr<int64_t>(st.perm), opt_ptr(st.phead), opt_ptr(st.rtail),
          f != nullptr ? ptr<int64_t>(f->pos) : nullptr, n, form, s.arg, bits, valid, o, ov, opt_ptr(src));
  }
  if (value) return col;
  ++st.nav_gather;
  return GatherColumn(c, src).with_name(name);
}

Column window_dist(WinState &st, const WindowSpec &s, const std::string &name) {
  Column col = make_fixed_column(name, win_result_type(s, nullptr), st.n, st.ex.device, false);
  st.nav = true;
  KCALL(st.ex, window_dist_apply, ptr<int64_t>(st.perm), ptr<int64_t>(st.phead), ptr<int64_t>(st.rtail),
        opt_ptr(st.qhead), opt_ptr(st.rqhead), st.n, s.func - WIN_NTILE, s.arg, out_data(col));
  return col;
}

}  // namespace ops
}  // namespace cylon
