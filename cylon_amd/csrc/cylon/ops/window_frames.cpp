// The framed window families (window_internal.hpp): ROLLING, RANGE and VAR / STD specs of one Window() call.
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
// A VAR / STD spec over a ROWS or a RANGE frame (kernels/frame_moments.hip) shares all of that again.  Every
// value column gets one moment pyramid of (count, mean, M2) states per call, whatever the number of specs,
// their frame kinds, offsets, ddof or min_periods; a RANGE spec reuses the bounds search of its
// (preceding, following), a ROWS spec computes its bounds from phead / rtail in the query launch.
#include <algorithm>

#include "../kernels/frame_moments_common.hpp"
#include "../kernels/frame_range_common.hpp"

#include "window_internal.hpp"

namespace cylon {
namespace ops {

namespace {

uint64_t *u64(const at::Tensor &x) { return reinterpret_cast<uint64_t *>(ptr<int64_t>(x)); }
uint32_t *u32(const at::Tensor &x) { return reinterpret_cast<uint32_t *>(ptr<int64_t>(x)); }

// the bounds of a RANGE frame, searched once per (mode, offset) of the two sides; the first call turns
// the order column into search keys
const WinBounds &bounds_of(WinState &st, const WindowSpec &s) {
  const Exec &ex = st.ex;
  const int64_t n = st.n;
  if (!st.rkeys.defined()) {
    const Column &oc = st.t->column(st.order_col);
    st.rfloat = oc.type.kind() == ValueKind::FLOAT;
    const WinDense &d = st.dense_of(st.order_col);
    st.rkeys = ex.empty_i64(n);
    st.rcls = ex.empty_u8(n);
    KCALL(ex, frame_range_keys, oc.view(), d.b(), d.v(), n, st.descending, u64(st.rkeys), ptr<uint8_t>(st.rcls));
  }
  // a side: unbounded, an integer distance (integer keys) or a float64 one (float keys)
  struct Side { int mode; uint64_t i; double f; };
  auto side = [&](int64_t i, double f) -> Side {
    if (i == kWindowUnbounded) return {FR_UNBOUNDED, 0, 0};
    if (st.rfloat) return {FR_FLOAT, 0, s.offset_is_float ? f : (double)i};
    return {FR_INT, (uint64_t)i, 0};
  };
  const Side p = side(s.preceding, s.preceding_f), f = side(s.following, s.following_f);
  const auto key =
      std::make_tuple(p.mode, st.rfloat ? fr_f64_bits(p.f) : p.i, f.mode, st.rfloat ? fr_f64_bits(f.f) : f.i);
  auto it = st.range_bounds.find(key);
  if (it != st.range_bounds.end()) return it->second;
  WinBounds b{ex.empty_i64((n + 1) / 2), ex.empty_i64((n + 1) / 2)};
  KCALL(ex, frame_range_bounds, u64(st.rkeys), ptr<uint8_t>(st.rcls), ptr<int64_t>(st.phead), ptr<int64_t>(st.rtail), n,
        st.rfloat, st.descending, p.mode, p.i, p.f, f.mode, f.i, f.f, b.lo(), b.hi());
  return st.range_bounds.emplace(key, b).first->second;
}

const WinPyramid &pyramid_of(WinState &st, int col, int func) {
  auto it = st.pyramids.find({col, func});
  if (it != st.pyramids.end()) return it->second;
  const Exec &ex = st.ex;
  const WinDense &d = st.dense_of(col);
  WinPyramid p{ex.empty_i64(fr_ps_slots(st.n)), ex.empty_i64(fr_ps_slots(st.n)), ex.empty_i64(fr_e_slots(st.n))};
  KCALL(ex, frame_range_pyramid, st.t->column(col).view(), st.n, func, d.b(), d.v(), p.P(), p.S(), p.E());
  return st.pyramids.emplace(std::make_pair(col, func), p).first->second;
}

const WinPyramid &moment_pyramid_of(WinState &st, int col) {
  auto it = st.moment_pyramids.find(col);
  if (it != st.moment_pyramids.end()) return it->second;
  const Exec &ex = st.ex;
  const int64_t n = st.n;
  const WinDense &d = st.dense_of(col);
  WinPyramid p{ex.empty_i64(fm_words(fm_ps_slots(n))), ex.empty_i64(fm_words(fm_ps_slots(n))),
               ex.empty_i64(fm_words(fm_e_slots(n)))};
  KCALL(ex, frame_moments_pyramid, st.t->column(col).view(), n, d.b(), d.v(), p.P(), p.S(), p.E());
  return st.moment_pyramids.emplace(col, p).first->second;
}

}  // namespace

Column window_rolling(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const Exec &ex = st.ex;
  const int64_t n = st.n, ntiles = st.ntiles;
  const int func = win_kernel(win_info(s.func), c);
  const WinDense &d = st.dense_of(s.col);
  const ColView cv = c.view();
  Column col = make_fixed_column(name, win_result_type(s, &c), n, ex.device, win_nullable_result(s, &c));
  const int64_t pre = std::min(s.preceding, n), fol = std::min(s.following, n), w = pre + fol + 1;  // n rows: unbounded
  const bool mean = s.func == WIN_ROLLING_MEAN;
  const int64_t minp = s.func == WIN_ROLLING_COUNT ? 0 : s.min_periods;  // COUNT ignores it
  if (w <= KSIZE(ex, window_frame_lds_rows)) {
    KCALL(ex, rolling_lds, cv, ptr<int64_t>(st.perm), ptr<uint8_t>(st.flags), ptr<int64_t>(st.phead),
          ptr<int64_t>(st.rtail), n, func, mean, pre, fol, minp, d.b(), d.v(), out_data(col), out_valid(col));
    ++st.frames_lds;
  } else {  // a windowed scan forwards and one over the reversed order, combined
    at::Tensor tagg = ex.empty_i64(ntiles), tflag = ex.empty_u8(ntiles), carry = ex.empty_i64(ntiles);
    at::Tensor scan[2] = {ex.empty_i64(n), ex.empty_i64(n)};
    at::Tensor cnt[2] = {ex.empty_i64((n + 1) / 2), ex.empty_i64((n + 1) / 2)};  // n uint32
    at::Tensor tcnt = ex.empty_i64(ntiles), ccnt = ex.empty_i64(ntiles);
    for (int rev = 0; rev < 2; ++rev) {
      const uint8_t *restarts = rev ? ptr<uint8_t>(st.rflags) : ptr<uint8_t>(st.flags);
      KCALL(ex, rolling_tile, cv, restarts, n, func, w, rev != 0, d.b(), d.v(), ptr<int64_t>(tagg), ptr<int64_t>(tcnt),
            ptr<uint8_t>(tflag));
      KCALL(ex, window_carry, ptr<int64_t>(tagg), ptr<uint8_t>(tflag), ntiles, 1, func, st.step, ptr<int64_t>(carry));
      KCALL(ex, window_carry, ptr<int64_t>(tcnt), ptr<uint8_t>(tflag), ntiles, 1, kCount, st.step, ptr<int64_t>(ccnt));
      KCALL(ex, rolling_scan, cv, restarts, n, func, w, rev != 0, d.b(), d.v(), ptr<int64_t>(carry), ptr<int64_t>(ccnt),
            u64(scan[rev]), u32(cnt[rev]));
    }
    KCALL(ex, rolling_combine, cv, ptr<int64_t>(st.perm), ptr<int64_t>(st.phead), ptr<int64_t>(st.rtail), n, func, mean,
          pre, fol, minp, u64(scan[0]), u32(cnt[0]), u64(scan[1]), u32(cnt[1]), out_data(col), out_valid(col));
    ++st.frames_wide;
  }
  ++st.scans;
  return col;
}

Column window_range(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const int func = win_kernel(win_info(s.func), c);
  const WinBounds &b = bounds_of(st, s);
  const WinDense &d = st.dense_of(s.col);
  // COUNT of a column without nulls is hi - lo + 1; with nulls the count pyramid also gives every
  // other function its m
  const WinPyramid cnt = d.valid.defined() ? pyramid_of(st, s.col, kCount) : WinPyramid();
  const WinPyramid val = func == kCount ? cnt : pyramid_of(st, s.col, func);
  Column col = make_fixed_column(name, win_result_type(s, &c), st.n, st.ex.device, win_nullable_result(s, &c));
  KCALL(st.ex, frame_range_apply, c.view(), ptr<int64_t>(st.perm), st.n, func, s.func == WIN_RANGE_MEAN,
        s.func == WIN_RANGE_COUNT ? 0 : s.min_periods, d.b(), d.v(), b.lo(), b.hi(), val.P(), val.S(), val.E(), cnt.P(),
        cnt.S(), cnt.E(), out_data(col), out_valid(col));
  ++st.range_specs;
  ++st.scans;
  return col;
}

Column window_moment(WinState &st, const WindowSpec &s, const Column &c, const std::string &name) {
  const WinBounds b = win_info(s.func).family == WinFamily::MomentRange ? bounds_of(st, s) : WinBounds();
  const WinDense &d = st.dense_of(s.col);
  const WinPyramid &mp = moment_pyramid_of(st, s.col);
  Column col = make_fixed_column(name, win_result_type(s, &c), st.n, st.ex.device, win_nullable_result(s, &c));
  KCALL(st.ex, frame_moments_apply, c.view(), ptr<int64_t>(st.perm), st.n,
        s.func == WIN_ROLLING_STD || s.func == WIN_RANGE_STD, (int64_t)s.ddof, s.min_periods, d.b(), d.v(), b.lo(),
        b.hi(), ptr<int64_t>(st.phead), ptr<int64_t>(st.rtail), s.preceding, s.following, mp.P(), mp.S(), mp.E(),
        out_data(col), out_valid(col));
  ++st.moment_specs;
  ++st.scans;
  return col;
}

}  // namespace ops
}  // namespace cylon
