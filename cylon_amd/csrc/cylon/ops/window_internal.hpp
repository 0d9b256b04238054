// What the window operator's files share (window.cpp, window_frames.cpp, window_nav.cpp): the table
// that describes every WindowFunc, the state of one Window() call, and one function per family.
#pragma once
#include <map>
#include <tuple>

#include "util.hpp"

namespace cylon {
namespace ops {

// kernels/window.hip WinFunc; kSum stands for kSumF on a float column and kSumI on every other
constexpr int kSumI = 0, kSumF = 1, kMin = 2, kMax = 3, kCount = 4, kRank = 5, kSum = -1, kNoKernel = -2;

enum class WinFamily { Ranking, Running, Shift, Rolling, Range, Pick, Fill, Dist, MomentRows, MomentRange };

// the rule for a spec's result type: INT64, DOUBLE, the group-by's SUM type of the column, the column's
// type written by a scan kernel, or the column itself gathered (any type, variable width included)
enum class WinResult { Int64, Double, Sum, Column, Gathered };

// what a function reads of the two rank scans: the partition heads (forward scan), the partition tails
// (the scan of the reversed flags; they need the reversed flags), the reversed flags alone, the heads /
// tails of the row's peers, and the forward scan's own outputs (kRankOut << ROW_NUMBER, RANK, DENSE_RANK)
// kFrame = kPhead | kRtail: both ends of the partition, which every framed and distribution function reads
enum : unsigned { kPhead = 1, kRtail = 2, kFrame = 3, kRflags = 4, kPeerHeads = 8, kPeerTails = 16, kRankOut = 32 };

struct WinFuncInfo {
  const char *name;
  WinFamily family;
  bool column;  // takes a value column
  unsigned needs;
  int kernel;
  WinResult result;
};

constexpr WinFuncInfo kWinFuncs[] = {
    {"row_number", WinFamily::Ranking, false, kRankOut << WIN_ROW_NUMBER, kNoKernel, WinResult::Int64},
    {"rank", WinFamily::Ranking, false, kRankOut << WIN_RANK, kNoKernel, WinResult::Int64},
    {"dense_rank", WinFamily::Ranking, false, kRankOut << WIN_DENSE_RANK, kNoKernel, WinResult::Int64},
    {"cumcount", WinFamily::Running, true, 0, kCount, WinResult::Int64},
    {"cumsum", WinFamily::Running, true, 0, kSum, WinResult::Sum},
    {"cummin", WinFamily::Running, true, 0, kMin, WinResult::Column},
    {"cummax", WinFamily::Running, true, 0, kMax, WinResult::Column},
    {"lag", WinFamily::Shift, true, kPhead, kNoKernel, WinResult::Gathered},
    {"lead", WinFamily::Shift, true, kPhead, kNoKernel, WinResult::Gathered},
    {"rolling_count", WinFamily::Rolling, true, kFrame, kCount, WinResult::Int64},
    {"rolling_sum", WinFamily::Rolling, true, kFrame, kSum, WinResult::Sum},
    {"rolling_mean", WinFamily::Rolling, true, kFrame, kSum, WinResult::Double},
    {"rolling_min", WinFamily::Rolling, true, kFrame, kMin, WinResult::Column},
    {"rolling_max", WinFamily::Rolling, true, kFrame, kMax, WinResult::Column},
    {"range_count", WinFamily::Range, true, kFrame, kCount, WinResult::Int64},
    {"range_sum", WinFamily::Range, true, kFrame, kSum, WinResult::Sum},
    {"range_mean", WinFamily::Range, true, kFrame, kSum, WinResult::Double},
    {"range_min", WinFamily::Range, true, kFrame, kMin, WinResult::Column},
    {"range_max", WinFamily::Range, true, kFrame, kMax, WinResult::Column},
    // with ignore_nulls FIRST_VALUE reads the reversed fill scan, which restarts at the reversed flags
    {"first_value", WinFamily::Pick, true, kPhead, kNoKernel, WinResult::Gathered},
    {"last_value", WinFamily::Pick, true, kRtail, kNoKernel, WinResult::Gathered},
    {"nth_value", WinFamily::Pick, true, kPhead | kRtail, kNoKernel, WinResult::Gathered},
    {"ffill", WinFamily::Fill, true, 0, kNoKernel, WinResult::Gathered},
    {"bfill", WinFamily::Fill, true, kRflags, kNoKernel, WinResult::Gathered},
    {"ntile", WinFamily::Dist, false, kFrame, kNoKernel, WinResult::Int64},
    {"percent_rank", WinFamily::Dist, false, kFrame | kPeerHeads, kNoKernel, WinResult::Double},
    {"cume_dist", WinFamily::Dist, false, kFrame | kPeerTails, kNoKernel, WinResult::Double},
    {"rolling_var", WinFamily::MomentRows, true, kFrame, kNoKernel, WinResult::Double},
    {"rolling_std", WinFamily::MomentRows, true, kFrame, kNoKernel, WinResult::Double},
    {"range_var", WinFamily::MomentRange, true, kFrame, kNoKernel, WinResult::Double},
    {"range_std", WinFamily::MomentRange, true, kFrame, kNoKernel, WinResult::Double},
};
static_assert(sizeof(kWinFuncs) / sizeof(kWinFuncs[0]) == WIN_RANGE_STD + 1, "one row per WindowFunc");

inline const WinFuncInfo &win_info(WindowFunc f) {
  CYLON_CHECK(f >= WIN_ROW_NUMBER && f <= WIN_RANGE_STD, Code::Invalid, "window function " << static_cast<int>(f));
  return kWinFuncs[f];
}
inline bool win_moment(WinFamily f) { return f == WinFamily::MomentRows || f == WinFamily::MomentRange; }
inline bool win_framed(WinFamily f) { return f == WinFamily::Rolling || f == WinFamily::Range || win_moment(f); }
// a RANGE frame over the one order column's values
inline bool win_by_value(WinFamily f) { return f == WinFamily::Range || f == WinFamily::MomentRange; }

// a column whose cells the kernels read and write as 1, 2, 4 or 8-byte words
inline bool win_word_cells(const Column &c) {
  return !c.is_var() && (c.type.width() == 1 || c.type.width() == 2 || c.type.width() == 4 || c.type.width() == 8);
}
// the kernel function of a value spec on column c
inline int win_kernel(const WinFuncInfo &fi, const Column &c) {
  return fi.kernel != kSum ? fi.kernel : c.type.kind() == ValueKind::FLOAT ? kSumF : kSumI;
}
// the result type of a spec and whether it has a validity array (c: the value column, if it takes one)
DataType win_result_type(const WindowSpec &s, const Column *c);
bool win_nullable_result(const WindowSpec &s, const Column *c);

struct WinDense {  // a value column gathered into sorted order
  at::Tensor bits, valid;
  uint64_t *b() const { return reinterpret_cast<uint64_t *>(ptr<int64_t>(bits)); }
  uint8_t *v() const { return valid.defined() ? ptr<uint8_t>(valid) : nullptr; }  // null: no nulls
};
struct WinBounds {  // a RANGE frame per sorted position; undefined (a ROWS frame): null
  at::Tensor lo_, hi_;  // n uint32 each
  uint32_t *lo() const { return lo_.defined() ? reinterpret_cast<uint32_t *>(ptr<int64_t>(lo_)) : nullptr; }
  uint32_t *hi() const { return hi_.defined() ? reinterpret_cast<uint32_t *>(ptr<int64_t>(hi_)) : nullptr; }
};
struct WinPyramid {  // a scan pyramid of frame_range.hip or frame_moments.hip; undefined: all null
  at::Tensor P_, S_, E_;
  uint64_t *P() const { return P_.defined() ? reinterpret_cast<uint64_t *>(ptr<int64_t>(P_)) : nullptr; }
  uint64_t *S() const { return S_.defined() ? reinterpret_cast<uint64_t *>(ptr<int64_t>(S_)) : nullptr; }
  uint64_t *E() const { return E_.defined() ? reinterpret_cast<uint64_t *>(ptr<int64_t>(E_)) : nullptr; }
};
// a fill scan's carries, and the fill position of every sorted position (IGNORE NULLS)
struct WinFill { at::Tensor carry, pos; };

inline int64_t *opt_ptr(const at::Tensor &t) { return t.defined() ? ptr<int64_t>(t) : nullptr; }
// the data and the validity bytes of an output column; null where it has none
inline uint8_t *out_data(const Column &c) { return c.data.defined() ? (uint8_t *)c.data.data_ptr() : nullptr; }
inline uint8_t *out_valid(const Column &c) { return c.validity.defined() ? c.validity.data_ptr<uint8_t>() : nullptr; }

// One Window() call on a table of n > 0 rows: what the sort and the shared scans left, the caches the
// specs fill in spec order, and the counters.  A plain struct; the families below are free functions.
struct WinState {
  Exec ex;
  TablePtr t;
  int order_col = -1;  // the first order column (RANGE frames have exactly one) and its direction
  bool descending = false;
  int64_t n = 0, ntiles = 0, step = 0;
  at::Tensor perm, flags, rflags;              // flags: bit 0 partition head, bit 1 peer head
  at::Tensor phead, rtail, qhead, rqhead;      // per sorted position; undefined where no spec needs them
  at::Tensor ranks[3];                         // ROW_NUMBER, RANK, DENSE_RANK per row

  std::map<int, WinDense> dense;  // by value column
  // RANGE frames: the order column's search keys once, the bounds once per (mode, offset) of the two
  // sides, a pyramid once per (value column, kernel function); moments: a pyramid once per value column
  at::Tensor rkeys, rcls;
  bool rfloat = false;
  std::map<std::tuple<int, uint64_t, int, uint64_t>, WinBounds> range_bounds;
  std::map<std::pair<int, int>, WinPyramid> pyramids;
  std::map<int, WinPyramid> moment_pyramids;
  std::map<std::pair<int, bool>, WinFill> fills;  // by (value column, reversed)

  int64_t scans = 0, frames_lds = 0, frames_wide = 0, range_specs = 0, moment_specs = 0, nav_gather = 0,
          nav_skipped = 0;
  bool nav = false;  // a navigation or distribution spec ran

  explicit WinState(const TablePtr &table) : ex(table->device()), t(table), n(table->Rows()) {}

  // The dense values of a column, gathered by its first user with a COUNT tile pass.  A caller that
  // passes `gather` runs window_tile itself and fuses the gather into that pass where *gather comes back true.
  const WinDense &dense_of(int col, bool *gather = nullptr);
};

// ---- window_frames.cpp
Column window_rolling(WinState &st, const WindowSpec &s, const Column &c, const std::string &name);
Column window_range(WinState &st, const WindowSpec &s, const Column &c, const std::string &name);
Column window_moment(WinState &st, const WindowSpec &s, const Column &c, const std::string &name);

// ---- window_nav.cpp
Column window_fill_or_pick(WinState &st, const WindowSpec &s, const Column &c, const std::string &name);
Column window_dist(WinState &st, const WindowSpec &s, const std::string &name);

}  // namespace ops
}  // namespace cylon
