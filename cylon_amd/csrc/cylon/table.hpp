// Table: the core data structure (L2), and the engine's operator API (L4/L5).
//
// Reference: cpp/src/cylon/table.hpp:46-468 (Table wraps arrow::Table; all
// relational operators are free functions over shared_ptr<Table>).
// Here a Table is a vector of device-resident Columns on the context's device
// (an MI355X under one-process-per-GPU), plus the reference's retain flag.
// Operators in namespace cylon::ops throw CylonError; the Status-returning
// reference-shaped API lives in api.hpp.
#pragma once
#include <functional>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "column.hpp"
#include "ctx/cylon_context.hpp"
#include "join/join_config.hpp"

namespace cylon {

namespace indexing {
class BaseIndex;
}

class Table;
using TablePtr = std::shared_ptr<Table>;

class Table {
 public:
  Table(std::shared_ptr<CylonContext> ctx, std::vector<Column> columns);

  static TablePtr Make(std::shared_ptr<CylonContext> ctx, std::vector<Column> columns) {
    return std::make_shared<Table>(std::move(ctx), std::move(columns));
  }

  int64_t Rows() const { return rows_; }
  int32_t Columns() const { return static_cast<int32_t>(columns_.size()); }
  std::vector<std::string> ColumnNames() const;
  const std::vector<Column> &columns() const { return columns_; }
  const Column &column(int i) const;
  int ColumnIndex(const std::string &name) const;  // -1 if absent
  const std::shared_ptr<CylonContext> &GetContext() const { return ctx_; }
  at::Device device() const;

  void retainMemory(bool retain) { retain_ = retain; }
  bool IsRetain() const { return retain_; }
  void Clear() {
    columns_.clear();
    rows_ = 0;
  }
  // retain = false (reference table.cpp:150-154, :358-362): an operator that has consumed this
  // table's rows drops its buffers early, so the memory returns to the allocator while the operator
  // still runs.  The columns keep their name, type and nullability, with 0 rows (the table is
  // empty afterwards).  A no-op for retained tables.
  void ReleaseIfNotRetained();
  // retain = false: drop one buffer of column c (its data, or its validity) while an operator that
  // consumes the table column group by column group still runs; ReleaseIfNotRetained() finishes.
  void ReleaseBufferIfNotRetained(int c, bool validity);

  // total bytes of all buffers
  int64_t nbytes() const;
  TablePtr to(at::Device dev) const;

  // C27: the table's index (reference table.cpp:1001-1055 Set_Index / GetIndex / ResetIndex);
  // none = the implicit range index 0..rows-1
  void SetIndex(std::shared_ptr<indexing::BaseIndex> index) { index_ = std::move(index); }
  const std::shared_ptr<indexing::BaseIndex> &GetIndex() const { return index_; }
  void ResetIndex() { index_.reset(); }

 private:
  std::shared_ptr<CylonContext> ctx_;
  std::vector<Column> columns_;
  std::shared_ptr<indexing::BaseIndex> index_;
  int64_t rows_ = 0;
  bool retain_ = true;
};

// Sort options for DistributedSort (reference table.hpp:388-393).
struct SortOptions {
  // DistributedSort samples num_samples rows per rank (0 -> 256 x world) for its exact
  // splitters; MapToSortPartitions (the reference's bin histogram) uses both fields.
  uint32_t num_bins = 0;     // 0 -> 16 * world
  uint64_t num_samples = 0;  // 0 -> DistributedSort: 256 x world per rank; MapToSortPartitions: 1% of rows
  static SortOptions Defaults() { return SortOptions(); }
};

// Window functions (docs/semantics.md "Window functions"), numbered as the C ABI and the bindings
// pass them.  Functions 0 .. 8 have the frame ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW; the
// ROLLING functions have ROWS BETWEEN preceding PRECEDING AND following FOLLOWING, the RANGE functions
// RANGE BETWEEN preceding PRECEDING AND following FOLLOWING over the one order column.  The navigation
// functions 19 .. 21 have the whole partition as their frame (not SQL's default frame), FFILL / BFILL
// read back / ahead inside the partition, and the distribution functions 24 .. 26 need no column
// (docs/semantics.md "Navigation and distribution functions").  Functions 27 .. 30 are VAR / STD over a
// ROLLING resp. RANGE frame (docs/semantics.md "Framed aggregates", VAR / STD).
enum WindowFunc : int {
  WIN_ROW_NUMBER = 0,
  WIN_RANK = 1,
  WIN_DENSE_RANK = 2,
  WIN_CUMCOUNT = 3,
  WIN_CUMSUM = 4,
  WIN_CUMMIN = 5,
  WIN_CUMMAX = 6,
  WIN_LAG = 7,
  WIN_LEAD = 8,
  WIN_ROLLING_COUNT = 9,
  WIN_ROLLING_SUM = 10,
  WIN_ROLLING_MEAN = 11,
  WIN_ROLLING_MIN = 12,
  WIN_ROLLING_MAX = 13,
  WIN_RANGE_COUNT = 14,
  WIN_RANGE_SUM = 15,
  WIN_RANGE_MEAN = 16,
  WIN_RANGE_MIN = 17,
  WIN_RANGE_MAX = 18,
  WIN_FIRST_VALUE = 19,
  WIN_LAST_VALUE = 20,
  WIN_NTH_VALUE = 21,
  WIN_FFILL = 22,
  WIN_BFILL = 23,
  WIN_NTILE = 24,
  WIN_PERCENT_RANK = 25,
  WIN_CUME_DIST = 26,
  WIN_ROLLING_VAR = 27,
  WIN_ROLLING_STD = 28,
  WIN_RANGE_VAR = 29,
  WIN_RANGE_STD = 30,
};

constexpr int64_t kWindowUnbounded = INT64_MAX;  // a RANGE offset: no bound on that side

struct WindowSpec {
  WindowFunc func;
  int col;           // value column; ignored by the ranking and the distribution functions
  int64_t arg;       // LAG / LEAD: the offset (>= 0); NTH_VALUE, NTILE: k (>= 1)
  std::string name;  // output column; empty: <func>_<column name>, or the bare function without a column
  // ROLLING functions: rows of the partition before and after the current one (>= 0; >= the table's
  // rows: unbounded), and the non-null values below which the result is null (>= 1)
  int64_t preceding = 0;
  int64_t following = 0;
  int64_t min_periods = 1;
  // RANGE functions: preceding / following are distances in the order column's values (>= 0;
  // kWindowUnbounded: no bound on that side).  offset_is_float: a side that is not unbounded reads
  // its distance from preceding_f / following_f instead (float order columns only; >= 0, not NaN).
  double preceding_f = 0;
  double following_f = 0;
  bool offset_is_float = false;
  // FIRST_VALUE / LAST_VALUE: the first / last non-null cell of the partition instead of the cell of
  // its first / last row (Invalid on NTH_VALUE)
  bool ignore_nulls = false;
  // FFILL / BFILL: at most this many consecutive nulls after / before a value are filled (>= 0; 0: all)
  int64_t limit = 0;
  // ROLLING / RANGE VAR and STD: the divisor is (non-null values of the frame) - ddof (>= 0); the result is
  // null where that is not positive
  int ddof = 1;
};

// As-of join (docs/semantics.md "As-of join"): every left row with the nearest right row of its group
// at or before it (BACKWARD), at or after it (FORWARD), or the nearer of the two (NEAREST).
enum AsofDirection : int { ASOF_BACKWARD = 0, ASOF_FORWARD = 1, ASOF_NEAREST = 2 };

struct AsofOptions {
  int direction = ASOF_BACKWARD;  // an AsofDirection; any other number is Invalid
  bool allow_exact_matches = true;
  // a match farther away than the tolerance (>= 0) is dropped: tolerance_i in the column's unit for an
  // integer or temporal `on` (tolerance_is_float = false), tolerance_f for a float `on` (true)
  bool has_tolerance = false;
  bool tolerance_is_float = false;
  int64_t tolerance_i = 0;
  double tolerance_f = 0;
  std::string left_prefix, right_prefix;
};

// Interval join (docs/semantics.md "Interval join"): every pair of a left row and a right row of its
// group whose `on` value lies between the left row's `lower` and `upper`.
enum IntervalClosed : int { INTERVAL_BOTH = 0, INTERVAL_LEFT = 1, INTERVAL_RIGHT = 2, INTERVAL_NEITHER = 3 };
enum IntervalHow : int { INTERVAL_INNER = 0, INTERVAL_LEFT_OUTER = 1 };

struct IntervalOptions {
  int closed = INTERVAL_BOTH;  // an IntervalClosed: which ends of [lower, upper] belong to the interval
  int how = INTERVAL_INNER;    // an IntervalHow; any other number of either is Invalid
  std::string left_prefix, right_prefix;
};

namespace ops {

// ---- plumbing -------------------------------------------------------------
TablePtr Gather(const TablePtr &t, const at::Tensor &idx);  // idx int64, -1 -> null row
TablePtr GatherNullable(const TablePtr &t, const at::Tensor &idx, bool may_null);
Column GatherColumn(const Column &c, const at::Tensor &idx);
// K15 string / binary select: row i = cond[i] ? a[i] : b[i] (b of one row: broadcast; no b: null)
Column SelectVar(const Column &a, const std::optional<Column> &b, const at::Tensor &cond);
// K15 casts between strings and numbers on the column's device (kernels/strcast.hip): string ->
// integer / floating column, nullopt when a float needs the host's correctly rounded parser
// (the caller then casts on the host); integer -> string.  Unparsable strings raise Invalid.
std::optional<Column> CastStringToNumber(const Column &c, const DataType &target);
Column CastIntegerToString(const Column &c, const DataType &target);
// K15 string predicates on the column's device (kernels/strmatch.hip; docs/semantics.md "String
// predicates").  a is a STRING or BINARY column; the result has a's length and name, is null where
// an input cell is null and has a validity array iff an input column has one.
//   StringCompare: BOOL a[i] op b[i], op a strmatch::StrCmpOp (== != < <= > >=); b has a's kind and
//     a's length, or one row (broadcast).
//   StringMatch: BOOL, kind a strmatch::StrMatchKind (STARTS_WITH, ENDS_WITH, CONTAINS with a literal
//     byte pattern; LIKE with % _ and the escape character, a unit being a code point of a STRING
//     column and a byte of a BINARY one).  A pattern of more than kStrMaxPatternBytes bytes, or a
//     LIKE pattern that ends in a lone escape, is Invalid.
//   StringLength: INT64, unit a strmatch::StrLenUnit (bytes; code points, STRING only).
Column StringCompare(const Column &a, const Column &b, int op);
Column StringMatch(const Column &a, int kind, const std::string &pattern, char escape);
Column StringLength(const Column &a, int unit);
int64_t StringTileBytes();  // kernels' string_tile_bytes(): the staged path's largest 256-row span
// K15 string transforms on the column's device (kernels/strxform.hip; docs/semantics.md "String
// transforms").  a is a STRING or BINARY column; the result has a's type and name, is null exactly
// where an input cell is null (a null row has length 0) and has a validity array iff an input has one.
//   StringSlice: units[start:stop] of every cell as Python slices, step 1 (no stop: the end of the
//     cell; a negative index counts from the end); a unit is a code point of a STRING column and a
//     byte of a BINARY one.
//   StringStrip: side a strxform::StrStripSide; chars the set of bytes to remove (none: ASCII
//     whitespace).  A non-ASCII set on a STRING column is Invalid.
//   StringCase: ASCII upper / lower, and whether a live row held a byte >= 0x80.
//   StringConcat: a[i] + sep + b[i]; a and b have the same kind, and either may have one row
//     (broadcast; a null one makes every row null).
//   StringReplace: leftmost non-overlapping replacement of the literal pat (not empty), at most
//     max_replacements times per cell (< 0: all).
// A literal (sep, pat, repl) of more than kStrMaxPatternBytes bytes is Invalid.
Column StringSlice(const Column &a, int64_t start, const std::optional<int64_t> &stop);
Column StringStrip(const Column &a, int side, const std::optional<std::string> &chars);
std::pair<Column, bool> StringCase(const Column &a, bool upper);
Column StringConcat(const Column &a, const Column &b, const std::string &sep);
Column StringReplace(const Column &a, const std::string &pat, const std::string &repl, int64_t max_replacements);
TablePtr Project(const TablePtr &t, const std::vector<int> &cols);
TablePtr Merge(const std::vector<TablePtr> &tables);  // vertical concat
TablePtr Slice(const TablePtr &t, int64_t offset, int64_t length);
TablePtr FilterByMask(const TablePtr &t, const at::Tensor &mask);  // uint8/bool mask
at::Tensor MaskToIndices(const at::Tensor &mask, bool invert = false);

// ---- partitioning (K1/K2/K3) --------------------------------------------
// pid[i] in [0, nparts) and per-partition row counts (host vector).
std::pair<at::Tensor, std::vector<int64_t>> MapToHashPartitions(const TablePtr &t, const std::vector<int> &cols,
                                                                uint32_t nparts);
// Reorders rows partition-major (stable); returns reordered table + counts.
std::pair<TablePtr, std::vector<int64_t>> PartitionReorder(const TablePtr &t, const at::Tensor &pid,
                                                           uint32_t nparts);
std::vector<TablePtr> Split(const TablePtr &t, const at::Tensor &pid, uint32_t nparts);
// the shuffle's partitioning: reference hash partition ids -> partition-major table + counts
// (one LDS-staged pass for a single non-null 8-byte integer key on the device)
std::pair<TablePtr, std::vector<int64_t>> ShufflePartition(const TablePtr &t, const std::vector<int> &hash_cols,
                                                           uint32_t nparts);
std::vector<TablePtr> HashPartition(const TablePtr &t, const std::vector<int> &cols, uint32_t nparts);

// ---- communication --------------------------------------------------------
// partition-major table + per-partition counts -> received table
TablePtr AllToAllTable(const TablePtr &partitioned, const std::vector<int64_t> &counts);
// Posted (non-blocking) form of AllToAllTable: the size / schema agreement collectives
// run now, the column all-to-alls are left in flight (RCCL: on its stream).
// PostedExchangeReady tests the transfers without blocking; FinishPostedExchange waits
// (stream-ordered on RCCL) and assembles the received table.
struct PostedExchange;
std::shared_ptr<PostedExchange> PostAllToAllTable(const TablePtr &partitioned, const std::vector<int64_t> &counts);
bool PostedExchangeReady(PostedExchange &x);
TablePtr FinishPostedExchange(PostedExchange &x);
TablePtr Shuffle(const TablePtr &t, const std::vector<int> &hash_cols);
// shuffle two tables with the second one's partitioning overlapped with the first's transfer
std::pair<TablePtr, TablePtr> ShufflePair(const TablePtr &a, const std::vector<int> &acols, const TablePtr &b,
                                          const std::vector<int> &bcols);
// pipelined shuffle of two tables in `chunks` hash-disjoint chunks: consume(k, a_k, b_k) runs
// on chunk k while the transfers of the later chunks are still in flight (fixed-width columns)
// chunk count for ShufflePairChunked (same on every rank; 1 = unchunked)
int ShuffleChunks(const TablePtr &a, const TablePtr &b);
void ShufflePairChunked(const TablePtr &a, const std::vector<int> &acols, const TablePtr &b,
                        const std::vector<int> &bcols, int chunks,
                        const std::function<void(int, const TablePtr &, const TablePtr &)> &consume);
// The binary operators' shuffle (DistributedJoin, distributed set operations): decides the chunk
// count itself and agrees on everything the exchange needs -- chunk count, per-chunk row counts of
// both tables, column nullability, narrowed wire columns -- in ONE all-gather of a per-rank
// descriptor before the first payload all-to-all is posted.  consume(k, K, a_k, b_k) runs once per
// chunk (K == 1: the whole shuffled pair).  Var-width tables take ShufflePair (K = 1).
void ShufflePairPlanned(const TablePtr &a, const std::vector<int> &acols, const TablePtr &b,
                        const std::vector<int> &bcols,
                        const std::function<void(int, int, const TablePtr &, const TablePtr &)> &consume);
// Stable merge of consecutive sorted runs of `runs` (run_rows[r] rows each, in order) by column
// `col` (pairwise merge-path rounds, kernels/merge.hip): the receive side of the pipelined sort.
TablePtr MergeSortedRuns(const TablePtr &runs, const std::vector<int64_t> &run_rows, int col, bool asc);
// Pipelined range exchange (distributed sort) of a table whose rows are ordered by destination
// sub-range: bounds has W*K + 1 entries and rows [bounds[d*K + k], bounds[d*K + k + 1]) go to rank
// d in chunk k.  One all-gather of (rows, nullability, sub-range counts) plans every chunk, all
// chunks are posted at once (the communicator runs them in order) and consume(k, K, runs,
// run_rows) receives chunk k -- the rows from every rank in rank order, run_rows[r] from rank r --
// while the later chunks are still in flight.  Fixed-width columns only.
void RangeExchange(const TablePtr &t, const std::vector<int64_t> &bounds, int K,
                   const std::function<void(int, int, const TablePtr &, const std::vector<int64_t> &)> &consume);
// single-table form (distributed group-by / unique): consume(k, K, t_k) per hash-disjoint chunk
void ShufflePlanned(const TablePtr &t, const std::vector<int> &cols,
                    const std::function<void(int, int, const TablePtr &)> &consume);

// ---- relational -----------------------------------------------------------
TablePtr Join(const TablePtr &left, const TablePtr &right, const join::config::JoinConfig &cfg);
TablePtr DistributedJoin(const TablePtr &left, const TablePtr &right, const join::config::JoinConfig &cfg);
// index pairs of a local join (li, ri; -1 for the unmatched side)
std::pair<at::Tensor, at::Tensor> JoinIndices(const TablePtr &left, const TablePtr &right,
                                              const join::config::JoinConfig &cfg);
// C27/K16: index row positions matching each label, grouped by label order then row order
at::Tensor IndexLookup(const std::shared_ptr<CylonContext> &ctx, const Column &index, const Column &labels);
// A/B hook of the stable hash partitions (ops/radix.cpp): digit bits per pass, 3..10 (default 10)
void SetPartitionDigitBits(int bits);

// grouping = true: only equal values must end adjacent (list columns then sort by their bytes)
at::Tensor SortIndices(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending,
                       bool grouping = false);
TablePtr Sort(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending);
// ORDER BY cols LIMIT k (ops/topk.cpp): the rows, and the row order, of the first min(k, rows) rows
// of the stable index sort.  DistributedTopK: the global k rows on rank 0 (ties by rank, then row),
// an empty table with the same schema on every other rank.
TablePtr TopK(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending, int64_t k);
TablePtr DistributedTopK(const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &ascending,
                         int64_t k);
// Window functions (ops/window.cpp): t's columns unchanged, in t's row order, followed by one column
// per spec, computed over the stable sort by partition_cols (ascending) ++ order_cols (ascending).
// carry_step_tiles > 0 (tests only) lowers the tiles one step of the carry scan covers.
// DistributedWindow: shuffle by the partition columns (at least one), then Window on every rank.
TablePtr Window(const TablePtr &t, const std::vector<int> &partition_cols, const std::vector<int> &order_cols,
                const std::vector<bool> &ascending, const std::vector<WindowSpec> &specs,
                int64_t carry_step_tiles = 0);
TablePtr DistributedWindow(const TablePtr &t, const std::vector<int> &partition_cols,
                           const std::vector<int> &order_cols, const std::vector<bool> &ascending,
                           const std::vector<WindowSpec> &specs);
// As-of join (ops/asof.cpp): left's rows in left's row order, followed by right's columns gathered
// from the match of every left row (null where there is none); names get the prefixes as Join's do.
// Neither input needs to be sorted.  AsofJoinIndices: the right row of every left row, -1 for none.
// carry_step_tiles > 0 (tests only) lowers the tiles one step of the carry scan covers.
// DistributedAsofJoin: shuffle both sides by their `by` columns (at least one), then AsofJoin on every
// rank; the output row order is unspecified.
at::Tensor AsofJoinIndices(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                           const std::vector<int> &left_by, const std::vector<int> &right_by,
                           const AsofOptions &options, int64_t carry_step_tiles = 0);
TablePtr AsofJoin(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                  const std::vector<int> &left_by, const std::vector<int> &right_by, const AsofOptions &options,
                  int64_t carry_step_tiles = 0);
TablePtr DistributedAsofJoin(const TablePtr &left, const TablePtr &right, int left_on, int right_on,
                             const std::vector<int> &left_by, const std::vector<int> &right_by,
                             const AsofOptions &options);
// Interval join (ops/interval.cpp): all of left's columns, then all of right's (names get the prefixes
// as Join's do), one row per pair of a left row and a right row of the same `by` group with lower <=
// on <= upper (`closed` opens either end); rows ordered by left row, then right `on`, then right row.
// how = LEFT adds one row with null right columns, in its place, for a left row without a match.
// Neither input needs to be sorted.  IntervalJoinIndices: the (left row, right row) pairs in that
// order, right row -1 for a LEFT filler.  IntervalJoinCounts: the matches of every left row (sort and
// rank pass only; `how` does not change them).  carry_step_tiles > 0 (tests only) lowers the tiles one
// step of the rank pass's carry scan covers.  DistributedIntervalJoin: shuffle both sides by their
// `by` columns (at least one), then IntervalJoin on every rank; the output row order is unspecified.
std::pair<at::Tensor, at::Tensor> IntervalJoinIndices(const TablePtr &left, const TablePtr &right, int left_lower,
                                                      int left_upper, int right_on, const std::vector<int> &left_by,
                                                      const std::vector<int> &right_by,
                                                      const IntervalOptions &options, int64_t carry_step_tiles = 0);
at::Tensor IntervalJoinCounts(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper,
                              int right_on, const std::vector<int> &left_by, const std::vector<int> &right_by,
                              const IntervalOptions &options, int64_t carry_step_tiles = 0);
TablePtr IntervalJoin(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper, int right_on,
                      const std::vector<int> &left_by, const std::vector<int> &right_by,
                      const IntervalOptions &options, int64_t carry_step_tiles = 0);
TablePtr DistributedIntervalJoin(const TablePtr &left, const TablePtr &right, int left_lower, int left_upper,
                                 int right_on, const std::vector<int> &left_by, const std::vector<int> &right_by,
                                 const IntervalOptions &options);

}  // namespace ops
}  // namespace cylon
