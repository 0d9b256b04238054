// What the join's files share (join.cpp, join_radix.cpp, join_bounded.cpp, join_keys.cpp,
// join_semi.cpp): the structs that cross them and the functions one file calls in another.
// Everything else in those files is static.
#pragma once
#include "relational.hpp"
#include "util.hpp"

namespace cylon {
namespace ops {

using join::config::JoinAlgorithm;
using join::config::JoinConfig;
using join::config::JoinType;

// ---- join.cpp
struct KeyEncoding {
  at::Tensor keys;  // int64 per row
  bool exact;       // keys equal <=> rows equal
};
bool simple_key(const Column &c);
KeyEncoding encode_keys(const Exec &ex, const TablePtr &t, const std::vector<int> &cols, bool exact_ok);
void check_join_keys(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg);
std::pair<at::Tensor, at::Tensor> hash_join_pairs(const Exec &ex, const at::Tensor &lk, const at::Tensor &rk);
std::pair<at::Tensor, at::Tensor> join_impl(TablePtr left, TablePtr right, const JoinConfig &cfg, bool allow_reorder,
                                            TablePtr *lout, TablePtr *rout);
inline bool left_may_null(JoinType jt) { return jt == JoinType::RIGHT || jt == JoinType::FULL_OUTER; }
inline bool right_may_null(JoinType jt) { return jt == JoinType::LEFT || jt == JoinType::FULL_OUTER; }

// ---- join_radix.cpp
struct RadixSide {
  at::Tensor keys, offs;  // offs: partition offsets [2^bits + 1], or (slot > 0) rows per partition
  int64_t slot = 0;       // slot mode: partition p's rows start at p * slot (RadixPartitionSlotted)
  at::Tensor overflow;    // slot mode: int32 device flag, set when a partition outgrew its slot
  std::vector<at::Tensor> data, valid;  // per table column (valid undefined if not nullable or packed)
  std::vector<bool> is_key;             // data[c] is the (partitioned) key array itself
  // validity bytes kept packed 8 per 8-byte word (radix.cpp): vpos[c] = byte position of
  // column c's validity in the words (-1: not packed); the write kernel moves the words
  std::vector<int> vpos;
  std::vector<at::Tensor> vwords;
};

// Partition every column of t (+ validity bytes) by the top `bits` bits of fmix64(key).
// slot > 0: try the slot-mode (histogram-free MSD) partition first
RadixSide radix_partition(const Exec &ex, const TablePtr &t, const at::Tensor &keys, int bits,
                          const RangeSpec *range = nullptr, int64_t slot = 0, const hip::NarrowKeys *nk = nullptr);

// Column pointer lists of one side for the write kernel (nullptr input = key column).
struct RadixCols {
  std::vector<const uint8_t *> in;
  std::vector<uint8_t *> out;
  std::vector<int> w;
};
RadixCols radix_cols(const TablePtr &t, const RadixSide *s, const std::vector<Column> *outs, int64_t out_off = 0,
                     const std::vector<at::Tensor> *word_outs = nullptr);
// output validity of the packed columns from the written words (at row offset out_off)
void unpack_validity_words(const Exec &ex, const TablePtr &t, const RadixSide &s, const std::vector<at::Tensor> &words,
                           std::vector<Column> &outs, int64_t out_off, int64_t m);

// A bounded-memory join chunk partitioned outside radix_join (radix_join_first_pass_chunks): both
// sides' partitions (narrowed keys), the chunk's partition bits and the narrowing base's source.
struct PrePartition {
  RadixSide L, R;
  int bits = 0;
  at::Tensor base_src;
  // set by radix_join (nothing written) when a side's slot pass overflowed: the flags ride with
  // radix_join's first host read instead of a read of their own
  mutable bool overflowed = false, overflow_l = false, overflow_r = false;
};

// Output accumulator of a chunked (pipelined) distributed join.  The radix join
// writes every chunk's rows straight into one set of output columns at the
// running row offset (capacity sized from the first chunk's output for all
// chunks, grown geometrically if a later chunk needs more), so the chunked join
// costs no concatenation pass; chunks that take another join path hand over
// whole tables, concatenated once at the end.
struct JoinSink {
  std::vector<Column> cols;  // left columns ++ right columns, `cap` rows each
  int64_t size = 0, cap = 0;
  int chunks_total = 1, chunks_done = 0;
  // the radix join's sampled skew check before its slot passes (off for the bounded-memory chunks:
  // a skewed chunk still completes -- an overflowing slot repartitions that side exactly)
  bool sample_skew = true;
  const PrePartition *pre = nullptr;  // this chunk arrives partitioned (radix_join skips its passes)
  std::vector<TablePtr> tables;

  // room for m more rows; returns the row offset to write at
  int64_t reserve(const Exec &ex, int64_t m, const std::vector<Column> &proto) {
    if (size + m > cap) {
      const int64_t left_chunks = std::max(1, chunks_total - chunks_done);
      const int64_t want = std::max(size + m + (m * (left_chunks - 1)) * 103 / 100 + 4096, 2 * cap);
      std::vector<Column> fresh;
      for (size_t c = 0; c < proto.size(); ++c) {
        Column n = make_fixed_column(proto[c].name, proto[c].type, want, ex.device, proto[c].nullable());
        if (size > 0) {
          n.data.slice(0, 0, size).copy_(cols[c].data.slice(0, 0, size));
          if (n.nullable()) n.validity.slice(0, 0, size).copy_(cols[c].validity.slice(0, 0, size));
        }
        fresh.push_back(std::move(n));
      }
      cols = std::move(fresh);
      cap = want;
    }
    const int64_t off = size;
    size += m;
    return off;
  }

  TablePtr finish(const std::shared_ptr<CylonContext> &ctx) {
    std::vector<TablePtr> parts;
    if (!cols.empty()) {
      std::vector<Column> out;
      for (const auto &c : cols) out.push_back(c.slice(0, size));
      parts.push_back(Table::Make(ctx, std::move(out)));
    }
    for (auto &t : tables) parts.push_back(t);
    if (parts.size() == 1) return parts[0];
    return Merge(parts);
  }
};

int64_t radix_join_min_rows();
bool radix_eligible(const TablePtr &t);
// Outer-join mode of the LDS join kernels (kernel_decls.inc radix_join_count): bit 0 = probe rows
// without a match are output rows, bit 1 = build rows without a match are.
int outer_mode(JoinType jt, bool build_left);
// the columns of t whose data buffer is the key tensor's (the key column itself; more than one when
// a table holds the same buffer twice).  Callers add their own condition.
std::vector<int> key_columns(const TablePtr &t, const at::Tensor &k);
// the partition bits with the RJ_EXTRA_BITS test knob (finer partitions) applied
int radix_extra_bits(int bits);

// Every size of one radix join, decided in one place (join_radix.cpp plan_radix_join).
struct RadixJoinPlan {
  int64_t nl = 0, nr = 0;  // rows of the left / right side
  bool build_left = false;
  int oj = 0;                 // outer_mode
  RadixCols shape;            // the build side's staged LDS row (key column: in == nullptr)
  bool narrow = false;        // the partitions carry uint32 key offsets (kernel_decls.inc NarrowKeys)
  int64_t cap4 = 0, cap8 = 0;  // LDS build rows per partition with 4-byte (narrowed) / 8-byte keys
  int bits = 0;
  int64_t nparts = 1;
  // Slot mode for two-pass partitions (>= 11 bits): the second pass claims fixed-size partition
  // slots (sizing::slot_rows) instead of reading the keys once more for exact offsets
  // (k_rp_hist_tiles + scans + k_part_offsets, ~2 ms per 1B-row side).  A partition beyond its
  // slot (skewed keys) sends that side through the exact passes.  0: exact passes (< 11 bits).
  int64_t slot_l = 0, slot_r = 0;
  // Skewed partitions are handled per partition, not per join: a partition whose build side exceeds
  // split_rows (<= the LDS capacity; test knob CYLON_RJ_SPLIT_ROWS) or whose probe side is hot (> 2
  // probe chunks) is skipped by the partition loop and covered by split work items (kernel_decls.inc
  // RJSplit): build chunks of <= cap rows x probe chunks of pch rows, so a hot key costs its own
  // rows, never the whole join (reference: one unordered_multimap, join/hash_join.cpp:255-298).
  int64_t pch = 0, split_rows = 0;
  int64_t bmean = 0;  // mean build rows per partition

  int64_t cap() const { return narrow ? cap4 : cap8; }
  // the same partitions joined on 8-byte keys: the smaller LDS capacity (fuller partitions become
  // split items)
  RadixJoinPlan without_narrowing() const;
  void set_bits(int b);  // bits and every size that follows from them
};
// build_is_key[c]: column c of the build side is the key array itself; pre_bits >= 0: the bits of
// partitions made elsewhere (PrePartition)
RadixJoinPlan plan_radix_join(const TablePtr &left, const TablePtr &right, const std::vector<bool> &build_is_key,
                              bool narrow, JoinType jt, int pre_bits = -1);

TablePtr radix_join(const Exec &ex, const TablePtr &left, const TablePtr &right, at::Tensor lk, at::Tensor rk,
                    const JoinConfig &cfg, JoinSink *sink = nullptr, bool hashed_key = false);

// ---- join_bounded.cpp
int radix_join_chunks(const Exec &ex, const TablePtr &l, const TablePtr &r, const at::Tensor &lk, const at::Tensor &rk,
                      JoinType jt);
// the radix join in C key-hash chunks into one sink; nullptr if a chunk's radix join fails
TablePtr radix_join_chunked(const Exec &ex, const TablePtr &l, const TablePtr &r, const at::Tensor &lk,
                            const at::Tensor &rk, const JoinConfig &cfg, int C, bool hashed_key = false);

// ---- join_keys.cpp
// Keys of the LDS radix join (K5).  One simple key column: the column itself.  Several non-null
// integer key columns: one EXACT composite -- each column's offset from its two-relation minimum,
// packed into 63 bits when the spans fit -- or else a 64-bit row hash whose matches are verified
// on the output (reference multi-key join: hash_join.cpp:92-186, TwoTableRowIndexHash).
struct RadixKeys {
  at::Tensor l, r;
  bool ok = false, verify = false;
  bool composite = false;  // l / r are exact composites: key column i = lo[i] + ((key >> shift[i]) & 2^bits[i]-1)
  std::vector<int64_t> lo;
  std::vector<int> shift, bits;
  std::vector<int64_t> ncode;  // composite: field value of a null in key i (-1: no nulls on either side)
  bool nulls = false;
  // one fixed-length string key per side: l / r are its invertible word keys (hash.hpp word_key_*,
  // carried by the proxies as a column in place of word 0) and lwords / rwords its words 1..W-1,
  // all from one read of the bytes
  std::vector<at::Tensor> lwords, rwords;
  int64_t wlen = -1;
  // one variable-length string key per side, every row <= 64 bytes: W = vw zero-padded words, l / r
  // the padded word keys (word 0's stand-in), lwords / rwords words 1..W-1, llen / rlen the lengths
  int vw = 0;
  at::Tensor llen, rlen;
  bool vtext = false;  // text mode (no zero bytes on either side): no length columns (partition.hip)
};
RadixKeys radix_keys(const Exec &ex, const TablePtr &left, const TablePtr &right, const JoinConfig &cfg, bool words_ok);
bool int_key(const Column &c);
bool nullable_int_key(const Column &c);
TablePtr radix_join_any(const Exec &ex, const TablePtr &left, const TablePtr &right, const JoinConfig &cfg,
                        JoinSink *sink);

// ---- join_semi.cpp
inline bool is_semi(JoinType jt) { return jt == JoinType::LEFT_SEMI || jt == JoinType::LEFT_ANTI; }
std::pair<at::Tensor, at::Tensor> semi_join_indices(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg);
TablePtr semi_join_local(const TablePtr &left, const TablePtr &right, const JoinConfig &cfg);

}  // namespace ops
}  // namespace cylon
