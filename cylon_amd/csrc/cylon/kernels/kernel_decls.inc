// Kernel primitive declarations, included into namespace cylon::hip and
// cylon::cpu (see kernels.hpp).  Every primitive takes the HIP stream as its
// last argument (ignored by the CPU twin).
/* K1/K2: h[i] = 31*h[i] + f(col[i]) over ncols columns (h initialised to 0). */
void row_partition_hash(const ColView *cols, int ncols, int64_t n, uint32_t *h, void *stream);
/* pid[i] = partitioner(h[i]); counts[p] += 1  (counts zeroed inside). */
void hash_to_partition(const uint32_t *h, int64_t n, uint32_t nparts, uint32_t *pid,
                       int64_t *counts, void *stream);
/* fused single int key: pid from modulo hash of a 1/2/4/8-byte int column */
/* K3: stable counting-sort destinations: pos[i] = offset of row i in partition-major order.*/
/* block_hist must hold partition_positions_workspace(n, nparts) int64 values.  */
int64_t partition_positions_workspace(int64_t n, uint32_t nparts);
void partition_positions(const uint32_t *pid, int64_t n, uint32_t nparts, int64_t *block_hist,
                         int64_t *pos, int64_t *counts, void *stream);
/* out[pos[i]] = in[i] for fixed width columns (validity scattered too). */
void scatter_columns(const ColView *in, const MutColView *out, int ncols, const int64_t *pos,
                     int64_t n, void *stream);
/* var width scatter: out_lens[pos[i]] = len(i) ; then after scan, bytes copy */
void scatter_var_lengths(const ColView &in, const int64_t *pos, int64_t n, int64_t *out_lens
                            , void *stream);
void scatter_var_bytes(const ColView &in, const int64_t *pos, int64_t n,
                       const int64_t *out_offsets, uint8_t *out_bytes, uint8_t *out_valid
                          , void *stream);
/* K4: out[j] = in[idx[j]] ; idx < 0 -> null. out validity written iff non-null ptr. */
void gather_columns(const ColView *in, const MutColView *out, int ncols, const int64_t *idx,
                    int64_t m, void *stream);
/* K15 var-width select (string where / fill_null): row i = a[i] where cond[i] != 0 (cond ==
   nullptr: always a), else b[b_bcast ? 0 : i]; b.offsets == nullptr selects a null row.  Output
   offsets = exclusive scan of the lengths; out_valid always written (may be nullptr) */
/* strcast.hip: string -> int64 / float64 parse (ok[i]: 1 parsed, 0 invalid, 2 float needing the
   host's correctly rounded parser; allow_neg false: an unsigned target, a leading '-' is invalid),
   int64 -> decimal string (lengths, then digits at offsets) */
void str_to_i64(const ColView &c, int64_t n, bool allow_neg, int64_t *out, uint8_t *ok, void *stream);
void str_to_f64(const ColView &c, int64_t n, double *out, uint8_t *ok, void *stream);
void i64_to_str_lengths(const int64_t *v, const uint8_t *valid, int64_t n, int64_t *lens, void *stream);
void i64_to_str_write(const int64_t *v, const uint8_t *valid, int64_t n, const int64_t *offs, uint8_t *bytes,
                      void *stream);
/* strmatch.hip: K15 string predicates (docs/semantics.md "String predicates"); out[i] = 0 on a null
   row, whose bytes are never read.  str_compare: a[i] op b[b_scalar ? 0 : i] (op: a StrCmpOp).
   str_match: kind a StrMatchKind; pat (device memory) holds plen <= kStrMaxPatternBytes pattern
   bytes, for STR_LIKE plen token kinds followed by plen token bytes; utf8 != 0: a match begins and
   ends at code-point boundaries (LIKE over a STRING column).  str_length: unit a StrLenUnit.
   string_tile_bytes: the largest byte span of 256 consecutive rows that takes the LDS-staged path */
int64_t string_tile_bytes();
void str_compare(const ColView &a, const ColView &b, int b_scalar, int op, int64_t n, uint8_t *out, void *stream);
void str_match(const ColView &a, int kind, const uint8_t *pat, int64_t plen, int utf8, int64_t n, uint8_t *out,
               void *stream);
void str_length(const ColView &a, int unit, int64_t n, int64_t *out, void *stream);
/* strxform.hip: K15 string transforms (docs/semantics.md "String transforms"): slice, strip, case,
   concat and replace as two passes around exclusive_scan.  x says which (strxform_common.hpp); lit
   (device memory) holds its literal bytes; b is read by SX_CONCAT only.  A row is live when a.valid
   and b.valid (each may be null; a broadcast operand's must be) say so; a row that is not live has
   length 0 and its bytes are never read.  strx_lengths: lens[i] = the output length of row i.
   strx_write: row i's bytes at out + out_off[i]; flag (SX_CASE, may be null): set to 1 when a live
   row holds a byte >= 0x80, else left alone.  strx_case_flat: upper / lower of a column without
   validity in one flat pass over its total = offsets[n] - offsets[0] bytes; out_off = the rebased
   offsets (n + 1), flag as above (not null). */
void strx_lengths(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                  int64_t *lens, void *stream);
void strx_write(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                const int64_t *out_off, uint8_t *out, uint32_t *flag, void *stream);
void strx_case_flat(const ColView &a, int upper, int64_t n, int64_t total, int64_t *out_off, uint8_t *out,
                    uint32_t *flag, void *stream);
void select_var_lengths(const ColView &a, const ColView &b, int b_bcast, const uint8_t *cond, int64_t n,
                        int64_t *out_lens, void *stream);
void select_var_bytes(const ColView &a, const ColView &b, int b_bcast, const uint8_t *cond, int64_t n,
                      const int64_t *out_offsets, uint8_t *out_bytes, uint8_t *out_valid, void *stream);
void gather_var_lengths(const ColView &in, const int64_t *idx, int64_t m, int64_t *out_lens
                           , void *stream);
void gather_var_bytes(const ColView &in, const int64_t *idx, int64_t m,
                      const int64_t *out_offsets, int64_t total_bytes, uint8_t *out_bytes, uint8_t *out_valid
                         , void *stream);
/* 64-bit row hash over key columns (null-aware) for generic keys. */
void row_hash64(const ColView *cols, int ncols, int64_t n, uint64_t *out, void *stream);
/* Raw 64-bit key of a single fixed-width (<= 8 byte) column, sign/zero-extended */
void key64_from_column(const ColView &col, int64_t n, int64_t *out, void *stream);
/* K5 exact composite key of nk <= kMaxCompositeKeys integer columns: out[i] = OR_k (key_k[i] - lo[k])
   << shift[k]; unpack writes key column k (its own width) = lo[k] + ((key >> shift[k]) & (2^bits[k] - 1)).
   ncode (nullptr: none): ncode[k] >= 0 is the field value of a null in key column k (pack: a row whose
   validity is 0; unpack: out[k].valid[i] = 0 where the field holds it) */
void composite_key_pack(const ColView *cols, int nk, const int64_t *lo, const int *shift, int64_t n, int64_t *out,
                        const int64_t *ncode, void *stream);
void composite_key_unpack(const int64_t *key, int64_t n, int nk, const int64_t *lo, const int *shift, const int *bits,
                          const MutColView *out, const int64_t *ncode, void *stream);
/* K8 float group key: float64 image bits, -0.0 -> +0.0, NaN -> one quiet NaN (float32 widened) */
void float_key_bits(const ColView &c, int64_t n, int64_t *out, void *stream);
/* K5: open-addressing multimap (linear probing, wrap at tsize). */
void hash_table_init(HashSlot *table, int64_t tsize, void *stream);
void hash_build(const int64_t *keys, int64_t n, HashTableRef t, void *stream);
/* atomic-free build: sorts (key,row) by slot into (ka,va)/(kb,va) ping-pong buffers, returns the
   buffer index holding the sorted pairs; the other buffer's key array receives the placement
   prefix-max; *maxpos (device) = last placement offset. Then hash_table_place. */
int64_t hash_build_sorted_workspace(int64_t n);
int hash_build_sorted(const int64_t *keys, int64_t n, int shift, int64_t *ws, uint64_t *ka, int64_t *va,
                      uint64_t *kb, int64_t *vb, int64_t *maxpos, void *stream);
void hash_table_place(const uint64_t *skeys, const int64_t *srows, const int64_t *pmax, int64_t n,
                      HashTableRef t, void *stream);
void hash_probe_count(const int64_t *keys, int64_t n, HashTableRef t, int64_t *counts, void *stream);
void hash_probe_write(const int64_t *keys, int64_t n, HashTableRef t, const int64_t *offsets,
                      int64_t *out_probe, int64_t *out_build, void *stream);
/* single pass, wave-aggregated output reservation; *counter = total matches (even on overflow) */
void hash_probe_emit(const int64_t *keys, int64_t n, HashTableRef t, int64_t capacity, int64_t *counter,
                     int64_t *out_probe, int64_t *out_build, void *stream);
/* inclusive max scan of int64 */
int64_t max_scan_workspace(int64_t n);
void inclusive_max_scan(const int64_t *in, int64_t n, int64_t *out, int64_t *ws, void *stream);
/* eq[j] = rows l[li[j]] and r[ri[j]] equal on all key columns (null == null) */
void rows_equal(const ColView *l, const ColView *r, int ncols, const int64_t *li,
                const int64_t *ri, int64_t m, uint8_t *eq, void *stream);
/* pid[i] = top `bits` bits of fmix64(key) (the join's locality partitioning, see hash.hpp slot_of) */
void radix_partition_ids(const int64_t *keys, int64_t n, int bits, uint32_t *pid, void *stream);
/* flags[idx[j]] = 1 for idx[j] >= 0 */
void mark_indices(const int64_t *idx, int64_t m, uint8_t *flags, void *stream);
/* exclusive scan of int64 counts; out has n+1 entries (out[n] = total) */
int64_t scan_workspace(int64_t n);
void exclusive_scan(const int64_t *in, int64_t n, int64_t *out, int64_t *ws, void *stream);
/* K11: out[k] = i for mask[i] != 0 (invert flips the mask); writes count to *count */
int64_t mask_to_indices_workspace(int64_t n);
void mask_to_indices(const uint8_t *mask, int64_t n, bool invert, int64_t *ws,
                     int64_t *out, int64_t *count, void *stream);
void iota(int64_t *out, int64_t n, int64_t start, void *stream);
/* K6: order-preserving unsigned images of a fixed-width column (optionally permuted) */
void sort_keys_from_column(const ColView &col, const int64_t *perm, int64_t n, bool desc, uint64_t *out,
                           void *stream);
/* K6: stable LSD radix sort of (key, value) pairs over bits [begin_bit, end_bit).
   Returns 0 if the result is in (keys, vals), 1 if in (keys_alt, vals_alt). */
int64_t radix_sort_workspace(int64_t n);
int radix_sort_pairs(uint64_t *keys, int64_t *vals, int64_t n, uint64_t *keys_alt, int64_t *vals_alt,
                     int begin_bit, int end_bit, int64_t *ws, void *stream);
/* K7: per sorted left key: lower bound + match count in sorted right keys */
void merge_join_count(const uint64_t *lk, int64_t nl, const uint64_t *rk, int64_t nr, int64_t *lo,
                      int64_t *counts, void *stream);
void merge_join_write(const int64_t *lperm, int64_t nl, const int64_t *rperm, const int64_t *lo,
                      const int64_t *offs, int64_t *out_l, int64_t *out_r, void *stream);
/* K8/K10: concurrent hash set over int64 keys. slot_keys[cap] init INT64_MIN, slot_first[cap+1] init
   INT64_MAX; writes slot_of_row[i] and min row per slot (the extra slot cap holds key == INT64_MIN). */
void group_insert(const int64_t *keys, int64_t n, int64_t *slot_keys, int64_t cap, int64_t *slot_of_row,
                  int64_t *slot_first, void *stream);
/* flags[v[j]] = 1 for 0 <= v[j] < INT64_MAX */
void mark_firsts(const int64_t *slot_first, int64_t m, uint8_t *flags, void *stream);
/* out[idx[g]] = g */
void scatter_iota(const int64_t *idx, int64_t m, int64_t *out, void *stream);
/* out[dst[i]] = table[src[i]]  (src == nullptr -> table[i]) */
void permute_assign(const int64_t *dst, const int64_t *src, const int64_t *table, int64_t n, int64_t *out,
                    void *stream);
/* out[i] = c[b[a[i]]] */
void gather_chain2(const int64_t *a, const int64_t *b, const int64_t *c, int64_t n, int64_t *out, void *stream);
/* heads[i] = rows perm[i], perm[i-1] differ on any column (null == null, NaN == NaN) */
void segment_heads(const ColView *cols, int ncols, const int64_t *perm, int64_t n, uint8_t *heads, void *stream);
/* K8/K12 accumulate: kind 0 SUM_F64, 1 SUM_I64, 2 MIN (u64 order image), 3 MAX (image), 4 COUNT, 5 M2 about mean.
   gid == nullptr <=> a single group. Accumulators must be pre-initialised. */
void agg_accumulate(const int64_t *gid, int64_t n, int64_t ngroups, const ColView &v, int kind, void *acc,
                    const double *mean, void *stream);
/* order images -> values of width w / kind */
void agg_unimage(const uint64_t *in, int64_t m, int width, int kind, uint8_t *out, void *stream);
/* type-2 quantile per group on (group, value)-sorted permutation */
void group_quantile(const ColView &v, const int64_t *perm, const int64_t *offs, int64_t ngroups, double q,
                    double *out, uint8_t *valid, void *stream);
/* K13 range partition: min/max (as double) of col over idx (or all rows); synchronises */
void range_minmax(const ColView &c, const int64_t *idx, int64_t m, double *out, void *stream);
void range_histogram(const ColView &c, const int64_t *idx, int64_t m, double vmin, double vmax, int64_t nbins,
                     int64_t *hist, void *stream);
/* counts must be zeroed by the caller */
void range_partition(const ColView &c, int64_t n, double vmin, double vmax, int64_t nbins, const uint32_t *b2p,
                     uint32_t nparts, bool desc, uint32_t *pid, int64_t *counts, void *stream);
/* K6 strings: chunk >= 0 -> big-endian 8-byte chunk of each string (zero padded), chunk == -1 -> length */
void sort_string_chunk_keys(const ColView &col, const int64_t *perm, int64_t n, int64_t chunk, bool desc,
                            uint64_t *out, void *stream);
/* K5 LDS radix join (GPU only; radix_join.hip).  One LSD pass moves every column
   (in[c] -> out[c], widths 1/2/4/8) by digit (part >> shift) & (2^digit_bits - 1) of
   part = top total_bits bits of fmix64(key); digit_bits <= 10.  stable = false ranks rows
   with LDS atomics (a bucket's rows of one tile land in no particular order: joins only). */
int64_t radix_rows_pass_workspace(int64_t n, int digit_bits);
/* GPU only: lane-order violations of same-address LDS atomics (precondition of the
   wave-atomic stable ranking; synchronous) */
int64_t lds_lane_order_violations(int blocks, int rounds, void *stream);
/* GPU only: the self-check's cached verdict (once per process; CYLON_RP_RANK=wave|ballot forces) */
bool lds_lane_order_ok(void *stream);
/* Load every kernel file's code object on the current device (context creation). */
void preload_device_code();
/* GPU only: did a stable radix pass since the last call see its ranking guard fire (a bucket run
   of a sorted tile whose input rows do not ascend)?  Reads and clears the device flag (host
   sync); on true the device's stable passes switch to ballot ranking for the rest of the process */
bool rp_take_order_violation(void *stream);
// the ranking guard's device flag (int), for callers that read it together with other device state
// in one copy; rp_note_order_violation clears it and switches the device to ballots, as the above
int *rp_order_flag();
void rp_note_order_violation(void *stream);
void rp_set_ranking(int mode);
/* Narrowed join partitions (radix_join.hip PartDigitN): column 0 travels as the uint32 offset
   key - base, base = base_src[0] - 2^31 (the left table's first key), and the partition is the top
   bits of fmix32(offset); *bad |= 1 when an int64 key lies outside [base, base + 2^32) (the caller
   repartitions without narrowing).  kin4: the pass's column 0 already holds offsets (width 4). */
struct NarrowKeys {
  const int64_t *base_src = nullptr;  // nullptr: not narrowed
  unsigned int *bad = nullptr;
  int kin4 = 0;
};
/* in[c] == nullptr (c > 0, width 8) is a row-id column the pass generates: value = input row index */
/* lb / nd_bits: look-back passes as in radix_sort_rows_pass (both passes of a two-pass partition
   stable; nd_bits = the next pass's digit bits when this pass counts for it) */
void radix_rows_pass(const int64_t *keys, int64_t n, int total_bits, int shift, int digit_bits,
                     const uint8_t *const *in, uint8_t *const *out, const int *widths, int ncols, int64_t *ws,
                     void *stream, bool stable = true, const SortLbArgs *lb = nullptr, int nd_bits = 0,
                     const NarrowKeys *nk = nullptr, bool tiles_prescanned = false, const uint16_t *nd_in = nullptr,
                     uint16_t *nd_out = nullptr);
/* the first pass's per-tile digit counts (uint16 [ceil(n / 8192)][2^digit_bits]) live at this int64
   offset of its workspace; a caller that wrote them there passes tiles_prescanned (XCD-tile passes) */
int64_t radix_rows_pass_th_offset(int64_t n, int digit_bits);
void radix_part_offsets(const int64_t *keys, int64_t n, int bits, int64_t *offs, void *stream);
void radix_part_offsets32(const uint32_t *keys, int64_t n, int bits, int64_t *offs, void *stream);
/* bounded-memory join chunks (GPU only): one exact pass of every column by the LOW cbits bits of
   fmix64(column 0 = int64 key) (ws: radix_rows_pass_workspace(n, cbits)); offs[c] (2^cbits + 1) =
   first row of chunk c in the output */
void radix_chunk_pass(const int64_t *keys, int64_t n, int cbits, const uint8_t *const *in, uint8_t *const *out,
                      const int *widths, int ncols, int64_t *ws, int64_t *offs, void *stream, bool stable = false);
/* bounded-memory join chunk: the slot second pass over nseg consecutive buckets of an exact narrowed
   first pass (bbase[g] = bucket g's first row in the chunk; ws: radix_slot_workspace(log2 nseg,
   second_bits)); digit d of bucket g -> slot g * 2^second_bits + d; counts[slot] rows per slot */
void radix_slot_segment_pass(const uint32_t *keys, int64_t n, int total_bits, int second_bits, const uint8_t *const *in,
                             uint8_t *const *out, const int *widths, int ncols, const uint32_t *bbase, int nseg,
                             int64_t slot, int64_t *ws, int64_t *counts, unsigned int *overflow, void *stream,
                             const NarrowKeys *nk);
/* Slot mode (histogram-free join partition passes, GPU only; MSD: the HIGH first_bits digit, then
   the low second_bits digit inside each first-pass bucket).  A slot pass claims fixed-size output
   slots (one atomic per tile and digit) instead of reading the keys for exact tile offsets; output
   columns hold nslots * slot + radix_slot_tile_rows() rows (the tail: trash rows of runs that did
   not fit: *overflow |= 1, the result is unusable and the caller partitions exactly); counts[g] =
   rows in slot g.
   radix_slot_first_pass: slot x * 2^first_bits + d = bucket d's rows of XCD x's eighth of the table
   (2^first_bits * 8 slots; needs radix_slot_first_pass_ok).
   radix_slot_rows_pass: slot b * 2^second_bits + d = partition id; input = the slots of
   radix_slot_first_pass (first_counts / first_slot), or (first_counts == nullptr) the exact buckets
   of a radix_rows_pass over the high digit (shift = second_bits) whose workspace is first_ws. */
bool radix_slot_eligible(int64_t n, int ncols, int first_bits, int second_bits);
bool radix_slot_first_pass_ok(int first_bits);
int64_t radix_slot_workspace(int first_bits, int second_bits);
int64_t radix_slot_tile_rows();
void radix_slot_first_pass(const int64_t *keys, int64_t n, int total_bits, int first_bits, int second_bits,
                           const uint8_t *const *in, uint8_t *const *out, const int *widths, int ncols, int64_t slot,
                           int64_t *ws, int64_t *counts, unsigned int *overflow, void *stream,
                           const NarrowKeys *nk = nullptr);
void radix_slot_rows_pass(const int64_t *keys, int64_t n, int total_bits, int first_bits, int second_bits,
                          const uint8_t *const *in, uint8_t *const *out, const int *widths, int ncols,
                          const int64_t *first_ws, const int64_t *first_counts, int64_t first_slot, int64_t slot,
                          int64_t *ws, int64_t *counts, unsigned int *overflow, void *stream,
                          const NarrowKeys *nk = nullptr);
/* Fixed-length strings (L bytes per row, row-major) <-> ceil(L / 8) <= 8 int64 word columns, and the
   rows whose word columns differ while both rows are present (GPU only; ops/join_keys.cpp) */
void var_len_minmax(const int64_t *offs, int64_t n, int64_t *mm, void *stream);  // mm[0..1] = min / max length
// hash: the row_hash64 of the string (one key column); inv: hash = the invertible word key
// (hash.hpp word_key_*) and word 0 is not written (words[0] unused)
void bytes_to_words(const uint8_t *bytes, int64_t n, int L, int64_t *const *words, void *stream,
                    uint64_t *hash = nullptr, bool inv = false);
// hash: word 0 from the invertible word key (words[0] unused)
void words_to_bytes(const int64_t *const *words, int64_t n, int L, uint8_t *bytes, void *stream,
                    const uint64_t *hash = nullptr);
void words_mismatch(const int64_t *const *a, const int64_t *const *b, int W, const uint8_t *va, const uint8_t *vb,
                    int64_t n, uint8_t *bad, int64_t *nbad, void *stream);  // *nbad (zeroed here) = rows set
/* Variable-length strings (every row <= 8 W bytes, W <= 8) <-> W zero-padded int64 word columns + a
   length column.  var_to_words: row i = bytes[offs[i], offs[i + 1]) (offs absolute into bytes);
   hash (required) = the invertible padded word key fmix64(w0 ^ g(L_i, w1..w_{W-1})) standing in for
   word 0 (words[0] unused); lens[i] = L_i; h2 (optional) = an independent 64-bit hash of the row.
   words_to_var: bytes at out_offs[i] (exclusive scan of lens), w0 rebuilt from the word key.
   text = true: the key is seeded with 0 (not the length) and no length is written (lens may be
   nullptr); *nul (optional) is set when some row holds a zero byte -- text mode is then invalid.
   padded_text_lens: text mode's row lengths from the words (the first zero byte). */
void var_to_words(const uint8_t *bytes, const int64_t *offs, int64_t n, int W, int64_t *const *words,
                  uint64_t *hash, int64_t *lens, uint64_t *h2, void *stream, bool text = false,
                  unsigned int *nul = nullptr);
void padded_text_lens(const int64_t *const *words, const uint64_t *hash, int64_t n, int W, int64_t *lens,
                      void *stream);
void words_to_var(const int64_t *const *words, const uint64_t *hash, const int64_t *lens, const int64_t *out_offs,
                  int64_t n, int W, uint8_t *bytes, void *stream, bool text = false);
// two independent 64-bit hashes of string / binary rows of any length (group-by key + its check)
// pack_row: h2 = (high 32 bits of the second hash) << 32 | row (n <= 2^32): one 8-byte column gives the
// group-by both its verification hash and a representative row (MIN)
void var_hash2(const uint8_t *bytes, const int64_t *offs, int64_t n, uint64_t *h1, uint64_t *h2, void *stream,
               bool pack_row = false);
/* join slot-mode decision (GPU only): hist[p] = sampled keys (every stride-th) of partition p, p the
   `bits`-bit join partition (narrowed digit when nk is set; nk->bad is left untouched) */
void radix_part_sample(const int64_t *keys, int64_t n, int bits, int64_t stride, uint32_t *hist,
                       const NarrowKeys *nk, void *stream);
/* MSD keys-only sort (GPU only; ops/sort.cpp): two passes over the top db1 + db2 bits of the hr-bit
   span of image - sub (image = key ^ key_xor; the first pass stores images; first_slot == 0: an exact
   first pass whose bucket bases stay in first_ws; the second pass fills slots), then
   seg_sort_local sorts every partition (<= seg_sort_capacity() rows: slot <= capacity) in LDS by
   its low local_bits bits and writes partition p at out_offs[p], XORed with out_xor. */
void radix_sort_msd_first_pass(const int64_t *keys, int64_t n, int hr, int db1, int db2, uint64_t key_xor,
                               uint64_t sub, int64_t *out, int64_t slot, int64_t *ws, int64_t *counts,
                               unsigned int *overflow, void *stream);
void radix_sort_msd_second_pass(const int64_t *images, int64_t n, int hr, int db1, int db2, uint64_t sub,
                                const int64_t *first_ws, const int64_t *first_counts, int64_t first_slot, int64_t *out,
                                int64_t slot, int64_t *ws, int64_t *counts, unsigned int *overflow, void *stream);
int64_t seg_sort_capacity();
void seg_sort_local(const int64_t *in, const int64_t *counts, int64_t slot, int64_t nparts, const int64_t *out_offs,
                    uint64_t sub, int local_bits, uint64_t out_xor, int64_t *out, void *stream);
/* K7 range join (GPU only): order-preserving partition id ((key ^ flip) - mn) >> rshift */
void radix_range_rows_pass(const int64_t *keys, int64_t n, uint64_t flip, uint64_t mn, int rshift, int shift,
                           int digit_bits, const uint8_t *const *in, uint8_t *const *out, const int *widths, int ncols,
                           int64_t *ws, void *stream);
void radix_range_part_offsets(const int64_t *keys, int64_t n, uint64_t flip, uint64_t mn, int rshift, int bits,
                              int64_t *offs, void *stream);
int64_t range_join_max_rows();
int range_join_max_shift();
void range_join_count(const int64_t *lkeys, const int64_t *loffs, const int64_t *rkeys, const int64_t *roffs,
                      int64_t nparts, uint64_t flip, uint64_t mn, int rshift, int64_t *counts, int *overflow,
                      void *stream);
void range_join_write(const int64_t *lkeys, const int64_t *loffs, const int64_t *rkeys, const int64_t *roffs,
                      int64_t nparts, uint64_t flip, uint64_t mn, int rshift, const int64_t *out_offs,
                      const uint8_t *const *lin, uint8_t *const *lout, const int *lw, int nlc,
                      const uint8_t *const *rin, uint8_t *const *rout, const int *rw, int nrc, void *stream);
/* max build rows per partition staged in LDS (in[q] == nullptr: the key column itself;
   match_flags: one more byte per row for a build-preserving outer join) */
int64_t radix_join_capacity(const int *widths, const uint8_t *const *in, int n, bool match_flags = false, int key_bytes = 8);
/* pstride > 1: count only partitions 0, pstride, ... into counts[p / pstride] (sampled estimate).
   outer: bit 0 = unmatched probe rows are output rows, bit 1 = unmatched build rows are */
/* Skewed partitions as work items (radix_join.hip "split partitions"): a partition whose build side
   exceeds the LDS capacity, or whose probe side is hot, is skipped (skip[p] = 1) and covered by items
   [nitems][kRJItemWords] = {probe first row, probe rows, build first row, build rows, flags}: build
   chunks of <= cap rows x probe chunks.  (The sampled partition count may get a wider skip mask: the
   host counts hot-ish partitions exactly instead of sampling them.)  flags: kRJItemPDefer / kRJItemBDefer = the side's unmatched
   rows are not emitted by the item but recorded in gprobe / gbuild (1 = matched, bytes indexed by
   partitioned row); kRJItemPEmit / kRJItemBEmit = emission items run afterwards: the side's rows whose
   flag is 0 are emitted unmatched. */
constexpr int kRJItemWords = 5;
constexpr int kRJItemPDefer = 1, kRJItemBDefer = 2, kRJItemPEmit = 4, kRJItemBEmit = 8;
struct RJSplit {
  const int64_t *items = nullptr;
  int64_t nitems = 0;
  const uint8_t *skip = nullptr;
  uint8_t *gprobe = nullptr;
  uint8_t *gbuild = nullptr;
};
/* counts[i] = output rows of partition i * pstride (or of item i when split->items: nparts ignored) */
void radix_join_count(const int64_t *pkeys, const int64_t *poffs, const int64_t *bkeys, const int64_t *boffs,
                      int64_t nparts, int64_t cap, int64_t *counts, int *overflow, void *stream, int64_t pstride = 1,
                      int outer = 0, int64_t pslot = 0, int64_t bslot = 0, const RJSplit *split = nullptr,
                      const int64_t *narrow_base = nullptr);
/* out_offs != nullptr: rows of partition p at out_offs[p]; else fused count: partitions claim
   rows from *cursor (int64, zeroed), claims past out_cap set *overflow |= 2, LDS overflow |= 1.
   pkey: index of the probe column that is the key itself (written from the probe key; -1 none).
   outer (see radix_join_count): bit 0 writes bpres[o] (1 = the build side holds a row), bit 1
   writes ppres[o]; unmatched build rows follow their partition's matches.
   Returns true when the exact-shape kernel ran (lds_join.hip k_rj_write_exact; never with exact_ok =
   false), false for the generic one */
bool radix_join_write(const int64_t *pkeys, const int64_t *poffs, const int64_t *bkeys, const int64_t *boffs,
                      int64_t nparts, int64_t cap, const int64_t *out_offs, const uint8_t *const *pin,
                      uint8_t *const *pout, const int *pw, int npc, const uint8_t *const *bin, uint8_t *const *bout,
                      const int *bw, int nbc, void *stream, int64_t *cursor = nullptr, int64_t out_cap = 0,
                      int *overflow = nullptr, int pkey = -1, int outer = 0, uint8_t *ppres = nullptr,
                      uint8_t *bpres = nullptr, int64_t pslot = 0, int64_t bslot = 0, const RJSplit *split = nullptr,
                      const int64_t *narrow_base = nullptr, bool exact_ok = true);
/* K8 LDS radix group-by (GPU only; radix_groupby.hip) */
int64_t distinct_estimate_workspace();  /* uint32 registers */
double distinct_estimate(const int64_t *keys, int64_t n, uint32_t *regs, void *stream);
int64_t radix_groupby_slots(int nacc);
/* per partition p of keys[offs[p]..offs[p+1]): groups -> slab at offs[p]; gcount[p] groups;
   oacc holds nacc planes of n uint64 states */
int radix_groupby_planes(int nacc);  // accumulator planes radix_groupby_agg writes (oacc: planes * n words)
void radix_groupby_agg(const int64_t *keys, const int64_t *offs, int64_t nparts, const RGAccDesc *acc, int nacc,
                       int64_t *okeys, uint64_t *oacc, int64_t n, int64_t *gcount, int *overflow, void *stream);
/* QUANTILE per group on the radix path: per partition p of (keys, vals[, valid])[offs[p]..offs[p+1])
   (<= radix_quantile_capacity() rows, else *overflow): groups -> slab at offs[p] (okeys, oq = the
   double's bits, ovalid = 0 / 1), gcount[p] groups; the global path's type-2 rule, nulls excluded */
int64_t radix_quantile_capacity();
/* fused (optional, 4 planes of n words): per group the valid values' sum (double bits), count, min and
   max (double bits; 0 when the count is 0) -- SUM / COUNT / MEAN / MIN / MAX of a float64 value column
   from the same sorted rows */
void radix_groupby_quantile(const int64_t *keys, const uint8_t *vals, int vwidth, int vkind, const uint8_t *valid,
                            const int64_t *offs, int64_t nparts, int bits, double q, int64_t *okeys, uint64_t *oq,
                            uint64_t *ovalid, int64_t *gcount, int *overflow, void *stream, uint64_t *fused = nullptr,
                            int64_t n = 0);
void radix_groupby_pack(const int64_t *offs, const int64_t *goff, int64_t nparts, const int64_t *okeys,
                        const uint64_t *oacc, int64_t n, int nacc, int64_t *keys_out, uint64_t *acc_out,
                        int64_t ngroups, void *stream);
/* K6 row-moving LSD sort pass (GPU only; radix_join.hip): digit = bits [shift, shift+digit_bits)
   of the uint64 image (column 0 XOR digit_flip: a first pass can read raw 8-byte integer keys);
   every column moves; column 0 is stored XORed with key_xor */
/* nd_in: this pass's digits, written by the previous pass (its tile histogram reads them instead
   of the keys); nd_out: write the NEXT pass's digits ((stored key >> nd_shift) & (2^nd_bits - 1))
   as column 0 is stored -- order images on every pass but the last).  sub: digits are taken of
   image - sub (the smallest image: keys that span fewer bits than vary need fewer digit bits) */
void radix_sort_rows_pass(const int64_t *keys, int64_t n, int shift, int digit_bits, const uint8_t *const *in,
                          uint8_t *const *out, const int *widths, int ncols, int64_t *ws, void *stream,
                          uint64_t key_xor, uint64_t digit_flip = 0, bool tiles_prescanned = false,
                          const uint16_t *nd_in = nullptr, uint16_t *nd_out = nullptr, int nd_shift = 0,
                          int nd_bits = 0, uint64_t sub = 0, const SortLbArgs *lb = nullptr);
/* Look-back sort passes (radix_join.hip "look-back sort passes"): every pass but the first takes
   its tile offsets from a decoupled look-back inside 8 chunks instead of a tile histogram; every
   pass but the last counts (chunk, next digit) for the next.  Eligible: XT, lean, 8-byte columns,
   digits of 3..9 bits, n < 2^31 - 2.  ws: radix_sort_lb_workspace(n) int64 words, one per sort;
   radix_sort_lb_args(ws, n, pass, npass) before each pass; radix_sort_lb_failed after the last
   (a look-back wait timed out: the result is unusable). */
bool radix_sort_lb_eligible(int64_t n, int ncols, const int *widths, const int *dbits, int npass, void *stream);
int64_t radix_sort_lb_workspace(int64_t n);
SortLbArgs radix_sort_lb_args(int64_t *ws, int64_t n, int pass, int npass, void *stream);
bool radix_sort_lb_failed(const int64_t *ws, void *stream);
/* Sort prologue (GPU only, XCD-tile passes): ONE read of int64 keys gives their varying bits
   (OR ^ AND, returned; host sync), the images' min / max (image = key ^ flip) and the per-tile
   histogram of the image's low 10 bits in pre_ws (radix_sort_prehist_workspace words).  When the
   first pass's digit is bits [0, db) of image - sub with db <= 10, radix_sort_prehist_fold writes
   its tile histogram into that pass's workspace and the pass runs with tiles_prescanned = true. */
int64_t radix_sort_prehist_workspace(int64_t n);
uint64_t radix_sort_prehist(const int64_t *keys, int64_t n, uint64_t flip, int64_t *pre_ws, void *stream,
                            uint64_t *img_min = nullptr, uint64_t *img_max = nullptr);
void radix_sort_prehist_fold(const int64_t *pre_ws, int64_t n, int db, int64_t *ws, void *stream, uint64_t sub = 0);
/* OR ^ AND over keys: bits that differ between keys (ws2: 2 int64) */
uint64_t varying_bits(const uint64_t *keys, int64_t n, int64_t *ws2, void *stream);
// order images of a column (no permutation) fused with varying_bits over them
uint64_t sort_keys_varying_bits(const ColView &col, int64_t n, bool desc, uint64_t *out, int64_t *ws2, void *stream);
/* K10 LDS radix set operations (GPU only; radix_setops.hip): L ++ R row hashes (nl left rows) with the first stable partition pass's per-tile digit counts
   (uint16 [ceil(n / 8192)][2^digit_bits], digit = low digit_bits of the top `bits` bits of fmix64(h);
   th == nullptr: hashes only) */
void setop_row_hash_tiles(const ColView *lcols, const ColView *rcols, int ncols, int64_t nl, int64_t n, uint64_t *h,
                          int bits, int digit_bits, uint16_t *th, void *colsets, void *stream);
int64_t setop_colsets_bytes();  // device bytes of setop_row_hash_tiles' colsets (both column sets)
int64_t setop_rows_per_part();
/* op 0 distinct (union / unique), 1 subtract, 2 intersect over radix-partitioned (hash, row id) pairs;
   writes keep-mask exceptions (see radix_setops.hip), *exc = their count, *bad = 1 on overflow/collision */
void setop_dedup(const uint64_t *ph, const int64_t *prow, const int64_t *offs, int64_t nparts, int64_t nl, int op,
                 bool keep_last, const ColView *lcols, const ColView *rcols, int ncols, uint8_t *mask, int64_t *exc,
                 int *bad, void *stream);
/* Left semi / anti join mark (semi_join.hip; CPU twin cpu_semi.cpp).  rkeys: right int64 key images,
   partition p = [roffs[p], roffs[p + 1]); lkeys / lrow: left (key, row id) pairs partitioned the same
   way by loffs (lrow == nullptr: row id = position, nparts == 1).  mask: one byte per left row,
   initialised by the caller to 0 (semi) or 1 (anti); only MATCHING rows are written (1 / 0).
   *matched = matching left rows; *overflow = 1 when a partition's distinct right keys exceed
   semi_join_capacity() (mask undefined; the CPU twin never overflows).
   GPU only: work items (ipart[i], islice[i]) = slice islice[i] (semi_join_slice_rows() rows) of left
   partition ipart[i] (both nullptr with nparts == 1: item i = slice i); dkeys / dmeta = workspace of
   as many int64 as rkeys and of nparts int64. */
int64_t semi_join_capacity();
int64_t semi_join_slice_rows();
void semi_join_mark(const int64_t *rkeys, const int64_t *roffs, const int64_t *lkeys, const int64_t *lrow,
                    const int64_t *loffs, int64_t nparts, int anti, uint8_t *mask, int64_t *matched, int *overflow,
                    const int64_t *ipart, const int64_t *islice, int64_t nitems, int64_t *dkeys, int64_t *dmeta,
                    void *stream);
/* Top-k radix select over a fixed-width column's sort image (topk.hip; CPU twin cpu_topk.cpp; the
   image is order_image.hpp sort_key_image; null rows take no part).  ws: topk_workspace() int64 words,
   the first topk_state_words() of them the state (topk.hip TKState) that the operator reads back.
   topk_scan: clears ws; OR / AND of the images and the non-null count.
   topk_start: select k_rem = k rows from bits [.., ihi) of the image, then [.., rhi) of the row number.
   topk_hist: histogram of the next db (<= topk_digit_bits()) undecided bits of the image (src 0) or
   the row number (src 1) over the rows whose decided bits equal the prefix; topk_pick: the bin where
   the running count crosses k_rem -> prefix, k_rem, sure, bucket; zeroes the histogram.
   topk_collect: (image, row) of the rows below the prefix -> sure list, equal to it -> candidate
   list, in any order; a list that outgrows its capacity sets the state's error word, nothing is
   written past it. */
int topk_digit_bits();
int64_t topk_state_words();
int64_t topk_workspace();
void topk_scan(const ColView &col, int64_t n, bool desc, int64_t *ws, void *stream);
void topk_start(int64_t *ws, int64_t k, int ihi, int rhi, void *stream);
void topk_hist(const ColView &col, int64_t n, bool desc, int64_t *ws, int src, int db, void *stream);
void topk_pick(int64_t *ws, int src, int db, void *stream);
void topk_collect(const ColView &col, int64_t n, bool desc, int64_t *ws, uint64_t *sure_img, int64_t *sure_row,
                  int64_t sure_cap, uint64_t *cand_img, int64_t *cand_row, int64_t cand_cap, void *stream);
/* shuffle wire format: int64 values shipped as uint32 offsets from a global base (range < 2^32) */
void narrow_i64(const int64_t *in, int64_t n, int64_t base, uint32_t *out, void *stream);
void widen_u32(const uint32_t *in, int64_t n, int64_t base, int64_t *out, void *stream);
/* K1 + K3 fast shuffle partition (GPU only; radix_join.hip) of a table whose partition key is one
   non-null 8-byte integer column: counts, then one LDS-staged pass moving every column
   (pid = (uint32)key % P, the reference's modulo partition; P <= 1024) */
// minmax (optional, int64[2]): the keys' min / max from the same read
void mod_partition_counts(const int64_t *keys, int64_t n, uint32_t nparts, int64_t *counts, void *stream,
                          int64_t *minmax = nullptr);
int64_t radix_mod_rows_pass_workspace(int64_t n, uint32_t nparts);
void radix_mod_rows_pass(const int64_t *keys, int64_t n, uint32_t nparts, const uint8_t *const *in, uint8_t *const *out,
                         const int *widths, int ncols, int64_t *ws, void *stream);
bool radix_mod_rows_pass_gapped(const int64_t *keys, int64_t n, uint32_t nparts, const uint8_t *const *in,
                                uint8_t *const *out, const int *widths, int ncols, int64_t *ws, void *stream,
                                const uint32_t *extra, int64_t out_rows);

// delay.hip: one wave spinning for `us` microseconds on `stream` (async test transport)
void spin_delay_us(double us, void *stream);

/* merge.hip: stable merge of two sorted (uint64 key, int64 payload) runs into ok / oi
   (na + nb pairs; ties take A first) */
void merge_sorted_pairs(const uint64_t *ak, const int64_t *ai, int64_t na, const uint64_t *bk, const int64_t *bi,
                        int64_t nb, uint64_t *ok, int64_t *oi, void *stream);
/* range.hip (sample sort): partition of every row by exact composite splitters.
   A row's composite key is (null_0, image_0, null_1, image_1, ..., gid) over `nkeys`
   sort columns (images: order-preserving uint64, direction applied; nulls: byte 1 =
   null, sorts after every value; gid = gid0 + row, the global row number that makes
   every key distinct).  splitters: (nparts - 1) x (2 * nkeys + 1) uint64 words in the
   same layout, sorted; pid = number of splitters < the row's key; counts[nparts]
   is incremented (caller zeroes it). */
void splitter_partition(const uint64_t *const *images, const uint8_t *const *nulls, int nkeys, int64_t n,
                        int64_t gid0, const uint64_t *splitters, uint32_t nparts, uint32_t *pid, int64_t *counts,
                        void *stream);

/* index.hip (K16 persistent indexes).  `sorted` = order images of the index column
   sorted ascending (stable: equal images keep row order), `sorted_pos` the rows.
   index_bounds: per probe image, lo = first sorted slot >= probe, cnt = slots == probe.
   hash_index_build: one open-addressing entry per distinct image (run start, run length);
   used[cap] must be zero on entry, cap a power of two >= 2 x distinct images.
   hash_index_probe: the entry of each probe image (cnt = 0 when absent).
   index_gather_positions: out[offs[i] + j] = sorted_pos[lo[i] + j] for j < cnt[i]. */
void index_bounds(const uint64_t *sorted, int64_t n, const uint64_t *probe, int64_t m, int64_t *lo, int64_t *cnt,
                  void *stream);
void hash_index_build(const uint64_t *sorted, int64_t n, uint64_t *tkeys, int32_t *used, int64_t *tlo, int64_t *tcnt,
                      int64_t cap, void *stream);
void hash_index_probe(const uint64_t *tkeys, const int32_t *used, const int64_t *tlo, const int64_t *tcnt, int64_t cap,
                      const uint64_t *probe, int64_t m, int64_t *lo, int64_t *cnt, void *stream);
void index_gather_positions(const int64_t *sorted_pos, const int64_t *lo, const int64_t *cnt, const int64_t *offs,
                            int64_t m, int64_t *out, void *stream);
/* byte-keyed hash index (string / binary / fixed-size-binary columns): the sorted images are
   64-bit hashes of the values, so a run can hold colliding values; keep[offs[i] + j] = 1 when
   the bytes of col row sorted_pos[lo[i] + j] equal the bytes of labels row i (verify on probe). */
void index_verify_bytes(const ColView &col, const ColView &labels, const int64_t *sorted_pos, const int64_t *lo,
                        const int64_t *cnt, const int64_t *offs, int64_t m, uint8_t *keep, void *stream);

/* bitmap.hip: Arrow validity bitmaps <-> byte masks at the Arrow boundary.
   pack: one wave64 per 64 rows, __ballot(byte != 0) is exactly one LSB-first bitmap
   word; returns nothing, null count via `nulls` (device int64, accumulated).
   unpack: bit (bit_offset + i) of `bits` -> byte i. */
void pack_validity(const uint8_t *bytes, int64_t n, uint64_t *bitmap, int64_t *nulls, void *stream);
void unpack_validity(const uint8_t *bits, int64_t bit_offset, int64_t n, uint8_t *bytes, void *stream);

/* copy.hip: n independent device-to-device copies in one launch (concatenation,
   sink growth): src[i] -> dst[i], bytes[i]; 16-byte vectors when aligned. */
void batched_copy(const void *const *src, void *const *dst, const int64_t *bytes, int n, void *stream);

/* bitmap.hip: k (<= 8 per word) byte columns <-> 8-byte words (byte j of word w = column
   8w + j), so that validity bytes travel through the all-8-byte radix passes as full
   8-byte rows instead of scattered 1-byte runs. */
void pack_byte_columns(const uint8_t *const *cols, int k, int64_t n, uint64_t *const *words, void *stream);
void unpack_byte_columns(const uint64_t *const *words, int k, int64_t n, uint8_t *const *cols, void *stream);

/* window.hip (CPU twin cpu_window.cpp): window functions over the sorted positions of a permutation
   (docs/semantics.md "Window functions").  flags[i]: bit 0 = position i starts a partition, bit 1 =
   it starts a run of peers (window_flags merges two segment_heads outputs; peer == nullptr: the
   partition heads; in place is fine).
   A value scan is three launches over tiles of window_tile_rows() positions:
     window_tile    gather = true: reads col at perm[i] (raw bits of widths 1/2/4/8, else 0, and the
                    validity byte) and stores both densely in sorted order (dense_valid == nullptr:
                    the column has no nulls); gather = false: reads the dense arrays of an earlier
                    call.  Writes one (flag, aggregate) pair per tile.
     window_carry   one block; the exclusive segmented scan of the tile pairs = each tile's carry-in,
                    `step` (<= window_carry_tiles(), <= 0: that) tiles per loop step.  words = int64
                    words per tile aggregate: 1 for a value scan, 3 for the rank scan (func 5).
     window_apply   re-scans each tile from the dense values and its carry-in; out[perm[i]] = the
                    running value (8 bytes for func 0, 1, 4; the column's width for 2, 3),
                    out_valid[perm[i]] = the value's validity byte when out_valid != nullptr.
   func: 0 sum of integers (mod 2^64), 1 sum of floats in float64, 2 min, 3 max (both on order_image,
   written back through order_unimage), 4 count of non-null values.  Null values are skipped.
   The rank scan needs no column: window_rank_tile / window_carry(words 3, func 5) / window_rank_apply
   write, where the pointer is not null, ROW_NUMBER, RANK and DENSE_RANK at out[perm[i]] and
   phead[i] = the sorted position of the head of position i's partition.
   window_shift: src[perm[i]] = perm[i + delta] when 0 <= i + delta < n lies in i's partition, else -1.
   The CPU twin is the definition: its window_tile only gathers, its window_carry does nothing, and
   its apply functions are one sequential loop over all positions. */
int64_t window_tile_rows();
int64_t window_carry_tiles();
void window_flags(const uint8_t *part, const uint8_t *peer, int64_t n, uint8_t *flags, void *stream);
void window_tile(const ColView &col, const int64_t *perm, const uint8_t *flags, int64_t n, int func, uint64_t *dense,
                 uint8_t *dense_valid, bool gather, int64_t *tile_agg, uint8_t *tile_flag, void *stream);
void window_carry(const int64_t *tile_agg, const uint8_t *tile_flag, int64_t ntiles, int words, int func,
                  int64_t step, int64_t *carry, void *stream);
void window_apply(const ColView &col, const int64_t *perm, const uint8_t *flags, int64_t n, int func,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry, uint8_t *out,
                  uint8_t *out_valid, void *stream);
void window_rank_tile(const uint8_t *flags, int64_t n, int64_t *tile_agg, uint8_t *tile_flag, void *stream);
void window_rank_apply(const int64_t *perm, const uint8_t *flags, int64_t n, const int64_t *carry,
                       int64_t *row_number, int64_t *rank, int64_t *dense_rank, int64_t *phead, void *stream);
void window_shift(const int64_t *perm, const int64_t *phead, int64_t n, int64_t delta, int64_t *src, void *stream);

/* rolling.hip (CPU twin cpu_rolling.cpp): aggregates over the frame [max(i - preceding, head),
   min(i + following, tail)] of sorted position i (docs/semantics.md "Framed aggregates"), from the dense
   values of window_tile, the flags, phead, and rtail = the phead of the rank scan run over
   window_rev_flags' output (rflags[k] = 3 where sorted position n - 1 - k ends a partition, else 0;
   the tail of position i is n - 1 - rtail[n - 1 - i]).  func as window_apply's (0 .. 4); mean: func
   0 / 1 divided by the frame's non-null count m, as float64.  out[perm[i]] = the result (8 bytes, or
   the column's width for func 2, 3), out_valid[perm[i]] = (m >= min_periods) when not nullptr.
   n < 2^32, 0 <= preceding, following <= n.
     rolling_lds      preceding + following + 1 <= window_frame_lds_rows(): one launch.
     rolling_tile / window_carry (twice: the aggregates with func, the counts with func 4, one tile
     flag array) / rolling_scan: the scan that restarts at partition edges and at the edges of the
                      blocks of w = preceding + following + 1 positions, forwards (restarts = flags) or,
                      reverse = true, over the reversed order (restarts = rflags); scan[k], scan_cnt[k]
                      are in scan order.
     rolling_combine  the results from the forward and the reversed scan.
   The CPU twin is sequential: its rolling_tile does nothing. */
int64_t window_frame_lds_rows();
void window_rev_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *stream);
void rolling_lds(const ColView &col, const int64_t *perm, const uint8_t *flags, const int64_t *phead,
                 const int64_t *rtail, int64_t n, int func, bool mean, int64_t preceding, int64_t following,
                 int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, uint8_t *out,
                 uint8_t *out_valid, void *stream);
void rolling_tile(const ColView &col, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
                  const uint64_t *dense, const uint8_t *dense_valid, int64_t *tile_agg, int64_t *tile_cnt,
                  uint8_t *tile_flag, void *stream);
void rolling_scan(const ColView &col, const uint8_t *restarts, int64_t n, int func, int64_t w, bool reverse,
                  const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry, const int64_t *carry_cnt,
                  uint64_t *scan, uint32_t *scan_cnt, void *stream);
void rolling_combine(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail, int64_t n,
                     int func, bool mean, int64_t preceding, int64_t following, int64_t min_periods,
                     const uint64_t *fwd, const uint32_t *fwd_cnt, const uint64_t *bwd, const uint32_t *bwd_cnt,
                     uint8_t *out, uint8_t *out_valid, void *stream);

/* frame_range.hip (CPU twin cpu_frame_range.cpp): aggregates over the RANGE frame of sorted position
   i, the positions j of i's partition whose order key lies within `preceding` below and `following`
   above i's (docs/semantics.md "Framed aggregates", RANGE).  Shared rules: frame_range_common.hpp.
     frame_range_keys     from the order column's dense values (window_tile's gather) the search key of
                          every sorted position: keys[i] = a 64-bit image that never decreases along a
                          partition's numbers (flipped for a descending column), cls[i] = 0 number,
                          1 NaN, 2 null (keys 0).
     frame_range_bounds   lo[i] / hi[i] = the first / last sorted position of i's frame, by binary
                          search over (cls, keys) inside [phead, tail] (rtail as rolling_lds takes it).
                          A side's mode: 0 unbounded (the partition's head / tail), 1 an integer
                          distance (integer keys), 2 a float64 distance (float keys).
     frame_range_pyramid  the radix-window_range_radix() two-sided scan pyramid of one (column, func):
                          per level P (scan from the 8-block's start to the entry) and S (from the entry
                          to the block's end), and E = one total per block = the next level's entries.
                          P, S: fr_ps_slots(n) words, E: fr_e_slots(n) words (frame_range_common.hpp).
     frame_range_apply    out[perm[i]] = the aggregate of [lo[i], hi[i]] read off the pyramid, at most two
                          words per level; the non-null count m = hi - lo + 1, or, for a column with
                          nulls, read off the count pyramid (func 4) cP / cS / cE.  func, mean,
                          min_periods, out and out_valid as rolling_combine's.  func 4 needs no
                          pyramid of a column without nulls.
   n < 2^32. */
int64_t window_range_radix();
int64_t window_range_halo();
void frame_range_keys(const ColView &order_col, const uint64_t *dense, const uint8_t *dense_valid, int64_t n,
                      bool descending, uint64_t *keys, uint8_t *cls, void *stream);
void frame_range_bounds(const uint64_t *keys, const uint8_t *cls, const int64_t *phead, const int64_t *rtail,
                        int64_t n, bool float_keys, bool descending, int pre_mode, uint64_t pre_i, double pre_f,
                        int fol_mode, uint64_t fol_i, double fol_f, uint32_t *lo, uint32_t *hi, void *stream);
void frame_range_pyramid(const ColView &col, int64_t n, int func, const uint64_t *dense, const uint8_t *dense_valid,
                         uint64_t *P, uint64_t *S, uint64_t *E, void *stream);
void frame_range_apply(const ColView &col, const int64_t *perm, int64_t n, int func, bool mean, int64_t min_periods,
                       const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo, const uint32_t *hi,
                       const uint64_t *P, const uint64_t *S, const uint64_t *E, const uint64_t *cP,
                       const uint64_t *cS, const uint64_t *cE, uint8_t *out, uint8_t *out_valid, void *stream);

/* frame_moments.hip (CPU twin cpu_frame_moments.cpp): VAR / STD over the ROWS or RANGE frame of sorted
   position i (docs/semantics.md "Framed aggregates", VAR / STD).  Shared rules:
   frame_moments_common.hpp.
     frame_moments_pyramid  the moment pyramid of one value column: frame_range_pyramid's geometry with
                            the state (count, mean, M2) of the non-null values, each converted to
                            float64, merged by fm_merge.  P, S: fm_words(fm_ps_slots(n)) 64-bit words
                            each, E: fm_words(fm_e_slots(n)), three planes per buffer.  Nothing to do
                            for n <= 8.
     frame_moments_apply    out[perm[i]] (float64) = M2 / (m - ddof) of the frame's state read off the
                            pyramid, or its square root (std_dev); out_valid[perm[i]] = m >= min_periods
                            and m - ddof > 0.  The frame: lo / hi of frame_range_bounds when they are
                            not nullptr (a RANGE spec), else max(i - preceding, phead[i]) ..
                            min(i + following, tail(i)) (a ROWS spec; rtail as rolling_lds takes it;
                            preceding, following >= 0 of any size).  ddof >= 0, min_periods >= 1.
   n < 2^32. */
void frame_moments_pyramid(const ColView &col, int64_t n, const uint64_t *dense, const uint8_t *dense_valid,
                           uint64_t *P, uint64_t *S, uint64_t *E, void *stream);
void frame_moments_apply(const ColView &col, const int64_t *perm, int64_t n, bool std_dev, int64_t ddof,
                         int64_t min_periods, const uint64_t *dense, const uint8_t *dense_valid, const uint32_t *lo,
                         const uint32_t *hi, const int64_t *phead, const int64_t *rtail, int64_t preceding,
                         int64_t following, const uint64_t *P, const uint64_t *S, const uint64_t *E, uint8_t *out,
                         uint8_t *out_valid, void *stream);

/* window_nav.hip (CPU twin cpu_window_nav.cpp): FIRST / LAST / NTH_VALUE, FFILL / BFILL, NTILE,
   PERCENT_RANK and CUME_DIST (docs/semantics.md "Navigation and distribution functions") from what the
   window operator already has: perm, the flags, the dense values and validity bytes of window_tile,
   phead, and rtail (the tail of position i is n - 1 - rtail[n - 1 - i]).
   The fill scan is the segmented running maximum of "scan position + 1 where the dense validity byte
   is set, else 0".  reverse = false: scan position k is sorted position k and restarts = the flags
   (bit 0); reverse = true: it is sorted position n - 1 - k and restarts = window_rev_flags' (or
   window_rev_peer_flags') output.  Three launches over tiles of window_tile_rows() positions:
     window_fill_tile   one (flag, aggregate) pair per tile.  dense_valid must not be nullptr: a column
                        without nulls needs no scan.
     window_carry       (words 1, func 3): each tile's carry-in.
     window_fill_apply  re-scans each tile.  The source of sorted position i is the nearest non-null
                        position j at or before it (reverse: at or after it) in its partition; there is
                        none when no such j exists or, for limit > 0, when it is more than limit
                        positions away.  Every output that is not nullptr is written (out and src
                        exclude each other):
                          out / out_valid (value mode, col's width 1, 2, 4 or 8): out[perm[i]] = dense[j],
                            out_valid[perm[i]] = 1; without a source out_valid[perm[i]] = 0 and the
                            value bytes are dense[i];
                          src (source mode): src[perm[i]] = perm[j], or -1;
                          pos: pos[i] = j, or -1, in sorted order.
   window_nav_pick: one sorted position j per row, form 0 FIRST_VALUE: phead[i]; 1 LAST_VALUE: tail[i];
   2 NTH_VALUE: phead[i] + k - 1 when <= tail[i], else none; 3 FIRST_VALUE ignoring nulls:
   fillpos[phead[i]] with fillpos = the pos of a reversed fill; 4 LAST_VALUE ignoring nulls:
   fillpos[tail[i]] with the pos of a forward one.  Value mode (out, out_valid): out[perm[i]] = dense[j],
   out_valid[perm[i]] = dense_valid[j] (1 when nullptr), 0 without a j; source mode (src):
   src[perm[i]] = perm[j] or -1.  phead may be nullptr for form 1, rtail for forms 0 and 3.
   window_rev_peer_flags: as window_rev_flags, and bit 1 is set where sorted position n - 1 - k ends a
   run of peers (bit 0 where it ends a partition; a partition's end ends a run of peers too).
   window_rank_heads: the apply of the rank scan (window_rank_tile / window_carry(words 3, func 5) over
   `flags`) that stores, in scan order, phead[k] = the last position with bit 0 at or before k and
   qhead[k] = the last one with bit 1 (either may be nullptr).  Over the flags qhead is the head of
   position k's peers (RANK = qhead - phead + 1); over window_rev_peer_flags' output the last peer of
   sorted position i is n - 1 - qhead[n - 1 - i].
   window_dist_apply: func 0 NTILE(k) (int64), 1 PERCENT_RANK, 2 CUME_DIST (float64), out[perm[i]].  With
   s = tail - phead + 1 and r = i - phead: NTILE as docs/semantics.md spells it out; PERCENT_RANK =
   (qhead[i] - phead[i]) / (s - 1), 0 when s == 1; CUME_DIST = (last peer - phead[i] + 1) / s; each one
   float64 division of two exactly converted integers.  qhead: func 1, rqhead: func 2, else nullptr.
   The CPU twin is the definition: its window_fill_tile does nothing, every other function is one
   sequential loop. */
void window_fill_tile(const uint8_t *restarts, int64_t n, bool reverse, const uint8_t *dense_valid,
                      int64_t *tile_agg, uint8_t *tile_flag, void *stream);
void window_fill_apply(const ColView &col, const int64_t *perm, const uint8_t *restarts, int64_t n, bool reverse,
                       int64_t limit, const uint64_t *dense, const uint8_t *dense_valid, const int64_t *carry,
                       uint8_t *out, uint8_t *out_valid, int64_t *src, int64_t *pos, void *stream);
void window_nav_pick(const ColView &col, const int64_t *perm, const int64_t *phead, const int64_t *rtail,
                     const int64_t *fillpos, int64_t n, int form, int64_t k, const uint64_t *dense,
                     const uint8_t *dense_valid, uint8_t *out, uint8_t *out_valid, int64_t *src, void *stream);
void window_rev_peer_flags(const uint8_t *flags, int64_t n, uint8_t *rflags, void *stream);
void window_rank_heads(const uint8_t *flags, int64_t n, const int64_t *carry, int64_t *phead, int64_t *qhead,
                       void *stream);
void window_dist_apply(const int64_t *perm, const int64_t *phead, const int64_t *rtail, const int64_t *qhead,
                       const int64_t *rqhead, int64_t n, int func, int64_t k, uint8_t *out, void *stream);

/* asof.hip (CPU twin cpu_asof.cpp): the as-of join's scan over the merged order of both sides' key
   rows (docs/semantics.md "As-of join").  perm = the stable sort of the n concatenated key rows, the
   first nfirst of them from one side; sorted position i holds a right row where
   (perm[i] < nfirst) == right_first.  reverse = false: scan position k is sorted position k and
   restarts = the partition heads (bit 0); reverse = true: it is sorted position n - 1 - k and
   restarts = window_rev_flags' output.  The scan is the segmented running maximum of "scan position
   + 1 for a right row whose `on` is neither null nor NaN, else 0", in three launches over tiles of
   window_tile_rows() positions:
     asof_tile     reads `on` (the concatenated column) at perm, writes code[k] (asof_common.hpp) in
                   scan order and one (flag, aggregate) pair per tile.
     window_carry  (words 1, func 3): each tile's carry-in.
     asof_apply    re-scans each tile; every left position writes match[left row] = the right row at
                   the carried scan position, -1 for none or for a null / NaN `on`.
   asof_pick: match[i] = asof_pick_one of the backward candidate back[i] and the forward one fwd[i]
   (fwd == nullptr: none; back may be match) -- the nearer one, the backward one on equal distances,
   -1 when farther than the tolerance (tolerance_i for an integer or temporal `on`, tolerance_f for a
   float one).  matched != nullptr: asof_apply / asof_pick add the left rows they gave a match to it.
   The CPU twin is the definition: its asof_tile only writes the codes, its asof_apply is one
   sequential loop over the positions. */
void asof_tile(const ColView &on, const int64_t *perm, const uint8_t *restarts, int64_t n, int64_t nfirst,
               bool right_first, bool reverse, uint8_t *code, int64_t *tile_agg, uint8_t *tile_flag, void *stream);
void asof_apply(const int64_t *perm, const uint8_t *restarts, const uint8_t *code, int64_t n, int64_t nfirst,
                bool right_first, bool reverse, const int64_t *carry, int64_t *match, int64_t *matched, void *stream);
void asof_pick(const ColView &left_on, const ColView &right_on, int64_t nl, const int64_t *back, const int64_t *fwd,
               bool has_tolerance, int64_t tolerance_i, double tolerance_f, int64_t *match, int64_t *matched,
               void *stream);

/* interval.hip (CPU twin cpu_interval.cpp): the interval join's rank pass, counts and expansion
   (docs/semantics.md "Interval join").  perm = the stable sort of the n = nr + 2 nl concatenated key
   rows (by .., value): the right rows (value = on) at [rbase, rbase + nr), the left rows' L-copies
   (value = lower) at [lbase, lbase + nl) and their U-copies (value = upper) at [ubase, ubase + nl);
   the three ranges tile [0, n).
     interval_rank    with c(p) = the right rows strictly before sorted position p: an L-copy stores
                      lo[left row] = c, a U-copy hi[left row] = c, a right row rrows[c] = its row
                      number (the right side in sorted order).  On the device: a tile count over
                      tiles of window_tile_rows() positions, window_carry (words 1, func 4, `step`
                      tiles per loop step, <= 0: window_carry_tiles()) and the scattering re-scan; ws =
                      interval_rank_workspace(n) int64 words.  perm must be 16-byte aligned.
     interval_counts  cnt[l] = hi[l] - lo[l] where lower[l] and upper[l] are neither null nor NaN and
                      hi > lo, else 0; *matched += their sum.  left: empty[l] = (cnt == 0) and cnt[l]
                      becomes max(cnt, 1) (the filler row of a LEFT join); else empty may be nullptr.
     interval_expand  off = the exclusive scan of cnt (nl + 1 entries, off[nl] = total).  Output row o
                      of left row l (off[l] <= o < off[l + 1]) gets li[o] = l and
                      ri[o] = rrows[lo[l] + (o - off[l])], or -1 where empty[l] (nullptr: no fillers).
                      One block per tile of interval_tile_rows() output rows.
   The CPU twin is the definition: three sequential loops; it ignores ws and step. */
int64_t interval_tile_rows();
int64_t interval_rank_workspace(int64_t n);
void interval_rank(const int64_t *perm, int64_t nl, int64_t nr, int64_t lbase, int64_t rbase, int64_t ubase,
                   int64_t step, int64_t *ws, int64_t *lo, int64_t *hi, int64_t *rrows, void *stream);
void interval_counts(const ColView &lower, const ColView &upper, const int64_t *lo, const int64_t *hi, int64_t nl,
                     bool left, int64_t *cnt, uint8_t *empty, int64_t *matched, void *stream);
void interval_expand(const int64_t *off, const int64_t *lo, const uint8_t *empty, const int64_t *rrows, int64_t nl,
                     int64_t nr, int64_t total, int64_t *li, int64_t *ri, void *stream);
