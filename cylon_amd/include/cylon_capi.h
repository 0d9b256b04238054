/* C ABI of cylon_amd (P8 / J2 base layer).
 *
 * Reference: python/pycylon/api/lib.pyx (Cython C-API wrap/unwrap) and
 * cpp/src/cylon/table_api.hpp + java/src/main/native (JNI over the string-ID
 * table registry).  Every function is exported from the cylon_amd._C shared
 * object with C linkage, so C, C++, JNI or ctypes code can drive the engine
 * without Python: tables live in the process-wide registry under string IDs.
 * Return value: 0 = OK, otherwise a cylon Code (see cylon_amd.Code);
 * cylon_last_error() describes the last failure of the calling thread.
 */
#ifndef CYLON_AMD_CAPI_H_
#define CYLON_AMD_CAPI_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int cylon_capi_version(void);
const char *cylon_last_error(void);

/* context: "cpu" or "cuda:<i>" (local, rank 0 of 1) */
int cylon_init(const char *device);
/* distributed context from the torchrun environment (RANK, WORLD_SIZE, MASTER_ADDR,
   MASTER_PORT, LOCAL_RANK): comm_type "rccl" (one GPU per rank, cuda:<LOCAL_RANK>),
   "tcp" / "gloo" (host tables over the native TCP mesh) or "mpi" (rccl if GPUs are
   visible, else tcp).  Reference: CylonContext::InitDistributed(MPIConfig). */
int cylon_init_distributed(const char *comm_type);
int cylon_get_rank(void);
int cylon_get_world_size(void);
int cylon_barrier(void);
int cylon_finalize(void);

/* tables (string IDs) */
int cylon_read_csv(const char *path, const char *table_id);
int cylon_write_csv(const char *table_id, const char *path);
int64_t cylon_row_count(const char *table_id);
int32_t cylon_column_count(const char *table_id);
int cylon_remove_table(const char *table_id);
/* join_type: 0 inner, 1 left, 2 right, 3 full outer, 4 left semi, 5 left anti (the last two return
   the left table's columns only); algorithm: 0 sort, 1 hash */
int cylon_join(const char *left_id, const char *right_id, int join_type, int algorithm, int left_col,
               int right_col, const char *dest_id);
int cylon_distributed_join(const char *left_id, const char *right_id, int join_type, int algorithm, int left_col,
                           int right_col, const char *dest_id);
/* set ops: op 0 union, 1 subtract, 2 intersect */
int cylon_set_op(const char *a_id, const char *b_id, int op, int distributed, const char *dest_id);
int cylon_sort(const char *table_id, int column, int ascending, const char *dest_id);
/* ORDER BY column LIMIT k: the first min(k, rows) rows of the stable sort; k < 0 is an error */
int cylon_topk(const char *table_id, int column, int ascending, int64_t k, const char *dest_id);
/* window functions over PARTITION BY partition_columns ORDER BY order_columns (ascending[i] != 0:
   ascending; NULL: all ascending); the frame is UNBOUNDED PRECEDING .. CURRENT ROW.  Spec i:
   funcs[i] = 0 ROW_NUMBER, 1 RANK, 2 DENSE_RANK, 3 CUMCOUNT, 4 CUMSUM, 5 CUMMIN, 6 CUMMAX, 7 LAG,
   8 LEAD; spec_columns[i] its value column (ignored by 0..2), spec_args[i] the LAG / LEAD offset,
   names[i] the output column (NULL or "": the default name).  The result holds the table's columns
   in its row order, then one column per spec.  distributed != 0 needs a partition column. */
int cylon_window(const char *table_id, const int32_t *partition_columns, int npartition,
                 const int32_t *order_columns, const int32_t *ascending, int norder, const int32_t *funcs,
                 const int32_t *spec_columns, const int64_t *spec_args, const char *const *names, int nspecs,
                 int distributed, const char *dest_id);
/* cylon_window with a frame per spec: also funcs[i] = 9 ROLLING_COUNT, 10 ROLLING_SUM, 11 ROLLING_MEAN,
   12 ROLLING_MIN, 13 ROLLING_MAX over ROWS BETWEEN preceding[i] PRECEDING AND following[i] FOLLOWING of
   the partition (>= 0; INT64_MAX, or anything >= the row count: unbounded), null where the frame
   holds fewer than min_periods[i] (>= 1) non-null values.  preceding / following NULL: 0;
   min_periods NULL: 1.  Functions 0..8 ignore the three arrays. */
int cylon_window_frames(const char *table_id, const int32_t *partition_columns, int npartition,
                        const int32_t *order_columns, const int32_t *ascending, int norder, const int32_t *funcs,
                        const int32_t *spec_columns, const int64_t *spec_args, const int64_t *preceding,
                        const int64_t *following, const int64_t *min_periods, const char *const *names, int nspecs,
                        int distributed, const char *dest_id);
/* cylon_window_frames with RANGE frames too: also funcs[i] = 14 RANGE_COUNT, 15 RANGE_SUM, 16 RANGE_MEAN,
   17 RANGE_MIN, 18 RANGE_MAX over RANGE BETWEEN preceding[i] PRECEDING AND following[i] FOLLOWING: the rows
   of the partition whose value of the one order column (an integer, a temporal type, float32 or float64)
   lies within those distances of the row's own, peers included.  preceding / following are in the
   column's unit (>= 0), INT64_MAX: unbounded on that side.  offset_is_float[i] != 0 (float order
   columns only): a side that is not unbounded reads preceding_f[i] / following_f[i] (>= 0, not NaN)
   instead.  The three new arrays may be NULL (0, 0, false).  Functions 0..13 ignore them. */
int cylon_window_range_frames(const char *table_id, const int32_t *partition_columns, int npartition,
                              const int32_t *order_columns, const int32_t *ascending, int norder,
                              const int32_t *funcs, const int32_t *spec_columns, const int64_t *spec_args,
                              const int64_t *preceding, const int64_t *following, const double *preceding_f,
                              const double *following_f, const int32_t *offset_is_float, const int64_t *min_periods,
                              const char *const *names, int nspecs, int distributed, const char *dest_id);
/* cylon_window_range_frames with the navigation and distribution functions too: also funcs[i] =
   19 FIRST_VALUE, 20 LAST_VALUE, 21 NTH_VALUE (the cell of the partition's first / last / spec_args[i]-th
   row in window order; the frame is the whole partition, not SQL's default frame; NTH_VALUE is null in
   a shorter partition), 22 FFILL, 23 BFILL (a null cell takes the nearest non-null cell before / after
   it in its partition, at most limit[i] positions away; 0: no limit), 24 NTILE (spec_args[i] buckets,
   int64), 25 PERCENT_RANK, 26 CUME_DIST (float64); 24..26 ignore spec_columns.  ignore_nulls[i] != 0
   makes FIRST_VALUE / LAST_VALUE the partition's first / last non-null cell (Invalid on NTH_VALUE).  Null
   is the validity byte: NaN is a value.  ignore_nulls / limit may be NULL (false, 0). */
int cylon_window_nav(const char *table_id, const int32_t *partition_columns, int npartition,
                     const int32_t *order_columns, const int32_t *ascending, int norder, const int32_t *funcs,
                     const int32_t *spec_columns, const int64_t *spec_args, const int64_t *preceding,
                     const int64_t *following, const double *preceding_f, const double *following_f,
                     const int32_t *offset_is_float, const int64_t *min_periods, const int32_t *ignore_nulls,
                     const int64_t *limit, const char *const *names, int nspecs, int distributed,
                     const char *dest_id);
/* cylon_window_nav with the framed VAR / STD too: also funcs[i] = 27 ROLLING_VAR, 28 ROLLING_STD (the frame
   of ROLLING_MEAN), 29 RANGE_VAR, 30 RANGE_STD (the frame of RANGE_MEAN).  With m the non-null values of
   the frame, each converted to float64, the result (float64) is sum (x - mean)^2 / (m - ddof[i]) or its
   square root, null where m < min_periods[i] or m - ddof[i] <= 0, NaN where the frame holds a NaN or an
   infinity; never negative.  ddof[i] >= 0; ddof may be NULL (1). */
int cylon_window_moment_frames(const char *table_id, const int32_t *partition_columns, int npartition,
                               const int32_t *order_columns, const int32_t *ascending, int norder,
                               const int32_t *funcs, const int32_t *spec_columns, const int64_t *spec_args,
                               const int64_t *preceding, const int64_t *following, const double *preceding_f,
                               const double *following_f, const int32_t *offset_is_float,
                               const int64_t *min_periods, const int32_t *ignore_nulls, const int64_t *limit,
                               const int32_t *ddof, const char *const *names, int nspecs, int distributed,
                               const char *dest_id);
/* as-of join: every row of the left table, in its row order, with the columns of the nearest right row
   whose `by` columns equal its own (nby may be 0) -- direction 0 BACKWARD: the last right_on <=
   left_on, 1 FORWARD: the first right_on >= left_on, 2 NEAREST: the nearer of the two, the backward
   one on equal distances; allow_exact == 0 makes the comparisons strict.  has_tolerance != 0 drops
   matches farther away than tolerance_i (integer or temporal `on`, in the column's unit) or
   tolerance_f (float `on`); the other one is ignored.  Right columns are null where there is no match;
   names get the prefixes (NULL: none).  distributed != 0 needs a `by` column at world sizes > 1. */
int cylon_asof_join(const char *left_id, const char *right_id, int left_on, int right_on, const int32_t *left_by,
                    const int32_t *right_by, int nby, int direction, int allow_exact, int has_tolerance,
                    int64_t tolerance_i, double tolerance_f, const char *left_prefix, const char *right_prefix,
                    const char *dest_id, int distributed);
/* interval join: one row per pair of a left row and a right row whose `by` columns equal its own (nby
   may be 0) and whose `on` value lies in the left row's [lower, upper] -- closed 0 BOTH, 1 LEFT (lower
   <= on < upper), 2 RIGHT (lower < on <= upper), 3 NEITHER; rows ordered by left row, then right `on`,
   then right row.  how 0 INNER, 1 LEFT: a left row without a match gives one row with null right
   columns.  A null or NaN bound or `on` never matches; names get the prefixes (NULL: none).
   distributed != 0 needs a `by` column at world sizes > 1. */
int cylon_interval_join(const char *left_id, const char *right_id, int left_lower, int left_upper, int right_on,
                        const int32_t *left_by, const int32_t *right_by, int nby, int closed, int how,
                        const char *left_prefix, const char *right_prefix, const char *dest_id, int distributed);
int cylon_project(const char *table_id, const int32_t *columns, int ncolumns, const char *dest_id);

int cylon_merge(const char *const *table_ids, int ntables, const char *dest_id);
/* print rows [row_begin, row_end) (row_end < 0: all) to stdout, reference Table::Print */
int cylon_print(const char *table_id, int64_t row_begin, int64_t row_end);

/* build a table from host buffers (copied; J1 ArrowTable path).  types: cylon Type numbering
   (INT64 = 8, DOUBLE = 11, STRING = 12, ...); validity: Arrow-style bitmaps (LSB first) or NULL;
   offsets: int32 Arrow offsets for STRING/BINARY columns (NULL otherwise). */
int cylon_table_from_buffers(const char *table_id, int ncols, const char *const *names, const int32_t *types,
                             int64_t nrows, const void *const *data, const uint8_t *const *validity,
                             const int32_t *const *offsets);

/* row predicate selection (reference Table::Select): keep rows for which pred returns non-zero */
typedef struct cylon_row cylon_row;
typedef int (*cylon_row_predicate)(const cylon_row *row, void *user);
int cylon_select(const char *table_id, cylon_row_predicate pred, void *user, const char *dest_id);
int64_t cylon_row_index(const cylon_row *row);
int cylon_row_is_null(const cylon_row *row, int col);
int64_t cylon_row_get_int64(const cylon_row *row, int col);
double cylon_row_get_double(const cylon_row *row, int col);
/* copies up to cap-1 bytes + NUL; returns the full length */
int64_t cylon_row_get_string(const cylon_row *row, int col, char *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
