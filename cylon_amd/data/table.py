"""pycylon-compatible Table (reference: python/pycylon/data/table.pyx:75-2531).

A Table is a handle on a native, device-resident table (cylon_amd._C.Table):
columns live in HBM on the context's MI355X (or in host memory for CPU
contexts) and every relational operator runs in the native engine.
"""
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import pyarrow as pa
import torch

from .._lib import C
from ..ctx.context import CylonContext
from . import arrow_bridge as ab
from .table_pandas import PandasOpsMixin

_JOIN_TYPES = {"inner": "inner", "left": "left", "right": "right", "outer": "outer", "full_outer": "outer",
               "fullouter": "outer", "semi": "semi", "left_semi": "semi", "leftsemi": "semi", "anti": "anti",
               "left_anti": "anti", "leftanti": "anti"}


def _ensure_ctx(ctx: Optional[CylonContext]) -> CylonContext:
    if ctx is None:
        return default_context()
    return ctx


_DEFAULT_CTX = None


def default_context() -> CylonContext:
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = CylonContext(config=None, distributed=False)
    return _DEFAULT_CTX


class SortOptions:
    """reference: python/pycylon/data/table.pyx:2512 / cylon/table.hpp:388-393"""

    def __init__(self, num_bins: int = 0, num_samples: int = 0):
        self.num_bins = int(num_bins)
        self.num_samples = int(num_samples)


class Table(PandasOpsMixin):
    def __init__(self, pyarrow_table=None, context: Optional[CylonContext] = None, _native=None):
        self._ctx = _ensure_ctx(context)
        if _native is not None:
            self._t = _native
        elif pyarrow_table is not None:
            self._t = ab.table_from_arrow(self._ctx._ctx, pyarrow_table, self._ctx.device)
        else:
            self._t = C.Table(self._ctx._ctx, [])
        self._index = None

    # ------------------------------------------------------------------ wrapping
    def _wrap(self, native) -> "Table":
        return Table(context=self._ctx, _native=native)

    @property
    def native(self):
        return self._t

    @property
    def context(self) -> CylonContext:
        return self._ctx

    # ------------------------------------------------------------ constructors
    @staticmethod
    def from_arrow(context: CylonContext, pyarrow_table: pa.Table) -> "Table":
        return Table(pyarrow_table, context)

    @staticmethod
    def from_pandas(context: CylonContext = None, df=None, preserve_index=False, nthreads=None, columns=None,
                    safe=False) -> "Table":
        if df is None and context is not None and not isinstance(context, CylonContext):
            context, df = None, context
        at = pa.Table.from_pandas(df, preserve_index=preserve_index, nthreads=nthreads, columns=columns, safe=safe)
        return Table(at, context)

    @staticmethod
    def from_pydict(context: CylonContext, dictionary: dict) -> "Table":
        return Table(pa.Table.from_pydict(dictionary), context)

    @staticmethod
    def from_list(context: CylonContext, col_names: List[str], data_list: List) -> "Table":
        return Table(pa.Table.from_arrays([pa.array(d) for d in data_list], names=col_names), context)

    @staticmethod
    def from_numpy(context: CylonContext, col_names: List[str], ar_list: List[np.ndarray]) -> "Table":
        return Table(pa.Table.from_arrays([pa.array(a) for a in ar_list], names=col_names), context)

    @staticmethod
    def from_torch(context: CylonContext, columns: Dict[str, torch.Tensor]) -> "Table":
        """Zero-copy from device tensors (DLPack-free: the tensors become the column buffers)."""
        ctx = _ensure_ctx(context)
        cols = [ab.column_from_tensor(k, v.to(ctx.device)) for k, v in columns.items()]
        return Table(context=ctx, _native=C.Table(ctx._ctx, cols))

    # ------------------------------------------------------------- conversions
    def to_arrow(self) -> pa.Table:
        return ab.table_to_arrow(self._t)

    def to_pandas(self):
        return self.to_arrow().to_pandas()

    def to_pydict(self, with_index=False):
        return self.to_arrow().to_pydict()

    def to_numpy(self, order: str = "F", zero_copy_only: bool = True, writable: bool = False):
        cols = [c.to_numpy(zero_copy_only=False) for c in self.to_arrow().columns]
        return np.array(cols).T.copy(order=order) if cols else np.empty((0, 0))

    # ---- Arrow PyCapsule interfaces ---------------------------------------------
    def __arrow_c_stream__(self, requested_schema=None):
        """Host Arrow C stream (pyarrow / polars / duckdb consumers)."""
        return self.to_arrow().__arrow_c_stream__(requested_schema)

    def __arrow_c_device_array__(self, requested_schema=None, **kwargs):
        """Arrow C Device Data Interface: a struct array whose buffers stay where the table
        lives (ARROW_DEVICE_ROCM in HBM, zero-copy for values / offsets / list children;
        bitmaps and packed booleans produced on the device; sync_event = a hipEvent_t)."""
        if requested_schema is not None:
            raise NotImplementedError("schema requests are not supported")
        return C.export_device_table(self._t)

    @staticmethod
    def from_arrow_device(context: CylonContext, obj) -> "Table":
        """Zero-copy import of an object exposing __arrow_c_device_array__ (or the capsule pair)."""
        ctx = _ensure_ctx(context)
        caps = obj.__arrow_c_device_array__() if hasattr(obj, "__arrow_c_device_array__") else obj
        return Table(context=ctx, _native=C.import_device_table(ctx._ctx, caps[0], caps[1]))

    def to_torch(self) -> Dict[str, torch.Tensor]:
        """Columns as device tensors (zero-copy, fixed width columns only).  Columns of one table
        may share a buffer natively (an inner join's two key columns hold the same values,
        docs/semantics.md); the second and later names of a shared buffer come back as copies, so an
        in-place write through one returned tensor never changes another."""
        out, seen = {}, set()
        for c in self._t.columns():
            if c.offsets is not None:
                raise TypeError(f"column {c.name} is variable width")
            d = c.data
            key = (d.device, d.untyped_storage().data_ptr()) if d.numel() else None
            if key is not None and key in seen:
                d = d.clone()
            elif key is not None:
                seen.add(key)
            out[c.name] = d
        return out

    def to_csv(self, path, csv_write_options=None):
        from ..io import write_csv
        write_csv(self, path, csv_write_options)

    def to_device(self, device: str) -> "Table":
        return self._wrap(self._t.to(device))

    def to_cpu(self) -> "Table":
        return self.to_device("cpu")

    # -------------------------------------------------------------- properties
    @property
    def column_names(self) -> List[str]:
        return self._t.column_names()

    @property
    def column_count(self) -> int:
        return self._t.num_columns()

    @property
    def row_count(self) -> int:
        return self._t.rows()

    @property
    def shape(self):
        return (self.row_count, self.column_count)

    @property
    def device(self) -> str:
        return self._t.device()

    def retain_memory(self, retain: bool):
        self._t.retain_memory(retain)

    def is_retain(self) -> bool:
        return self._t.is_retain()

    def clear(self):
        self._t.clear()

    def __len__(self):
        return self.row_count

    # ---------------------------------------------------------- column helpers
    def _resolve_column(self, c) -> int:
        if isinstance(c, (int, np.integer)):
            if not 0 <= int(c) < self.column_count:
                raise IndexError(f"column index {c} out of range")
            return int(c)
        idx = self._t.column_index(str(c))
        if idx < 0:
            raise KeyError(f"column '{c}' not found in {self.column_names}")
        return idx

    def _resolve_columns(self, cols) -> List[int]:
        if cols is None:
            return list(range(self.column_count))
        if isinstance(cols, (int, str, np.integer)):
            cols = [cols]
        return [self._resolve_column(c) for c in cols]

    def _resolve_join_columns(self, table: "Table", kwargs):
        left_on, right_on, on = kwargs.get("left_on"), kwargs.get("right_on"), kwargs.get("on")
        if left_on is not None and right_on is not None:
            lc, rc = self._resolve_columns(left_on), table._resolve_columns(right_on)
        elif on is not None:
            lc, rc = self._resolve_columns(on), table._resolve_columns(on)
        else:
            raise TypeError("kwargs 'on' or 'left_on' and 'right_on' must be provided")
        if not lc or len(lc) != len(rc):
            raise ValueError("Provided Column Names or Column Indices not valid.")
        return lc, rc

    # --------------------------------------------------------------- relational
    def join(self, table: "Table", join_type: str = "inner", algorithm: str = "sort", **kwargs) -> "Table":
        lc, rc = self._resolve_join_columns(table, kwargs)
        jt = _JOIN_TYPES[join_type.lower()]
        return self._wrap(C.join(self._t, table._t, jt, algorithm.lower(), lc, rc, kwargs.get("left_prefix", ""),
                                 kwargs.get("right_prefix", "")))

    def distributed_join(self, table: "Table", join_type: str = "inner", algorithm: str = "sort",
                         **kwargs) -> "Table":
        lc, rc = self._resolve_join_columns(table, kwargs)
        jt = _JOIN_TYPES[join_type.lower()]
        return self._wrap(C.distributed_join(self._t, table._t, jt, algorithm.lower(), lc, rc,
                                             kwargs.get("left_prefix", ""), kwargs.get("right_prefix", "")))

    # set operations (distinct semantics over all columns; reference table.pyx:383-430)
    def union(self, table: "Table") -> "Table":
        return self._wrap(C.union(self._t, table._t))

    def distributed_union(self, table: "Table") -> "Table":
        return self._wrap(C.distributed_union(self._t, table._t))

    def subtract(self, table: "Table") -> "Table":
        return self._wrap(C.subtract(self._t, table._t))

    def distributed_subtract(self, table: "Table") -> "Table":
        return self._wrap(C.distributed_subtract(self._t, table._t))

    def intersect(self, table: "Table") -> "Table":
        return self._wrap(C.intersect(self._t, table._t))

    def distributed_intersect(self, table: "Table") -> "Table":
        return self._wrap(C.distributed_intersect(self._t, table._t))

    def unique(self, columns: List = None, keep: str = "first", inplace=False) -> Optional["Table"]:
        out = self._wrap(C.unique(self._t, self._resolve_columns(columns), keep == "first"))
        if inplace:
            self._t = out._t
            return None
        return out

    def distributed_unique(self, columns: List = None, keep: str = "first", inplace=False):
        out = self._wrap(C.distributed_unique(self._t, self._resolve_columns(columns), keep == "first"))
        if inplace:
            self._t = out._t
            return None
        return out

    # aggregates (global across ranks, reference table.pyx:548-586)
    def _agg_op(self, column, op, quantile=0.5, ddof=1) -> "Table":
        from .aggregates import resolve_op
        return self._wrap(C.aggregate(self._t, self._resolve_column(column), int(resolve_op(op)), quantile, ddof,
                                      True))

    def sum(self, column):
        return self._agg_op(column, "sum")

    def count(self, column):
        return self._agg_op(column, "count")

    def min(self, column):
        return self._agg_op(column, "min")

    def max(self, column):
        return self._agg_op(column, "max")

    def mean(self, column):
        return self._agg_op(column, "mean")

    def var(self, column, ddof=1):
        return self._agg_op(column, "var", ddof=ddof)

    def std(self, column, ddof=1):
        return self._agg_op(column, "std", ddof=ddof)

    def nunique(self, column):
        return self._agg_op(column, "nunique")

    def quantile(self, column, q=0.5):
        return self._agg_op(column, "quantile", quantile=q)

    def groupby(self, index, agg: dict, algorithm: str = "hash") -> "Table":
        """Distributed group-by (reference table.pyx:587-647 -> DistributedHashGroupBy).

        agg: {column: op | [ops]} with ops as names ('sum','cnt'/'count','min','max','mean','var','std',
        'nunique','quantile'/'median') or AggregationOp values.
        """
        from .aggregates import parse_agg
        if not agg or not isinstance(agg, dict):
            raise ValueError("agg should be non-empty and dict type")
        keys = self._resolve_columns(index)
        cols, ops, qs, ddofs = parse_agg(self, agg)
        fn = C.distributed_hash_groupby if algorithm == "hash" else C.distributed_pipeline_groupby
        return self._wrap(fn(self._t, keys, cols, ops, qs, ddofs))

    def local_groupby(self, index, agg: dict, algorithm: str = "hash") -> "Table":
        from .aggregates import parse_agg
        keys = self._resolve_columns(index)
        cols, ops, qs, ddofs = parse_agg(self, agg)
        fn = C.hash_groupby if algorithm == "hash" else C.pipeline_groupby
        return self._wrap(fn(self._t, keys, cols, ops, qs, ddofs))

    def distributed_sort(self, order_by=None, ascending: Union[bool, List[bool]] = True,
                         sort_options: SortOptions = None) -> "Table":
        cols = self._resolve_columns(order_by if order_by is not None else 0)
        asc = [bool(a) for a in ascending] if isinstance(ascending, (list, tuple)) else [bool(ascending)] * len(cols)
        so = sort_options or SortOptions()
        return self._wrap(C.distributed_sort(self._t, cols, asc, so.num_bins, so.num_samples))

    def project(self, columns: List) -> "Table":
        return self._wrap(C.project(self._t, self._resolve_columns(columns)))

    @staticmethod
    def merge(tables: List["Table"], ctx: CylonContext = None) -> "Table":
        if not tables:
            raise ValueError("merge needs at least one table")
        return tables[0]._wrap(C.merge([t._t for t in tables]))

    def sort(self, order_by=None, ascending: Union[bool, List[bool]] = True) -> "Table":
        cols = self._resolve_columns(order_by if order_by is not None else 0)
        asc = [bool(a) for a in ascending] if isinstance(ascending, (list, tuple)) else [bool(ascending)]
        return self._wrap(C.sort(self._t, cols, asc))

    def _topk_args(self, k, order_by, ascending):
        if int(k) < 0:
            raise ValueError(f"top-k needs k >= 0, got {k}")
        cols = self._resolve_columns(order_by if order_by is not None else 0)
        asc = [bool(a) for a in ascending] if isinstance(ascending, (list, tuple)) else [bool(ascending)] * len(cols)
        return cols, asc, int(k)

    def topk(self, k: int, order_by=None, ascending: Union[bool, List[bool]] = True) -> "Table":
        """ORDER BY order_by LIMIT k: the first min(k, rows) rows of the stable sort, all columns.
        Ties at the cut keep the lower row number; NaN sorts after every number and null after NaN
        in both directions (docs/semantics.md "Top-k")."""
        return self._wrap(C.topk(self._t, *self._topk_args(k, order_by, ascending)))

    def distributed_topk(self, k: int, order_by=None, ascending: Union[bool, List[bool]] = True) -> "Table":
        """The global top k rows on rank 0 (ties by rank, then row); 0 rows on every other rank."""
        return self._wrap(C.distributed_topk(self._t, *self._topk_args(k, order_by, ascending)))

    def nlargest(self, n: int, columns) -> "Table":
        return self.topk(n, columns, ascending=False)

    def nsmallest(self, n: int, columns) -> "Table":
        return self.topk(n, columns, ascending=True)

    # function name -> (WindowFunc number of csrc/cylon/table.hpp, the family that says how its spec reads)
    _WINDOW_FUNCS = {
        "row_number": (0, "ranking"), "rank": (1, "ranking"), "dense_rank": (2, "ranking"),
        "cumcount": (3, "running"), "cumsum": (4, "running"), "cummin": (5, "running"), "cummax": (6, "running"),
        "lag": (7, "shift"), "lead": (8, "shift"),
        "rolling_count": (9, "rolling"), "rolling_sum": (10, "rolling"), "rolling_mean": (11, "rolling"),
        "rolling_min": (12, "rolling"), "rolling_max": (13, "rolling"),
        "range_count": (14, "range"), "range_sum": (15, "range"), "range_mean": (16, "range"),
        "range_min": (17, "range"), "range_max": (18, "range"),
        "first_value": (19, "pick"), "last_value": (20, "pick"), "nth_value": (21, "nth"),
        "ffill": (22, "fill"), "bfill": (23, "fill"),
        "ntile": (24, "ntile"), "percent_rank": (25, "dist"), "cume_dist": (26, "dist"),
        "rolling_var": (27, "moment"), "rolling_std": (28, "moment"), "range_var": (29, "moment"),
        "range_std": (30, "moment")}
    # The engine's entry points, narrowest first.  Each takes the functions up to its largest WindowFunc
    # number and these fields of a _window_record, one list per field, in this order.
    _WINDOW_BASE = ("fid", "col", "arg", "name")
    _WINDOW_RANGE = _WINDOW_BASE + ("pre", "fol", "pre_f", "fol_f", "is_float", "minp")
    _WINDOW_LEVELS = (("window", 8, _WINDOW_BASE),
                      ("window_frames", 13, _WINDOW_BASE + ("pre", "fol", "minp")),
                      ("window_range_frames", 18, _WINDOW_RANGE),
                      ("window_nav", 26, _WINDOW_RANGE + ("ignore_nulls", "limit")),
                      ("window_moment_frames", 30, _WINDOW_RANGE + ("ignore_nulls", "limit", "ddof")))
    _UNBOUNDED = (1 << 63) - 1

    def _window_keys(self, partition_by, order_by, ascending):
        part = self._resolve_columns(partition_by) if partition_by is not None else []
        order = self._resolve_columns(order_by) if order_by is not None else []
        asc = [bool(a) for a in ascending] if isinstance(ascending, (list, tuple)) else [bool(ascending)] * len(order)
        if len(asc) != len(order):
            raise ValueError(f"{len(asc)} ascending flags for {len(order)} order columns")
        return part, order, asc

    def _window_record(self, spec, level=4):
        """A spec as a dict of fid (WindowFunc number), col (value column, -1: none), arg (LAG / LEAD offset,
        k of nth_value and ntile), pre, fol, pre_f, fol_f, is_float (the frame; in a range frame a float
        offset makes both offsets floats -- an int beside it is converted -- and None stays the integer
        that means unbounded), minp, ignore_nulls, limit and ddof, each at the engine's default where the
        function does not read it.  A function above _WINDOW_LEVELS[level], or a framed one given as a bare
        string, is unknown.  Values the engine refuses (k < 1, a negative limit or ddof, min_periods < 1,
        ignore_nulls on nth_value) are left to it."""
        bare = isinstance(spec, str)
        spec = (spec,) if bare else tuple(spec)
        fn = str(spec[0]).lower() if spec else ""
        fid, family = self._WINDOW_FUNCS.get(fn, (None, None))
        if fid is None or fid > self._WINDOW_LEVELS[level][1] or (bare and family in ("rolling", "range", "moment")):
            raise ValueError(f"unknown window function {spec[0] if spec else spec!r}; "
                             f"one of {sorted(n for n, (i, _) in self._WINDOW_FUNCS.items() if i <= 8)}")
        rec = dict(fid=fid, col=-1, arg=0, pre=0, fol=0, pre_f=0.0, fol_f=0.0, is_float=False, minp=1,
                   ignore_nulls=False, limit=0, ddof=1)

        def expect(lo, hi, form):
            if len(spec) < lo or len(spec) > hi:
                raise ValueError(f"window spec {spec!r}: expected {form}")

        if family == "ranking" or family == "dist":
            if len(spec) != 1:
                raise ValueError(f"window function {fn} takes no " + ("column" if family == "ranking" else "argument"))
        elif family == "ntile":
            expect(2, 2, "('ntile', k)")
            rec.update(arg=int(spec[1]))
        elif family == "running":
            expect(2, 2, f"({fn!r}, column)")
            rec.update(col=self._resolve_column(spec[1]))
        elif family == "shift":
            expect(2, 3, f"({fn!r}, column, offset)")
            rec.update(col=self._resolve_column(spec[1]), arg=int(spec[2]) if len(spec) == 3 else 1)
        elif family == "rolling":
            expect(4, 5, f"({fn!r}, column, preceding, following[, min_periods])")
            pre, fol = (self._UNBOUNDED if b is None else int(b) for b in spec[2:4])
            rec.update(pre=pre, fol=fol, col=self._resolve_column(spec[1]), minp=int(spec[4]) if len(spec) == 5 else 1)
        elif family == "range":
            expect(4, 5, f"({fn!r}, column, preceding, following[, min_periods])")
            for b in spec[2:4]:
                if b is not None and (isinstance(b, bool) or not isinstance(b, (int, float))):
                    raise ValueError(f"window spec {spec!r}: an offset is an int, a float or None, not {b!r}")
            is_float = any(isinstance(b, float) for b in spec[2:4])
            pre, fol = (self._UNBOUNDED if b is None else (0 if is_float else int(b)) for b in spec[2:4])
            pre_f, fol_f = (float(b) if is_float and b is not None else 0.0 for b in spec[2:4])
            rec.update(pre=pre, fol=fol, pre_f=pre_f, fol_f=fol_f, is_float=is_float,
                       col=self._resolve_column(spec[1]), minp=int(spec[4]) if len(spec) == 5 else 1)
        elif family == "moment":  # the frame is read as rolling_mean resp. range_mean read theirs
            expect(4, 6, f"({fn!r}, column, preceding, following[, min_periods[, ddof]])")
            ddof = int(spec[5]) if len(spec) == 6 else 1
            rec = self._window_record((fn.split("_")[0] + "_mean",) + spec[1:5])
            rec.update(fid=fid, ddof=ddof)
        elif family == "nth":
            expect(3, 4, "('nth_value', column, k)")
            rec.update(col=self._resolve_column(spec[1]), arg=int(spec[2]),
                       ignore_nulls=bool(spec[3]) if len(spec) == 4 else False)
        elif family == "pick":
            expect(2, 3, f"({fn!r}, column[, ignore_nulls])")
            rec.update(col=self._resolve_column(spec[1]), ignore_nulls=bool(spec[2]) if len(spec) == 3 else False)
        else:  # fill
            expect(2, 3, f"({fn!r}, column[, limit])")
            limit = spec[2] if len(spec) == 3 else None
            rec.update(col=self._resolve_column(spec[1]), limit=0 if limit is None else int(limit))
        return rec

    def _window_level(self, funcs):
        """the narrowest entry point that takes every spec of the call (a spec that does not parse: the first)"""
        fids = []
        for spec in (funcs or {}).values():
            fn = spec if isinstance(spec, str) else (spec[0] if len(spec) > 0 else None)
            fid, family = self._WINDOW_FUNCS.get(fn.lower(), (0, "")) if isinstance(fn, str) else (0, "")
            fids.append(0 if isinstance(spec, str) and family in ("rolling", "range", "moment") else fid)
        return next(k for k, (_, top, _) in enumerate(self._WINDOW_LEVELS) if max(fids, default=0) <= top)

    def _window_level_args(self, level, partition_by, order_by, ascending, funcs):
        """(partition columns, order columns, ascending flags, one list per field of _WINDOW_LEVELS[level])"""
        part, order, asc = self._window_keys(partition_by, order_by, ascending)
        recs = [dict(self._window_record(spec, level), name="" if name is None else str(name))
                for name, spec in (funcs or {}).items()]
        return (part, order, asc, *([r[f] for r in recs] for f in self._WINDOW_LEVELS[level][2]))

    def _window_args(self, partition_by, order_by, ascending, funcs):
        return self._window_level_args(0, partition_by, order_by, ascending, funcs)

    def _window_frame_args(self, partition_by, order_by, ascending, funcs):
        """_window_args plus the three frame lists, for a call with at least one rolling spec"""
        return self._window_level_args(1, partition_by, order_by, ascending, funcs)

    def _window_range_args(self, partition_by, order_by, ascending, funcs):
        """_window_frame_args plus the float offsets, for a call with at least one range spec"""
        return self._window_level_args(2, partition_by, order_by, ascending, funcs)

    def _window_nav_args(self, partition_by, order_by, ascending, funcs):
        """_window_range_args plus ignore_nulls and limit, for a call with at least one navigation or
        distribution spec"""
        return self._window_level_args(3, partition_by, order_by, ascending, funcs)

    def _window_moment_args(self, partition_by, order_by, ascending, funcs):
        """_window_nav_args plus ddof, for a call with at least one moment (framed VAR / STD) spec"""
        return self._window_level_args(4, partition_by, order_by, ascending, funcs)

    def _window_call(self, prefix, partition_by, order_by, ascending, funcs):
        level = self._window_level(funcs)
        entry = getattr(C, prefix + self._WINDOW_LEVELS[level][0])
        return self._wrap(entry(self._t, *self._window_level_args(level, partition_by, order_by, ascending, funcs)))

    def window(self, partition_by=None, order_by=None, ascending: Union[bool, List[bool]] = True,
               funcs: dict = None) -> "Table":
        """Window functions OVER (PARTITION BY partition_by ORDER BY order_by), frame UNBOUNDED PRECEDING ..
        CURRENT ROW: this table's columns in its row order plus one column per entry of `funcs`, a dict
        from output name to "row_number" | "rank" | "dense_rank" | ("cumcount" | "cumsum" | "cummin" |
        "cummax", column) | ("lag" | "lead", column[, offset = 1]).  Ties keep row order; NaN sorts
        after every number and null after NaN in both directions (docs/semantics.md "Window functions").

        Rolling aggregates take a frame of their own, ROWS BETWEEN preceding PRECEDING AND following
        FOLLOWING of the partition: ("rolling_sum" | "rolling_mean" | "rolling_min" | "rolling_max" |
        "rolling_count", column, preceding, following[, min_periods = 1]), None meaning unbounded, e.g.
        ("rolling_mean", "v", 6, 0) for a 7-row moving average.  Nulls are skipped; the result is null
        where the frame holds fewer than min_periods values (rolling_count is never null).

        Range aggregates frame by the order column's VALUES instead, RANGE BETWEEN preceding PRECEDING AND
        following FOLLOWING: ("range_sum" | "range_mean" | "range_min" | "range_max" | "range_count",
        column, preceding, following[, min_periods = 1]) aggregates the rows of the partition whose order
        value lies within `preceding` below and `following` above the row's own (the other way round
        in a descending order), peers included.  They need exactly one order column -- an integer, a
        temporal type (offsets in its unit) or float32 / float64; offsets are ints, floats (float
        columns only) or None = unbounded, e.g. ("range_mean", "v", 5_000_000_000, 0) over a
        timestamp[ns] column for the mean of the last 5 seconds (pandas rolling('5s', closed='both')
        on unique timestamps).  Everything else is as for the rolling aggregates.

        Navigation functions read one cell of the partition, whatever the column's type:
        ("first_value" | "last_value", column[, ignore_nulls = False]) the cell of the partition's first /
        last row in window order -- the frame is the WHOLE partition, not SQL's default frame, under which
        last_value would be the row's last peer -- or, with ignore_nulls, its first / last non-null cell;
        ("nth_value", column, k) the cell of its k-th row (k >= 1), null in a shorter partition;
        ("ffill" | "bfill", column[, limit = None]) the cell itself, or for a null cell the nearest
        non-null one before / after it in the partition, at most `limit` positions away (the pandas
        groupby().ffill(limit=)).  Null is the validity byte: NaN is a value, it is copied and it stops a
        fill.  Distribution functions take no column: ("ntile", k) the bucket 1 .. k of the row when the
        partition is cut into k runs whose sizes differ by at most one (the larger first),
        "percent_rank" = (rank - 1) / (rows - 1), 0.0 in a one-row partition, and "cume_dist" = the rows
        at or before the row's last peer / rows (docs/semantics.md "Navigation and distribution
        functions").

        Framed variance and standard deviation take the frames above: ("rolling_var" | "rolling_std",
        column, preceding, following[, min_periods = 1[, ddof = 1]]) over the ROWS frame of rolling_mean,
        ("range_var" | "range_std", ...) over the RANGE frame of range_mean, e.g. ("rolling_std", "v", 19,
        0) for pandas rolling(20, min_periods=1).std() and ("rolling_std", "v", None, 0) for
        expanding().std().  With m the frame's non-null values, each converted to float64, the float64
        result is sum((x - mean)^2) / (m - ddof) or its square root: null where m < min_periods or
        m - ddof <= 0, NaN where the frame holds a NaN or an infinity, never negative.  Every moment spec
        of a column reads one pyramid of merged (count, mean, M2) states, so nothing cancels on data far
        from zero (docs/semantics.md "Framed aggregates")."""
        return self._window_call("", partition_by, order_by, ascending, funcs)

    def distributed_window(self, partition_by=None, order_by=None, ascending: Union[bool, List[bool]] = True,
                           funcs: dict = None) -> "Table":
        """window() after a shuffle by the partition columns (at least one when the world is larger than
        1); the output row order is unspecified.  Rolling, range, navigation, distribution and moment specs
        as in window()."""
        return self._window_call("distributed_", partition_by, order_by, ascending, funcs)

    def _fill(self, fn, by, order_by, ascending, limit, columns):
        part = self._resolve_columns(by) if by is not None else []
        order = self._resolve_columns(order_by) if order_by is not None else []
        if limit is not None and int(limit) <= 0:
            raise ValueError("limit must be greater than 0")
        keys = set(part) | set(order)
        cols = self._resolve_columns(columns) if columns is not None else \
            [c for c in range(self.column_count) if c not in keys]
        if not cols:
            return self
        names = self.column_names
        tmp = [f"__{fn}_{i}__" for i in range(len(cols))]
        w = self.window(part or None, order or None, ascending,
                        {t: (fn, c) if limit is None else (fn, c, int(limit)) for t, c in zip(tmp, cols)})
        filled = dict(zip(cols, range(self.column_count, self.column_count + len(cols))))
        out = w.project([filled.get(c, c) for c in range(self.column_count)])
        out.rename(names)
        return out

    def ffill(self, by=None, order_by=None, limit=None, columns=None,
              ascending: Union[bool, List[bool]] = True) -> "Table":
        """Forward fill (the pandas groupby(by).ffill(limit=)): the named columns -- by default every column
        that is neither a `by` nor an `order_by` column -- with each null cell replaced by the nearest
        non-null cell before it in its `by` group, in `order_by` order (neither given: input row order), at
        most `limit` positions back.  Rows, column order and names stay.  NaN is a value, not a null."""
        return self._fill("ffill", by, order_by, ascending, limit, columns)

    def bfill(self, by=None, order_by=None, limit=None, columns=None,
              ascending: Union[bool, List[bool]] = True) -> "Table":
        """Backward fill: ffill with the nearest non-null cell after the row."""
        return self._fill("bfill", by, order_by, ascending, limit, columns)

    _ASOF_DIRECTIONS = {"backward": 0, "forward": 1, "nearest": 2}

    def _asof_column(self, c) -> int:
        """a name -> its index; an integer goes to the engine as it is (out of range: Code::Invalid)"""
        if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
            return int(c)
        idx = self._t.column_index(str(c))
        if idx < 0:
            raise KeyError(f"column '{c}' not found in {self.column_names}")
        return idx

    def _asof_args(self, table: "Table", on, left_on, right_on, by, left_by, right_by, direction, allow_exact_matches,
                   tolerance):
        if on is not None:
            left_on = right_on = on
        if left_on is None or right_on is None or isinstance(left_on, (list, tuple)) or isinstance(right_on, (list, tuple)):
            raise ValueError("asof_join needs one `on` column: pass on=, or left_on= and right_on=")
        if by is not None:
            left_by = right_by = by
        as_list = lambda b: [] if b is None else (list(b) if isinstance(b, (list, tuple)) else [b])
        lby, rby = as_list(left_by), as_list(right_by)
        if len(lby) != len(rby):
            raise ValueError(f"asof_join: {len(lby)} left and {len(rby)} right `by` columns")
        if isinstance(direction, str):
            if direction.lower() not in self._ASOF_DIRECTIONS:
                raise ValueError(f"unknown asof direction {direction!r}; one of {sorted(self._ASOF_DIRECTIONS)}")
            direction = self._ASOF_DIRECTIONS[direction.lower()]
        if tolerance is not None:
            if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
                raise ValueError(f"asof_join: tolerance must be an int or a float, got {tolerance!r}")
            tolerance = int(tolerance) if isinstance(tolerance, (int, np.integer)) else float(tolerance)
            if isinstance(tolerance, int) and not -(1 << 63) <= tolerance < (1 << 63):
                raise ValueError(f"asof_join: tolerance {tolerance} does not fit 64 bits")
        return (self._asof_column(left_on), table._asof_column(right_on), [self._asof_column(c) for c in lby],
                [table._asof_column(c) for c in rby], int(direction), bool(allow_exact_matches), tolerance)

    def asof_join(self, table: "Table", on=None, left_on=None, right_on=None, by=None, left_by=None, right_by=None,
                  direction: str = "backward", allow_exact_matches: bool = True, tolerance=None,
                  left_prefix: str = "", right_prefix: str = "") -> "Table":
        """As-of join (pandas.merge_asof, SQL ASOF JOIN): this table's rows in its row order, followed by the
        columns of the nearest row of `table` whose `by` columns equal the row's own -- direction
        "backward": the last one with right_on <= left_on, "forward": the first one with right_on >=
        left_on, "nearest": the nearer of the two, the backward one on equal distances.
        allow_exact_matches=False makes the comparisons strict; a match farther away than `tolerance` (an
        int in the column's unit for an integer or temporal `on`, a float for a float `on`) is dropped.
        Right columns are null where there is no match.  Neither table needs to be sorted; a null or NaN
        `on` never matches (docs/semantics.md "As-of join")."""
        args = self._asof_args(table, on, left_on, right_on, by, left_by, right_by, direction, allow_exact_matches,
                               tolerance)
        return self._wrap(C.asof_join(self._t, table._t, *args, left_prefix, right_prefix))

    def distributed_asof_join(self, table: "Table", on=None, left_on=None, right_on=None, by=None, left_by=None,
                              right_by=None, direction: str = "backward", allow_exact_matches: bool = True,
                              tolerance=None, left_prefix: str = "", right_prefix: str = "") -> "Table":
        """asof_join() after a shuffle of both tables by their `by` columns (at least one when the world is
        larger than 1); the output row order is unspecified."""
        args = self._asof_args(table, on, left_on, right_on, by, left_by, right_by, direction, allow_exact_matches,
                               tolerance)
        return self._wrap(C.distributed_asof_join(self._t, table._t, *args, left_prefix, right_prefix))

    _INTERVAL_CLOSED = {"both": 0, "left": 1, "right": 2, "neither": 3}
    _INTERVAL_HOW = {"inner": 0, "left": 1}

    def _interval_args(self, table: "Table", lower, upper, on, by, left_by, right_by, closed, how=None):
        """-> (lower, upper, on, left_by, right_by, closed[, how]) as the engine takes them"""
        if any(c is None or isinstance(c, (list, tuple)) for c in (lower, upper, on)):
            raise ValueError("interval_join needs one `lower`, one `upper` and one `on` column")
        if by is not None:
            left_by = right_by = by
        as_list = lambda b: [] if b is None else (list(b) if isinstance(b, (list, tuple)) else [b])
        lby, rby = as_list(left_by), as_list(right_by)
        if len(lby) != len(rby):
            raise ValueError(f"interval_join: {len(lby)} left and {len(rby)} right `by` columns")
        if isinstance(closed, str):
            if closed.lower() not in self._INTERVAL_CLOSED:
                raise ValueError(f"unknown closed {closed!r}; one of {sorted(self._INTERVAL_CLOSED)}")
            closed = self._INTERVAL_CLOSED[closed.lower()]
        args = (self._asof_column(lower), self._asof_column(upper), table._asof_column(on),
                [self._asof_column(c) for c in lby], [table._asof_column(c) for c in rby], int(closed))
        if how is None:
            return args
        if isinstance(how, str):
            if how.lower() not in self._INTERVAL_HOW:
                raise ValueError(f"unknown interval join type {how!r}; one of {sorted(self._INTERVAL_HOW)}")
            how = self._INTERVAL_HOW[how.lower()]
        return args + (int(how),)

    def interval_join(self, table: "Table", lower, upper, on, by=None, left_by=None, right_by=None,
                      closed: str = "both", how: str = "inner", left_prefix: str = "",
                      right_prefix: str = "") -> "Table":
        """Interval join (SQL `r.on BETWEEN l.lower AND l.upper`, a range join): one row for every pair of a
        row of this table and a row of `table` whose `by` columns equal its own and whose `on` value lies
        in [lower, upper] -- this table's columns, then `table`'s.  closed: "both", "left" (lower <= on <
        upper), "right" or "neither".  Rows are ordered by this table's row, then `on`, then `table`'s
        row.  how="left" adds one row with null right columns for a row without a match.  A null or NaN
        bound or `on` never matches; +-inf and the integer extremes are ordinary values, which is how an
        unbounded side is written (docs/semantics.md "Interval join")."""
        args = self._interval_args(table, lower, upper, on, by, left_by, right_by, closed, how)
        return self._wrap(C.interval_join(self._t, table._t, *args, left_prefix, right_prefix))

    def distributed_interval_join(self, table: "Table", lower, upper, on, by=None, left_by=None, right_by=None,
                                  closed: str = "both", how: str = "inner", left_prefix: str = "",
                                  right_prefix: str = "") -> "Table":
        """interval_join() after a shuffle of both tables by their `by` columns (at least one when the world
        is larger than 1); the output row order is unspecified."""
        args = self._interval_args(table, lower, upper, on, by, left_by, right_by, closed, how)
        return self._wrap(C.distributed_interval_join(self._t, table._t, *args, left_prefix, right_prefix))

    def interval_join_counts(self, table: "Table", lower, upper, on, by=None, left_by=None, right_by=None,
                             closed: str = "both") -> torch.Tensor:
        """How many rows of `table` fall into each row's interval: an int64 tensor of one count per row of
        this table, on its device.  The pairs themselves are never built."""
        args = self._interval_args(table, lower, upper, on, by, left_by, right_by, closed)
        return C.interval_join_counts(self._t, table._t, *args)

    def shuffle(self, hash_columns: List = None) -> "Table":
        return self._wrap(C.shuffle(self._t, self._resolve_columns(hash_columns)))

    def hash_partition(self, hash_columns: List, num_partitions: int) -> List["Table"]:
        return [self._wrap(t) for t in C.hash_partition(self._t, self._resolve_columns(hash_columns),
                                                         int(num_partitions))]

    def take(self, indices) -> "Table":
        idx = torch.as_tensor(indices, dtype=torch.int64)
        return self._wrap(C.gather(self._t, idx.to(self.device)))

    def filter_mask(self, mask) -> "Table":
        m = torch.as_tensor(mask)
        if m.dtype != torch.uint8:
            m = m.to(torch.uint8)
        return self._wrap(C.filter_by_mask(self._t, m.to(self.device)))

    def slice(self, offset: int, length: int) -> "Table":
        return self._wrap(C.slice(self._t, int(offset), int(length)))

    # ------------------------------------------------------------------ display
    def to_string(self, row_limit: int = 10):
        return self.to_arrow().slice(0, row_limit).to_pandas().to_string()

    def __repr__(self):
        return self.to_string()

    def show(self, row1=-1, row2=-1, col1=-1, col2=-1):
        at = self.to_arrow()
        if row1 >= 0 and row2 >= 0:
            at = at.slice(row1, row2 - row1)
        if col1 >= 0 and col2 >= 0:
            at = at.select(list(range(col1, col2)))
        print(at.to_pandas().to_string())
