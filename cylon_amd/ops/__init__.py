"""cylon_amd.ops: functional operator API over Tables (mirrors the C++ `cylon::ops` /
reference `cylon/table.hpp` free functions: Join, DistributedJoin, Union, ..., Sort,
DistributedSort, Shuffle, HashPartition, Unique, GroupBy, aggregates).

Every function is a thin call into the native extension; the Table methods of
`cylon_amd.Table` are the object-style spelling of the same operators.
"""
from typing import Dict, List, Sequence, Union

from ..data.table import SortOptions, Table


def join(left: Table, right: Table, join_type: str = "inner", algorithm: str = "sort", **kw) -> Table:
    return left.join(right, join_type, algorithm, **kw)


def distributed_join(left: Table, right: Table, join_type: str = "inner", algorithm: str = "sort", **kw) -> Table:
    return left.distributed_join(right, join_type, algorithm, **kw)


def union(a: Table, b: Table) -> Table:
    return a.union(b)


def subtract(a: Table, b: Table) -> Table:
    return a.subtract(b)


def intersect(a: Table, b: Table) -> Table:
    return a.intersect(b)


def distributed_union(a: Table, b: Table) -> Table:
    return a.distributed_union(b)


def distributed_subtract(a: Table, b: Table) -> Table:
    return a.distributed_subtract(b)


def distributed_intersect(a: Table, b: Table) -> Table:
    return a.distributed_intersect(b)


def sort(t: Table, order_by=None, ascending: Union[bool, List[bool]] = True) -> Table:
    return t.sort(order_by, ascending)


def distributed_sort(t: Table, order_by=None, ascending: Union[bool, List[bool]] = True,
                     sort_options: SortOptions = None) -> Table:
    return t.distributed_sort(order_by, ascending, sort_options)


def topk(t: Table, k: int, order_by=None, ascending: Union[bool, List[bool]] = True) -> Table:
    return t.topk(k, order_by, ascending)


def distributed_topk(t: Table, k: int, order_by=None, ascending: Union[bool, List[bool]] = True) -> Table:
    return t.distributed_topk(k, order_by, ascending)


def window(t: Table, partition_by=None, order_by=None, ascending: Union[bool, List[bool]] = True,
           funcs: dict = None) -> Table:
    """Table.window: ranking, running aggregates, lag / lead and rolling aggregates over a ROWS frame,
    ("rolling_sum" | "rolling_mean" | "rolling_min" | "rolling_max" | "rolling_count", column, preceding,
    following[, min_periods]), or over a RANGE frame of the one order column's values, ("range_sum" | ... |
    "range_count", column, preceding, following[, min_periods]), and the navigation and distribution
    functions ("first_value" | "last_value", column[, ignore_nulls]), ("nth_value", column, k), ("ffill" |
    "bfill", column[, limit]), ("ntile", k), "percent_rank", "cume_dist", and the framed variance and
    standard deviation ("rolling_var" | "rolling_std" | "range_var" | "range_std", column, preceding,
    following[, min_periods[, ddof]])."""
    return t.window(partition_by, order_by, ascending, funcs)


def distributed_window(t: Table, partition_by=None, order_by=None, ascending: Union[bool, List[bool]] = True,
                       funcs: dict = None) -> Table:
    return t.distributed_window(partition_by, order_by, ascending, funcs)


def asof_join(left: Table, right: Table, **kwargs) -> Table:
    """Table.asof_join: on= | left_on=, right_on=; by= | left_by=, right_by=; direction, allow_exact_matches,
    tolerance, left_prefix, right_prefix."""
    return left.asof_join(right, **kwargs)


def distributed_asof_join(left: Table, right: Table, **kwargs) -> Table:
    return left.distributed_asof_join(right, **kwargs)


def interval_join(left: Table, right: Table, lower, upper, on, **kwargs) -> Table:
    """Table.interval_join: lower, upper (columns of left), on (a column of right); by= | left_by=, right_by=;
    closed, how, left_prefix, right_prefix."""
    return left.interval_join(right, lower, upper, on, **kwargs)


def distributed_interval_join(left: Table, right: Table, lower, upper, on, **kwargs) -> Table:
    return left.distributed_interval_join(right, lower, upper, on, **kwargs)


def shuffle(t: Table, hash_columns: List = None) -> Table:
    return t.shuffle(hash_columns)


def hash_partition(t: Table, hash_columns: List, num_partitions: int) -> List[Table]:
    return t.hash_partition(hash_columns, num_partitions)


def unique(t: Table, columns: Sequence = None, keep: str = "first") -> Table:
    return t.unique(columns, keep)


def distributed_unique(t: Table, columns: Sequence = None) -> Table:
    return t.distributed_unique(columns)


def groupby(t: Table, index, agg: Dict, algorithm: str = "hash") -> Table:
    """Distributed (two-phase) group-by; equals local_groupby on a single rank."""
    return t.groupby(index, agg, algorithm)


def local_groupby(t: Table, index, agg: Dict, algorithm: str = "hash") -> Table:
    return t.local_groupby(index, agg, algorithm)


def project(t: Table, columns: Sequence) -> Table:
    return t.project(columns)


def merge(tables: Sequence[Table]) -> Table:
    return Table.merge(list(tables))


__all__ = ["join", "distributed_join", "union", "subtract", "intersect", "distributed_union",
           "distributed_subtract", "distributed_intersect", "sort", "distributed_sort", "topk",
           "distributed_topk", "window", "distributed_window", "asof_join", "distributed_asof_join", "interval_join",
           "distributed_interval_join", "shuffle",
           "hash_partition", "unique", "distributed_unique", "groupby", "local_groupby", "project", "merge"]
