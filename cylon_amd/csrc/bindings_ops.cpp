// Bindings for the extended relational operators (set ops, unique, group-by,
// aggregates, range partition, distributed sort).
#include <map>
#include <torch/extension.h>

#include "cylon/kernels/kernels.hpp"
#include <tuple>

#include "cylon/api.hpp"
#include "cylon/io/arrow_io.hpp"
#include "cylon/io/csv.hpp"
#include "cylon/indexing/index.hpp"
#include "cylon/io/device_interop.hpp"
#include "cylon/io/h2d.hpp"
#include "cylon/knobs.hpp"
#include "cylon/ops/api_ext.hpp"
#include "cylon/ops/graph.hpp"
#include "cylon/ops/radix_sizing.hpp"
#include "cylon/ops/relational.hpp"
#include "cylon/ops/util.hpp"
#include "cylon/table.hpp"

namespace py = pybind11;
using namespace cylon;

join::config::JoinType parse_join_type(const std::string &t);  // bindings.cpp

// join type of the operator / registry bindings: the semi / anti spellings through parse_join_type,
// every other string as these bindings always read it
static join::config::JoinType op_join_type(const std::string &type) {
  using namespace join::config;
  for (const char *s : {"semi", "left_semi", "leftsemi", "anti", "left_anti", "leftanti"})
    if (type == s) return parse_join_type(type);
  return type == "left" ? LEFT : type == "right" ? RIGHT : type == "outer" ? FULL_OUTER : INNER;
}

static std::vector<ops::AggSpec> make_specs(const std::vector<int> &cols, const std::vector<int> &op_ids,
                                            const std::vector<double> &qs, const std::vector<int> &ddofs) {
  CYLON_CHECK(cols.size() == op_ids.size(), Code::Invalid, "aggregate columns and ops differ in length");
  std::vector<ops::AggSpec> specs;
  for (size_t i = 0; i < cols.size(); ++i) {
    ops::AggSpec s{cols[i], op_ids[i]};
    if (i < qs.size()) s.quantile = qs[i];
    if (i < ddofs.size()) s.ddof = ddofs[i];
    specs.push_back(s);
  }
  return specs;
}

// Window specs as flat lists, one entry per spec.  max_func is the largest WindowFunc the entry point
// accepts; it also says which lists the entry point has (each must be as long as funcs).  A list it does
// not have arrives empty and leaves WindowSpec's default in every spec.
using I64List = std::vector<int64_t>;
static std::vector<WindowSpec> window_specs(int max_func, const std::vector<int> &funcs, const std::vector<int> &cols,
                                            const I64List &args, const std::vector<std::string> &names,
                                            const I64List &preceding = {}, const I64List &following = {},
                                            const std::vector<double> &preceding_f = {},
                                            const std::vector<double> &following_f = {},
                                            const std::vector<bool> &offset_is_float = {},
                                            const I64List &min_periods = {}, const std::vector<bool> &ignore_nulls = {},
                                            const I64List &limit = {}, const std::vector<int> &ddof = {}) {
  const size_t k = funcs.size();
  auto fits = [&](size_t size, int since) { return size == (max_func >= since ? k : 0); };
  CYLON_CHECK(cols.size() == k && args.size() == k && names.size() == k && fits(preceding.size(), WIN_ROLLING_COUNT) &&
                  fits(following.size(), WIN_ROLLING_COUNT) && fits(min_periods.size(), WIN_ROLLING_COUNT) &&
                  fits(preceding_f.size(), WIN_RANGE_COUNT) && fits(following_f.size(), WIN_RANGE_COUNT) &&
                  fits(offset_is_float.size(), WIN_RANGE_COUNT) && fits(ignore_nulls.size(), WIN_FIRST_VALUE) &&
                  fits(limit.size(), WIN_FIRST_VALUE) && fits(ddof.size(), WIN_ROLLING_VAR),
              Code::Invalid, "window spec lists differ in length");
  std::vector<WindowSpec> specs(k);
  for (size_t i = 0; i < k; ++i) {
    CYLON_CHECK(funcs[i] >= WIN_ROW_NUMBER && funcs[i] <= max_func, Code::Invalid, "window function " << funcs[i]);
    WindowSpec &s = specs[i];
    s.func = static_cast<WindowFunc>(funcs[i]);
    s.col = cols[i];
    s.arg = args[i];
    s.name = names[i];
    if (!preceding.empty()) s.preceding = preceding[i];
    if (!following.empty()) s.following = following[i];
    if (!min_periods.empty()) s.min_periods = min_periods[i];
    if (!preceding_f.empty()) s.preceding_f = preceding_f[i];
    if (!following_f.empty()) s.following_f = following_f[i];
    if (!offset_is_float.empty()) s.offset_is_float = offset_is_float[i];
    if (!ignore_nulls.empty()) s.ignore_nulls = ignore_nulls[i];
    if (!limit.empty()) s.limit = limit[i];
    if (!ddof.empty()) s.ddof = ddof[i];
  }
  return specs;
}

// C.window_frames' list order: min_periods follows the ROWS frame
static std::vector<WindowSpec> window_specs(int max_func, const std::vector<int> &funcs, const std::vector<int> &cols,
                                            const I64List &args, const std::vector<std::string> &names,
                                            const I64List &preceding, const I64List &following,
                                            const I64List &min_periods) {
  return window_specs(max_func, funcs, cols, args, names, preceding, following, {}, {}, {}, min_periods);
}

// NAME(table, partition_cols, order_cols, ascending, lists..., carry_step_tiles = 0) and distributed_NAME
// without the carry step; Lists = the types of the spec lists, list_args their Python names
template <typename... Lists, typename... Args>
static void def_window(py::module &m, const std::string &name, int max_func, const Args &...list_args) {
  const auto rel = py::call_guard<py::gil_scoped_release>();
  m.def(
      name.c_str(),
      [max_func](const TablePtr &t, const std::vector<int> &part, const std::vector<int> &order,
                 const std::vector<bool> &asc, const Lists &...lists, int64_t carry_step_tiles) {
        return ops::Window(t, part, order, asc, window_specs(max_func, lists...), carry_step_tiles);
      },
      py::arg("table"), py::arg("partition_cols"), py::arg("order_cols"), py::arg("ascending"), list_args...,
      py::arg("carry_step_tiles") = 0, rel);
  m.def(
      ("distributed_" + name).c_str(),
      [max_func](const TablePtr &t, const std::vector<int> &part, const std::vector<int> &order,
                 const std::vector<bool> &asc, const Lists &...lists) {
        return ops::DistributedWindow(t, part, order, asc, window_specs(max_func, lists...));
      },
      py::arg("table"), py::arg("partition_cols"), py::arg("order_cols"), py::arg("ascending"), list_args..., rel);
}

void register_extended_ops(py::module &m) {
  auto rel = py::call_guard<py::gil_scoped_release>();

  m.def("index_lookup", &ops::IndexLookup, py::arg("ctx"), py::arg("index"), py::arg("labels"), rel);

  // ---- device self-check behind the radix passes' wave-atomic stable ranking (radix_join.hip)
  m.def("rp_set_ranking", [](int mode) { hip::rp_set_ranking(mode); });
  m.def("partition_digit_bits", [](int bits) { ops::SetPartitionDigitBits(bits); });
  m.def("knob_registry", []() {  // (name without CYLON_, group, effect) of every native knob
    std::vector<std::tuple<std::string, std::string, std::string>> r;
    for (const auto &k : knobs::Registry()) r.emplace_back(k.name, k.group, k.effect);
    return r;
  });
  m.def("rp_take_order_violation", [](const std::string &device) {
    ops::Exec ex{at::Device(device)};
    CYLON_CHECK(ex.gpu, Code::Invalid, "rp_take_order_violation needs a GPU device");
    return hip::rp_take_order_violation(ex.stream);
  });
  m.def("lds_lane_order_violations", [](const std::string &device, int blocks, int rounds) {
    ops::Exec ex{at::Device(device)};
    CYLON_CHECK(ex.gpu, Code::Invalid, "lds_lane_order_violations needs a GPU device");
    return hip::lds_lane_order_violations(blocks, rounds, ex.stream);
  }, py::arg("device") = "cuda:0", py::arg("blocks") = 256, py::arg("rounds") = 4096,
     py::call_guard<py::gil_scoped_release>());

  // ---- validity bitmaps <-> byte masks at the Arrow boundary (bitmap.hip)
  m.def("pack_validity", [](at::Tensor bytes) {
    ops::Exec ex(bytes.device());
    bytes = bytes.contiguous().to(at::kByte);
    const int64_t n = bytes.numel();
    at::Tensor words = at::empty({std::max<int64_t>((n + 63) / 64, 1)}, ex.opts(at::kLong));
    at::Tensor nulls = at::zeros({1}, ex.opts(at::kLong));
    KCALL(ex, pack_validity, bytes.data_ptr<uint8_t>(), n, reinterpret_cast<uint64_t *>(words.data_ptr<int64_t>()),
          nulls.data_ptr<int64_t>());
    return std::make_pair(words.slice(0, 0, (n + 63) / 64), nulls.item<int64_t>());
  }, py::call_guard<py::gil_scoped_release>());
  m.def("unpack_validity", [](at::Tensor bits, int64_t bit_offset, int64_t n) {
    ops::Exec ex(bits.device());
    bits = bits.contiguous();
    at::Tensor out = at::empty({n}, ex.opts(at::kByte));
    if (n) KCALL(ex, unpack_validity, reinterpret_cast<const uint8_t *>(bits.data_ptr()), bit_offset, n,
                 out.data_ptr<uint8_t>());
    return out;
  }, py::call_guard<py::gil_scoped_release>());

  m.def("merge_sorted_runs", &ops::MergeSortedRuns, py::arg("runs"), py::arg("run_rows"), py::arg("col"),
        py::arg("ascending") = true, rel);

  // ---- pinned, pipelined host -> device ingest (io/h2d.cpp); src = host address of nbytes
  m.def("h2d_copy", [](uintptr_t src, int64_t nbytes, at::Tensor dst, int threads) {
    CYLON_CHECK(dst.is_cuda() && dst.is_contiguous(), Code::Invalid, "h2d_copy: contiguous device tensor expected");
    CYLON_CHECK(nbytes >= 0 && nbytes <= (int64_t)(dst.numel() * dst.element_size()), Code::Invalid,
                "h2d_copy: " << nbytes << " bytes do not fit the destination");
    io::H2DStats st;
    io::StagedH2D(reinterpret_cast<const void *>(src), dst.data_ptr(), (size_t)nbytes, dst.device().index(), threads,
                  &st);
    return st.seconds;
  }, py::arg("src"), py::arg("nbytes"), py::arg("dst"), py::arg("threads") = 0,
     py::call_guard<py::gil_scoped_release>());

  // ---- Arrow C Device Data Interface (PyCapsules "arrow_schema" / "arrow_device_array")
  m.def("export_device_table", [](const TablePtr &t) {
    auto *sch = new ArrowSchema();
    auto *arr = new ArrowDeviceArray();
    {
      py::gil_scoped_release nogil;
      io::ExportDeviceTable(t, sch, arr);
    }
    PyObject *cs = PyCapsule_New(sch, "arrow_schema", [](PyObject *o) {
      auto *p = static_cast<ArrowSchema *>(PyCapsule_GetPointer(o, "arrow_schema"));
      if (p && p->release) p->release(p);
      delete p;
    });
    PyObject *ca = PyCapsule_New(arr, "arrow_device_array", [](PyObject *o) {
      auto *p = static_cast<ArrowDeviceArray *>(PyCapsule_GetPointer(o, "arrow_device_array"));
      if (p && p->array.release) p->array.release(&p->array);
      delete p;
    });
    return py::make_tuple(py::reinterpret_steal<py::object>(cs), py::reinterpret_steal<py::object>(ca));
  });
  m.def("import_device_table", [](std::shared_ptr<CylonContext> ctx, py::object schema, py::object array) {
    auto *sch = static_cast<ArrowSchema *>(PyCapsule_GetPointer(schema.ptr(), "arrow_schema"));
    auto *arr = static_cast<ArrowDeviceArray *>(PyCapsule_GetPointer(array.ptr(), "arrow_device_array"));
    CYLON_CHECK(sch && arr, Code::Invalid, "expected 'arrow_schema' and 'arrow_device_array' capsules");
    py::gil_scoped_release nogil;
    return io::ImportDeviceTable(ctx, sch, arr);  // moves the structs (the capsules then only free them)
  });

  // ---- C27 persistent indexes + loc / iloc indexers (cylon/indexing/index.hpp)
  py::enum_<indexing::IndexingSchema>(m, "IndexingSchema")
      .value("RANGE", indexing::IndexingSchema::Range)
      .value("LINEAR", indexing::IndexingSchema::Linear)
      .value("HASH", indexing::IndexingSchema::Hash)
      .value("BINARYTREE", indexing::IndexingSchema::BinaryTree)
      .value("BTREE", indexing::IndexingSchema::BTree);
  py::class_<indexing::BaseIndex, std::shared_ptr<indexing::BaseIndex>>(m, "NativeIndex")
      .def("locations_of", &indexing::BaseIndex::LocationsOf, rel)
      .def("range_of", &indexing::BaseIndex::RangeOf, rel)
      .def("schema", &indexing::BaseIndex::GetSchema)
      .def("size", &indexing::BaseIndex::Size)
      .def("persistent_rows", [](const indexing::BaseIndex &i) {
        auto *s = dynamic_cast<const indexing::SortedIndex *>(&i);
        return s ? s->BuiltRows() : int64_t(0);
      });
  m.def("build_index", &indexing::BuildIndex, py::arg("table"), py::arg("col"), py::arg("schema"), rel);
  m.def("index_from_column", [](std::shared_ptr<CylonContext> ctx, const Column &c, indexing::IndexingSchema schema) {
    return indexing::BuildIndex(Table::Make(ctx, {c}), 0, schema);
  }, rel);
  m.def("table_set_index", [](const TablePtr &t, std::shared_ptr<indexing::BaseIndex> i) { t->SetIndex(i); }, rel);
  m.def("table_get_index", [](const TablePtr &t) { return t->GetIndex(); }, rel);
  m.def("table_reset_index", [](const TablePtr &t) { t->ResetIndex(); }, rel);
  m.def("loc", [](const TablePtr &t, const Column &values, const std::vector<int> &cols, indexing::IndexingSchema s) {
    return indexing::LocIndexer(s).Loc(t, values, cols);
  }, rel);
  m.def("loc_range", [](const TablePtr &t, const Column &start, const Column &end, const std::vector<int> &cols,
                        indexing::IndexingSchema s) { return indexing::LocIndexer(s).LocRange(t, start, end, cols); },
        rel);
  m.def("iloc", [](const TablePtr &t, at::Tensor pos, const std::vector<int> &cols) {
    return indexing::ILocIndexer().ILoc(t, pos, cols);
  }, rel);

  // ---- C25 native CSV I/O
  m.def(
      "read_csv",
      [](const std::shared_ptr<CylonContext> &ctx, const std::vector<std::string> &paths, const std::string &delimiter,
         bool header, bool autogen, const std::vector<std::string> &column_names, int64_t skip_rows,
         bool ignore_empty_lines, const std::vector<std::string> &include_columns,
         const std::vector<std::string> &null_values, const std::vector<std::string> &true_values,
         const std::vector<std::string> &false_values, bool strings_can_be_null, bool quoting,
         const std::string &quote_char, bool double_quote, int threads, bool escaping, const std::string &escape_char,
         bool newlines_in_values, const std::map<std::string, int> &column_types, bool include_missing_columns,
         int64_t block_size, bool concurrent_file_reads) {
        io::CSVReadOptions o;
        o.escaping = escaping;
        if (!escape_char.empty()) o.escape_char = escape_char[0];
        o.newlines_in_values = newlines_in_values;
        for (const auto &kv : column_types) o.column_types.emplace(kv.first, DataType(static_cast<Type>(kv.second)));
        o.include_missing_columns = include_missing_columns;
        o.block_size = (int32_t)std::min<int64_t>(block_size, INT32_MAX);
        o.concurrent_file_reads = concurrent_file_reads;
        o.delimiter = delimiter.empty() ? ',' : delimiter[0];
        o.header = header;
        o.autogenerate_column_names = autogen;
        o.column_names = column_names;
        o.skip_rows = skip_rows;
        o.ignore_empty_lines = ignore_empty_lines;
        o.include_columns = include_columns;
        o.null_values = null_values;
        if (!true_values.empty()) o.true_values = true_values;
        if (!false_values.empty()) o.false_values = false_values;
        o.strings_can_be_null = strings_can_be_null;
        o.quoting = quoting;
        o.quote_char = quote_char.empty() ? '"' : quote_char[0];
        o.double_quote = double_quote;
        o.threads = threads;
        return io::ReadCSVs(ctx, paths, o);
      },
      py::arg("ctx"), py::arg("paths"), py::arg("delimiter") = ",", py::arg("header") = true,
      py::arg("autogenerate_column_names") = false, py::arg("column_names") = std::vector<std::string>{},
      py::arg("skip_rows") = 0, py::arg("ignore_empty_lines") = true,
      py::arg("include_columns") = std::vector<std::string>{}, py::arg("null_values") = std::vector<std::string>{},
      py::arg("true_values") = std::vector<std::string>{}, py::arg("false_values") = std::vector<std::string>{},
      py::arg("strings_can_be_null") = false, py::arg("quoting") = true, py::arg("quote_char") = "\"",
      py::arg("double_quote") = true, py::arg("threads") = 0, py::arg("escaping") = false,
      py::arg("escape_char") = "\\", py::arg("newlines_in_values") = false,
      py::arg("column_types") = std::map<std::string, int>{}, py::arg("include_missing_columns") = false,
      py::arg("block_size") = int64_t(1) << 20, py::arg("concurrent_file_reads") = true, rel);
  m.def(
      "write_csv",
      [](const TablePtr &t, const std::string &path, const std::string &delimiter,
         const std::vector<std::string> &names) {
        io::CSVWriteOptions o;
        o.delimiter = delimiter.empty() ? ',' : delimiter[0];
        o.column_names = names;
        io::WriteCSV(t, path, o);
      },
      py::arg("table"), py::arg("path"), py::arg("delimiter") = ",",
      py::arg("column_names") = std::vector<std::string>{}, rel);

  // ---- C25 native Parquet I/O (Arrow / Parquet C++ from pyarrow's libraries)
  m.def(
      "read_parquet",
      [](const std::shared_ptr<CylonContext> &ctx, const std::vector<std::string> &paths,
         const std::vector<std::string> &columns, bool use_threads, bool concurrent_file_reads) {
        io::ParquetOptions o;
        o.columns = columns;
        o.use_threads = use_threads;
        o.concurrent_file_reads = concurrent_file_reads;
        return io::ReadParquets(ctx, paths, o);
      },
      py::arg("ctx"), py::arg("paths"), py::arg("columns") = std::vector<std::string>{},
      py::arg("use_threads") = true, py::arg("concurrent_file_reads") = true, rel);
  m.def(
      "write_parquet",
      [](const TablePtr &t, const std::string &path, const std::string &compression, int64_t chunk_size) {
        io::ParquetOptions o;
        o.compression = compression;
        o.chunk_size = chunk_size;
        io::WriteParquet(t, path, o);
      },
      py::arg("table"), py::arg("path"), py::arg("compression") = "snappy", py::arg("chunk_size") = 1 << 20, rel);

  py::enum_<AggOp>(m, "AggregationOp")
      .value("SUM", AGG_SUM).value("MIN", AGG_MIN).value("MAX", AGG_MAX).value("COUNT", AGG_COUNT)
      .value("MEAN", AGG_MEAN).value("VAR", AGG_VAR).value("NUNIQUE", AGG_NUNIQUE)
      .value("QUANTILE", AGG_QUANTILE).value("STDDEV", AGG_STDDEV);

  m.def("union", &ops::Union, rel);
  m.def("subtract", &ops::Subtract, rel);
  m.def("intersect", &ops::Intersect, rel);
  m.def("distributed_union", &ops::DistributedUnion, rel);
  m.def("distributed_subtract", &ops::DistributedSubtract, rel);
  m.def("distributed_intersect", &ops::DistributedIntersect, rel);
  m.def("unique", &ops::Unique, rel);
  m.def("distributed_unique", &ops::DistributedUnique, rel);

  m.def("group_ids", [](const TablePtr &t, const std::vector<int> &cols, bool presorted) {
    auto g = ops::GroupIds(t, cols, presorted);
    return std::make_tuple(g.gid, g.ngroups, g.first_rows);
  }, py::call_guard<py::gil_scoped_release>());

  auto groupby_fn = [](TablePtr (*fn)(const TablePtr &, const std::vector<int> &, const std::vector<ops::AggSpec> &)) {
    return [fn](const TablePtr &t, const std::vector<int> &keys, const std::vector<int> &cols,
                const std::vector<int> &op_ids, const std::vector<double> &qs, const std::vector<int> &ddofs) {
      return fn(t, keys, make_specs(cols, op_ids, qs, ddofs));
    };
  };
  m.def("hash_groupby", groupby_fn(&ops::HashGroupBy), py::call_guard<py::gil_scoped_release>());
  m.def("pipeline_groupby", groupby_fn(&ops::PipelineGroupBy), py::call_guard<py::gil_scoped_release>());
  m.def("distributed_hash_groupby", groupby_fn(&ops::DistributedHashGroupBy), py::call_guard<py::gil_scoped_release>());
  m.def("distributed_pipeline_groupby", groupby_fn(&ops::DistributedPipelineGroupBy), py::call_guard<py::gil_scoped_release>());

  m.def("aggregate", &ops::Aggregate, py::arg("table"), py::arg("col"), py::arg("op"), py::arg("quantile") = 0.5,
        py::arg("ddof") = 1, py::arg("distributed") = true, rel);

  m.def(
      "distributed_sort",
      [](const TablePtr &t, const std::vector<int> &cols, const std::vector<bool> &asc, uint32_t num_bins,
         uint64_t num_samples) {
        SortOptions o;
        o.num_bins = num_bins;
        o.num_samples = num_samples;
        return ops::DistributedSort(t, cols, asc, o);
      },
      rel);
  m.def("topk", &ops::TopK, py::arg("table"), py::arg("cols"), py::arg("ascending"), py::arg("k"), rel);
  m.def("distributed_topk", &ops::DistributedTopK, py::arg("table"), py::arg("cols"), py::arg("ascending"),
        py::arg("k"), rel);
  // Window functions, one entry point per level (window_specs above); each accepts the functions of the
  // levels before it too.  args: LAG / LEAD offsets, and k of NTH_VALUE and NTILE.
  using Ints = std::vector<int>;
  using Names = std::vector<std::string>;
  using Doubles = std::vector<double>;
  using Bools = std::vector<bool>;
  const py::arg funcs("funcs"), cols("cols"), args("args"), names("names"), preceding("preceding"),
      following("following"), preceding_f("preceding_f"), following_f("following_f"),
      offset_is_float("offset_is_float"), min_periods("min_periods"), ignore_nulls("ignore_nulls"), limit("limit"),
      ddof("ddof");
  def_window<Ints, Ints, I64List, Names>(m, "window", WIN_LEAD, funcs, cols, args, names);
  // ROLLING functions: a ROWS frame per spec (rows before and after the current one, >= the table's rows
  // meaning unbounded) and min_periods
  def_window<Ints, Ints, I64List, Names, I64List, I64List, I64List>(m, "window_frames", WIN_ROLLING_MAX, funcs, cols,
                                                                    args, names, preceding, following, min_periods);
  // RANGE functions: preceding / following are then distances in the order column's values, INT64_MAX
  // meaning unbounded; where offset_is_float[i], a side that is not unbounded reads preceding_f[i] /
  // following_f[i] instead
  def_window<Ints, Ints, I64List, Names, I64List, I64List, Doubles, Doubles, Bools, I64List>(
      m, "window_range_frames", WIN_RANGE_MAX, funcs, cols, args, names, preceding, following, preceding_f, following_f,
      offset_is_float, min_periods);
  // navigation and distribution functions: ignore_nulls[i] for FIRST_VALUE / LAST_VALUE, limit[i] (0: none)
  // for FFILL / BFILL
  def_window<Ints, Ints, I64List, Names, I64List, I64List, Doubles, Doubles, Bools, I64List, Bools, I64List>(
      m, "window_nav", WIN_CUME_DIST, funcs, cols, args, names, preceding, following, preceding_f, following_f,
      offset_is_float, min_periods, ignore_nulls, limit);
  // VAR / STD over ROWS and RANGE frames: ddof[i]; they read their frame as ROLLING_MEAN resp. RANGE_MEAN do
  def_window<Ints, Ints, I64List, Names, I64List, I64List, Doubles, Doubles, Bools, I64List, Bools, I64List, Ints>(
      m, "window_moment_frames", WIN_RANGE_STD, funcs, cols, args, names, preceding, following, preceding_f,
      following_f, offset_is_float, min_periods, ignore_nulls, limit, ddof);
  // as-of join: tolerance = None, an int (integer / temporal `on`) or a float (float `on`)
  auto asof_options = [](int direction, bool allow_exact, const py::object &tolerance, const std::string &left_prefix,
                         const std::string &right_prefix) {
    AsofOptions o;
    o.direction = direction;
    o.allow_exact_matches = allow_exact;
    if (!tolerance.is_none()) {
      CYLON_CHECK(!py::isinstance<py::bool_>(tolerance) &&
                      (py::isinstance<py::int_>(tolerance) || py::isinstance<py::float_>(tolerance)),
                  Code::Invalid, "asof join: tolerance must be an int or a float");
      o.has_tolerance = true;
      o.tolerance_is_float = py::isinstance<py::float_>(tolerance);
      if (o.tolerance_is_float) o.tolerance_f = tolerance.cast<double>();
      else o.tolerance_i = tolerance.cast<int64_t>();
    }
    o.left_prefix = left_prefix;
    o.right_prefix = right_prefix;
    return o;
  };
  m.def(
      "asof_join",
      [asof_options](const TablePtr &l, const TablePtr &r, int left_on, int right_on, const std::vector<int> &left_by,
                     const std::vector<int> &right_by, int direction, bool allow_exact, const py::object &tolerance,
                     const std::string &left_prefix, const std::string &right_prefix, int64_t carry_step_tiles) {
        const AsofOptions o = asof_options(direction, allow_exact, tolerance, left_prefix, right_prefix);
        py::gil_scoped_release nogil;
        return ops::AsofJoin(l, r, left_on, right_on, left_by, right_by, o, carry_step_tiles);
      },
      py::arg("left"), py::arg("right"), py::arg("left_on"), py::arg("right_on"), py::arg("left_by"),
      py::arg("right_by"), py::arg("direction") = 0, py::arg("allow_exact_matches") = true,
      py::arg("tolerance") = py::none(), py::arg("left_prefix") = "", py::arg("right_prefix") = "",
      py::arg("carry_step_tiles") = 0);
  m.def(
      "distributed_asof_join",
      [asof_options](const TablePtr &l, const TablePtr &r, int left_on, int right_on, const std::vector<int> &left_by,
                     const std::vector<int> &right_by, int direction, bool allow_exact, const py::object &tolerance,
                     const std::string &left_prefix, const std::string &right_prefix) {
        const AsofOptions o = asof_options(direction, allow_exact, tolerance, left_prefix, right_prefix);
        py::gil_scoped_release nogil;
        return ops::DistributedAsofJoin(l, r, left_on, right_on, left_by, right_by, o);
      },
      py::arg("left"), py::arg("right"), py::arg("left_on"), py::arg("right_on"), py::arg("left_by"),
      py::arg("right_by"), py::arg("direction") = 0, py::arg("allow_exact_matches") = true,
      py::arg("tolerance") = py::none(), py::arg("left_prefix") = "", py::arg("right_prefix") = "");
  // the right row of every left row (-1: none): AsofJoin is left ++ GatherNullable(right, that, true)
  m.def(
      "asof_join_indices",
      [asof_options](const TablePtr &l, const TablePtr &r, int left_on, int right_on, const std::vector<int> &left_by,
                     const std::vector<int> &right_by, int direction, bool allow_exact, const py::object &tolerance,
                     int64_t carry_step_tiles) {
        const AsofOptions o = asof_options(direction, allow_exact, tolerance, "", "");
        py::gil_scoped_release nogil;
        return ops::AsofJoinIndices(l, r, left_on, right_on, left_by, right_by, o, carry_step_tiles);
      },
      py::arg("left"), py::arg("right"), py::arg("left_on"), py::arg("right_on"), py::arg("left_by"),
      py::arg("right_by"), py::arg("direction") = 0, py::arg("allow_exact_matches") = true,
      py::arg("tolerance") = py::none(), py::arg("carry_step_tiles") = 0);
  // interval join: closed 0 BOTH / 1 LEFT / 2 RIGHT / 3 NEITHER, how 0 INNER / 1 LEFT
  auto interval_options = [](int closed, int how, const std::string &left_prefix, const std::string &right_prefix) {
    IntervalOptions o;
    o.closed = closed;
    o.how = how;
    o.left_prefix = left_prefix;
    o.right_prefix = right_prefix;
    return o;
  };
  m.def(
      "interval_join",
      [interval_options](const TablePtr &l, const TablePtr &r, int left_lower, int left_upper, int right_on,
                         const std::vector<int> &left_by, const std::vector<int> &right_by, int closed, int how,
                         const std::string &left_prefix, const std::string &right_prefix, int64_t carry_step_tiles) {
        const IntervalOptions o = interval_options(closed, how, left_prefix, right_prefix);
        py::gil_scoped_release nogil;
        return ops::IntervalJoin(l, r, left_lower, left_upper, right_on, left_by, right_by, o, carry_step_tiles);
      },
      py::arg("left"), py::arg("right"), py::arg("left_lower"), py::arg("left_upper"), py::arg("right_on"),
      py::arg("left_by"), py::arg("right_by"), py::arg("closed") = 0, py::arg("how") = 0,
      py::arg("left_prefix") = "", py::arg("right_prefix") = "", py::arg("carry_step_tiles") = 0);
  m.def(
      "distributed_interval_join",
      [interval_options](const TablePtr &l, const TablePtr &r, int left_lower, int left_upper, int right_on,
                         const std::vector<int> &left_by, const std::vector<int> &right_by, int closed, int how,
                         const std::string &left_prefix, const std::string &right_prefix) {
        const IntervalOptions o = interval_options(closed, how, left_prefix, right_prefix);
        py::gil_scoped_release nogil;
        return ops::DistributedIntervalJoin(l, r, left_lower, left_upper, right_on, left_by, right_by, o);
      },
      py::arg("left"), py::arg("right"), py::arg("left_lower"), py::arg("left_upper"), py::arg("right_on"),
      py::arg("left_by"), py::arg("right_by"), py::arg("closed") = 0, py::arg("how") = 0,
      py::arg("left_prefix") = "", py::arg("right_prefix") = "");
  // (li, ri): the pairs in the specified order, ri = -1 for the filler of a LEFT join:
  // IntervalJoin is Gather(left, li) ++ GatherNullable(right, ri, how == LEFT)
  m.def(
      "interval_join_indices",
      [interval_options](const TablePtr &l, const TablePtr &r, int left_lower, int left_upper, int right_on,
                         const std::vector<int> &left_by, const std::vector<int> &right_by, int closed, int how,
                         int64_t carry_step_tiles) {
        const IntervalOptions o = interval_options(closed, how, "", "");
        py::gil_scoped_release nogil;
        return ops::IntervalJoinIndices(l, r, left_lower, left_upper, right_on, left_by, right_by, o, carry_step_tiles);
      },
      py::arg("left"), py::arg("right"), py::arg("left_lower"), py::arg("left_upper"), py::arg("right_on"),
      py::arg("left_by"), py::arg("right_by"), py::arg("closed") = 0, py::arg("how") = 0,
      py::arg("carry_step_tiles") = 0);
  // the matches of every left row: the sort and the rank pass only
  m.def(
      "interval_join_counts",
      [interval_options](const TablePtr &l, const TablePtr &r, int left_lower, int left_upper, int right_on,
                         const std::vector<int> &left_by, const std::vector<int> &right_by, int closed,
                         int64_t carry_step_tiles) {
        const IntervalOptions o = interval_options(closed, 0, "", "");
        py::gil_scoped_release nogil;
        return ops::IntervalJoinCounts(l, r, left_lower, left_upper, right_on, left_by, right_by, o, carry_step_tiles);
      },
      py::arg("left"), py::arg("right"), py::arg("left_lower"), py::arg("left_upper"), py::arg("right_on"),
      py::arg("left_by"), py::arg("right_by"), py::arg("closed") = 0, py::arg("carry_step_tiles") = 0);
  // output rows per tile of the interval join's expansion (kernels/interval.hip); the CPU twin reports the same
  m.def("interval_tile_rows", []() { return hip::interval_tile_rows(); });
  // rows per tile of the window scans and tiles per step of their carry scan (kernels/window.hip); the
  // CPU twin is one sequential loop and reports the same numbers
  m.def("window_tile_rows", []() { return hip::window_tile_rows(); });
  m.def("window_carry_tiles", []() { return hip::window_carry_tiles(); });
  // the widest frame (preceding + following + 1) that the one-launch LDS kernel of kernels/rolling.hip takes
  m.def("window_frame_lds_rows", []() { return hip::window_frame_lds_rows(); });
  // RANGE frames (kernels/frame_range.hip): entries per block of the scan pyramid, and the keys staged on
  // either side of a tile by the bounds search (a bound further away is found in global memory)
  m.def("window_range_radix", []() { return hip::window_range_radix(); });
  m.def("window_range_halo", []() { return hip::window_range_halo(); });
  // the radix partitions' sizing rules (ops/radix_sizing.hpp): partition bits of `rows` build rows against
  // an LDS capacity, and the slot-mode rows per partition of `rows` rows in `nparts` partitions
  m.def("radix_partition_bits", [](int64_t rows, int64_t cap) { return ops::sizing::partition_bits(rows, cap); });
  m.def("radix_slot_rows",
        [](int64_t rows, int64_t nparts) { return ops::sizing::slot_rows((double)rows / (double)nparts); });
  // ---- streaming op graph (C24) ------------------------------------------
  m.def(
      "dis_join_op",
      [](std::shared_ptr<CylonContext> ctx, const std::vector<TablePtr> &lefts, const std::vector<TablePtr> &rights,
         const std::string &type, const std::string &algo, const std::vector<int> &lc, const std::vector<int> &rc,
         const std::string &lp, const std::string &rp, int num_splits) {
        using namespace join::config;
        const JoinType jt = op_join_type(type);
        const JoinAlgorithm ja = algo == "hash" ? HASH : SORT;
        graph::DisJoinOpConfig cfg{num_splits, JoinConfig(jt, lc, rc, ja, lp, rp)};
        std::vector<TablePtr> out;
        graph::DisJoinOP op(ctx, 0, [&out](int, const TablePtr &t) { out.push_back(t); }, cfg);
        for (const auto &t : lefts) op.InsertTable(graph::DisJoinOP::kLeftTag, t);
        for (const auto &t : rights) op.InsertTable(graph::DisJoinOP::kRightTag, t);
        op.WaitForCompletion();
        return out;
      },
      rel);
  m.def(
      "dis_union_op",
      [](std::shared_ptr<CylonContext> ctx, const std::vector<TablePtr> &tables) {
        std::vector<TablePtr> out;
        graph::DisUnionOp op(ctx, 0, [&out](int, const TablePtr &t) { out.push_back(t); });
        for (const auto &t : tables) op.InsertTable(0, t);
        op.WaitForCompletion();
        return out;
      },
      rel);

  // ---- string-ID registry (reference table_api.hpp) ----------------------------
  m.def("registry_put", &PutTable, py::call_guard<py::gil_scoped_release>());
  m.def("registry_get", &GetTable, py::call_guard<py::gil_scoped_release>());
  m.def("registry_remove", &RemoveTable, py::call_guard<py::gil_scoped_release>());
  m.def("registry_list", &ListTables, py::call_guard<py::gil_scoped_release>());
  m.def("registry_row_count", &RowCount, py::call_guard<py::gil_scoped_release>());
  m.def("registry_column_count", &ColumnCount, py::call_guard<py::gil_scoped_release>());
  m.def(
      "registry_join",
      [](const std::string &l, const std::string &r, const std::string &type, const std::string &algo,
         const std::vector<int> &lc, const std::vector<int> &rc, const std::string &dest, bool distributed) {
        using namespace join::config;
        const JoinType jt = op_join_type(type);
        JoinConfig cfg(jt, lc, rc, algo == "hash" ? HASH : SORT);
        Status s = distributed ? DistributedJoinTables(l, r, cfg, dest) : JoinTables(l, r, cfg, dest);
        return std::make_pair(s.get_code(), s.get_msg());  // converted after the GIL is re-acquired
      },
      rel);
  m.def(
      "registry_union",
      [](const std::string &a, const std::string &b, const std::string &dest, bool distributed) {
        Status s = UnionTables(a, b, dest, distributed);
        return std::make_pair(s.get_code(), s.get_msg());  // converted after the GIL is re-acquired
      },
      rel);

  // ---- all-to-all with the reference's insert/finish/isComplete protocol ----------
  struct A2AHandle {
    std::vector<std::tuple<int, TablePtr, int>> received;
    std::unique_ptr<TableAllToAll> impl;
  };
  py::class_<A2AHandle, std::shared_ptr<A2AHandle>>(m, "TableAllToAll")
      .def(py::init([](std::shared_ptr<CylonContext> ctx) {
        auto h = std::make_shared<A2AHandle>();
        A2AHandle *raw = h.get();
        h->impl = std::make_unique<TableAllToAll>(ctx, [raw](int src, const TablePtr &t, int ref) {
          raw->received.emplace_back(src, t, ref);
          return true;
        });
        return h;
      }), py::call_guard<py::gil_scoped_release>())
      .def("insert", [](A2AHandle &h, const TablePtr &t, int target, int ref) { return h.impl->insert(t, target, ref); },
           py::arg("table"), py::arg("target"), py::arg("reference") = 0, py::call_guard<py::gil_scoped_release>())
      .def("finish", [](A2AHandle &h) { h.impl->finish(); }, py::call_guard<py::gil_scoped_release>())
      .def("is_complete", [](A2AHandle &h) { return h.impl->isComplete(); }, rel)
      .def("close", [](A2AHandle &h) { h.impl->close(); }, py::call_guard<py::gil_scoped_release>())
      .def("received", [](A2AHandle &h) { return h.received; }, py::call_guard<py::gil_scoped_release>());

  m.def("map_to_sort_partitions", &ops::MapToSortPartitions, rel);
  m.def("partition_reorder", &ops::PartitionReorder, rel);
  m.def("shuffle_partition", &ops::ShufflePartition, rel);
  m.def("all_to_all_table", &ops::AllToAllTable, rel);
}
