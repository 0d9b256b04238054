// Host sanitizer check of the CPU twin of the interval join (kernels/cpu_interval.cpp): interval_rank /
// interval_counts / interval_expand driven as ops/interval.cpp drives them -- the three blocks of key
// rows concatenated in the order `closed` asks for, one stable sort, an exclusive scan of the counts --
// over tiny random inputs in exactly-sized heap buffers, against a brute-force double loop.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/interval_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_interval.cpp -o interval_sanitize
//   ./interval_sanitize          # prints "interval_sanitize: ok", exit status 0
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

#include "cylon/kernels/kernels.hpp"
#include "cylon/kernels/order_image.hpp"

namespace {

using namespace cylon;

int failures = 0;

template <typename V>
ColView view_of(const std::vector<V> &v, const std::vector<uint8_t> &valid) {
  ColView c;
  c.data = reinterpret_cast<const uint8_t *>(v.data());
  c.valid = valid.empty() ? nullptr : valid.data();
  c.width = (int32_t)sizeof(V);
  c.kind = static_cast<int>(std::is_floating_point<V>::value ? ValueKind::FLOAT
                            : std::is_signed<V>::value       ? ValueKind::SIGNED_INT
                                                             : ValueKind::UNSIGNED_INT);
  return c;
}

template <typename V>
bool usable(const std::vector<V> &v, const std::vector<uint8_t> &valid, int64_t i) {
  if (!valid.empty() && !valid[(size_t)i]) return false;
  if (std::is_floating_point<V>::value) return !std::isnan((double)v[(size_t)i]);
  return true;
}

template <typename V>
struct Column {
  std::vector<V> v;
  std::vector<uint8_t> valid;
};

template <typename V>
struct Left {
  std::vector<int> g;
  Column<V> lower, upper;
};

template <typename V>
struct Right {
  std::vector<int> g;
  Column<V> on;
};

using Pairs = std::vector<std::pair<int64_t, int64_t>>;

// the definition, by brute force: closed 0 both, 1 left, 2 right, 3 neither; how 0 inner, 1 left
template <typename V>
Pairs brute(const Left<V> &l, const Right<V> &r, int closed, int how) {
  Pairs out;
  for (size_t i = 0; i < l.g.size(); ++i) {
    std::vector<int64_t> own;
    if (usable(l.lower.v, l.lower.valid, (int64_t)i) && usable(l.upper.v, l.upper.valid, (int64_t)i)) {
      const V lo = l.lower.v[i], up = l.upper.v[i];
      for (size_t j = 0; j < r.g.size(); ++j) {
        if (r.g[j] != l.g[i] || !usable(r.on.v, r.on.valid, (int64_t)j)) continue;
        const V y = r.on.v[j];
        const bool above = (closed == 0 || closed == 1) ? lo <= y : lo < y;
        const bool below = (closed == 0 || closed == 2) ? y <= up : y < up;
        if (above && below) own.push_back((int64_t)j);
      }
    }
    std::stable_sort(own.begin(), own.end(), [&](int64_t a, int64_t b) { return r.on.v[(size_t)a] < r.on.v[(size_t)b]; });
    for (int64_t j : own) out.emplace_back((int64_t)i, j);
    if (own.empty() && how == 1) out.emplace_back((int64_t)i, (int64_t)-1);
  }
  return out;
}

// the join as ops/interval.cpp runs it; *matched = the pairs with a right row
template <typename V>
Pairs join(const Left<V> &l, const Right<V> &r, int closed, int how, int64_t *matched, std::vector<int64_t> *counts) {
  const int64_t nl = (int64_t)l.g.size(), nr = (int64_t)r.g.size(), n = nr + 2 * nl;
  int64_t lbase, rbase, ubase;
  switch (closed) {
    case 0: lbase = 0, rbase = nl, ubase = nl + nr; break;
    case 1: lbase = 0, ubase = nl, rbase = 2 * nl; break;
    case 2: rbase = 0, lbase = nr, ubase = nr + nl; break;
    default: ubase = 0, rbase = nl, lbase = nl + nr; break;
  }
  // the concatenated key rows (group, value, validity)
  std::vector<int> g((size_t)n);
  std::vector<V> v((size_t)n);
  std::vector<uint8_t> ok((size_t)n);
  for (int64_t i = 0; i < nl; ++i) {
    g[(size_t)(lbase + i)] = g[(size_t)(ubase + i)] = l.g[(size_t)i];
    v[(size_t)(lbase + i)] = l.lower.v[(size_t)i];
    v[(size_t)(ubase + i)] = l.upper.v[(size_t)i];
    ok[(size_t)(lbase + i)] = l.lower.valid.empty() || l.lower.valid[(size_t)i];
    ok[(size_t)(ubase + i)] = l.upper.valid.empty() || l.upper.valid[(size_t)i];
  }
  for (int64_t j = 0; j < nr; ++j) {
    g[(size_t)(rbase + j)] = r.g[(size_t)j];
    v[(size_t)(rbase + j)] = r.on.v[(size_t)j];
    ok[(size_t)(rbase + j)] = r.on.valid.empty() || r.on.valid[(size_t)j];
  }
  // stable sort by (group, value) with NaN after the numbers and nulls last
  auto cls = [&](int64_t i) { return !ok[(size_t)i] ? 2 : usable(v, ok, i) ? 0 : 1; };
  std::vector<int64_t> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
    if (g[(size_t)x] != g[(size_t)y]) return g[(size_t)x] < g[(size_t)y];
    if (cls(x) != cls(y)) return cls(x) < cls(y);
    return cls(x) == 0 && v[(size_t)x] < v[(size_t)y];
  });
  std::vector<int64_t> lo((size_t)nl, -7), hi((size_t)nl, -7), rrows((size_t)nr, -7), ws(1);
  cpu::interval_rank(perm.data(), nl, nr, lbase, rbase, ubase, 0, ws.data(), lo.data(), hi.data(), rrows.data(), nullptr);
  if (counts != nullptr) {
    counts->assign((size_t)nl, -7);
    cpu::interval_counts(view_of(l.lower.v, l.lower.valid), view_of(l.upper.v, l.upper.valid), lo.data(), hi.data(), nl,
                         false, counts->data(), nullptr, nullptr, nullptr);
  }
  std::vector<int64_t> cnt((size_t)nl, -7), off((size_t)nl + 1, 0);
  std::vector<uint8_t> empty((size_t)(how == 1 ? nl : 0), 7);
  cpu::interval_counts(view_of(l.lower.v, l.lower.valid), view_of(l.upper.v, l.upper.valid), lo.data(), hi.data(), nl,
                       how == 1, cnt.data(), how == 1 ? empty.data() : nullptr, matched, nullptr);
  for (int64_t i = 0; i < nl; ++i) off[(size_t)i + 1] = off[(size_t)i] + cnt[(size_t)i];
  const int64_t total = off[(size_t)nl];
  std::vector<int64_t> li((size_t)total, -7), ri((size_t)total, -7);
  cpu::interval_expand(off.data(), lo.data(), how == 1 ? empty.data() : nullptr, rrows.data(), nl, nr, total, li.data(),
                       ri.data(), nullptr);
  Pairs out;
  for (int64_t o = 0; o < total; ++o) out.emplace_back(li[(size_t)o], ri[(size_t)o]);
  return out;
}

template <typename V>
void one_case(std::mt19937_64 &rng, int64_t nl, int64_t nr, int groups, bool nulls) {
  auto column = [&](int64_t n, int shift) {
    Column<V> c;
    for (int64_t i = 0; i < n; ++i) {
      V v = (V)((int64_t)(rng() % 23) + shift - (std::is_signed<V>::value || std::is_floating_point<V>::value ? 11 : 0));
      if (std::is_floating_point<V>::value) {
        v = v / (V)2;
        if (rng() % 11 == 0) v = std::numeric_limits<V>::quiet_NaN();
        if (rng() % 13 == 0) v = (V)-0.0;
        if (rng() % 17 == 0) v = rng() % 2 ? std::numeric_limits<V>::infinity() : -std::numeric_limits<V>::infinity();
      } else if (rng() % 17 == 0) {
        v = rng() % 2 ? std::numeric_limits<V>::max() : std::numeric_limits<V>::lowest();
      }
      c.v.push_back(v);
      if (nulls) c.valid.push_back(rng() % 5 != 0);
    }
    return c;
  };
  Left<V> l;
  Right<V> r;
  for (int64_t i = 0; i < nl; ++i) l.g.push_back((int)(rng() % (uint64_t)groups));
  for (int64_t j = 0; j < nr; ++j) r.g.push_back((int)(rng() % (uint64_t)groups));
  l.lower = column(nl, 0);
  l.upper = column(nl, 4);
  r.on = column(nr, 2);
  for (int closed = 0; closed < 4; ++closed)
    for (int how = 0; how < 2; ++how) {
      const Pairs want = brute(l, r, closed, how);
      int64_t matched = 0;
      std::vector<int64_t> counts, want_counts((size_t)nl, 0);
      const Pairs got = join(l, r, closed, how, &matched, &counts);
      int64_t hits = 0;
      for (const auto &p : want)
        if (p.second >= 0) {
          ++hits;
          ++want_counts[(size_t)p.first];
        }
      if (got != want || matched != hits || counts != want_counts) {
        if (++failures <= 10)
          std::fprintf(stderr, "interval_sanitize: differs (nl %lld, nr %lld, width %d, float %d, closed %d, how %d)\n",
                       (long long)nl, (long long)nr, (int)sizeof(V), (int)std::is_floating_point<V>::value, closed, how);
      }
    }
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  const int64_t sizes[] = {1, 2, 7, 64, 200};  // an empty side never reaches the kernels (ops/interval.cpp)
  for (int64_t nl : sizes)
    for (int64_t nr : sizes)
      for (int groups : {1, 3})
        for (int nulls = 0; nulls < 2; ++nulls) {
          one_case<int8_t>(rng, nl, nr, groups, nulls != 0);
          one_case<uint16_t>(rng, nl, nr, groups, nulls != 0);
          one_case<int32_t>(rng, nl, nr, groups, nulls != 0);
          one_case<int64_t>(rng, nl, nr, groups, nulls != 0);
          one_case<uint64_t>(rng, nl, nr, groups, nulls != 0);
          one_case<float>(rng, nl, nr, groups, nulls != 0);
          one_case<double>(rng, nl, nr, groups, nulls != 0);
        }
  if (failures) {
    std::fprintf(stderr, "interval_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("interval_sanitize: ok\n");
  return 0;
}
