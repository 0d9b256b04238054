// Host sanitizer check of the CPU twin of the as-of join's scan (kernels/cpu_asof.cpp, with
// window_rev_flags of cpu_rolling.cpp for the reversed order): asof_tile / asof_apply / asof_pick driven
// as ops/asof.cpp drives them, over tiny random inputs in exactly-sized heap buffers, against a
// brute-force loop over all right rows.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/asof_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_asof.cpp \
//       cylon_amd/csrc/cylon/kernels/cpu_rolling.cpp cylon_amd/csrc/cylon/kernels/cpu_window.cpp -o asof_sanitize
//   ./asof_sanitize          # prints "asof_sanitize: ok", exit status 0
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <type_traits>
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

// |a - b|: exact for the integers (in unsigned __int128), one subtraction for the floats
template <typename V>
long double distance(V a, V b) {
  if (std::is_floating_point<V>::value) return a == b ? 0.0L : (long double)std::fabs((double)a - (double)b);
  const __int128 d = (__int128)a - (__int128)b;
  return (long double)(d < 0 ? -d : d);
}

template <typename V>
struct Side {
  std::vector<int> g;
  std::vector<V> on;
  std::vector<uint8_t> valid;
};

// the definition, by brute force: direction 0 backward, 1 forward, 2 nearest
template <typename V>
std::vector<int64_t> brute(const Side<V> &l, const Side<V> &r, int direction, bool exact, bool has_tol, long double tol) {
  std::vector<int64_t> out(l.g.size(), -1);
  for (size_t i = 0; i < l.g.size(); ++i) {
    if (!usable(l.on, l.valid, (int64_t)i)) continue;
    const V x = l.on[i];
    int64_t b = -1, f = -1;
    for (size_t j = 0; j < r.g.size(); ++j) {
      if (r.g[j] != l.g[i] || !usable(r.on, r.valid, (int64_t)j)) continue;
      const V y = r.on[j];
      if ((exact ? y <= x : y < x) && (b < 0 || y >= r.on[(size_t)b])) b = (int64_t)j;  // ties: the highest row
      if ((exact ? y >= x : y > x) && (f < 0 || y < r.on[(size_t)f])) f = (int64_t)j;   // ties: the lowest row
    }
    int64_t m = direction == 0 ? b : direction == 1 ? f : b;
    if (direction == 2 && f >= 0 && (b < 0 || distance(x, r.on[(size_t)f]) < distance(x, r.on[(size_t)b]))) m = f;
    if (m >= 0 && has_tol && distance(x, r.on[(size_t)m]) > tol) m = -1;
    out[i] = m;
  }
  return out;
}

// one scan as ops/asof.cpp runs it: concatenate, stable sort by (group, on) with NaN after the numbers
// and nulls last, heads, asof_tile, asof_apply
template <typename V>
std::vector<int64_t> scan(const Side<V> &l, const Side<V> &r, bool right_first, bool reverse, int64_t *matched) {
  const Side<V> &a = right_first ? r : l, &b = right_first ? l : r;
  const int64_t nfirst = (int64_t)a.g.size(), n = nfirst + (int64_t)b.g.size(), nl = (int64_t)l.g.size();
  Side<V> k = a;
  k.g.insert(k.g.end(), b.g.begin(), b.g.end());
  k.on.insert(k.on.end(), b.on.begin(), b.on.end());
  if (!a.valid.empty() || !b.valid.empty()) {
    k.valid.assign((size_t)nfirst, 1);
    if (!a.valid.empty()) k.valid = a.valid;
    k.valid.resize((size_t)n, 1);
    if (!b.valid.empty()) std::copy(b.valid.begin(), b.valid.end(), k.valid.begin() + nfirst);
  }
  auto cls = [&](int64_t i) { return (!k.valid.empty() && !k.valid[(size_t)i]) ? 2 : usable(k.on, k.valid, i) ? 0 : 1; };
  std::vector<int64_t> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
    if (k.g[(size_t)x] != k.g[(size_t)y]) return k.g[(size_t)x] < k.g[(size_t)y];
    if (cls(x) != cls(y)) return cls(x) < cls(y);
    return cls(x) == 0 && k.on[(size_t)x] < k.on[(size_t)y];
  });
  std::vector<uint8_t> heads((size_t)n), rheads((size_t)n), code((size_t)n);
  for (int64_t i = 0; i < n; ++i) heads[(size_t)i] = i == 0 || k.g[(size_t)perm[(size_t)i]] != k.g[(size_t)perm[(size_t)i - 1]];
  cpu::window_rev_flags(heads.data(), n, rheads.data(), nullptr);
  const uint8_t *restarts = reverse ? rheads.data() : heads.data();
  std::vector<int64_t> match((size_t)nl, -7);
  const ColView on = view_of(k.on, k.valid);
  cpu::asof_tile(on, perm.data(), restarts, n, nfirst, right_first, reverse, code.data(), nullptr, nullptr, nullptr);
  cpu::asof_apply(perm.data(), restarts, code.data(), n, nfirst, right_first, reverse, nullptr, match.data(), matched,
                  nullptr);
  return match;
}

template <typename V>
void one_case(std::mt19937_64 &rng, int64_t nl, int64_t nr, int groups, bool nulls) {
  auto side = [&](int64_t n) {
    Side<V> s;
    for (int64_t i = 0; i < n; ++i) {
      s.g.push_back((int)(rng() % (uint64_t)groups));
      V v = (V)((int64_t)(rng() % 23) - (std::is_signed<V>::value || std::is_floating_point<V>::value ? 11 : 0));
      if (std::is_floating_point<V>::value) {
        v = v / (V)2;
        if (rng() % 11 == 0) v = std::numeric_limits<V>::quiet_NaN();
        if (rng() % 13 == 0) v = (V)-0.0;
      } else if (rng() % 17 == 0) {
        v = rng() % 2 ? std::numeric_limits<V>::max() : std::numeric_limits<V>::lowest();
      }
      s.on.push_back(v);
      if (nulls) s.valid.push_back(rng() % 5 != 0);
    }
    return s;
  };
  const Side<V> l = side(nl), r = side(nr);
  const bool isf = std::is_floating_point<V>::value;
  for (int direction = 0; direction < 3; ++direction)
    for (int exact = 0; exact < 2; ++exact)
      for (int has_tol = 0; has_tol < 2; ++has_tol) {
        const int64_t tol_i = (int64_t)(rng() % 6);
        const double tol_f = (double)(rng() % 6) / 2;
        const std::vector<int64_t> want = brute(l, r, direction, exact != 0, has_tol != 0, isf ? (long double)tol_f : (long double)tol_i);
        const bool nearest = direction == 2, pick = nearest || has_tol;
        int64_t matched = 0;
        std::vector<int64_t> back, fwd;
        if (direction != 1) back = scan(l, r, exact != 0, false, pick ? nullptr : &matched);
        if (direction != 0) fwd = scan(l, r, nearest ? true : !exact, true, pick ? nullptr : &matched);
        std::vector<int64_t> &got = direction == 1 ? fwd : back;
        if (pick && nl > 0 && nr > 0)  // no right rows: every scan result is already -1, as in ops/asof.cpp
          cpu::asof_pick(view_of(l.on, l.valid), view_of(r.on, r.valid), nl, got.data(), nearest ? fwd.data() : nullptr,
                         has_tol != 0, tol_i, tol_f, got.data(), &matched, nullptr);
        const int64_t hits = (int64_t)std::count_if(want.begin(), want.end(), [](int64_t m) { return m >= 0; });
        if (got != want || matched != hits) {
          if (++failures <= 10)
            std::fprintf(stderr, "asof_sanitize: differs (nl %lld, nr %lld, width %d, direction %d, exact %d, tolerance %d)\n",
                         (long long)nl, (long long)nr, (int)sizeof(V), direction, exact, has_tol);
        }
      }
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  const int64_t sizes[] = {0, 1, 2, 7, 64, 200};
  for (int64_t nl : sizes)
    for (int64_t nr : sizes)
      for (int groups : {1, 3}) {
        if (nl == 0 && nr == 0) continue;
        for (int nulls = 0; nulls < 2; ++nulls) {
          one_case<int8_t>(rng, nl, nr, groups, nulls != 0);
          one_case<uint16_t>(rng, nl, nr, groups, nulls != 0);
          one_case<int32_t>(rng, nl, nr, groups, nulls != 0);
          one_case<int64_t>(rng, nl, nr, groups, nulls != 0);
          one_case<uint64_t>(rng, nl, nr, groups, nulls != 0);
          one_case<float>(rng, nl, nr, groups, nulls != 0);
          one_case<double>(rng, nl, nr, groups, nulls != 0);
        }
      }
  if (failures) {
    std::fprintf(stderr, "asof_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("asof_sanitize: ok\n");
  return 0;
}
