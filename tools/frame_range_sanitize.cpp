// Host sanitizer check of the CPU twin of the RANGE frames (kernels/cpu_frame_range.cpp), driven as
// ops/window.cpp drives it -- the flags, the gathers and the two rank scans of cpu_window.cpp, then
// frame_range_keys / frame_range_bounds / frame_range_pyramid / frame_range_apply -- over small inputs in
// exactly-sized heap buffers (the pyramid's too: frame_range_common.hpp's slot counts), against a
// brute-force walk that tests every row of the partition against the frame's definition.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/frame_range_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_frame_range.cpp \
//       cylon_amd/csrc/cylon/kernels/cpu_window.cpp cylon_amd/csrc/cylon/kernels/cpu_rolling.cpp \
//       -o frame_range_sanitize
//   ./frame_range_sanitize      # prints "frame_range_sanitize: ok", exit status 0
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "cylon/kernels/frame_range_common.hpp"
#include "cylon/kernels/kernels.hpp"

namespace {

using namespace cylon;

int failures = 0;

void expect(bool ok, const char *what, int64_t n, int func, double p, double f) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "frame_range_sanitize: %s differs (n = %lld, func %d, frame %g, %g)\n", what, (long long)n,
                 func, p, f);
}

constexpr int kSumI = 0, kSumF = 1, kMin = 2, kMax = 3, kCount = 4, kRank = 5;
constexpr double kNone = -1;  // an unbounded side

// K = int64_t or double order keys (a NaN double key is a NaN row), V = int32_t or double values
// (integer-valued: every summation order is exact)
template <typename K, typename V>
void run_case(const std::vector<int> &g, const std::vector<K> &key, const std::vector<uint8_t> &kvalid,
              const std::vector<V> &v, const std::vector<uint8_t> &valid, bool asc, double pre, double fol,
              int64_t minp) {
  const int64_t n = (int64_t)g.size();
  const bool fkey = std::is_floating_point<K>::value, fval = std::is_floating_point<V>::value;
  auto cls = [&](int64_t r) {
    if (!kvalid.empty() && !kvalid[r]) return 2;
    return (fkey && key[r] != key[r]) ? 1 : 0;
  };
  // the order: partition, then (class, key in the direction), stable
  std::vector<int64_t> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
    if (g[a] != g[b]) return g[a] < g[b];
    if (cls(a) != cls(b)) return cls(a) < cls(b);
    if (cls(a) != 0 || key[a] == key[b]) return false;
    return asc ? key[a] < key[b] : key[a] > key[b];
  });
  std::vector<uint8_t> part((size_t)n), flags((size_t)n), rflags((size_t)n);
  for (int64_t i = 0; i < n; ++i) part[i] = i == 0 || g[perm[i]] != g[perm[i - 1]];
  cpu::window_flags(part.data(), nullptr, n, flags.data(), nullptr);
  const int64_t T = cpu::window_tile_rows(), ntiles = (n + T - 1) / T;
  std::vector<int64_t> tagg3((size_t)(3 * ntiles)), carry3((size_t)(3 * ntiles)), phead((size_t)n), rtail((size_t)n);
  std::vector<uint8_t> tflag((size_t)ntiles);
  cpu::window_rank_tile(flags.data(), n, tagg3.data(), tflag.data(), nullptr);
  cpu::window_carry(tagg3.data(), tflag.data(), ntiles, 3, kRank, 0, carry3.data(), nullptr);
  cpu::window_rank_apply(perm.data(), flags.data(), n, carry3.data(), nullptr, nullptr, nullptr, phead.data(), nullptr);
  cpu::window_rev_flags(flags.data(), n, rflags.data(), nullptr);
  cpu::window_rank_tile(rflags.data(), n, tagg3.data(), tflag.data(), nullptr);
  cpu::window_carry(tagg3.data(), tflag.data(), ntiles, 3, kRank, 0, carry3.data(), nullptr);
  cpu::window_rank_apply(perm.data(), rflags.data(), n, carry3.data(), nullptr, nullptr, nullptr, rtail.data(), nullptr);

  auto view = [](const void *data, const std::vector<uint8_t> &val, size_t width, bool is_float) {
    ColView c;
    c.data = reinterpret_cast<const uint8_t *>(data);
    c.valid = val.empty() ? nullptr : val.data();
    c.width = (int32_t)width;
    c.kind = static_cast<int>(is_float ? ValueKind::FLOAT : ValueKind::SIGNED_INT);
    return c;
  };
  const ColView kc = view(key.data(), kvalid, sizeof(K), fkey), vc = view(v.data(), valid, sizeof(V), fval);
  std::vector<int64_t> tagg((size_t)ntiles);
  std::vector<uint64_t> kdense((size_t)n), dense((size_t)n), keys((size_t)n);
  std::vector<uint8_t> kdvalid(kvalid.empty() ? 0 : (size_t)n), dvalid(valid.empty() ? 0 : (size_t)n), kcls((size_t)n);
  uint8_t *kdv = kdvalid.empty() ? nullptr : kdvalid.data(), *dv = dvalid.empty() ? nullptr : dvalid.data();
  cpu::window_tile(kc, perm.data(), flags.data(), n, kCount, kdense.data(), kdv, true, tagg.data(), tflag.data(), nullptr);
  cpu::window_tile(vc, perm.data(), flags.data(), n, kCount, dense.data(), dv, true, tagg.data(), tflag.data(), nullptr);
  cpu::frame_range_keys(kc, kdense.data(), kdv, n, !asc, keys.data(), kcls.data(), nullptr);
  std::vector<uint32_t> lo((size_t)n), hi((size_t)n);
  const int bounded = fkey ? FR_FLOAT : FR_INT;
  const bool pu = pre == kNone, fu = fol == kNone;
  cpu::frame_range_bounds(keys.data(), kcls.data(), phead.data(), rtail.data(), n, fkey, !asc,
                          pu ? FR_UNBOUNDED : bounded, fkey || pu ? 0 : (uint64_t)pre, fkey && !pu ? pre : 0,
                          fu ? FR_UNBOUNDED : bounded, fkey || fu ? 0 : (uint64_t)fol, fkey && !fu ? fol : 0, lo.data(),
                          hi.data(), nullptr);

  // brute force, per sorted position: every row of the partition against the definition
  std::vector<int64_t> want_cnt((size_t)n);
  std::vector<double> want_sum((size_t)n), want_min((size_t)n), want_max((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t head = i, tail = i;
    while (head > 0 && !part[head]) --head;
    while (tail + 1 < n && !part[tail + 1]) ++tail;
    const int64_t ri = perm[i];
    const int ci = cls(ri);
    int64_t m = 0;
    double s = 0, mn = 0, mx = 0;
    for (int64_t j = head; j <= tail; ++j) {
      const int64_t rj = perm[j];
      bool in;
      if (j == i) {
        in = true;
      } else if (j < i ? pre == kNone : fol == kNone) {
        in = true;  // positional
      } else if (ci != 0 || cls(rj) != 0) {
        in = ci == cls(rj);
      } else if (fkey) {
        // ascending: o_i - a <= o_j <= o_i + b; descending: o_i + a >= o_j >= o_i - b
        double first = asc ? (double)key[ri] - pre : (double)key[ri] + pre;
        double last = asc ? (double)key[ri] + fol : (double)key[ri] - fol;
        if (first != first) first = (double)key[ri];
        if (last != last) last = (double)key[ri];
        const double o = (double)key[rj];
        in = j < i ? (asc ? o >= first : o <= first) : (asc ? o <= last : o >= last);
      } else {
        const __int128 oi = (__int128)key[ri], oj = (__int128)key[rj];
        const __int128 a = (__int128)pre, b = (__int128)fol;
        in = j < i ? (asc ? oj >= oi - a : oj <= oi + a) : (asc ? oj <= oi + b : oj >= oi - b);
      }
      if (!in) continue;
      expect(j >= lo[i] && j <= hi[i], "frame (row missing)", n, -1, pre, fol);
      if (!valid.empty() && !valid[rj]) continue;
      const double x = (double)v[rj];
      s += x;
      mn = m ? std::min(mn, x) : x;
      mx = m ? std::max(mx, x) : x;
      ++m;
    }
    expect(lo[i] >= head && lo[i] <= i && hi[i] >= i && hi[i] <= tail, "bounds", n, -1, pre, fol);
    want_cnt[i] = m;
    want_sum[i] = s;
    want_min[i] = mn;
    want_max[i] = mx;
  }

  const int sum = fval ? kSumF : kSumI;
  std::vector<uint64_t> cP((size_t)fr_ps_slots(n)), cS((size_t)fr_ps_slots(n)), cE((size_t)fr_e_slots(n));
  if (dv != nullptr) cpu::frame_range_pyramid(vc, n, kCount, dense.data(), dv, cP.data(), cS.data(), cE.data(), nullptr);
  struct Plan {
    int func;
    bool mean;
  };
  for (const Plan pl : {Plan{kCount, false}, Plan{sum, false}, Plan{sum, true}, Plan{kMin, false}, Plan{kMax, false}}) {
    const size_t ow = (pl.func == kMin || pl.func == kMax) ? sizeof(V) : 8;
    std::vector<uint64_t> P((size_t)fr_ps_slots(n)), S((size_t)fr_ps_slots(n)), E((size_t)fr_e_slots(n));
    cpu::frame_range_pyramid(vc, n, pl.func, dense.data(), dv, P.data(), S.data(), E.data(), nullptr);
    std::vector<uint8_t> out((size_t)n * ow), ovalid(pl.func == kCount ? 0 : (size_t)n);
    uint8_t *ov = ovalid.empty() ? nullptr : ovalid.data();
    cpu::frame_range_apply(vc, perm.data(), n, pl.func, pl.mean, pl.func == kCount ? 0 : minp, dense.data(), dv,
                           lo.data(), hi.data(), P.data(), S.data(), E.data(), dv ? cP.data() : nullptr,
                           dv ? cS.data() : nullptr, dv ? cE.data() : nullptr, out.data(), ov, nullptr);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = perm[i];
      if (pl.func == kCount) {
        int64_t got;
        std::memcpy(&got, out.data() + r * 8, 8);
        expect(got == want_cnt[i], "count", n, pl.func, pre, fol);
        continue;
      }
      const bool live = want_cnt[i] >= minp;
      expect((ovalid[r] != 0) == live, "validity", n, pl.func, pre, fol);
      if (!live) continue;
      double got;
      if (pl.func == kMin || pl.func == kMax) {
        V x;
        std::memcpy(&x, out.data() + r * sizeof(V), sizeof(V));
        got = (double)x;
      } else if (pl.mean || fval) {
        std::memcpy(&got, out.data() + r * 8, 8);
      } else {
        int64_t x;
        std::memcpy(&x, out.data() + r * 8, 8);
        got = (double)x;
      }
      const double want = pl.func == kMin ? want_min[i] : pl.func == kMax ? want_max[i]
                          : pl.mean ? want_sum[i] / (double)want_cnt[i] : want_sum[i];
      expect(got == want, "result", n, pl.func, pre, fol);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t sizes[] = {1, 2, 7, 8, 9, 33, 64, 65, 100, 513, 600};
  const double int_bounds[] = {kNone, 0, 1, 3, 40, 9e18};
  const double float_bounds[] = {kNone, 0, 0.5, 3, inf};
  for (int64_t n : sizes) {
    for (int groups : {1, 3, (int)n}) {
      for (int nullable = 0; nullable < 2; ++nullable) {
        std::vector<int> g((size_t)n);
        std::vector<int64_t> ki((size_t)n);
        std::vector<double> kd((size_t)n), vd((size_t)n);
        std::vector<int32_t> vi((size_t)n);
        std::vector<uint8_t> valid(nullable ? (size_t)n : 0), kvalid(nullable ? (size_t)n : 0);
        const int64_t spread = 1 + (int64_t)(rng() % (unsigned)(2 * n));
        for (int64_t i = 0; i < n; ++i) {
          g[i] = (int)(rng() % (unsigned)groups);
          const unsigned pick = rng() % 16;
          ki[i] = pick == 0 ? INT64_MIN + (int64_t)(rng() % 3) : pick == 1 ? INT64_MAX - (int64_t)(rng() % 3)
                                                                           : (int64_t)(rng() % spread) - spread / 2;
          kd[i] = pick == 0 ? -inf : pick == 1 ? inf : pick == 2 ? nan : pick == 3 ? -0.0
                                                                                   : (double)((int64_t)(rng() % spread)) / 4;
          vi[i] = (int32_t)(rng() % 2001) - 1000;
          vd[i] = (double)((int)(rng() % 2001) - 1000);
          if (nullable) {
            valid[i] = rng() % 4 != 0;
            kvalid[i] = rng() % 8 != 0;
          }
        }
        for (int asc = 0; asc < 2; ++asc) {
          const int64_t minp = 1 + (int64_t)(rng() % 3);
          for (double p : int_bounds)
            for (double f : int_bounds) {
              run_case<int64_t, int32_t>(g, ki, kvalid, vi, valid, asc != 0, p, f, minp);
              if (n <= 100) run_case<int64_t, double>(g, ki, kvalid, vd, valid, asc != 0, p, f, minp);
            }
          for (double p : float_bounds)
            for (double f : float_bounds) {
              run_case<double, double>(g, kd, kvalid, vd, valid, asc != 0, p, f, minp);
              if (n <= 100) run_case<double, int32_t>(g, kd, kvalid, vi, valid, asc != 0, p, f, minp);
            }
        }
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "frame_range_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("frame_range_sanitize: ok\n");
  return 0;
}
