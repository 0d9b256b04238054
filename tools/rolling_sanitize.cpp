// Host sanitizer check of the CPU twin of the framed aggregates (kernels/cpu_rolling.cpp), driven as
// ops/window.cpp drives it -- the flags, the gather and the two rank scans of cpu_window.cpp, then
// rolling_lds, and rolling_tile / rolling_scan / rolling_combine for the same frame -- over tiny inputs
// in exactly-sized heap buffers, against a brute-force walk of every frame.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/rolling_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_rolling.cpp \
//       cylon_amd/csrc/cylon/kernels/cpu_window.cpp -o rolling_sanitize
//   ./rolling_sanitize          # prints "rolling_sanitize: ok", exit status 0
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "cylon/kernels/kernels.hpp"
#include "cylon/kernels/order_image.hpp"

namespace {

using namespace cylon;

int failures = 0;

void expect(bool ok, const char *what, int64_t n, int func, int64_t p, int64_t f) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "rolling_sanitize: %s differs (n = %lld, func %d, frame %lld, %lld)\n", what, (long long)n,
                 func, (long long)p, (long long)f);
}

constexpr int kSumI = 0, kSumF = 1, kMin = 2, kMax = 3, kCount = 4, kRank = 5;

// V = int32_t or double (integer-valued: every summation order is exact)
template <typename V>
void run_case(const std::vector<int> &g, const std::vector<V> &v, const std::vector<uint8_t> &valid, int64_t p,
              int64_t f, int64_t minp) {
  const int64_t n = (int64_t)g.size();
  const bool is_float = sizeof(V) == 8;
  // the order, the flags, the heads and the reversed tails, as ops/window.cpp forms them
  std::vector<int64_t> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return g[a] < g[b]; });
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

  ColView c;
  c.data = reinterpret_cast<const uint8_t *>(v.data());
  c.valid = valid.empty() ? nullptr : valid.data();
  c.width = (int32_t)sizeof(V);
  c.kind = static_cast<int>(is_float ? ValueKind::FLOAT : ValueKind::SIGNED_INT);
  std::vector<uint64_t> dense((size_t)n);
  std::vector<uint8_t> dvalid(valid.empty() ? 0 : (size_t)n);
  std::vector<int64_t> tagg((size_t)ntiles), tcnt((size_t)ntiles), carry((size_t)ntiles), ccnt((size_t)ntiles);
  uint8_t *dv = dvalid.empty() ? nullptr : dvalid.data();
  cpu::window_tile(c, perm.data(), flags.data(), n, kCount, dense.data(), dv, true, tagg.data(), tflag.data(), nullptr);

  // brute force, per sorted position
  std::vector<int64_t> want_cnt((size_t)n);
  std::vector<double> want_sum((size_t)n), want_min((size_t)n), want_max((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t head = i, tail = i;
    while (head > 0 && !part[head]) --head;
    while (tail + 1 < n && !part[tail + 1]) ++tail;
    const int64_t lo = std::max(i - p, head), hi = std::min(i + f, tail);
    int64_t m = 0;
    double s = 0, mn = 0, mx = 0;
    for (int64_t j = lo; j <= hi; ++j) {
      const int64_t r = perm[j];
      if (!valid.empty() && !valid[r]) continue;
      const double x = (double)v[r];
      s += x;
      mn = m ? std::min(mn, x) : x;
      mx = m ? std::max(mx, x) : x;
      ++m;
    }
    want_cnt[i] = m;
    want_sum[i] = s;
    want_min[i] = mn;
    want_max[i] = mx;
  }

  const int64_t w = p + f + 1;
  const int sum = is_float ? kSumF : kSumI;
  struct Plan {
    int func;
    bool mean;
  };
  for (const Plan pl : {Plan{kCount, false}, Plan{sum, false}, Plan{sum, true}, Plan{kMin, false}, Plan{kMax, false}}) {
    const size_t ow = (pl.func == kMin || pl.func == kMax) ? sizeof(V) : 8;
    for (int path = 0; path < 2; ++path) {
      if (path == 0 && w > cpu::window_frame_lds_rows()) continue;
      std::vector<uint8_t> out((size_t)n * ow), ovalid(pl.func == kCount ? 0 : (size_t)n);
      uint8_t *ov = ovalid.empty() ? nullptr : ovalid.data();
      if (path == 0) {
        cpu::rolling_lds(c, perm.data(), flags.data(), phead.data(), rtail.data(), n, pl.func, pl.mean, p, f, minp,
                         dense.data(), dv, out.data(), ov, nullptr);
      } else {
        std::vector<uint64_t> scan[2] = {std::vector<uint64_t>((size_t)n), std::vector<uint64_t>((size_t)n)};
        std::vector<uint32_t> cnt[2] = {std::vector<uint32_t>((size_t)n), std::vector<uint32_t>((size_t)n)};
        for (int rev = 0; rev < 2; ++rev) {
          const uint8_t *rs = rev ? rflags.data() : flags.data();
          cpu::rolling_tile(c, rs, n, pl.func, w, rev != 0, dense.data(), dv, tagg.data(), tcnt.data(), tflag.data(),
                            nullptr);
          cpu::window_carry(tagg.data(), tflag.data(), ntiles, 1, pl.func, 0, carry.data(), nullptr);
          cpu::window_carry(tcnt.data(), tflag.data(), ntiles, 1, kCount, 0, ccnt.data(), nullptr);
          cpu::rolling_scan(c, rs, n, pl.func, w, rev != 0, dense.data(), dv, carry.data(), ccnt.data(),
                            scan[rev].data(), cnt[rev].data(), nullptr);
        }
        cpu::rolling_combine(c, perm.data(), phead.data(), rtail.data(), n, pl.func, pl.mean, p, f, minp, scan[0].data(),
                             cnt[0].data(), scan[1].data(), cnt[1].data(), out.data(), ov, nullptr);
      }
      for (int64_t i = 0; i < n; ++i) {
        const int64_t r = perm[i];
        if (pl.func == kCount) {
          int64_t got;
          std::memcpy(&got, out.data() + r * 8, 8);
          expect(got == want_cnt[i], "count", n, pl.func, p, f);
          continue;
        }
        const bool live = want_cnt[i] >= minp;
        expect((ovalid[r] != 0) == live, "validity", n, pl.func, p, f);
        if (!live) continue;
        double got;
        if (pl.func == kMin || pl.func == kMax) {
          V x;
          std::memcpy(&x, out.data() + r * sizeof(V), sizeof(V));
          got = (double)x;
        } else if (pl.mean || is_float) {
          std::memcpy(&got, out.data() + r * 8, 8);
        } else {
          int64_t x;
          std::memcpy(&x, out.data() + r * 8, 8);
          got = (double)x;
        }
        const double want = pl.func == kMin ? want_min[i] : pl.func == kMax ? want_max[i]
                            : pl.mean ? want_sum[i] / (double)want_cnt[i] : want_sum[i];
        expect(got == want, path ? "wide result" : "lds result", n, pl.func, p, f);
      }
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  const int64_t sizes[] = {1, 2, 3, 7, 33, 100};
  const int64_t bounds[] = {0, 1, 2, 5, 40, 99, 100, 600};
  for (int64_t n : sizes) {
    for (int groups : {1, 3, (int)n}) {
      for (int nullable = 0; nullable < 2; ++nullable) {
        std::vector<int> g((size_t)n);
        std::vector<int32_t> vi((size_t)n);
        std::vector<double> vd((size_t)n);
        std::vector<uint8_t> valid(nullable ? (size_t)n : 0);
        for (int64_t i = 0; i < n; ++i) {
          g[i] = (int)(rng() % (unsigned)groups);
          vi[i] = (int32_t)(rng() % 2001) - 1000;
          vd[i] = (double)((int)(rng() % 2001) - 1000);
          if (nullable) valid[i] = rng() % 4 != 0;
        }
        for (int64_t p : bounds) {
          for (int64_t f : bounds) {
            if (p > n || f > n) continue;  // the operator clamps both to n
            const int64_t minp = 1 + (int64_t)(rng() % 3);
            run_case<int32_t>(g, vi, valid, p, f, minp);
            run_case<double>(g, vd, valid, p, f, minp);
          }
        }
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "rolling_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("rolling_sanitize: ok\n");
  return 0;
}
