// Host sanitizer check of the CPU twin of the framed VAR / STD (kernels/cpu_frame_moments.cpp):
// frame_moments_pyramid / frame_moments_apply over small inputs in exactly-sized heap buffers (the
// pyramid's too: frame_moments_common.hpp's word counts), with the ROWS bounds computed by the twin from
// phead / rtail and with explicit lo / hi arrays (the RANGE form), against a brute-force two-pass variance
// of every frame.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/frame_moments_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_frame_moments.cpp \
//       -o frame_moments_sanitize
//   ./frame_moments_sanitize      # prints "frame_moments_sanitize: ok", exit status 0
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "cylon/kernels/frame_moments_common.hpp"
#include "cylon/kernels/kernels.hpp"

namespace {

using namespace cylon;

int failures = 0;

void expect(bool ok, const char *what, int64_t n, int64_t i, double got, double want) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "frame_moments_sanitize: %s differs (n = %lld, position %lld: %g, expected %g)\n", what,
                 (long long)n, (long long)i, got, want);
}

// values v (NaN / inf allowed) with validity bytes, partitions of the given sizes in sorted order,
// perm = a rotation (out is written at perm[i])
void run_case(const std::vector<double> &v, const std::vector<uint8_t> &valid, const std::vector<int64_t> &sizes,
              int64_t pre, int64_t fol, int64_t minp, int64_t ddof, bool std_dev, bool nulls) {
  const int64_t n = (int64_t)v.size();
  std::vector<int64_t> phead((size_t)n), tail((size_t)n), rtail((size_t)n), perm((size_t)n);
  int64_t at = 0;
  for (int64_t s : sizes)
    for (int64_t j = 0; j < s && at < n; ++j, ++at) phead[at] = at - j;
  for (int64_t i = n - 1; i >= 0; --i) tail[i] = (i == n - 1 || phead[i + 1] == i + 1) ? i : tail[i + 1];
  for (int64_t i = 0; i < n; ++i) rtail[n - 1 - i] = n - 1 - tail[i];  // as the reversed rank scan stores it
  for (int64_t i = 0; i < n; ++i) perm[i] = (i + 3) % n;
  std::vector<uint64_t> dense((size_t)n);
  std::memcpy(dense.data(), v.data(), (size_t)n * 8);
  ColView col;
  col.width = 8;
  col.kind = static_cast<int>(ValueKind::FLOAT);
  // exactly-sized buffers: a read or write past the pyramid's words is a heap overflow
  std::vector<uint64_t> P((size_t)fm_words(fm_ps_slots(n))), S((size_t)fm_words(fm_ps_slots(n))),
      E((size_t)fm_words(fm_e_slots(n)));
  const uint8_t *dv = nulls ? valid.data() : nullptr;
  cpu::frame_moments_pyramid(col, n, dense.data(), dv, P.data(), S.data(), E.data(), nullptr);
  std::vector<uint32_t> lo((size_t)n), hi((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    lo[i] = (uint32_t)std::max(phead[i], pre > i ? (int64_t)0 : i - pre);
    hi[i] = (uint32_t)std::min(tail[i], fol >= n - 1 - i ? n - 1 : i + fol);
  }
  for (int form = 0; form < 2; ++form) {  // 0: ROWS from phead / rtail, 1: explicit bounds
    std::vector<double> out((size_t)n, -7.0);
    std::vector<uint8_t> ov((size_t)n, 9);
    cpu::frame_moments_apply(col, perm.data(), n, std_dev, ddof, minp, dense.data(), dv, form ? lo.data() : nullptr,
                             form ? hi.data() : nullptr, phead.data(), rtail.data(), pre, fol, P.data(), S.data(),
                             E.data(), reinterpret_cast<uint8_t *>(out.data()), ov.data(), nullptr);
    for (int64_t i = 0; i < n; ++i) {
      int64_t m = 0;
      bool bad = false;
      long double sum = 0;
      for (int64_t j = lo[i]; j <= (int64_t)hi[i]; ++j) {
        if (nulls && !valid[j]) continue;
        ++m;
        if (!std::isfinite(v[j])) bad = true;
        else sum += v[j];
      }
      const bool live = m >= minp && m - ddof > 0;
      const double got = out[perm[i]];
      expect(ov[perm[i]] == (live ? 1 : 0), "validity", n, i, ov[perm[i]], live);
      if (!live) continue;
      if (bad) {
        expect(got != got, "NaN of a non-finite frame", n, i, got, NAN);
        continue;
      }
      long double m2 = 0;
      for (int64_t j = lo[i]; j <= (int64_t)hi[i]; ++j)
        if (!nulls || valid[j]) m2 += (v[j] - sum / m) * (v[j] - sum / m);
      double want = (double)(m2 / (m - ddof));
      if (std_dev) want = std::sqrt(want);
      expect(got >= 0 && !std::signbit(got) && std::fabs(got - want) <= 1e-9 * (1 + std::fabs(want)), "value", n, i,
             got, want);
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  const int64_t unbounded = std::numeric_limits<int64_t>::max();
  const int64_t frames[][2] = {{0, 0}, {1, 0}, {3, 4}, {7, 0}, {8, 8}, {63, 64}, {511, 0}, {0, unbounded},
                               {unbounded, 0}, {unbounded, unbounded}, {599, 3}};
  int cases = 0;
  for (int64_t n : {1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 600}) {
    std::vector<double> v((size_t)n);
    std::vector<uint8_t> valid((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      v[i] = 1e6 + (double)((int64_t)(rng() % 2001) - 1000);
      valid[i] = rng() % 4 != 0;
    }
    if (n > 20) {
      v[5] = std::numeric_limits<double>::infinity();
      v[11] = std::nan("");
      v[(size_t)n - 2] = -std::numeric_limits<double>::infinity();
      for (int64_t i = 14; i < std::min<int64_t>(n, 14 + 70); ++i) valid[i] = i % 35 == 0;  // long null runs
    }
    const std::vector<std::vector<int64_t>> layouts = {{n}, {1, 2, 7, 8, 9, 65, 64, 512}, {8, 8, 64, 8}};
    for (const auto &sizes : layouts) {
      std::vector<int64_t> s;
      for (int64_t total = 0; total < n;)
        for (int64_t x : sizes) {
          s.push_back(x);
          total += x;
          if (total >= n) break;
        }
      for (const auto &f : frames)
        for (int k = 0; k < 4; ++k, ++cases)
          run_case(v, valid, s, f[0], f[1], k == 3 ? 3 : 1, k, k % 2 == 1, k != 2);
    }
  }
  if (failures) {
    std::fprintf(stderr, "frame_moments_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("frame_moments_sanitize: ok (%d cases)\n", cases);
  return 0;
}
