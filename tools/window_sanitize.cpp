// Host sanitizer check of the CPU twin of the window functions (kernels/cpu_window.cpp): flags / tile /
// carry / apply, the rank scan and the LAG / LEAD shift driven as ops/window.cpp drives them, over tiny
// inputs in exactly-sized heap buffers, against a brute-force walk of every partition.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/window_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_window.cpp -o window_sanitize
//   ./window_sanitize          # prints "window_sanitize: ok", exit status 0
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <type_traits>
#include <vector>

#include "cylon/kernels/kernels.hpp"
#include "cylon/kernels/order_image.hpp"

namespace {

using namespace cylon;

int failures = 0;

void expect(bool ok, const char *what, int64_t n, int func) {
  if (ok) return;
  if (++failures <= 10) std::fprintf(stderr, "window_sanitize: %s differs (n = %lld, func %d)\n", what, (long long)n, func);
}

template <typename V>
ColView view_of(const std::vector<V> &v, const std::vector<uint8_t> &valid, ValueKind kind) {
  ColView c;
  c.data = reinterpret_cast<const uint8_t *>(v.data());
  c.valid = valid.empty() ? nullptr : valid.data();
  c.width = (int32_t)sizeof(V);
  c.kind = static_cast<int>(kind);
  return c;
}

// partition ids and order keys per row -> perm (stable), partition heads, peer heads
struct Order {
  std::vector<int64_t> perm;
  std::vector<uint8_t> part, peer;
};

Order make_order(const std::vector<int> &g, const std::vector<int> &o) {
  const int64_t n = (int64_t)g.size();
  Order r;
  r.perm.resize((size_t)n);
  std::iota(r.perm.begin(), r.perm.end(), 0);
  std::stable_sort(r.perm.begin(), r.perm.end(),
                   [&](int64_t a, int64_t b) { return g[a] != g[b] ? g[a] < g[b] : o[a] < o[b]; });
  r.part.resize((size_t)n);
  r.peer.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t a = r.perm[i], b = i ? r.perm[i - 1] : 0;
    r.part[i] = i == 0 || g[a] != g[b];
    r.peer[i] = r.part[i] || o[a] != o[b];
  }
  return r;
}

// one value function of the twin against a direct walk; V = value type, func = kernels/window.hip WinFunc
template <typename V>
void value_case(const std::vector<V> &v, const std::vector<uint8_t> &valid, ValueKind kind, const Order &ord,
                const std::vector<uint8_t> &flags, int func) {
  const int64_t n = (int64_t)v.size();
  const ColView c = view_of(v, valid, kind);
  const int64_t T = cpu::window_tile_rows(), ntiles = (n + T - 1) / T;
  std::vector<uint64_t> dense((size_t)n);
  std::vector<uint8_t> dvalid(valid.empty() ? 0 : (size_t)n);
  std::vector<int64_t> tagg((size_t)ntiles), carry((size_t)ntiles);
  std::vector<uint8_t> tflag((size_t)ntiles);
  const bool wide = func == 0 || func == 1 || func == 4;  // 8-byte results
  std::vector<uint8_t> out((size_t)n * (wide ? 8 : sizeof(V))), ovalid(valid.empty() ? 0 : (size_t)n);
  uint8_t *dv = dvalid.empty() ? nullptr : dvalid.data();
  for (int pass = 0; pass < 2; ++pass)  // gather, then again from the dense values
    cpu::window_tile(c, ord.perm.data(), flags.data(), n, func, dense.data(), dv, pass == 0, tagg.data(), tflag.data(),
                     nullptr);
  cpu::window_carry(tagg.data(), tflag.data(), ntiles, 1, func, 0, carry.data(), nullptr);
  cpu::window_apply(c, ord.perm.data(), flags.data(), n, func, dense.data(), dv, carry.data(), out.data(),
                    ovalid.empty() ? nullptr : ovalid.data(), nullptr);
  // brute force: for every position, walk back to its partition head
  for (int64_t i = 0; i < n; ++i) {
    int64_t h = i;
    while (!ord.part[h]) --h;
    uint64_t isum = 0, cnt = 0, lo = 0, hi = 0;
    double fsum = 0;
    bool seen = false;
    for (int64_t j = h; j <= i; ++j) {
      const int64_t r = ord.perm[j];
      if (!valid.empty() && !valid[r]) continue;
      uint64_t bits = 0;
      std::memcpy(&bits, &v[r], sizeof(V));
      const uint64_t im = order_image(bits, (int)sizeof(V), static_cast<int>(kind));
      if constexpr (std::is_integral<V>::value) isum += (uint64_t)(int64_t)v[r];
      if constexpr (std::is_floating_point<V>::value) fsum += (double)v[r];
      ++cnt;
      lo = seen ? std::min(lo, im) : im;
      hi = seen ? std::max(hi, im) : im;
      seen = true;
    }
    const int64_t r = ord.perm[i];
    const bool live = valid.empty() || valid[r];
    if (!ovalid.empty()) expect(ovalid[r] == (live ? 1 : 0), "validity", n, func);
    if (!live && func != 4) continue;  // a null row's bytes are unspecified
    uint64_t got = 0;
    std::memcpy(&got, out.data() + r * (wide ? 8 : sizeof(V)), wide ? 8 : sizeof(V));
    uint64_t want;
    if (func == 0) want = isum;
    else if (func == 1) std::memcpy(&want, &fsum, 8);
    else if (func == 4) want = cnt;
    else want = order_unimage(func == 2 ? lo : hi, (int)sizeof(V), static_cast<int>(kind));
    expect(got == want, "running value", n, func);
  }
}

void run_shape(const std::vector<int> &g, const std::vector<int> &o, std::mt19937_64 &rng) {
  const int64_t n = (int64_t)g.size();
  const Order ord = make_order(g, o);
  std::vector<uint8_t> flags((size_t)n);
  cpu::window_flags(ord.part.data(), ord.peer.data(), n, flags.data(), nullptr);
  for (int64_t i = 0; i < n; ++i) expect(flags[i] == (ord.part[i] | (ord.peer[i] << 1)), "flags", n, -1);
  {  // no order columns: the peer heads are the partition heads, in place
    std::vector<uint8_t> f2 = ord.part;
    cpu::window_flags(f2.data(), nullptr, n, f2.data(), nullptr);
    for (int64_t i = 0; i < n; ++i) expect(f2[i] == (ord.part[i] ? 3 : 0), "flags in place", n, -1);
  }
  // ranking and LAG / LEAD
  const int64_t T = cpu::window_tile_rows(), ntiles = (n + T - 1) / T;
  std::vector<int64_t> tagg((size_t)(3 * ntiles)), carry((size_t)(3 * ntiles));
  std::vector<uint8_t> tflag((size_t)ntiles);
  std::vector<int64_t> rn((size_t)n), rk((size_t)n), dr((size_t)n), ph((size_t)n), src((size_t)n);
  cpu::window_rank_tile(flags.data(), n, tagg.data(), tflag.data(), nullptr);
  cpu::window_carry(tagg.data(), tflag.data(), ntiles, 3, 5, 0, carry.data(), nullptr);
  cpu::window_rank_apply(ord.perm.data(), flags.data(), n, carry.data(), rn.data(), rk.data(), dr.data(), ph.data(),
                         nullptr);
  cpu::window_rank_apply(ord.perm.data(), flags.data(), n, carry.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  for (int64_t i = 0; i < n; ++i) {
    int64_t h = i, peers = 0, q = i;
    while (!ord.part[h]) --h;
    while (!ord.peer[q]) --q;
    for (int64_t j = h; j <= i; ++j) peers += ord.peer[j];
    const int64_t r = ord.perm[i];
    expect(rn[r] == i - h + 1 && rk[r] == q - h + 1 && dr[r] == peers && ph[i] == h, "ranking", n, 5);
  }
  for (int64_t off : {int64_t(0), int64_t(1), int64_t(2), n - 1, n}) {
    if (off < 0 || off > n) continue;  // the operator clamps an offset to n
    for (int sign : {-1, 1}) {
      cpu::window_shift(ord.perm.data(), ph.data(), n, sign * off, src.data(), nullptr);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t j = i + sign * off;
        const bool in = j >= 0 && j < n && ph[j] == ph[i];
        expect(src[ord.perm[i]] == (in ? ord.perm[j] : -1), "shift", n, 7);
      }
    }
  }
  // value functions over every width, with and without nulls (the first rows of a partition among them)
  std::vector<uint8_t> some((size_t)n), lead((size_t)n, 1);
  for (auto &b : some) b = rng() % 10 < 7;
  for (int64_t i = 0; i < n; ++i)  // null: every partition's head and the position after it
    if (ord.part[i] || (i > 0 && ord.part[i - 1])) lead[ord.perm[i]] = 0;
  std::vector<int8_t> v8((size_t)n);
  std::vector<int16_t> v16((size_t)n);
  std::vector<uint32_t> v32((size_t)n);
  std::vector<int64_t> v64((size_t)n);
  std::vector<uint64_t> u64((size_t)n);
  std::vector<float> f32((size_t)n);
  std::vector<double> f64((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t x = rng();
    v8[i] = (int8_t)x;
    v16[i] = (int16_t)x;
    v32[i] = (uint32_t)x;
    v64[i] = (int64_t)x;  // sums wrap
    u64[i] = x;
    f32[i] = (float)((int64_t)(x % 2001) - 1000) / 8.0f;  // exact in any order
    f64[i] = (double)((int64_t)(x % 2000001) - 1000000) / 64.0;
  }
  if (n > 2) {
    f64[0] = -0.0;
    f64[1] = 0.0;
    f64[2] = std::numeric_limits<double>::quiet_NaN();
  }
  for (const auto &valid : {std::vector<uint8_t>(), some, lead, std::vector<uint8_t>((size_t)n, 0)}) {
    for (int func : {0, 2, 3, 4}) {
      value_case(v8, valid, ValueKind::SIGNED_INT, ord, flags, func);
      value_case(v16, valid, ValueKind::SIGNED_INT, ord, flags, func);
      value_case(v32, valid, ValueKind::UNSIGNED_INT, ord, flags, func);
      value_case(v64, valid, ValueKind::SIGNED_INT, ord, flags, func);
      value_case(u64, valid, ValueKind::UNSIGNED_INT, ord, flags, func);
    }
    value_case(f32, valid, ValueKind::FLOAT, ord, flags, 1);
    for (int func : {2, 3, 4}) {
      value_case(f32, valid, ValueKind::FLOAT, ord, flags, func);
      value_case(f64, valid, ValueKind::FLOAT, ord, flags, func);
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(13);
  const int64_t T = cpu::window_tile_rows();
  for (int64_t n : {int64_t(0), int64_t(1), int64_t(2), int64_t(63), int64_t(64), int64_t(65), T - 1, T, T + 1}) {
    std::vector<int> g((size_t)n), o((size_t)n);
    // one partition; every row its own; random partitions with tied order keys; no ties
    for (int shape = 0; shape < 4; ++shape) {
      for (int64_t i = 0; i < n; ++i) {
        g[i] = shape == 0 ? 0 : shape == 1 ? (int)i : (int)(rng() % 7);
        o[i] = shape == 3 ? (int)(n - i) : (int)(rng() % 5);
      }
      run_shape(g, o, rng);
    }
  }
  if (failures) {
    std::fprintf(stderr, "window_sanitize: %d mismatches\n", failures);
    return 1;
  }
  std::printf("window_sanitize: ok\n");
  return 0;
}
