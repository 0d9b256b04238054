// Host sanitizer check of the CPU twin of the navigation and distribution window functions
// (kernels/cpu_window_nav.cpp), driven as ops/window.cpp drives it -- the flags, the gather and the two
// rank scans of cpu_window.cpp, the reversed flags with and without the peer tails, then the fill scan in
// value mode, source mode and position mode, window_nav_pick in its five forms and window_dist_apply --
// over tiny inputs in exactly-sized heap buffers, against a brute-force walk of every partition.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/window_nav_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_window_nav.cpp \
//       cylon_amd/csrc/cylon/kernels/cpu_window.cpp cylon_amd/csrc/cylon/kernels/cpu_rolling.cpp \
//       -o window_nav_sanitize
//   ./window_nav_sanitize          # prints "window_nav_sanitize: ok", exit status 0
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

void expect(bool ok, const char *what, int64_t n, int64_t arg) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "window_nav_sanitize: %s differs (n = %lld, arg %lld)\n", what, (long long)n, (long long)arg);
}

constexpr int kMax = 3, kCount = 4, kRank = 5;

// V = int16_t, int32_t or double: the value mode's widths 2, 4 and 8
template <typename V>
void run_case(const std::vector<int> &g, const std::vector<int> &o, const std::vector<V> &v,
              const std::vector<uint8_t> &valid, int64_t limit, int64_t k) {
  const int64_t n = (int64_t)g.size();
  // the order, the flags, the heads and the reversed tails, as ops/window.cpp forms them
  std::vector<int64_t> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(),
                   [&](int64_t a, int64_t b) { return g[a] != g[b] ? g[a] < g[b] : o[a] < o[b]; });
  std::vector<uint8_t> part((size_t)n), peer((size_t)n), flags((size_t)n), rflags((size_t)n), rpflags((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    part[i] = i == 0 || g[perm[i]] != g[perm[i - 1]];
    peer[i] = part[i] || o[perm[i]] != o[perm[i - 1]];
  }
  cpu::window_flags(part.data(), peer.data(), n, flags.data(), nullptr);
  const int64_t T = cpu::window_tile_rows(), ntiles = (n + T - 1) / T;
  std::vector<int64_t> tagg3((size_t)(3 * ntiles)), carry3((size_t)(3 * ntiles));
  std::vector<int64_t> phead((size_t)n), rtail((size_t)n), rtail2((size_t)n), qhead((size_t)n), rqhead((size_t)n);
  std::vector<uint8_t> tflag((size_t)ntiles);
  cpu::window_rank_tile(flags.data(), n, tagg3.data(), tflag.data(), nullptr);
  cpu::window_carry(tagg3.data(), tflag.data(), ntiles, 3, kRank, 0, carry3.data(), nullptr);
  cpu::window_rank_apply(perm.data(), flags.data(), n, carry3.data(), nullptr, nullptr, nullptr, phead.data(), nullptr);
  cpu::window_rank_heads(flags.data(), n, carry3.data(), nullptr, qhead.data(), nullptr);
  cpu::window_rev_flags(flags.data(), n, rflags.data(), nullptr);
  cpu::window_rev_peer_flags(flags.data(), n, rpflags.data(), nullptr);
  cpu::window_rank_tile(rpflags.data(), n, tagg3.data(), tflag.data(), nullptr);
  cpu::window_carry(tagg3.data(), tflag.data(), ntiles, 3, kRank, 0, carry3.data(), nullptr);
  cpu::window_rank_apply(perm.data(), rpflags.data(), n, carry3.data(), nullptr, nullptr, nullptr, rtail.data(), nullptr);
  cpu::window_rank_heads(rpflags.data(), n, carry3.data(), rtail2.data(), rqhead.data(), nullptr);
  for (int64_t i = 0; i < n; ++i) {
    expect((rpflags[i] & 1) == (rflags[i] & 1), "reversed flags", n, i);
    expect(rtail[i] == rtail2[i], "reversed tails", n, i);
  }

  ColView c;
  c.data = reinterpret_cast<const uint8_t *>(v.data());
  c.valid = valid.empty() ? nullptr : valid.data();
  c.width = (int32_t)sizeof(V);
  c.kind = static_cast<int>(sizeof(V) == 8 ? ValueKind::FLOAT : ValueKind::SIGNED_INT);
  std::vector<uint64_t> dense((size_t)n);
  std::vector<uint8_t> dvalid(valid.empty() ? 0 : (size_t)n);
  std::vector<int64_t> tagg((size_t)ntiles), carry((size_t)ntiles);
  uint8_t *dv = dvalid.empty() ? nullptr : dvalid.data();
  cpu::window_tile(c, perm.data(), flags.data(), n, kCount, dense.data(), dv, true, tagg.data(), tflag.data(), nullptr);

  // brute force, per sorted position: the partition, the peers and the nearest non-null positions
  std::vector<int64_t> head((size_t)n), tail((size_t)n), ptail((size_t)n), phd((size_t)n), back((size_t)n), fwd((size_t)n);
  auto live = [&](int64_t i) { return valid.empty() || valid[perm[i]] != 0; };
  for (int64_t i = 0; i < n; ++i) {
    int64_t h = i, t = i, qt = i, qh = i;
    while (h > 0 && !part[h]) --h;
    while (t + 1 < n && !part[t + 1]) ++t;
    while (qt + 1 < n && !peer[qt + 1]) ++qt;
    while (qh > 0 && !peer[qh]) --qh;
    head[i] = h;
    tail[i] = t;
    ptail[i] = qt;
    phd[i] = qh;
    back[i] = fwd[i] = -1;
    for (int64_t j = i; j >= h; --j)
      if (live(j)) {
        back[i] = j;
        break;
      }
    for (int64_t j = i; j <= t; ++j)
      if (live(j)) {
        fwd[i] = j;
        break;
      }
  }
  auto value_at = [&](const std::vector<uint8_t> &out, int64_t r) {
    V x;
    std::memcpy(&x, out.data() + r * sizeof(V), sizeof(V));
    return x;
  };

  // fills: a column without nulls runs no scan in the operator
  if (!valid.empty()) {
    for (int rev = 0; rev < 2; ++rev) {
      const uint8_t *rs = rev ? rflags.data() : flags.data();
      const std::vector<int64_t> &near = rev ? fwd : back;
      cpu::window_fill_tile(rs, n, rev != 0, dv, tagg.data(), tflag.data(), nullptr);
      cpu::window_carry(tagg.data(), tflag.data(), ntiles, 1, kMax, 0, carry.data(), nullptr);
      std::vector<uint8_t> out((size_t)n * sizeof(V)), ovalid((size_t)n);
      std::vector<int64_t> src((size_t)n), pos((size_t)n);
      cpu::window_fill_apply(c, perm.data(), rs, n, rev != 0, limit, dense.data(), dv, carry.data(), out.data(),
                             ovalid.data(), nullptr, nullptr, nullptr);
      cpu::window_fill_apply(c, perm.data(), rs, n, rev != 0, limit, dense.data(), dv, carry.data(), nullptr, nullptr,
                             src.data(), nullptr, nullptr);
      cpu::window_fill_apply(c, perm.data(), rs, n, rev != 0, 0, dense.data(), dv, carry.data(), nullptr, nullptr,
                             nullptr, pos.data(), nullptr);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t r = perm[i];
        int64_t j = near[i];
        expect(pos[i] == j, "fill position", n, rev);
        if (j >= 0 && limit > 0 && (rev ? j - i : i - j) > limit) j = -1;
        expect((ovalid[r] != 0) == (j >= 0), "fill validity", n, limit);
        expect(src[r] == (j >= 0 ? perm[j] : -1), "fill source", n, limit);
        if (j >= 0) expect(std::memcmp(out.data() + r * sizeof(V), &v[perm[j]], sizeof(V)) == 0, "fill value", n, limit);
      }
      // FIRST / LAST_VALUE ignoring nulls read these positions at the partition's head / tail
      const int form = rev ? 3 : 4;
      cpu::window_nav_pick(c, perm.data(), rev ? phead.data() : nullptr, rev ? nullptr : rtail.data(), pos.data(), n,
                           form, 0, dense.data(), dv, out.data(), ovalid.data(), nullptr, nullptr);
      cpu::window_nav_pick(c, perm.data(), rev ? phead.data() : nullptr, rev ? nullptr : rtail.data(), pos.data(), n,
                           form, 0, nullptr, nullptr, nullptr, nullptr, src.data(), nullptr);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t r = perm[i], j = rev ? fwd[head[i]] : back[tail[i]];
        expect((ovalid[r] != 0) == (j >= 0), "ignore-nulls validity", n, rev);
        expect(src[r] == (j >= 0 ? perm[j] : -1), "ignore-nulls source", n, rev);
        if (j >= 0) expect(value_at(out, r) == v[perm[j]], "ignore-nulls value", n, rev);
      }
    }
  }

  // FIRST / LAST / NTH_VALUE
  for (int form = 0; form < 3; ++form) {
    std::vector<uint8_t> out((size_t)n * sizeof(V)), ovalid((size_t)n);
    std::vector<int64_t> src((size_t)n);
    const int64_t *ph = form == 1 ? nullptr : phead.data(), *rt = form == 0 ? nullptr : rtail.data();
    cpu::window_nav_pick(c, perm.data(), ph, rt, nullptr, n, form, k, dense.data(), dv, out.data(), ovalid.data(),
                         nullptr, nullptr);
    cpu::window_nav_pick(c, perm.data(), ph, rt, nullptr, n, form, k, nullptr, nullptr, nullptr, nullptr, src.data(),
                         nullptr);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = perm[i];
      const int64_t j = form == 0 ? head[i] : form == 1 ? tail[i] : (head[i] + k - 1 <= tail[i] ? head[i] + k - 1 : -1);
      expect(src[r] == (j >= 0 ? perm[j] : -1), "navigation source", n, form);
      expect((ovalid[r] != 0) == (j >= 0 && live(j)), "navigation validity", n, form);
      if (j >= 0 && live(j)) expect(value_at(out, r) == v[perm[j]], "navigation value", n, form);
    }
  }

  // NTILE / PERCENT_RANK / CUME_DIST
  {
    std::vector<uint8_t> nt((size_t)n * 8), pr((size_t)n * 8), cd((size_t)n * 8);
    cpu::window_dist_apply(perm.data(), phead.data(), rtail.data(), nullptr, nullptr, n, 0, k, nt.data(), nullptr);
    cpu::window_dist_apply(perm.data(), phead.data(), rtail.data(), qhead.data(), nullptr, n, 1, 0, pr.data(), nullptr);
    cpu::window_dist_apply(perm.data(), phead.data(), rtail.data(), nullptr, rqhead.data(), n, 2, 0, cd.data(), nullptr);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = perm[i], s = tail[i] - head[i] + 1, at = i - head[i];
      // the bucket by construction: the first s % k buckets hold one row more
      int64_t b = 0, seen = 0;
      while (true) {
        const int64_t size = s / k + (b < s % k ? 1 : 0);
        if (at < seen + size) break;
        seen += size;
        ++b;
      }
      int64_t got;
      double gp, gc;
      std::memcpy(&got, nt.data() + r * 8, 8);
      std::memcpy(&gp, pr.data() + r * 8, 8);
      std::memcpy(&gc, cd.data() + r * 8, 8);
      expect(got == b + 1, "ntile", n, k);
      expect(gp == (s == 1 ? 0.0 : (double)(phd[i] - head[i]) / (double)(s - 1)), "percent_rank", n, i);
      expect(gc == (double)(ptail[i] - head[i] + 1) / (double)s, "cume_dist", n, i);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(11);
  const int64_t sizes[] = {1, 2, 3, 7, 33, 100};
  for (int64_t n : sizes) {
    for (int groups : {1, 3, (int)n}) {
      for (int nulls : {0, 4, 1}) {  // no validity array, a quarter null, all null
        std::vector<int> g((size_t)n), o((size_t)n);
        std::vector<int16_t> vs((size_t)n);
        std::vector<int32_t> vi((size_t)n);
        std::vector<double> vd((size_t)n);
        std::vector<uint8_t> valid(nulls ? (size_t)n : 0);
        for (int64_t i = 0; i < n; ++i) {
          g[i] = (int)(rng() % (unsigned)groups);
          o[i] = (int)(rng() % 5);  // peers
          vi[i] = (int32_t)(rng() % 2001) - 1000;
          vs[i] = (int16_t)vi[i];
          vd[i] = (double)vi[i] / 8;
          if (nulls) valid[i] = nulls == 1 ? 0 : rng() % 4 != 0;
        }
        for (int64_t limit : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)5, n, (int64_t)1 << 40}) {
          const int64_t k = 1 + (int64_t)(rng() % (unsigned)(n + 2));
          run_case<int16_t>(g, o, vs, valid, limit, k);
          run_case<int32_t>(g, o, vi, valid, limit, k);
          run_case<double>(g, o, vd, valid, limit, k);
        }
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "window_nav_sanitize: %d failures\n", failures);
    return 1;
  }
  std::printf("window_nav_sanitize: ok\n");
  return 0;
}
