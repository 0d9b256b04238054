// Host sanitizer check of the CPU twin of the top-k radix select (kernels/cpu_topk.cpp): scan / start /
// hist / pick / collect driven as ops/topk.cpp drives them, over tiny inputs in exactly-sized heap
// buffers, against a brute-force std::stable_sort.  Also the collect's capacity check: lists that are
// too short must set the error word and never be written past.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/topk_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_topk.cpp -o topk_sanitize
//   ./topk_sanitize          # prints "topk_sanitize: ok", exit status 0
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

// the k first non-null rows in (image, row) order
std::vector<int64_t> brute(const std::vector<int64_t> &keys, const std::vector<uint8_t> &valid, bool desc, int64_t k) {
  std::vector<int64_t> rows;
  for (size_t i = 0; i < keys.size(); ++i)
    if (valid.empty() || valid[i]) rows.push_back((int64_t)i);
  auto img = [&](int64_t r) {
    return sort_key_image((uint64_t)keys[r], 8, static_cast<int>(ValueKind::SIGNED_INT), desc);
  };
  std::stable_sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) { return img(a) < img(b); });
  if ((int64_t)rows.size() > k) rows.resize(k);
  return rows;
}

// short_by: allocate the lists this many entries short of what the state says (the capacity check)
void run_case(const std::vector<int64_t> &keys, const std::vector<uint8_t> &valid, bool desc, int64_t k,
              int64_t candidates, int64_t short_by = 0) {
  const int64_t n = (int64_t)keys.size();
  ColView c;
  c.data = reinterpret_cast<const uint8_t *>(keys.data());
  c.valid = valid.empty() ? nullptr : valid.data();
  c.width = 8;
  c.kind = static_cast<int>(ValueKind::SIGNED_INT);
  std::vector<int64_t> ws((size_t)cpu::topk_workspace());
  cpu::topk_scan(c, n, desc, ws.data(), nullptr);
  const int64_t nonnull = ws[9], take = std::min(k, nonnull);
  const std::vector<int64_t> want = brute(keys, valid, desc, k);
  if ((int64_t)want.size() != take) ++failures;
  if (take == 0) return;
  const uint64_t diff = (uint64_t)ws[10] ^ (uint64_t)ws[11];
  const int ihi = diff ? 64 - __builtin_clzll(diff) : 0, ifloor = diff ? __builtin_ctzll(diff) : 0;
  const int rbits = n > 1 ? 64 - __builtin_clzll((uint64_t)(n - 1)) : 0;
  cpu::topk_start(ws.data(), take, ihi, rbits, nullptr);
  const int D = cpu::topk_digit_bits();
  while (ws[8] > candidates && ((int)ws[1] > ifloor || ws[4] > 0)) {
    const int src = (int)ws[1] > ifloor ? 0 : 1;
    const int db = std::min(D, src ? (int)ws[4] : (int)ws[1] - ifloor);
    cpu::topk_hist(c, n, desc, ws.data(), src, db, nullptr);
    cpu::topk_pick(ws.data(), src, db, nullptr);
    if (ws[14] != 0) {
      ++failures;
      return;
    }
  }
  const int64_t sure = ws[7], bucket = ws[8], krem = ws[6];
  const int64_t scap = std::max<int64_t>(0, sure - short_by), ccap = std::max<int64_t>(0, bucket - short_by);
  std::vector<uint64_t> simg((size_t)scap), cimg((size_t)ccap);
  std::vector<int64_t> srow((size_t)scap), crow((size_t)ccap);
  cpu::topk_collect(c, n, desc, ws.data(), simg.data(), srow.data(), scap, cimg.data(), crow.data(), ccap, nullptr);
  if (short_by > 0) {  // at least the candidate list (bucket >= 1) was too short
    if (ws[14] != 1) ++failures;
    return;
  }
  if (ws[14] != 0 || ws[12] != sure || ws[13] != bucket || krem < 1 || krem > bucket || sure + krem != take) {
    ++failures;
    return;
  }
  auto by_image_row = [](std::vector<uint64_t> &img, std::vector<int64_t> &row) {
    std::vector<size_t> p(img.size());
    std::iota(p.begin(), p.end(), 0);
    std::sort(p.begin(), p.end(),
              [&](size_t a, size_t b) { return img[a] != img[b] ? img[a] < img[b] : row[a] < row[b]; });
    std::vector<uint64_t> i2;
    std::vector<int64_t> r2;
    for (size_t x : p) i2.push_back(img[x]), r2.push_back(row[x]);
    img.swap(i2);
    row.swap(r2);
  };
  by_image_row(cimg, crow);
  simg.insert(simg.end(), cimg.begin(), cimg.begin() + krem);
  srow.insert(srow.end(), crow.begin(), crow.begin() + krem);
  by_image_row(simg, srow);
  if (srow != want) ++failures;
}

}  // namespace

int main() {
  std::mt19937_64 rng(11);
  for (int64_t n : {0, 1, 63, 64, 65, 3000}) {
    std::vector<std::vector<int64_t>> keysets;
    std::vector<int64_t> v((size_t)n);
    for (auto &x : v) x = (int64_t)rng();
    if (n > 4) v[0] = INT64_MIN, v[1] = INT64_MAX, v[2] = 0, v[3] = -1;
    keysets.push_back(v);
    keysets.push_back(std::vector<int64_t>((size_t)n, 42));  // all equal: the row number decides
    for (auto &x : v) x = (int64_t)(rng() % 5) - 2;          // heavy ties
    keysets.push_back(v);
    for (const auto &keys : keysets) {
      std::vector<uint8_t> some((size_t)n), none((size_t)n, 0);
      for (auto &b : some) b = rng() % 10 < 7;
      for (const auto &valid : {std::vector<uint8_t>(), some, none}) {
        if (n == 0 && !valid.empty()) continue;
        for (int desc = 0; desc < 2; ++desc)
          for (int64_t k : {int64_t(1), n / 2, n - 1, n})  // both ends
            for (int64_t candidates : {int64_t(1), int64_t(8), int64_t(1) << 20}) {
              if (k < 1) continue;
              run_case(keys, valid, desc != 0, k, candidates);
              run_case(keys, valid, desc != 0, k, candidates, 1);
            }
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "topk_sanitize: %d mismatches\n", failures);
    return 1;
  }
  std::printf("topk_sanitize: ok\n");
  return 0;
}
