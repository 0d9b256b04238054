// Host sanitizer check of the CPU twin of the semi / anti join mark (kernels/cpu_semi.cpp): a few
// partition layouts, empty partitions, lrow == nullptr, against a brute-force scan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__=1 -I cylon_amd/csrc -I $ROCM_PATH/include \
//       tools/semi_join_sanitize.cpp cylon_amd/csrc/cylon/kernels/cpu_semi.cpp -o semi_join_sanitize
//   ./semi_join_sanitize          # prints "semi_join_sanitize: ok", exit status 0
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cylon/hash.hpp"
#include "cylon/kernels/kernels.hpp"

namespace {

int failures = 0;

// partition both sides by the top `bits` bits of fmix64(key), as RadixPartition does
void partition(const std::vector<int64_t> &keys, int bits, std::vector<int64_t> *pk, std::vector<int64_t> *prow,
               std::vector<int64_t> *offs) {
  const int64_t nparts = int64_t(1) << bits;
  auto part = [&](int64_t k) { return bits ? (int64_t)(cylon::hashing::fmix64((uint64_t)k) >> (64 - bits)) : 0; };
  offs->assign(nparts + 1, 0);
  for (int64_t k : keys) ++(*offs)[part(k) + 1];
  for (int64_t p = 0; p < nparts; ++p) (*offs)[p + 1] += (*offs)[p];
  std::vector<int64_t> at(offs->begin(), offs->end() - 1);
  pk->resize(keys.size());
  prow->resize(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    const int64_t d = at[part(keys[i])]++;
    (*pk)[d] = keys[i];
    (*prow)[d] = (int64_t)i;
  }
}

void run_case(const std::vector<int64_t> &lk, const std::vector<int64_t> &rk, int bits, bool anti, bool with_rows) {
  std::vector<int64_t> plk, plrow, loffs, prk, prrow, roffs;
  partition(lk, bits, &plk, &plrow, &loffs);
  partition(rk, bits, &prk, &prrow, &roffs);
  // exactly-sized heap buffers: an access one element out of range is a sanitizer report
  std::vector<uint8_t> mask(lk.size(), anti ? 1 : 0);
  int64_t matched = -1;
  int overflow = -1;
  cylon::cpu::semi_join_mark(prk.data(), roffs.data(), plk.data(), with_rows ? plrow.data() : nullptr, loffs.data(),
                             int64_t(1) << bits, anti ? 1 : 0, mask.data(), &matched, &overflow, nullptr, nullptr, 0,
                             nullptr, nullptr, nullptr);
  int64_t want = 0;
  for (size_t i = 0; i < lk.size(); ++i) {
    // without row ids the mask is indexed by position in the (identity-partitioned) left keys
    const int64_t key = with_rows ? lk[i] : plk[i];
    const bool hit = std::find(rk.begin(), rk.end(), key) != rk.end();
    want += hit;
    if (mask[i] != (uint8_t)(hit != anti)) ++failures;
  }
  if (matched != want || overflow != 0) ++failures;
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  auto keys = [&](size_t n, int64_t hi) {
    std::vector<int64_t> v(n);
    for (auto &x : v) x = (int64_t)(rng() % (uint64_t)hi) - hi / 4;
    if (n > 4) v[0] = INT64_MIN, v[1] = INT64_MAX, v[2] = 0, v[3] = -1;
    return v;
  };
  for (int anti = 0; anti < 2; ++anti) {
    run_case(keys(2000, 600), keys(700, 900), 0, anti, false);  // one partition, row id = position
    run_case(keys(2000, 600), keys(700, 900), 0, anti, true);
    run_case(keys(2000, 600), keys(700, 900), 3, anti, true);
    run_case(keys(300, 100000), keys(40, 100000), 8, anti, true);  // most partitions empty on either side
    run_case(keys(500, 50), {}, 4, anti, true);                    // empty right
    run_case({}, keys(500, 50), 4, anti, true);                    // empty left
    run_case({}, {}, 0, anti, false);
    run_case(std::vector<int64_t>(1000, 42), keys(64, 60), 2, anti, true);  // one hot left key
  }
  if (failures) {
    std::fprintf(stderr, "semi_join_sanitize: %d mismatches\n", failures);
    return 1;
  }
  std::printf("semi_join_sanitize: ok\n");
  return 0;
}
