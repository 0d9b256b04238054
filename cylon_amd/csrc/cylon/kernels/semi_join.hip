// LDS key-set existence join: left semi / left anti (gfx950).
//
// Semantics (docs/semantics.md, "Semi / anti join"): a left row survives a semi join iff some
// right row has an equal key, and an anti join iff none has.  Only the keys take part: exact
// int64 key images (ops/join_keys.cpp radix_keys), so key equality is image equality.
//
// MI355X design (no sort, no global hash table, no payload staging):
//   1. the host radix-partitions the right keys (8 B/row) and the left (key, row id) pairs
//      (16 B/row) by the top bits of fmix64(key), so that a partition's DISTINCT right keys fit
//      one LDS table.  A small right side is one partition and nothing is partitioned.
//   2. k_sj_build, one workgroup per partition: streams the partition's right keys once through
//      an LDS open-addressing set (64-bit LDS compare-and-swap) and writes each key that claims a
//      slot to a global buffer (<= kSJCap keys per partition) with their count.  A
//      duplicate finds its key by a plain LDS read, so a hot right key costs one slot and no
//      atomics, and can never overflow the table.
//   3. k_sj_probe, one work item = (partition, slice of <= kSJSlice of its left rows): loads the
//      partition's distinct keys (<= 32 KB) into its own LDS set and probes its slice.  A long
//      left partition (a hot left key, or the one partition of a small right side) is spread
//      over as many workgroups as its length warrants; consecutive items of one workgroup that
//      share a partition keep the table.
//   4. a matching row writes one byte of the mask at its row id (semi: 1 into zeros, anti: 0 into
//      ones); the host compacts the mask in ascending row id = left's input order.  *matched lets
//      the host skip the compaction when every row or no row survives.
//
// Every 64-bit value is a legal key.  The value 0 marks an empty slot, so the key 0 never enters
// the table: its presence is a flag of its own (szero / bit 32 of the partition's meta word).
//
// A partition with more than kSJCap distinct right keys sets *overflow; the mask is then
// undefined and the host takes the general path.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_sj_build: 32 VGPRs, 0 scratch, no spills, LDS 65552 B, occupancy 4 waves/SIMD;
//   k_sj_probe: 36 VGPRs, 0 scratch, no spills, LDS 65544 B, occupancy 4 waves/SIMD.
// The 64 KB table is what bounds both: two 512-thread workgroups per CU (160 KiB LDS).
#include "device_common.hpp"

namespace cylon {
namespace hip {

constexpr int kSJThreads = 512;
constexpr int kSJSlots = 8192;           // 8 B each: 64 KB, two workgroups per CU
constexpr int kSJCap = kSJSlots / 2;     // distinct keys per partition (load <= 0.5)
constexpr int64_t kSJSlice = 16384;      // left rows per work item
constexpr int kSJUnroll = 4;             // loads in flight per thread
constexpr unsigned long long kSJEmpty = 0ull;

static_assert((kSJSlots & (kSJSlots - 1)) == 0, "slot mask");

// the partition function takes the TOP bits of fmix64(key); the home slot takes the low ones
__device__ __forceinline__ uint32_t sj_home(uint64_t k) { return (uint32_t)hashing::fmix64(k) & (kSJSlots - 1); }

// k != kSJEmpty.  1: claimed a slot now, 0: already present, -1: no free slot
__device__ __forceinline__ int sj_insert(unsigned long long *tab, unsigned long long k) {
  uint32_t s = sj_home(k);
  for (int probes = 0; probes < kSJSlots; ++probes) {
    const unsigned long long cur = tab[s];
    if (cur == k) return 0;
    if (cur == kSJEmpty) {
      const unsigned long long prev = atomicCAS(&tab[s], kSJEmpty, k);
      if (prev == kSJEmpty) return 1;
      if (prev == k) return 0;
    }
    s = (s + 1) & (kSJSlots - 1);
  }
  return -1;
}

// k != kSJEmpty; the table holds <= kSJCap keys, so an empty slot ends every miss
__device__ __forceinline__ bool sj_contains(const unsigned long long *tab, unsigned long long k) {
  uint32_t s = sj_home(k);
  for (int probes = 0; probes < kSJSlots; ++probes) {
    const unsigned long long cur = tab[s];
    if (cur == k) return true;
    if (cur == kSJEmpty) return false;
    s = (s + 1) & (kSJSlots - 1);
  }
  return false;
}

// dkeys: the distinct non-zero keys of partition p, from dkeys[roffs[p]] on (never more than the
// partition's rows, so the buffer is as long as rkeys); dmeta[p] = their count, bit 32 set when the
// key 0 occurs, or -1 when the partition overflowed
__global__ __launch_bounds__(kSJThreads) void k_sj_build(const int64_t *__restrict__ rkeys,
                                                         const int64_t *__restrict__ roffs, int64_t nparts,
                                                         int64_t *__restrict__ dkeys, int64_t *__restrict__ dmeta,
                                                         int *overflow) {
  __shared__ unsigned long long tab[kSJSlots];
  __shared__ int scount, szero, sover;
  for (int64_t p = blockIdx.x; p < nparts; p += gridDim.x) {
    __syncthreads();  // the previous partition's meta word is written
    for (int s = threadIdx.x; s < kSJSlots; s += kSJThreads) tab[s] = kSJEmpty;
    if (threadIdx.x == 0) scount = szero = sover = 0;
    __syncthreads();
    const int64_t rb = roffs[p], re = roffs[p + 1];
    int64_t *out = dkeys + rb;  // distinct keys <= rows: stays inside the partition's range
    for (int64_t r0 = rb; r0 < re; r0 += kSJThreads * kSJUnroll) {
      if (*(volatile int *)&sover) break;  // the result is discarded: stop streaming
      unsigned long long k[kSJUnroll];
#pragma unroll
      for (int u = 0; u < kSJUnroll; ++u) {
        const int64_t r = r0 + u * kSJThreads + threadIdx.x;
        k[u] = r < re ? (unsigned long long)rkeys[r] : kSJEmpty;
      }
#pragma unroll
      for (int u = 0; u < kSJUnroll; ++u) {
        const int64_t r = r0 + u * kSJThreads + threadIdx.x;
        if (r >= re) continue;
        if (k[u] == kSJEmpty) {
          szero = 1;
          continue;
        }
        const int c = sj_insert(tab, k[u]);
        if (c > 0) {
          const int idx = atomicAdd(&scount, 1);
          if (idx < kSJCap) out[idx] = (int64_t)k[u];
          else sover = 1;
        } else if (c < 0) {
          sover = 1;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (sover) {
        atomicExch(overflow, 1);
        dmeta[p] = -1;
      } else {
        dmeta[p] = (int64_t)scount | ((int64_t)szero << 32);
      }
    }
  }
}

// item i: partition ipart[i], slice islice[i] (both nullptr: one partition, slice i)
__global__ __launch_bounds__(kSJThreads) void k_sj_probe(const int64_t *__restrict__ dkeys,
                                                         const int64_t *__restrict__ roffs,
                                                         const int64_t *__restrict__ dmeta,
                                                         const int64_t *__restrict__ lkeys,
                                                         const int64_t *__restrict__ lrow,
                                                         const int64_t *__restrict__ loffs,
                                                         const int64_t *__restrict__ ipart,
                                                         const int64_t *__restrict__ islice, int64_t nitems,
                                                         uint8_t val, uint8_t *__restrict__ mask,
                                                         unsigned long long *matched) {
  __shared__ unsigned long long tab[kSJSlots];
  __shared__ int szero;
  int64_t cur = -1;
  bool usable = false;
  unsigned long long wcount = 0;  // wave-uniform: this wave's matching rows
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t p = ipart ? ipart[item] : 0;
    const int64_t sl = islice ? islice[item] : item;
    if (p != cur) {  // block-uniform
      __syncthreads();  // every wave is done probing the previous table
      const int64_t meta = dmeta[p];
      for (int s = threadIdx.x; s < kSJSlots; s += kSJThreads) tab[s] = kSJEmpty;
      if (threadIdx.x == 0) szero = meta >= 0 && ((meta >> 32) & 1);
      __syncthreads();
      const int cnt = meta < 0 ? 0 : (int)(meta & 0xffffffff);  // <= kSJCap
      const int64_t *dk = dkeys + roffs[p];
      for (int i = threadIdx.x; i < cnt; i += kSJThreads) sj_insert(tab, (unsigned long long)dk[i]);
      __syncthreads();
      cur = p;
      usable = meta >= 0;
    }
    if (!usable) continue;  // overflowed partition: *overflow is set and the mask is discarded
    const int64_t pb = loffs[p], pe = loffs[p + 1];
    const int64_t b = pb + sl * kSJSlice;
    const int64_t e = b + kSJSlice < pe ? b + kSJSlice : pe;
    const bool has_zero = szero != 0;
    for (int64_t r0 = b; r0 < e; r0 += kSJThreads * kSJUnroll) {  // wave-uniform trip count
      unsigned long long k[kSJUnroll];
      int64_t rid[kSJUnroll];
#pragma unroll
      for (int u = 0; u < kSJUnroll; ++u) {
        const int64_t r = r0 + u * kSJThreads + threadIdx.x;
        k[u] = r < e ? (unsigned long long)lkeys[r] : kSJEmpty;
        rid[u] = r < e && lrow ? lrow[r] : r;
      }
#pragma unroll
      for (int u = 0; u < kSJUnroll; ++u) {
        const int64_t r = r0 + u * kSJThreads + threadIdx.x;
        const bool hit = r < e && (k[u] == kSJEmpty ? has_zero : sj_contains(tab, k[u]));
        if (hit) mask[rid[u]] = val;
        wcount += (unsigned long long)__popcll(__ballot(hit));
      }
    }
  }
  if (lane_id() == 0 && wcount) atomicAdd(matched, wcount);
}

int64_t semi_join_capacity() { return kSJCap; }
int64_t semi_join_slice_rows() { return kSJSlice; }

void semi_join_mark(const int64_t *rkeys, const int64_t *roffs, const int64_t *lkeys, const int64_t *lrow,
                    const int64_t *loffs, int64_t nparts, int anti, uint8_t *mask, int64_t *matched, int *overflow,
                    const int64_t *ipart, const int64_t *islice, int64_t nitems, int64_t *dkeys, int64_t *dmeta,
                    void *stream) {
  hipStream_t s = as_stream(stream);
  HIP_CHECK(hipMemsetAsync(matched, 0, sizeof(int64_t), s));
  HIP_CHECK(hipMemsetAsync(overflow, 0, sizeof(int), s));
  if (nparts == 0 || nitems == 0) return;
  CYLON_CHECK(nparts == 1 || (ipart && islice && lrow), Code::Invalid, "semi join: partitioned input without items");
  const int bgrid = (int)std::min<int64_t>(nparts, (int64_t)kNumCUs * 8);
  hipLaunchKernelGGL(k_sj_build, dim3(bgrid), dim3(kSJThreads), 0, s, rkeys, roffs, nparts, dkeys, dmeta, overflow);
  HIP_LAUNCH_CHECK();
  const int pgrid = (int)std::min<int64_t>(nitems, (int64_t)kNumCUs * 4);
  hipLaunchKernelGGL(k_sj_probe, dim3(pgrid), dim3(kSJThreads), 0, s, dkeys, roffs, dmeta, lkeys, lrow, loffs, ipart,
                     islice,
                     nitems, (uint8_t)(anti ? 0 : 1), mask, reinterpret_cast<unsigned long long *>(matched));
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_semi_join() { preload_code(reinterpret_cast<const void *>(&k_sj_build)); }

}  // namespace hip
}  // namespace cylon
