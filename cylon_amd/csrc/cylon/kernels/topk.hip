// Top-k row selection (ORDER BY c LIMIT k): multi-pass MSD radix select over the key column's
// order image (gfx950).  No row is moved: the key column is read a few times and the operator
// (ops/topk.cpp) gathers k rows at the end.
//
// Semantics (docs/semantics.md, "Top-k"): the k rows that come first in the stable sort by the
// column.  The image is k_sort_keys' (order_image.hpp sort_key_image), so the select always looks
// for the k SMALLEST images; ties are broken by the lower row number; a row whose validity byte
// is 0 takes part in no histogram and no list.
//
// The select key of a row is the pair (image, row number).  A pass decides the next D = 11 bits
// of it from the top: first the varying bits of the image, then -- only when the image bits are
// exhausted and too many exact ties remain -- the bits of the row number.
//   k_topk_scan     one key read: OR / AND of the images and the non-null count.
//   k_topk_hist     one key read on persistent blocks: per-block LDS histogram (2048 x uint32 =
//                   8 KB) of the pass's digit over the rows whose decided bits equal the prefix,
//                   flushed with one global atomic per non-empty bin (integer counts: deterministic).
//                   LDS atomics on one address serialise, so a wave whose active lanes all hold
//                   the same digit adds its lane count once (sorted / constant / filtered input).
//   k_topk_pick     one block: the bin where the running count crosses k_rem; updates the state
//                   and zeroes the histogram.
//   k_topk_collect  one key read: rows below the threshold prefix -> "sure" (image, row) list,
//                   rows equal to it -> "candidate" list; one cursor atomic per wave and list.
//                   Both capacities are checked: nothing is written past a buffer.
//
// Loads: a lane reads 16 bytes per load (2 keys of 8 bytes, 16 of 1 byte), kTKUnroll loads are
// issued before the first is used, full tiles are unpredicated; the unaligned head of a sliced
// column and the partial last tile go through a bounds-checked element loop.
//
// State (int64 words at the start of the workspace, TKState below); the host reads it once per
// pass, which is the pass's only synchronisation.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): docs/design.md.
#include "device_common.hpp"
#include "order_image.hpp"

namespace cylon {
namespace hip {

constexpr int kTKThreads = 256;
constexpr int kTKUnroll = 4;      // 16-byte loads in flight per lane
constexpr int kTKDigitBits = 11;  // 2048 bins x 4 B = 8 KB of LDS: never the occupancy limit
constexpr int kTKBins = 1 << kTKDigitBits;

enum TKState : int {
  TK_PIMG = 0,   // decided image bits [ilo, ihi) as a number
  TK_ILO = 1,
  TK_IHI = 2,
  TK_PROW = 3,   // decided row-number bits [rlo, rhi)
  TK_RLO = 4,
  TK_RHI = 5,
  TK_KREM = 6,   // rows still to take from the threshold bucket
  TK_SURE = 7,   // rows strictly below the threshold prefix
  TK_BUCKET = 8, // rows equal to it
  TK_NONNULL = 9,
  TK_OR = 10,
  TK_AND = 11,
  TK_CUR_SURE = 12,
  TK_CUR_CAND = 13,
  TK_ERROR = 14,  // 1: a list outgrew its capacity, 2: the histogram does not reach k_rem
  TK_WORDS = 16,  // the histogram (kTKBins int64) follows
};

template <int W>
__device__ __forceinline__ uint64_t tk_extract(const uint4 &v, int e) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if (W == 8) return (uint64_t)w[2 * e] | ((uint64_t)w[2 * e + 1] << 32);
  if (W == 4) return w[e];
  if (W == 2) return (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
  return (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
}

// f(row, raw bits, live) for every row of the column; live = the row is not null.  Full tiles: every
// lane of the block calls f the same number of times.  head = leading elements before the first
// 16-byte boundary of c.data (< 16 / W, <= n).
template <int W, typename F>
__device__ __forceinline__ void tk_rows(const ColView &c, int64_t n, int64_t head, F &&f) {
  constexpr int E = 16 / W;
  constexpr int64_t kTile = (int64_t)kTKThreads * kTKUnroll * E;
  const uint4 *body = reinterpret_cast<const uint4 *>(c.data + head * W);
  const int64_t ntiles = (n - head) / kTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint4 v[kTKUnroll];
    const int64_t l0 = t * kTKUnroll * kTKThreads + threadIdx.x;  // index of this lane's first load
#pragma unroll
    for (int u = 0; u < kTKUnroll; ++u) v[u] = body[l0 + u * kTKThreads];
#pragma unroll
    for (int u = 0; u < kTKUnroll; ++u) {
      const int64_t r0 = head + (l0 + u * kTKThreads) * E;  // r0 + E <= head + ntiles * kTile <= n
#pragma unroll
      for (int e = 0; e < E; ++e) f(r0 + e, tk_extract<W>(v[u], e), c.valid == nullptr || c.valid[r0 + e] != 0);
    }
  }
  // the head and the partial last tile, element by element
  const int64_t tail0 = head + ntiles * kTile;
  const int64_t nrest = head + (n - tail0);
  for (int64_t i = (int64_t)blockIdx.x * kTKThreads + threadIdx.x; i < nrest; i += (int64_t)gridDim.x * kTKThreads) {
    const int64_t r = i < head ? i : tail0 + (i - head);  // r < n
    f(r, load_bits(c.data, r, W), c.valid == nullptr || c.valid[r] != 0);
  }
}

__global__ __launch_bounds__(kTKThreads) void k_topk_clear(int64_t *st) {
  for (int i = threadIdx.x; i < TK_WORDS + kTKBins; i += kTKThreads) st[i] = i == TK_AND ? -1 : 0;
}

template <int W>
__global__ __launch_bounds__(kTKThreads) void k_topk_scan(ColView c, int64_t n, int64_t head, bool desc,
                                                          int64_t *st) {
  uint64_t o = 0, a = ~0ull;
  unsigned long long cnt = 0;
  tk_rows<W>(c, n, head, [&](int64_t, uint64_t bits, bool live) {
    if (!live) return;
    const uint64_t k = sort_key_image(bits, W, c.kind, desc);
    o |= k;
    a &= k;
    ++cnt;
  });
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    o |= __shfl_xor(o, d, kWave);
    a &= __shfl_xor(a, d, kWave);
    cnt += __shfl_xor(cnt, d, kWave);
  }
  if (lane_id() == 0 && cnt) {
    unsigned long long *u = reinterpret_cast<unsigned long long *>(st);
    atomicOr(&u[TK_OR], (unsigned long long)o);
    atomicAnd(&u[TK_AND], (unsigned long long)a);
    atomicAdd(&u[TK_NONNULL], cnt);
  }
}

__global__ void k_topk_start(int64_t *st, int64_t k, int ihi, int rhi) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st[TK_PIMG] = 0;
  st[TK_ILO] = st[TK_IHI] = ihi;
  st[TK_PROW] = 0;
  st[TK_RLO] = st[TK_RHI] = rhi;
  st[TK_KREM] = k;
  st[TK_SURE] = 0;
  st[TK_BUCKET] = st[TK_NONNULL];
}

// the decided part of a row's select key
struct TKPrefix {
  uint64_t pimg, prow;
  int ilo, ihi, rlo, rhi;
};

__device__ __forceinline__ TKPrefix tk_prefix(const int64_t *st) {
  TKPrefix p;
  p.pimg = (uint64_t)st[TK_PIMG];
  p.prow = (uint64_t)st[TK_PROW];
  p.ilo = (int)st[TK_ILO];
  p.ihi = (int)st[TK_IHI];
  p.rlo = (int)st[TK_RLO];
  p.rhi = (int)st[TK_RHI];
  return p;
}

// one histogram increment per taking lane; a wave whose active lanes all take the same digit adds
// its lane count once
__device__ __forceinline__ void tk_hist_add(uint32_t *h, bool take, uint32_t digit) {
  const uint32_t v = take ? digit : 0xffffffffu;
  const uint32_t d0 = __builtin_amdgcn_readfirstlane(v);
  if (__all(v == d0)) {
    if (d0 == 0xffffffffu) return;  // no lane takes
    const unsigned long long act = __ballot(1);
    if (lane_id() == __ffsll(act) - 1) atomicAdd(&h[d0], (uint32_t)__popcll(act));
  } else if (take) {
    atomicAdd(&h[digit], 1u);
  }
}

// src 0: digit = image bits [ilo - db, ilo); src 1: row-number bits [rlo - db, rlo)
template <int W>
__global__ __launch_bounds__(kTKThreads) void k_topk_hist(ColView c, int64_t n, int64_t head, bool desc,
                                                          int64_t *st, int src, int db) {
  __shared__ uint32_t h[kTKBins];
  for (int b = threadIdx.x; b < kTKBins; b += kTKThreads) h[b] = 0;
  const TKPrefix p = tk_prefix(st);
  const int top = src ? p.rlo : p.ilo;
  __syncthreads();
  tk_rows<W>(c, n, head, [&](int64_t row, uint64_t bits, bool live) {
    const uint64_t k = sort_key_image(bits, W, c.kind, desc);
    const bool take = live && bit_field(k, p.ilo, p.ihi) == p.pimg && bit_field((uint64_t)row, p.rlo, p.rhi) == p.prow;
    tk_hist_add(h, take, (uint32_t)bit_field(src ? (uint64_t)row : k, top - db, top));
  });
  __syncthreads();
  unsigned long long *gh = reinterpret_cast<unsigned long long *>(st + TK_WORDS);
  for (int b = threadIdx.x; b < kTKBins; b += kTKThreads)
    if (h[b]) atomicAdd(&gh[b], (unsigned long long)h[b]);
}

__global__ __launch_bounds__(kTKThreads) void k_topk_pick(int64_t *st, int src, int db) {
  constexpr int kPer = kTKBins / kTKThreads;
  __shared__ int64_t part[kTKThreads];
  int64_t *gh = st + TK_WORDS;
  int64_t s = 0;
  for (int j = 0; j < kPer; ++j) s += gh[threadIdx.x * kPer + j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t krem = st[TK_KREM];
    int64_t cum = 0;
    int g = 0;
    while (g < kTKThreads && cum + part[g] < krem) cum += part[g++];
    int b = g * kPer;
    const int bend = g < kTKThreads ? b + kPer : b;
    while (b < bend && cum + gh[b] < krem) cum += gh[b++];
    if (b >= bend || krem <= 0) {
      st[TK_ERROR] = 2;
    } else {
      st[TK_SURE] += cum;
      st[TK_KREM] = krem - cum;
      st[TK_BUCKET] = gh[b];
      if (src) {
        st[TK_PROW] = (int64_t)(((uint64_t)st[TK_PROW] << db) | (uint64_t)b);
        st[TK_RLO] -= db;
      } else {
        st[TK_PIMG] = (int64_t)(((uint64_t)st[TK_PIMG] << db) | (uint64_t)b);
        st[TK_ILO] -= db;
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kTKBins; b += kTKThreads) gh[b] = 0;
}

// append (img, row) of every lane with p set: one cursor atomic per wave
__device__ __forceinline__ void tk_append(bool p, uint64_t img, int64_t row, uint64_t *oimg, int64_t *orow,
                                          int64_t cap, unsigned long long *cursor, int64_t *error) {
  const unsigned long long m = __ballot(p);
  if (m == 0) return;
  const int leader = __ffsll(m) - 1;
  unsigned long long base = 0;
  if (lane_id() == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, kWave);
  if (!p) return;
  const int64_t pos = (int64_t)base + __popcll(m & lanemask_lt());
  if (pos < cap) {
    oimg[pos] = img;
    orow[pos] = row;
  } else {
    *error = 1;
  }
}

template <int W>
__global__ __launch_bounds__(kTKThreads) void k_topk_collect(ColView c, int64_t n, int64_t head, bool desc,
                                                             int64_t *st, uint64_t *simg, int64_t *srow,
                                                             int64_t scap, uint64_t *cimg, int64_t *crow,
                                                             int64_t ccap) {
  const TKPrefix p = tk_prefix(st);
  unsigned long long *u = reinterpret_cast<unsigned long long *>(st);
  tk_rows<W>(c, n, head, [&](int64_t row, uint64_t bits, bool live) {
    const uint64_t k = sort_key_image(bits, W, c.kind, desc);
    const uint64_t fi = bit_field(k, p.ilo, p.ihi), fr = bit_field((uint64_t)row, p.rlo, p.rhi);
    const bool sure = live && (fi < p.pimg || (fi == p.pimg && fr < p.prow));
    const bool cand = live && fi == p.pimg && fr == p.prow;
    tk_append(sure, k, row, simg, srow, scap, &u[TK_CUR_SURE], &st[TK_ERROR]);
    tk_append(cand, k, row, cimg, crow, ccap, &u[TK_CUR_CAND], &st[TK_ERROR]);
  });
}

int topk_digit_bits() { return kTKDigitBits; }
int64_t topk_state_words() { return TK_WORDS; }
int64_t topk_workspace() { return TK_WORDS + kTKBins; }

static int64_t tk_head(const ColView &c, int64_t n) {
  const uint64_t mis = reinterpret_cast<uintptr_t>(c.data) % 16;
  const int64_t head = mis ? (int64_t)((16 - mis) / c.width) : 0;  // data is aligned to its width
  return std::min(head, n);
}

static int tk_grid(int64_t n, int w) {
  return grid_for(n, (int64_t)kTKThreads * kTKUnroll * (16 / w), (int64_t)kNumCUs * 8);
}

static void tk_check(const ColView &c) {
  CYLON_CHECK(c.data != nullptr && (c.width == 1 || c.width == 2 || c.width == 4 || c.width == 8) &&
                  reinterpret_cast<uintptr_t>(c.data) % c.width == 0,
              Code::Invalid, "top-k select: key column of width " << c.width);
}

#define TK_DISPATCH(kernel, c, ...)                                                                       \
  do {                                                                                                    \
    const dim3 g(tk_grid(n, (c).width)), b(kTKThreads);                                                   \
    switch ((c).width) {                                                                                  \
      case 1: hipLaunchKernelGGL(kernel<1>, g, b, 0, s, c, n, tk_head(c, n), __VA_ARGS__); break;         \
      case 2: hipLaunchKernelGGL(kernel<2>, g, b, 0, s, c, n, tk_head(c, n), __VA_ARGS__); break;         \
      case 4: hipLaunchKernelGGL(kernel<4>, g, b, 0, s, c, n, tk_head(c, n), __VA_ARGS__); break;         \
      default: hipLaunchKernelGGL(kernel<8>, g, b, 0, s, c, n, tk_head(c, n), __VA_ARGS__); break;        \
    }                                                                                                     \
    HIP_LAUNCH_CHECK();                                                                                   \
  } while (0)

void topk_scan(const ColView &col, int64_t n, bool desc, int64_t *ws, void *stream) {
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_topk_clear, dim3(1), dim3(kTKThreads), 0, s, ws);
  HIP_LAUNCH_CHECK();
  if (n == 0) return;
  tk_check(col);
  TK_DISPATCH(k_topk_scan, col, desc, ws);
}

void topk_start(int64_t *ws, int64_t k, int ihi, int rhi, void *stream) {
  hipLaunchKernelGGL(k_topk_start, dim3(1), dim3(1), 0, as_stream(stream), ws, k, ihi, rhi);
  HIP_LAUNCH_CHECK();
}

void topk_hist(const ColView &col, int64_t n, bool desc, int64_t *ws, int src, int db, void *stream) {
  CYLON_CHECK(db >= 1 && db <= kTKDigitBits, Code::Invalid, "top-k select: digit of " << db << " bits");
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  tk_check(col);
  TK_DISPATCH(k_topk_hist, col, desc, ws, src, db);
}

void topk_pick(int64_t *ws, int src, int db, void *stream) {
  hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kTKThreads), 0, as_stream(stream), ws, src, db);
  HIP_LAUNCH_CHECK();
}

void topk_collect(const ColView &col, int64_t n, bool desc, int64_t *ws, uint64_t *sure_img, int64_t *sure_row,
                  int64_t sure_cap, uint64_t *cand_img, int64_t *cand_row, int64_t cand_cap, void *stream) {
  if (n == 0) return;
  hipStream_t s = as_stream(stream);
  tk_check(col);
  TK_DISPATCH(k_topk_collect, col, desc, ws, sure_img, sure_row, sure_cap, cand_img, cand_row, cand_cap);
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_topk() { preload_code(reinterpret_cast<const void *>(&k_topk_pick)); }

}  // namespace hip
}  // namespace cylon
