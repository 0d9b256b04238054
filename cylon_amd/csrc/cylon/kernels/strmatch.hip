// K15 string predicates on the device (gfx950): comparison (== != < <= > >=) of a string / binary
// column with a scalar or a column, starts_with / ends_with / contains, SQL LIKE and the byte /
// code-point length, without a host round trip through Arrow (docs/semantics.md "String
// predicates").  The cell matchers are the __host__ __device__ functions of strmatch_common.hpp,
// shared with the CPU twin (cpu_strings.cpp).
//
// Every predicate is a bandwidth problem over (offsets, bytes) with one output byte or word per
// row.  Two kinds of kernel:
//   * prefix kind (k_str_prefix, k_str_byte_length): comparison with a scalar, starts_with,
//     ends_with, equality and the byte length need at most |pattern| + 1 bytes of a row, so nothing
//     is staged.  One thread per row; the pattern is read once per block into LDS (a scalar longer
//     than kStrMaxPatternBytes is read from global memory, where every lane reads the same bytes).
//   * whole-row kind (k_str_rows: contains, the general LIKE matcher, the code-point length;
//     k_str_compare_cols: column against column): a block owns kBlock = 256 consecutive rows.
//       - staged path, byte span of the 256 rows <= kTile: the block copies the span into LDS with
//         coalesced loads (16-byte vectors over the aligned body, byte loads for the ragged head and
//         tail; the LDS image keeps the source's alignment modulo 16), then one thread per row runs
//         its matcher out of LDS.  A block with a null row copies row by row instead and skips the
//         null rows, so their bytes are never read.
//       - long-row path otherwise (the choice is uniform per block): the block's four waves take
//         its rows one wave per row.  contains: the lanes test 64 consecutive start positions per
//         step against the pattern in LDS and ballot.  Column against column: 64 bytes per step,
//         the first differing lane decides.  Code-point length: per-lane counts and a wave
//         reduction.  General LIKE: lane 0 walks the row from global memory -- the accepted slow
//         path (a LIKE pattern of another shape than lit%, %lit, %lit% over long rows).
// kTile = 16 KiB: a k_str_rows block holds one tile and the pattern (18.7 KB), so even the eight
// 256-thread blocks that would fill a CU's 32 wave slots take 150 KB of its 160 KiB of LDS -- LDS
// never bounds the occupancy (the kernel's 78 VGPRs do, at six blocks per CU).
// k_str_compare_cols holds two tiles (33 KB): four blocks = 16 waves per CU, enough to cover the
// copy's latency.  At the engine's usual 8-32-byte keys a block's span is 2-8 KiB, far inside the
// tile.
//
// Memory safety: no load touches a byte outside [data + offsets[0], data + offsets[n]) of the
// column it reads -- the vector loads cover only whole 16-byte groups inside the block's span --
// and none touches the bytes of a null row.  All positions and spans are 64-bit.
// Reference: pycylon compute (python/pycylon/pycylon/data/compute.pyx) compares string columns
// with Arrow's host kernels; it has no substring / LIKE operators.
#include "device_common.hpp"
#include "strmatch_common.hpp"
#include "strstage.hpp"

namespace cylon {
namespace hip {

using namespace strmatch;

constexpr int kTile = kStrTileBytes;

int64_t string_tile_bytes() { return kTile; }

// k_str_prefix modes beyond the StrMatchKind values it takes as they are
constexpr int kPrefixCompare = 16;

// pat_offs != nullptr: the pattern is row 0 of a one-row column (pat = its bytes, plen unused)
__global__ void __launch_bounds__(kBlock)
k_str_prefix(ColView a, int mode, int op, const uint8_t *__restrict__ pat, const int64_t *__restrict__ pat_offs,
             int64_t plen, int utf8, int64_t n, uint8_t *__restrict__ out) {
  __shared__ uint8_t spat[kStrMaxPatternBytes];
  if (pat_offs != nullptr) {
    plen = pat_offs[1] - pat_offs[0];
    pat += pat_offs[0];
  }
  const uint8_t *p = pat;
  if (plen <= kStrMaxPatternBytes) {
    for (int k = threadIdx.x; k < plen; k += blockDim.x) spat[k] = pat[k];
    __syncthreads();
    p = spat;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint8_t r = 0;
    if (a.valid == nullptr || a.valid[i] != 0) {
      const int64_t b = a.offsets[i], len = a.offsets[i + 1] - b;
      const uint8_t *s = a.data + b;
      switch (mode) {
        case STR_STARTS_WITH: r = sm_starts_with(s, len, p, plen, utf8); break;
        case STR_ENDS_WITH: r = sm_ends_with(s, len, p, plen, utf8); break;
        case STR_EQUALS: r = sm_equals(s, len, p, plen); break;
        default: r = sm_cmp_result(sm_compare(s, len, p, plen), op); break;
      }
    }
    out[i] = r;
  }
}

__global__ void __launch_bounds__(kBlock)
k_str_byte_length(ColView a, int64_t n, int64_t *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = (a.valid == nullptr || a.valid[i] != 0) ? a.offsets[i + 1] - a.offsets[i] : 0;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor((long long)v, d, kWave);
  return v;
}

// fn: STR_CONTAINS (pat: plen bytes), STR_LIKE (pat: plen token kinds, then plen token bytes) or
// -1 = code-point length (out64)
__global__ void __launch_bounds__(kBlock)
k_str_rows(ColView a, int fn, const uint8_t *__restrict__ pat, int plen, int utf8, int64_t n,
           uint8_t *__restrict__ out8, int64_t *__restrict__ out64) {
  __shared__ __align__(16) uint8_t tile[kTile + 16];
  __shared__ uint8_t spat[2 * kStrMaxPatternBytes];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int pbytes = fn == STR_LIKE ? 2 * plen : (fn == STR_CONTAINS ? plen : 0);
  for (int k = tid; k < pbytes; k += kBlock) spat[k] = pat[k];
  __syncthreads();
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r0 = blk * kBlock, r1 = r0 + kBlock < n ? r0 + kBlock : n;
    const int64_t b0 = a.offsets[r0], span = a.offsets[r1] - b0;
    if (span <= kTile) {
      const int shift = stage_rows(a, a.valid, nullptr, r0, r1, tile);
      const int64_t r = r0 + tid;
      if (r < r1) {
        int64_t v = 0;
        if (a.valid == nullptr || a.valid[r] != 0) {
          const int64_t b = a.offsets[r], len = a.offsets[r + 1] - b;
          const uint8_t *s = tile + shift + (int)(b - b0);
          if (fn == STR_CONTAINS) v = sm_contains(s, len, spat, plen, utf8);
          else if (fn == STR_LIKE) v = sm_like(s, len, spat, spat + plen, plen, utf8);
          else v = sm_count_chars(s, len);
        }
        if (out64 != nullptr) out64[r] = v;
        else out8[r] = (uint8_t)v;
      }
      __syncthreads();  // the next block of rows overwrites the tile
    } else {
      for (int64_t r = r0 + tid / kWave; r < r1; r += kRowWaves) {  // r is uniform in a wave
        int64_t v = 0;
        if (a.valid == nullptr || a.valid[r] != 0) {
          const int64_t b = a.offsets[r], len = a.offsets[r + 1] - b;
          const uint8_t *s = a.data + b;
          if (fn == STR_CONTAINS) {
            for (int64_t base = 0; base + plen <= len; base += kWave) {
              const int64_t i = base + lane;
              const bool hit = i + plen <= len && sm_match_at(s, len, i, spat, plen, utf8);
              if (__ballot(hit) != 0) {
                v = 1;
                break;
              }
            }
          } else if (fn == STR_LIKE) {
            if (lane == 0) v = sm_like(s, len, spat, spat + plen, plen, utf8);
          } else {
            int64_t c = 0;
            for (int64_t i = lane; i < len; i += kWave) c += sm_is_cont(s[i]) ? 0 : 1;
            v = wave_sum(c);
          }
        }
        if (lane == 0) {
          if (out64 != nullptr) out64[r] = v;
          else out8[r] = (uint8_t)v;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock)
k_str_compare_cols(ColView a, ColView b, int op, int64_t n, uint8_t *__restrict__ out) {
  __shared__ __align__(16) uint8_t tile_a[kTile + 16];
  __shared__ __align__(16) uint8_t tile_b[kTile + 16];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r0 = blk * kBlock, r1 = r0 + kBlock < n ? r0 + kBlock : n;
    const int64_t a0 = a.offsets[r0], b0 = b.offsets[r0];
    if (a.offsets[r1] - a0 <= kTile && b.offsets[r1] - b0 <= kTile) {
      const int sha = stage_rows(a, a.valid, b.valid, r0, r1, tile_a);
      const int shb = stage_rows(b, a.valid, b.valid, r0, r1, tile_b);
      const int64_t r = r0 + tid;
      if (r < r1) {
        uint8_t v = 0;
        if (row_live(a.valid, b.valid, r)) {
          const int64_t ab = a.offsets[r], bb = b.offsets[r];
          v = sm_cmp_result(sm_compare(tile_a + sha + (int)(ab - a0), a.offsets[r + 1] - ab,
                                       tile_b + shb + (int)(bb - b0), b.offsets[r + 1] - bb), op);
        }
        out[r] = v;
      }
      __syncthreads();  // the next block of rows overwrites the tiles
    } else {
      for (int64_t r = r0 + tid / kWave; r < r1; r += kRowWaves) {  // r is uniform in a wave
        uint8_t v = 0;
        if (row_live(a.valid, b.valid, r)) {
          const int64_t ab = a.offsets[r], bb = b.offsets[r];
          const int64_t la = a.offsets[r + 1] - ab, lb = b.offsets[r + 1] - bb, m = la < lb ? la : lb;
          const uint8_t *sa = a.data + ab, *sb = b.data + bb;
          int c = 0;
          for (int64_t base = 0; base < m; base += kWave) {
            const int64_t i = base + lane;
            const uint64_t diff = __ballot(i < m && sa[i] != sb[i]);
            if (diff != 0) {
              const int64_t f = base + __builtin_ctzll(diff);
              c = sa[f] < sb[f] ? -1 : 1;
              break;
            }
          }
          if (c == 0) c = la < lb ? -1 : (la > lb ? 1 : 0);
          v = sm_cmp_result(c, op);
        }
        if (lane == 0) out[r] = v;
      }
    }
  }
}

void str_compare(const ColView &a, const ColView &b, int b_scalar, int op, int64_t n, uint8_t *out, void *stream) {
  if (n == 0) return;
  if (b_scalar) {
    hipLaunchKernelGGL(k_str_prefix, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, kPrefixCompare, op,
                       b.data, b.offsets, (int64_t)0, 0, n, out);
  } else {
    hipLaunchKernelGGL(k_str_compare_cols, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, b, op, n, out);
  }
  HIP_LAUNCH_CHECK();
}

void str_match(const ColView &a, int kind, const uint8_t *pat, int64_t plen, int utf8, int64_t n, uint8_t *out,
               void *stream) {
  CYLON_CHECK(plen >= 0 && plen <= kStrMaxPatternBytes, Code::Invalid,
              "string match: a pattern of " << plen << " bytes (at most " << kStrMaxPatternBytes << ")");
  CYLON_CHECK(kind >= STR_STARTS_WITH && kind <= STR_EQUALS, Code::Invalid, "string match: kind " << kind);
  if (n == 0) return;
  if (kind == STR_CONTAINS || kind == STR_LIKE) {
    hipLaunchKernelGGL(k_str_rows, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, kind, pat, (int)plen,
                       utf8, n, out, (int64_t *)nullptr);
  } else {
    hipLaunchKernelGGL(k_str_prefix, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, kind, 0, pat,
                       (const int64_t *)nullptr, plen, utf8, n, out);
  }
  HIP_LAUNCH_CHECK();
}

void str_length(const ColView &a, int unit, int64_t n, int64_t *out, void *stream) {
  if (n == 0) return;
  if (unit == STR_LEN_BYTES) {
    hipLaunchKernelGGL(k_str_byte_length, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, n, out);
  } else {
    hipLaunchKernelGGL(k_str_rows, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, -1,
                       (const uint8_t *)nullptr, 0, 1, n, (uint8_t *)nullptr, out);
  }
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_strmatch() { preload_code(reinterpret_cast<const void *>(&k_str_prefix)); }

}  // namespace hip
}  // namespace cylon
