// K15 string transforms on the device (gfx950): slice, strip / lstrip / rstrip, ASCII upper / lower,
// element-wise concat and literal replace of a string / binary column, each producing a new
// variable-width column without a host round trip through Arrow (docs/semantics.md "String
// transforms").  The cell functions are the __host__ __device__ functions of strxform_common.hpp,
// shared with the CPU twin (cpu_strxform.cpp).
//
// Every function is two passes around the engine's exclusive scan:
//   * lengths.  The byte slice, concat and case need only the offsets: one thread per row
//     (k_strx_len_offsets).  The code-point slice, strip and replace need the bytes: a block of
//     kBlock = 256 rows stages its input span in LDS and runs one thread per row, as strmatch.hip's
//     k_str_rows does (k_strx_len_rows).
//   * write (k_strx_write<FN>).  A block owns 256 consecutive rows (128 for concat, see below).  When
//     its input span(s) and its output span fit their tiles:
//       1. the input rows are staged (strstage.hpp; null rows are skipped, so their bytes are never
//          read);
//       2. each thread composes its row into a second LDS tile at out_off[r] - out_off[r0] + shift,
//          shift = the destination address modulo 16;
//       3. the block flushes that tile: byte stores for the ragged head and tail, uint4 stores for
//          the whole 16-byte groups strictly inside the block's output span -- a 16-byte group shared
//          with a neighbouring block is never written as a vector.
//     Otherwise (the choice is uniform per block) the block's four waves take its rows one wave per
//     row and copy from global memory: slice and strip find their kept range with ballots over 64
//     bytes per step, replace tests 64 start positions per step and resolves the leftmost
//     non-overlapping matches from the ballot mask (uniform in the wave), copying the pieces between
//     them.  This is the slow path: its stores are as ragged as the rows.
//   * case on a column without validity stages nothing: one flat map over [offsets[0], offsets[n])
//     with 16-byte vector stores, and the rebased offsets (k_strx_case_flat).  With validity it
//     takes the general path, so that the bytes of null rows stay unread.
//   * upper / lower also report whether a live row held a byte >= 0x80: one block-level OR and one
//     vector atomic per block into a device word.
//
// LDS: k_strx_write holds an input tile and an output tile of kTile = 16 KiB (+16 for the shift) and
// 2 KiB of literals (pattern and replacement, or the strip set, or the separator): 34.9 KB per block,
// four blocks = 16 waves per CU of its 160 KiB -- the budget strmatch.hip's k_str_compare_cols argues
// for.  Concat stages two inputs; with three full tiles (51 KB) only three blocks would fit, so its
// block owns 128 rows and its input tiles are 8 KiB each: the same 34.9 KB.
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch or VGPR
// spills; the SGPR spills go to VGPR lanes.  Every write kernel fits 4 waves per SIMD = 16 waves = four
// blocks per CU by registers, which is exactly what its LDS allows, so neither bound wastes the other:
//   kernel                      VGPRs  SGPR spills  LDS bytes  waves/SIMD
//   k_strx_write<SX_SLICE>        105       25        35 104       4
//   k_strx_write<SX_STRIP>        105       25        35 104       4
//   k_strx_write<SX_CASE>          93        0        33 056       4
//   k_strx_write<SX_CONCAT>       119       25        35 120       4
//   k_strx_write<SX_REPLACE>      110       38        35 104       4
//   k_strx_len_rows                87        6        18 704       5
//   k_strx_len_offsets             12        0             0       8
//   k_strx_case_flat               28        0           256       8
//
// Memory safety: no load touches a byte outside [data + offsets[0], data + offsets[n]) of a column it
// reads, and none touches the bytes of a null row; no store touches a byte outside [out, out + total),
// total = out_off[n]: a row writes exactly the length the lengths pass computed for it with the same
// cell function, and the vector stores cover only whole 16-byte groups inside a block's own output
// span.  All spans and positions are 64-bit.
// Reference: pycylon has no string transforms; pandas-style callers run them on the host.
#include "device_common.hpp"
#include "strstage.hpp"
#include "strxform_common.hpp"

namespace cylon {
namespace hip {

using namespace strxform;

namespace {

constexpr int kTile = strmatch::kStrTileBytes;
constexpr int kLitBytes = 2 * kStrMaxPatternBytes;

__device__ __forceinline__ int lit_bytes(const StrXform &x) {
  return x.fn == SX_STRIP ? kStrSetBytes : (x.fn == SX_CONCAT ? x.len1 : (x.fn == SX_REPLACE ? x.len1 + x.len2 : 0));
}

__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor((long long)v, d, kWave);
  return v;
}

// one wave copies len bytes: 16-byte vectors when src and dst agree modulo 16, else bytes
__device__ __forceinline__ void wave_copy(const uint8_t *src, uint8_t *dst, int64_t len, int lane) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
  if (len >= 64 && ((sa ^ da) & 15u) == 0) {
    const int64_t head = (int64_t)((16u - (sa & 15u)) & 15u);
    for (int64_t k = lane; k < head; k += kWave) dst[k] = src[k];
    const int64_t nv = (len - head) >> 4;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (int64_t k = lane; k < nv; k += kWave) d4[k] = s4[k];
    for (int64_t k = head + (nv << 4) + lane; k < len; k += kWave) dst[k] = src[k];
  } else {
    for (int64_t k = lane; k < len; k += kWave) dst[k] = src[k];
  }
}

// ---- one wave over one long row in global memory (every result is uniform in the wave) ----------
__device__ __forceinline__ int64_t wave_count_units(const uint8_t *s, int64_t n, int lane) {
  int64_t c = 0;
  for (int64_t i = lane; i < n; i += kWave) c += sx_unit_start(s, i) ? 1 : 0;
  return wave_sum64(c);
}

// sx_unit_pos: the byte at which unit k begins, n when there is no such unit
__device__ __forceinline__ int64_t wave_unit_pos(const uint8_t *s, int64_t n, int64_t k, int lane) {
  for (int64_t base = 0; base < n; base += kWave) {
    const int64_t i = base + lane;
    uint64_t m = __ballot(i < n && sx_unit_start(s, i));
    const int c = __popcll(m);
    if (k < c) {
      for (int64_t j = 0; j < k; ++j) m &= m - 1;
      return base + __builtin_ctzll(m);
    }
    k -= c;
  }
  return n;
}

// sx_slice_range / sx_strip_range
__device__ __forceinline__ void wave_range(const StrXform &x, const uint8_t *s, int64_t n, const uint8_t *set,
                                           int lane, int64_t *b, int64_t *e) {
  if (x.fn == SX_SLICE) {
    if (!x.utf8) {
      sx_slice_units(n, x.start, x.stop, x.has_stop, b, e);
      return;
    }
    const bool from_end = x.start < 0 || (x.has_stop && x.stop < 0);
    int64_t ub, ue;
    if (from_end) {
      sx_slice_units(wave_count_units(s, n, lane), x.start, x.stop, x.has_stop, &ub, &ue);
    } else {
      ub = x.start;
      ue = x.has_stop ? (x.stop < ub ? ub : x.stop) : -1;
    }
    *b = wave_unit_pos(s, n, ub, lane);
    *e = ue < 0 ? n : (ue == ub ? *b : wave_unit_pos(s, n, ue, lane));
    return;
  }
  int64_t lo = 0, hi = n;
  if (x.side & SX_LEFT) {
    lo = n;
    for (int64_t base = 0; base < n; base += kWave) {
      const int64_t i = base + lane;
      const uint64_t m = __ballot(i < n && !sx_in_set(set, s[i]));
      if (m != 0) {
        lo = base + __builtin_ctzll(m);
        break;
      }
    }
  }
  if (x.side & SX_RIGHT) {
    int64_t top = n;
    hi = lo;
    for (; top > lo; top -= kWave) {
      const int64_t i = top - 1 - lane;  // lane 0 tests the last byte
      const uint64_t m = __ballot(i >= lo && !sx_in_set(set, s[i]));
      if (m != 0) {
        hi = top - __builtin_ctzll(m);
        break;
      }
    }
  }
  *b = lo;
  *e = hi;
}

// sx_replace_len / sx_replace_write: p (np > 0 bytes) and r (nr bytes) are in LDS.  Returns the output
// length; kWrite: also writes it at d.
template <bool kWrite>
__device__ __forceinline__ int64_t wave_replace(const uint8_t *s, int64_t n, const uint8_t *p, int64_t np,
                                                const uint8_t *r, int64_t nr, int64_t max_repl, uint8_t *d,
                                                int lane) {
  int64_t cnt = 0, next = 0, src = 0, o = 0;
  bool capped = max_repl == 0;
  for (int64_t base = 0; base + np <= n && !capped; base += kWave) {
    const int64_t i = base + lane;
    uint64_t m = __ballot(i + np <= n && strmatch::sm_bytes_equal(s + i, p, np));
    while (m != 0) {
      const int64_t pos = base + __builtin_ctzll(m);
      m &= m - 1;
      if (pos < next) continue;  // overlaps the match before it
      ++cnt;
      next = pos + np;
      if (kWrite) {
        wave_copy(s + src, d + o, pos - src, lane);
        o += pos - src;
        for (int64_t k = lane; k < nr; k += kWave) d[o + k] = r[k];
        o += nr;
        src = next;
      }
      if (max_repl >= 0 && cnt >= max_repl) {
        capped = true;
        break;
      }
    }
  }
  if (kWrite) wave_copy(s + src, d + o, n - src, lane);
  return n + cnt * (nr - np);
}

// ---- lengths ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_strx_len_offsets(ColView a, ColView b, StrXform x, int64_t n, int64_t *__restrict__ lens) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint8_t *vb = x.fn == SX_CONCAT ? b.valid : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t v = 0;
    if (row_live(a.valid, vb, i)) {
      const int64_t ra = x.a_bcast ? 0 : i;
      const int64_t la = a.offsets[ra + 1] - a.offsets[ra];
      if (x.fn == SX_CONCAT) {
        const int64_t rb = x.b_bcast ? 0 : i;
        v = la + x.len1 + (b.offsets[rb + 1] - b.offsets[rb]);
      } else if (x.fn == SX_SLICE) {
        int64_t lo, hi;
        sx_slice_units(la, x.start, x.stop, x.has_stop, &lo, &hi);
        v = hi - lo;
      } else {
        v = la;
      }
    }
    lens[i] = v;
  }
}

__global__ void __launch_bounds__(kBlock)
k_strx_len_rows(ColView a, StrXform x, const uint8_t *__restrict__ lit, int64_t n, int64_t *__restrict__ lens) {
  __shared__ __align__(16) uint8_t tile[kTile + 16];
  __shared__ uint8_t slit[kLitBytes];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int nlit = lit_bytes(x);
  for (int k = tid; k < nlit; k += kBlock) slit[k] = lit[k];
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
        if (row_live(a.valid, nullptr, r)) {
          const int64_t rb = a.offsets[r];
          v = sx_cell_len(x, tile + shift + (int)(rb - b0), a.offsets[r + 1] - rb, slit);
        }
        lens[r] = v;
      }
      __syncthreads();  // the next block of rows overwrites the tile
    } else {
      for (int64_t r = r0 + tid / kWave; r < r1; r += kRowWaves) {  // r is uniform in a wave
        int64_t v = 0;
        if (row_live(a.valid, nullptr, r)) {
          const int64_t rb = a.offsets[r], len = a.offsets[r + 1] - rb;
          const uint8_t *s = a.data + rb;
          if (x.fn == SX_REPLACE) {
            v = wave_replace<false>(s, len, slit, x.len1, slit + x.len1, x.len2, x.max_repl, nullptr, lane);
          } else {
            int64_t lo, hi;
            wave_range(x, s, len, slit, lane, &lo, &hi);
            v = hi - lo;
          }
        }
        if (lane == 0) lens[r] = v;
      }
    }
  }
}

// ---- write --------------------------------------------------------------------------------------
template <int FN>
__global__ void __launch_bounds__(kBlock)
k_strx_write(ColView a, ColView b, StrXform x, const uint8_t *__restrict__ lit, int64_t n,
             const int64_t *__restrict__ out_off, uint8_t *__restrict__ out, unsigned int *__restrict__ flag) {
  constexpr bool kCat = FN == SX_CONCAT;
  constexpr int kRows = kCat ? kBlock / 2 : kBlock;
  constexpr int kIn = kCat ? kTile / 2 : kTile;
  __shared__ __align__(16) uint8_t tile_a[kIn + 16];
  __shared__ __align__(16) uint8_t tile_b[kCat ? kIn + 16 : 16];
  __shared__ __align__(16) uint8_t tile_o[kTile + 16];
  __shared__ uint8_t slit[kLitBytes];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int nlit = lit_bytes(x);
  for (int k = tid; k < nlit; k += kBlock) slit[k] = lit[k];
  __syncthreads();
  const uint8_t *va = a.valid, *vb = kCat ? b.valid : nullptr;  // a broadcast operand has no validity here
  const int abc = kCat ? x.a_bcast : 0, bbc = kCat ? x.b_bcast : 0;
  unsigned int high = 0;  // SX_CASE: the OR of the live bytes
  const int64_t nblk = (n + kRows - 1) / kRows;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r0 = blk * kRows, r1 = r0 + kRows < n ? r0 + kRows : n;
    const int64_t ar0 = abc ? 0 : r0, ar1 = abc ? 1 : r1, br0 = bbc ? 0 : r0, br1 = bbc ? 1 : r1;
    const int64_t a0 = a.offsets[ar0], aspan = a.offsets[ar1] - a0;
    int64_t b0 = 0, bspan = 0;
    if (kCat) {
      b0 = b.offsets[br0];
      bspan = b.offsets[br1] - b0;
    }
    const int64_t o0 = out_off[r0], ospan = out_off[r1] - o0;
    uint8_t *dst = out + o0;
    if (aspan <= kIn && bspan <= kIn && ospan <= kTile) {
      const int sha = stage_rows(a, abc ? nullptr : va, abc ? nullptr : vb, ar0, ar1, tile_a);
      int shb = 0;
      if (kCat) shb = stage_rows(b, bbc ? nullptr : va, bbc ? nullptr : vb, br0, br1, tile_b);
      const int osh = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
      const int64_t r = r0 + tid;
      if (tid < kRows && r < r1 && row_live(va, vb, r)) {
        uint8_t *d = tile_o + osh + (int)(out_off[r] - o0);
        const int64_t ra = abc ? 0 : r;
        const int64_t ab = a.offsets[ra], la = a.offsets[ra + 1] - ab;
        const uint8_t *sa = tile_a + sha + (int)(ab - a0);
        if (kCat) {
          const int64_t rb = bbc ? 0 : r;
          const int64_t bb = b.offsets[rb], lb = b.offsets[rb + 1] - bb;
          const uint8_t *sb = tile_b + shb + (int)(bb - b0);
          for (int64_t i = 0; i < la; ++i) d[i] = sa[i];
          d += la;
          for (int i = 0; i < x.len1; ++i) d[i] = slit[i];
          d += x.len1;
          for (int64_t i = 0; i < lb; ++i) d[i] = sb[i];
        } else if (FN == SX_CASE) {
          for (int64_t i = 0; i < la; ++i) {
            const uint8_t c = sa[i];
            high |= c;
            d[i] = sx_case(c, x.upper);
          }
        } else {
          sx_cell_write(x, sa, la, slit, d);
        }
      }
      __syncthreads();
      // flush: only whole 16-byte groups inside [dst, dst + ospan) are stored as vectors
      const int span = (int)ospan;
      int head = (16 - osh) & 15;
      if (head > span) head = span;
      for (int k = tid; k < head; k += kBlock) dst[k] = tile_o[osh + k];
      const int nv = (span - head) >> 4;
      if (nv > 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(tile_o + osh + head);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
        for (int k = tid; k < nv; k += kBlock) d4[k] = s4[k];
      }
      for (int k = head + (nv << 4) + tid; k < span; k += kBlock) dst[k] = tile_o[osh + k];
      __syncthreads();  // the next block of rows overwrites the tiles
    } else {
      for (int64_t r = r0 + tid / kWave; r < r1; r += kRowWaves) {  // r is uniform in a wave
        if (!row_live(va, vb, r)) continue;
        uint8_t *d = out + out_off[r];
        const int64_t ra = abc ? 0 : r;
        const int64_t ab = a.offsets[ra], la = a.offsets[ra + 1] - ab;
        const uint8_t *sa = a.data + ab;
        if (kCat) {
          const int64_t rb = bbc ? 0 : r;
          const int64_t bb = b.offsets[rb], lb = b.offsets[rb + 1] - bb;
          wave_copy(sa, d, la, lane);
          for (int k = lane; k < x.len1; k += kWave) d[la + k] = slit[k];
          wave_copy(b.data + bb, d + la + x.len1, lb, lane);
        } else if (FN == SX_CASE) {
          for (int64_t i = lane; i < la; i += kWave) {
            const uint8_t c = sa[i];
            high |= c;
            d[i] = sx_case(c, x.upper);
          }
        } else if (FN == SX_REPLACE) {
          wave_replace<true>(sa, la, slit, x.len1, slit + x.len1, x.len2, x.max_repl, d, lane);
        } else {
          int64_t lo, hi;
          wave_range(x, sa, la, slit, lane, &lo, &hi);
          wave_copy(sa + lo, d, hi - lo, lane);
        }
      }
    }
  }
  if (FN == SX_CASE && flag != nullptr) {
    const int any = __syncthreads_or((int)(high & 0x80u));
    if (tid == 0 && any) atomicOr(flag, 1u);
  }
}

// upper / lower of a column without validity: dst[k] = map(src[k]) for k < total, src = data +
// offsets[0]; out_off[i] = offsets[i] - offsets[0].  The stores are 16-byte vectors over the aligned
// body of dst; the loads of a group are whole inside [src, src + total).
__global__ void __launch_bounds__(kBlock)
k_strx_case_flat(const uint8_t *__restrict__ data, const int64_t *__restrict__ offs, int64_t n, int upper,
                 int64_t *__restrict__ out_off, uint8_t *__restrict__ dst, unsigned int *__restrict__ flag) {
  const int64_t base = offs[0], total = offs[n] - base;
  const uint8_t *src = data + base;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gid; i <= n; i += stride) out_off[i] = offs[i] - base;
  unsigned int high = 0;
  int64_t head = (int64_t)((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
  if (head > total) head = total;
  const int64_t nv = (total - head) >> 4;
  for (int64_t k = gid; k < head; k += stride) {
    const uint8_t c = src[k];
    high |= c;
    dst[k] = sx_case(c, upper);
  }
  for (int64_t g = gid; g < nv; g += stride) {
    uint4 v;
    __builtin_memcpy(&v, src + head + (g << 4), 16);  // src need not share dst's alignment
    high |= (v.x | v.y | v.z | v.w) & 0x80808080u;
    v.x = sx_case_word(v.x, upper);
    v.y = sx_case_word(v.y, upper);
    v.z = sx_case_word(v.z, upper);
    v.w = sx_case_word(v.w, upper);
    *reinterpret_cast<uint4 *>(dst + head + (g << 4)) = v;
  }
  for (int64_t k = head + (nv << 4) + gid; k < total; k += stride) {
    const uint8_t c = src[k];
    high |= c;
    dst[k] = sx_case(c, upper);
  }
  const int any = __syncthreads_or((int)(high & 0x80808080u));
  if (threadIdx.x == 0 && any) atomicOr(flag, 1u);
}

void check_xform(const StrXform &x) {
  CYLON_CHECK(x.fn >= SX_SLICE && x.fn <= SX_REPLACE, Code::Invalid, "string transform: function " << x.fn);
  CYLON_CHECK(x.len1 >= 0 && x.len2 >= 0 && x.len1 <= kStrMaxPatternBytes && x.len2 <= kStrMaxPatternBytes,
              Code::Invalid, "string transform: a literal of more than " << kStrMaxPatternBytes << " bytes");
  CYLON_CHECK(x.fn != SX_REPLACE || x.len1 > 0, Code::Invalid, "string replace: the pattern is empty");
}

bool needs_bytes(const StrXform &x) {
  return x.fn == SX_STRIP || x.fn == SX_REPLACE || (x.fn == SX_SLICE && x.utf8);
}

}  // namespace

void strx_lengths(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                  int64_t *lens, void *stream) {
  check_xform(x);
  if (n == 0) return;
  if (needs_bytes(x)) {
    hipLaunchKernelGGL(k_strx_len_rows, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, x, lit, n, lens);
  } else {
    hipLaunchKernelGGL(k_strx_len_offsets, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), a, b, x, n, lens);
  }
  HIP_LAUNCH_CHECK();
}

void strx_write(const ColView &a, const ColView &b, const strxform::StrXform &x, const uint8_t *lit, int64_t n,
                const int64_t *out_off, uint8_t *out, uint32_t *flag, void *stream) {
  check_xform(x);
  if (n == 0) return;
  const dim3 grid(grid_for(n, x.fn == SX_CONCAT ? kBlock / 2 : kBlock)), block(kBlock);
  hipStream_t s = as_stream(stream);
  switch (x.fn) {
    case SX_SLICE: hipLaunchKernelGGL(k_strx_write<SX_SLICE>, grid, block, 0, s, a, b, x, lit, n, out_off, out, flag); break;
    case SX_STRIP: hipLaunchKernelGGL(k_strx_write<SX_STRIP>, grid, block, 0, s, a, b, x, lit, n, out_off, out, flag); break;
    case SX_CASE: hipLaunchKernelGGL(k_strx_write<SX_CASE>, grid, block, 0, s, a, b, x, lit, n, out_off, out, flag); break;
    case SX_CONCAT: hipLaunchKernelGGL(k_strx_write<SX_CONCAT>, grid, block, 0, s, a, b, x, lit, n, out_off, out, flag); break;
    default: hipLaunchKernelGGL(k_strx_write<SX_REPLACE>, grid, block, 0, s, a, b, x, lit, n, out_off, out, flag); break;
  }
  HIP_LAUNCH_CHECK();
}

void strx_case_flat(const ColView &a, int upper, int64_t n, int64_t total, int64_t *out_off, uint8_t *out,
                    uint32_t *flag, void *stream) {
  const int64_t work = (total >> 4) > n + 1 ? (total >> 4) : n + 1;
  hipLaunchKernelGGL(k_strx_case_flat, dim3(grid_for(work)), dim3(kBlock), 0, as_stream(stream), a.data, a.offsets, n,
                     upper, out_off, out, flag);
  HIP_LAUNCH_CHECK();
}

// this file's code object is loaded at context creation (preload_device_code), not on first use
void preload_strxform() { preload_code(reinterpret_cast<const void *>(&k_strx_len_offsets)); }

}  // namespace hip
}  // namespace cylon
