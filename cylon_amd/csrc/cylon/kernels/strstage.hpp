// Device helpers shared by the string kernels that stage a block's rows in LDS (strmatch.hip,
// strxform.hip): the liveness test of a row and the copy of the bytes of rows [r0, r1) of a column
// into an LDS tile.  Memory safety: the copy loads only bytes inside [data + offsets[r0],
// data + offsets[r1]) -- the vector loads cover only whole 16-byte groups inside that span -- and
// none of a row that is not live.
#pragma once
#include "device_common.hpp"

namespace cylon {
namespace hip {

constexpr int kRowWaves = kBlock / kWave;

__device__ __forceinline__ bool row_live(const uint8_t *va, const uint8_t *vb, int64_t r) {
  return (va == nullptr || va[r] != 0) && (vb == nullptr || vb[r] != 0);
}

// Copy the bytes of rows [r0, r1) of c (span <= the tile) to tile + shift, shift = the source's
// address modulo 16; rows that are not live (va / vb) are skipped.  Ends with a barrier.
__device__ __forceinline__ int stage_rows(const ColView &c, const uint8_t *va, const uint8_t *vb, int64_t r0,
                                          int64_t r1, uint8_t *tile) {
  const int64_t b0 = c.offsets[r0];
  const int span = (int)(c.offsets[r1] - b0);
  if (span == 0) {
    __syncthreads();
    return 0;
  }
  const uint8_t *src = c.data + b0;
  const int shift = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
  const int tid = threadIdx.x;
  int any_dead = 0;
  if (va != nullptr || vb != nullptr) {
    const int64_t r = r0 + tid;
    any_dead = __syncthreads_or(r < r1 && !row_live(va, vb, r));
  }
  if (!any_dead) {
    int head = (16 - shift) & 15;
    if (head > span) head = span;
    for (int k = tid; k < head; k += kBlock) tile[shift + k] = src[k];
    const int nv = (span - head) >> 4;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(tile + shift + head);
    for (int k = tid; k < nv; k += kBlock) d4[k] = s4[k];
    for (int k = head + (nv << 4) + tid; k < span; k += kBlock) tile[shift + k] = src[k];
  } else {
    const int lane = tid & (kWave - 1);
    for (int64_t r = r0 + tid / kWave; r < r1; r += kRowWaves) {
      if (!row_live(va, vb, r)) continue;
      const int s = (int)(c.offsets[r] - b0), e = (int)(c.offsets[r + 1] - b0);
      for (int k = s + lane; k < e; k += kWave) tile[shift + k] = src[k];
    }
  }
  __syncthreads();
  return shift;
}

}  // namespace hip
}  // namespace cylon
