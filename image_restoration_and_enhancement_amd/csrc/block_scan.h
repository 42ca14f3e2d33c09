// irx — prefix sums over the 256 lanes of a workgroup, shared by the JPEG encoder (jpeg_encode.hip) and decoder
// (jpeg_decode.hip).  Device code only; include from .hip files.
#pragma once
#include "ops.h"

namespace irx {

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// exclusive prefix of v over the 256 lanes of the block; *total: the block's sum.  `part`: 4 shared slots.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* part, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_incl_scan(v, lane);
  __syncthreads();                                           // part[] of a previous call has been read
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const T p = part[w];
    before += w < wave ? p : 0;
    sum += p;
  }
  *total = sum;
  return before + incl - v;
}

}  // namespace irx
