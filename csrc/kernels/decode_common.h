// What the decode attention kernels of decode_attention.hip (bf16 cache) and decode_attention_fp8.hip
// (e4m3 cache) share: the workgroup size, the chunk of keys one workgroup serves, the layout of the fp32
// partials a chunk writes and the kernel that merges them.
//
//   po [B, Hq, nchunks, D]   unnormalised sum_j p_j v_j of the chunk, p_j = exp(s_j - pm)
//   pm [B, Hq, nchunks]      the chunk's largest score
//   pl [B, Hq, nchunks]      sum_j p_j
//   nchunks = ceil(max_keys / kChunk); chunk c of a row is valid when c * kChunk < min(lens[b], max_keys).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

constexpr int kT = 256;
constexpr int kChunk = 256;  // keys per workgroup

// One workgroup of D threads per (batch row, query head): merge the row's valid partials in order.
template <int D>
__global__ __launch_bounds__(D) void decode_combine_kernel(const float* __restrict__ po,
                                                           const float* __restrict__ pm,
                                                           const float* __restrict__ pl,
                                                           const int* __restrict__ lens, uint16_t* __restrict__ o,
                                                           int max_keys, int Hq, int nchunks) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const long r = (long)b * Hq + h;
  float out = 0.f;
  if (n > 0) {
    const int nc = (n + kChunk - 1) / kChunk;  // <= nchunks, as n <= max_keys
    const float* m = pm + r * nchunks;
    const float* l = pl + r * nchunks;
    float M = m[0];
    for (int c = 1; c < nc; ++c) M = fmaxf(M, m[c]);
    float num = 0.f, den = 0.f;
    for (int c = 0; c < nc; ++c) {
      const float f = __expf(m[c] - M);
      num = fmaf(f, po[(r * nchunks + c) * D + d], num);
      den = fmaf(f, l[c], den);
    }
    out = num / den;
  }
  pto::store1(o + r * D + d, out);
}

inline unsigned grid_for(long work) {
  const long b = (work + kT - 1) / kT;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
