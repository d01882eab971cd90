// What the multi-token decode attention kernels share (decode_attention_multi.hip: bf16 cache;
// decode_attention_multi_fp8.hip: e4m3 cache): the split of a chunk's keys over the waves, the MFMA with its
// lane map, the two-term bf16 split of P and the kernel that merges the partials of S query rows per head.
#pragma once
#include "decode_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
using pto::f32x4;

constexpr int kTiles = 4;    // 16-key tiles per wave: kChunk / 16 / (kT / 64)
constexpr int kWaveKeys = 16 * kTiles;
constexpr int kMaxRows = 16; // query rows per kv head: the MFMA's columns

// lane map (gfx950): A[i = lane & 15][k = 8 (lane >> 4) + e], B[k = 8 (lane >> 4) + e][j = lane & 15],
// D: j = lane & 15, i = 4 (lane >> 4) + reg.
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                 0, 0, 0);
}

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// Two rounded values and what the rounding left of them, rounded again: hi + lo = p to 2^-16.
struct HiLo {
  uint32_t hi, lo;
};
__device__ __forceinline__ HiLo split2(float p0, float p1) {
  const uint32_t hi = pk_bf16(p0, p1);
  return {hi, pk_bf16(p0 - pto::bf_lo(hi), p1 - pto::bf_hi(hi))};
}

// One workgroup of D threads per (sequence, query position, query head): merge the partials of the chunks
// the row's own n_s makes valid, in order.  decode_combine_kernel with S Hq heads and the causal offset.
template <int D>
__global__ __launch_bounds__(D) void decode_combine_multi_kernel(const float* __restrict__ po,
                                                                 const float* __restrict__ pm,
                                                                 const float* __restrict__ pl,
                                                                 const int* __restrict__ lens,
                                                                 uint16_t* __restrict__ o, int max_keys, int Hq, int S,
                                                                 int nchunks) {
  const int sh = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int n = lens[b];
  n = (n < max_keys ? n : max_keys) - (S - 1 - sh / Hq);
  const long r = (long)b * S * Hq + sh;
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

}  // namespace
