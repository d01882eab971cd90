// bf16 <-> fp32 conversion, N-element vector load/store "as fp32 in registers" and a block sum:
// the helpers the Llama elementwise kernels (llm_fused, rmsnorm, adamw, gradclip) share.
//
// Storage is told apart by size alone: a 4-byte T is fp32, a 2-byte T is bf16 bits, whether the
// kernel spells it uint16_t or __hip_bfloat16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_common.h"

namespace pto {

__device__ __forceinline__ float bf2f(uint32_t bits) { return __uint_as_float(bits << 16); }
// The two bf16 halves of one 32-bit word (element 2i in the low half, 2i + 1 in the high half).
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// fp32 -> bf16 bits, round to nearest even.  A NaN stays a NaN (quiet, same sign): the rounding
// carry would run out of an all-ones mantissa into the exponent and sign (0xffffffff -> +0.0,
// 0x7fffffff -> -0.0).
__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// One 32-bit word of two rounded values, the first in the low half.
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }

template <typename T>
__device__ __forceinline__ float load1(const T* p) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 2, "fp32 or bf16 storage");
  if constexpr (sizeof(T) == 4) return *reinterpret_cast<const float*>(p);
  else return bf2f(*reinterpret_cast<const uint16_t*>(p));
}
template <typename T>
__device__ __forceinline__ void store1(T* p, float v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 2, "fp32 or bf16 storage");
  if constexpr (sizeof(T) == 4) *reinterpret_cast<float*>(p) = v;
  else *reinterpret_cast<uint16_t*>(p) = (uint16_t)bf16_rne(v);
}

// M = 4 or 2 32-bit words (two bf16 each) in one 16- or 8-byte access.
template <int M>
__device__ __forceinline__ void load_words(const void* p, uint32_t (&w)[M]) {
  if constexpr (M == 4) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
  } else {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    w[0] = q.x; w[1] = q.y;
  }
}
template <int M>
__device__ __forceinline__ void store_words(void* p, const uint32_t (&w)[M]) {
  if constexpr (M == 4) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

// N consecutive elements at p as fp32: N = 8 or 4 (p aligned to the access: 16-byte units of fp32,
// 16 / 8 bytes of bf16), or N = 1.
template <typename T, int N>
__device__ __forceinline__ void vload(const T* p, float (&v)[N]) {
  static_assert(N == 8 || N == 4 || N == 1, "8, 4 or 1 elements per access");
  if constexpr (N == 1) {
    v[0] = load1(p);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const float4 a = reinterpret_cast<const float4*>(p)[i];
      v[4 * i] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
    }
  } else {
    uint32_t w[N / 2];
    load_words(p, w);
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      v[2 * i] = bf_lo(w[i]);
      v[2 * i + 1] = bf_hi(w[i]);
    }
  }
}
template <typename T, int N>
__device__ __forceinline__ void vstore(T* p, const float (&v)[N]) {
  static_assert(N == 8 || N == 4 || N == 1, "8, 4 or 1 elements per access");
  if constexpr (N == 1) {
    store1(p, v[0]);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      reinterpret_cast<float4*>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
    uint32_t w[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) w[i] = bf16_pack(v[2 * i], v[2 * i + 1]);
    store_words(p, w);
  }
}

// The same as a value: `const Vec<8> a = vload<8>(p); ... vstore(q, a);`
template <int N>
struct Vec {
  float v[N];
};
template <int N, typename T>
__device__ __forceinline__ Vec<N> vload(const T* p) {
  Vec<N> r;
  vload(p, r.v);
  return r;
}
template <typename T, int N>
__device__ __forceinline__ void vstore(T* p, const Vec<N>& r) {
  vstore(p, r.v);
}

// Sum of v over a 256-thread block, returned to every thread; sh holds one float per wave.  The
// first barrier lets a caller reuse sh from one call to the next; the waves are added in order.
constexpr int kBlockSumThreads = 256;
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kBlockSumThreads / kWave; ++k) t += sh[k];
  return t;
}

}  // namespace pto
