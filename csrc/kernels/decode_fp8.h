// What the kernels on the e4m3 KV cache share (decode_attention_fp8.hip: one token per step;
// decode_attention_multi_fp8.hip: S tokens per step): the per-head quantiser behind the appends and the exact
// widening of eight e4m3 bytes to a bf16 MFMA fragment.  decode_attention_fp8.hip's header has the format.
#pragma once
#include "decode_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------- the quantiser
// x: this thread's 8 values of a head's row, already bf16 values; lpg = D / 8 consecutive lanes hold the
// row.  Every lane of the group must be active.  Stores 8 e4m3 bytes at dst and, from the group's first
// lane, the scale at sdst.
__device__ __forceinline__ void head_quantize(const float (&x)[8], int lpg, bool first, uint8_t* dst, float* sdst) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
  for (int o = lpg >> 1; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const uint32_t u = __float_as_uint(amax);
  // amax = m 2^e: e - 8, or e - 7 when m > 1.75 (a bf16's fraction is the top 7 of the 23 bits);
  // a subnormal amax (exponent field 0) falls below the clamp either way
  int se = (int)(u >> 23) - 127 - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  se = se < -126 ? -126 : se;
  if (amax == 0.f) se = 0;
  const float inv = __uint_as_float((uint32_t)(127 - se) << 23);  // 2^-se, exponent in [6, 253]
  uint32_t lo = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false);
  lo = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, (int)lo, true);
  uint32_t hi = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, 0, false);
  hi = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, (int)hi, true);
  *reinterpret_cast<u32x2*>(dst) = u32x2{lo, hi};
  if (first) *sdst = __uint_as_float((uint32_t)(127 + se) << 23);
}

// Eight e4m3 bytes (two dwords, k ascending) -> eight bf16 (an A fragment), exactly.
__device__ __forceinline__ u32x4 widen(uint32_t lo, uint32_t hi) {
  u32x4 a;
  a[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
  a[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
  a[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
  a[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  return a;
}

inline bool scales_ok(const void* ks, const void* vs, int sstride, int max_len) {
  return sstride >= max_len && sstride % 4 == 0 && aligned16(ks) && aligned16(vs);
}

}  // namespace
