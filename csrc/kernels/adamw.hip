// Fused mixed-precision AdamW step for the Llama DDP worker (BASELINE "Llama-3 8B DDP bf16").
//
// The matmul weights live in bf16 (the tensors autocast matmuls read, so no per-step
// fp32->bf16 weight cast) and their gradients arrive in bf16 (no bf16->fp32 grad cast);
// the optimizer owns an fp32 master copy plus the fp32 moments.  One pass per parameter:
//
//   read  g (bf16 or fp32), master, m, v          write master, m, v, and the bf16 weight
//
// = 28 B per bf16-weight element, the same HBM traffic as torch's fused fp32 AdamW alone,
// with the two cast kernels (12 B/element) gone.  fp32 parameters (embedding, norm
// weights) use the same kernel with the parameter itself as the master and no bf16 copy.
// Semantics match torch.optim.AdamW (decoupled weight decay, bias-corrected moments):
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= lr * (m / bc1) / (sqrt(v / bc2) + eps),   bc_i = 1 - b_i^t
//
// bf16 moments (pto_adamw_bf16state_*): m and v are stored as bf16 bits, widened on load, and
// rounded STOCHASTICALLY on store; the master is updated from the fp32 moments before they are
// rounded.  20 B per bf16-weight element instead of 28.  Round-to-nearest would be wrong, not
// noisy: with b2 = 0.999 the per-step decay of v (0.1 %) is below half a bf16 ulp, so v would
// never come down.  The random bits are a counter hash of (key, base + element index), plain
// integer arithmetic that the CPU path and the tests reproduce bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

constexpr int kT = 256;

struct AdamArgs {
  float lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2, gscale;
};

// The fused multiply-adds are spelled out and the compiler's own contraction is off: left to
// choose, it fused different products in different instantiations (and in different lanes of one
// float4), so the clipped kernel with a coefficient of exactly 1 did not give the unclipped
// kernel's bits.  Now every instantiation and lane rounds alike.
__device__ __forceinline__ float adam1(float& p, float& m, float& v, float g, const AdamArgs& a) {
#pragma clang fp contract(off)
  g *= a.gscale;  // 1, or the data-parallel 1/W of an unscaled gradient sum (exact for W = 2^k)
  p *= 1.f - a.lr * a.wd;
  m = fmaf(a.b1, m, (1.f - a.b1) * g);
  v = fmaf(a.b2, v, (1.f - a.b2) * g * g);
  // torch: denom = sqrt(v) / sqrt(bc2) + eps ; p -= (lr / bc1) * m / denom
  p -= a.lr * a.inv_bc1 * m / fmaf(sqrtf(v), a.inv_sqrt_bc2, a.eps);
  return p;
}

// CLIP: global-norm gradient clipping.  `sumsq` is the device scalar sum(g^2) over ALL gradients
// of the step (gradclip.hip); every thread loads it once and folds torch.nn.utils.clip_grad_norm_'s
// coefficient min(1, max_norm / (norm + 1e-6)) into the gradient scale.  A NaN norm propagates
// (the comparison is false), as torch's clamp does.
template <bool GBF16, bool OUTBF16, bool CLIP>
__global__ __launch_bounds__(kT) void adamw_kernel(float* __restrict__ master, float* __restrict__ mom,
                                                   float* __restrict__ var, const void* __restrict__ grad,
                                                   uint16_t* __restrict__ out, long n, AdamArgs a,
                                                   const float* __restrict__ sumsq, float max_norm) {
  if (CLIP) {
    const float c = max_norm / (sqrtf(sumsq[0]) + 1e-6f);
    a.gscale *= c > 1.f ? 1.f : c;
  }
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i <= n4; i += (long)gridDim.x * kT) {
    if (i < n4) {
      float4 p = reinterpret_cast<float4*>(master)[i];
      float4 m = reinterpret_cast<float4*>(mom)[i];
      float4 v = reinterpret_cast<float4*>(var)[i];
      float g[4];
      if (GBF16) pto::vload(reinterpret_cast<const uint16_t*>(grad) + 4 * i, g);
      else pto::vload(reinterpret_cast<const float*>(grad) + 4 * i, g);
      adam1(p.x, m.x, v.x, g[0], a);
      adam1(p.y, m.y, v.y, g[1], a);
      adam1(p.z, m.z, v.z, g[2], a);
      adam1(p.w, m.w, v.w, g[3], a);
      reinterpret_cast<float4*>(master)[i] = p;
      reinterpret_cast<float4*>(mom)[i] = m;
      reinterpret_cast<float4*>(var)[i] = v;
      if (OUTBF16)
        reinterpret_cast<uint2*>(out)[i] = make_uint2(pto::bf16_pack(p.x, p.y), pto::bf16_pack(p.z, p.w));
    } else {
      for (long j = n4 * 4; j < n; ++j) {
        const float g = GBF16 ? pto::load1(reinterpret_cast<const uint16_t*>(grad) + j)
                              : pto::load1(reinterpret_cast<const float*>(grad) + j);
        const float p = adam1(master[j], mom[j], var[j], g, a);
        if (OUTBF16) pto::store1(out + j, p);
      }
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

AdamArgs adam_args(float lr, float b1, float b2, float eps, float wd, int step, float grad_scale) {
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd; a.gscale = grad_scale;
  a.inv_bc1 = (float)(1.0 / (1.0 - pow((double)b1, step)));
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
  return a;
}

template <bool CLIP>
int launch_adamw(float* master, float* m, float* v, const void* grad, void* out, long n, int grad_bf16, float lr,
                 float b1, float b2, float eps, float wd, int step, float grad_scale, const float* sumsq,
                 float max_norm, void* stream) {
  if (n <= 0 || step < 1) return -1;
  if (!aligned16(master) || !aligned16(m) || !aligned16(v) || !aligned16(grad) || (out && !aligned16(out)))
    return -2;
  const AdamArgs a = adam_args(lr, b1, b2, eps, wd, step, grad_scale);
  const long work = n / 4 + 1;
  long blocks = (work + kT - 1) / kT;
  if (blocks > 8192) blocks = 8192;  // 32 waves per CU resident at most; grid-stride beyond
  const dim3 grid((unsigned)blocks), block(kT);
  hipStream_t s = (hipStream_t)stream;
  if (grad_bf16 && out) hipLaunchKernelGGL((adamw_kernel<true, true, CLIP>), grid, block, 0, s, master, m, v, grad,
                                           (uint16_t*)out, n, a, sumsq, max_norm);
  else if (grad_bf16) hipLaunchKernelGGL((adamw_kernel<true, false, CLIP>), grid, block, 0, s, master, m, v, grad,
                                         (uint16_t*)nullptr, n, a, sumsq, max_norm);
  else if (out) hipLaunchKernelGGL((adamw_kernel<false, true, CLIP>), grid, block, 0, s, master, m, v, grad,
                                   (uint16_t*)out, n, a, sumsq, max_norm);
  else hipLaunchKernelGGL((adamw_kernel<false, false, CLIP>), grid, block, 0, s, master, m, v, grad,
                          (uint16_t*)nullptr, n, a, sumsq, max_norm);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------- bf16 moments
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 32 random bits of element c (base + index within the launch): the low half rounds m, the high half v.
__device__ __forceinline__ uint32_t sr_bits(uint64_t c, uint32_t key) {
  return mix32(mix32((uint32_t)c ^ key) + (uint32_t)(c >> 32));
}

// fp32 -> bf16 bits, rounded up in magnitude with probability (low 16 bits) / 65536: r is uniform
// in [0, 65535].  A representable value (+-0, +-inf included) never changes; the largest finite
// values may reach inf; a NaN is pto::bf16_rne's quiet NaN.
__device__ __forceinline__ uint32_t bf16_sr(float f, uint32_t r) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return pto::bf16_rne(f);
  return (u + r) >> 16;
}

// adam1 on one element whose moments are bf16 bits; returns the new master, writes the rounded moments.
__device__ __forceinline__ void adam1_sr(float& p, float& m, float& v, float g, const AdamArgs& a, uint64_t c,
                                         uint32_t key, uint32_t& mb, uint32_t& vb) {
  adam1(p, m, v, g, a);
  const uint32_t h = sr_bits(c, key);
  mb = bf16_sr(m, h & 0xffffu);
  vb = bf16_sr(v, h >> 16);
}

// Eight elements per thread: every access is 16 bytes (two for the fp32 master and an fp32 gradient).
template <bool GBF16, bool OUTBF16, bool CLIP>
__global__ __launch_bounds__(kT) void adamw_bf16state_kernel(float* __restrict__ master, uint16_t* __restrict__ mom,
                                                             uint16_t* __restrict__ var, const void* __restrict__ grad,
                                                             uint16_t* __restrict__ out, long n, AdamArgs a,
                                                             const float* __restrict__ sumsq, float max_norm,
                                                             uint32_t key, uint64_t base) {
  if (CLIP) {
    const float c = max_norm / (sqrtf(sumsq[0]) + 1e-6f);
    a.gscale *= c > 1.f ? 1.f : c;
  }
  const long n8 = n / 8;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i <= n8; i += (long)gridDim.x * kT) {
    if (i < n8) {
      float p[8], m[8], v[8], g[8];
      pto::vload(master + 8 * i, p);
      pto::vload(mom + 8 * i, m);
      pto::vload(var + 8 * i, v);
      if (GBF16) pto::vload(reinterpret_cast<const uint16_t*>(grad) + 8 * i, g);
      else pto::vload(reinterpret_cast<const float*>(grad) + 8 * i, g);
      const uint64_t c = base + (uint64_t)(8 * i);
      uint32_t mw[4], vw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t m0, v0, m1, v1;
        adam1_sr(p[2 * k], m[2 * k], v[2 * k], g[2 * k], a, c + 2 * k, key, m0, v0);
        adam1_sr(p[2 * k + 1], m[2 * k + 1], v[2 * k + 1], g[2 * k + 1], a, c + 2 * k + 1, key, m1, v1);
        mw[k] = m0 | (m1 << 16);
        vw[k] = v0 | (v1 << 16);
      }
      pto::vstore(master + 8 * i, p);
      pto::store_words(mom + 8 * i, mw);
      pto::store_words(var + 8 * i, vw);
      if (OUTBF16) pto::vstore(out + 8 * i, p);
    } else {
      for (long j = n8 * 8; j < n; ++j) {
        const float g = GBF16 ? pto::load1(reinterpret_cast<const uint16_t*>(grad) + j)
                              : pto::load1(reinterpret_cast<const float*>(grad) + j);
        float m = pto::load1(mom + j), v = pto::load1(var + j);
        uint32_t mb, vb;
        adam1_sr(master[j], m, v, g, a, base + (uint64_t)j, key, mb, vb);
        mom[j] = (uint16_t)mb;
        var[j] = (uint16_t)vb;
        if (OUTBF16) pto::store1(out + j, master[j]);
      }
    }
  }
}

template <bool CLIP>
int launch_adamw_bf16state(float* master, uint16_t* m, uint16_t* v, const void* grad, void* out, long n,
                           int grad_bf16, float lr, float b1, float b2, float eps, float wd, int step,
                           float grad_scale, const float* sumsq, float max_norm, uint32_t key, uint64_t base,
                           void* stream) {
  if (n <= 0 || step < 1) return -1;
  if (!aligned16(master) || !aligned16(m) || !aligned16(v) || !aligned16(grad) || (out && !aligned16(out)))
    return -2;
  const AdamArgs a = adam_args(lr, b1, b2, eps, wd, step, grad_scale);
  const long work = n / 8 + 1;
  long blocks = (work + kT - 1) / kT;
  if (blocks > 8192) blocks = 8192;  // as launch_adamw
  const dim3 grid((unsigned)blocks), block(kT);
  hipStream_t s = (hipStream_t)stream;
  if (grad_bf16 && out) hipLaunchKernelGGL((adamw_bf16state_kernel<true, true, CLIP>), grid, block, 0, s, master, m, v,
                                           grad, (uint16_t*)out, n, a, sumsq, max_norm, key, base);
  else if (grad_bf16) hipLaunchKernelGGL((adamw_bf16state_kernel<true, false, CLIP>), grid, block, 0, s, master, m, v,
                                         grad, (uint16_t*)nullptr, n, a, sumsq, max_norm, key, base);
  else if (out) hipLaunchKernelGGL((adamw_bf16state_kernel<false, true, CLIP>), grid, block, 0, s, master, m, v,
                                   grad, (uint16_t*)out, n, a, sumsq, max_norm, key, base);
  else hipLaunchKernelGGL((adamw_bf16state_kernel<false, false, CLIP>), grid, block, 0, s, master, m, v, grad,
                          (uint16_t*)nullptr, n, a, sumsq, max_norm, key, base);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// grad_bf16: gradient dtype (1 = bf16, 0 = fp32).  out: bf16 weight to refresh (nullptr for
// fp32 parameters, whose master IS the parameter).  step >= 1.  grad_scale multiplies the
// gradient first (ZeRO's gradient-view buckets hold the unscaled sum over ranks).
int pto_adamw_step_scaled(float* master, float* m, float* v, const void* grad, void* out, long n, int grad_bf16,
                          float lr, float b1, float b2, float eps, float wd, int step, float grad_scale,
                          void* stream) {
  return launch_adamw<false>(master, m, v, grad, out, n, grad_bf16, lr, b1, b2, eps, wd, step, grad_scale, nullptr,
                             0.f, stream);
}

// pto_adamw_step_scaled with the gradient also multiplied by min(1, max_norm / (sqrt(*sumsq) + 1e-6)):
// sumsq is the DEVICE scalar pto_grad_sumsq_finish wrote (the host never reads it).
int pto_adamw_step_clipped(float* master, float* m, float* v, const void* grad, void* out, long n, int grad_bf16,
                           float lr, float b1, float b2, float eps, float wd, int step, float grad_scale,
                           const float* sumsq, float max_norm, void* stream) {
  if (!sumsq || ((uintptr_t)sumsq & 3u)) return -2;
  if (!(max_norm > 0.f)) return -1;
  return launch_adamw<true>(master, m, v, grad, out, n, grad_bf16, lr, b1, b2, eps, wd, step, grad_scale, sumsq,
                            max_norm, stream);
}

// The same two passes with the moments stored as bf16 bits and rounded stochastically (see the
// header).  rng_key = mix32(seed + 0x9E3779B9 * step), computed by the caller; rng_base is the
// counter of element 0, so a tensor updated by several launches (ZeRO shards) gets the bits of one.
int pto_adamw_bf16state_scaled(float* master, uint16_t* m, uint16_t* v, const void* grad, void* out, long n,
                               int grad_bf16, float lr, float b1, float b2, float eps, float wd, int step,
                               float grad_scale, uint32_t rng_key, uint64_t rng_base, void* stream) {
  return launch_adamw_bf16state<false>(master, m, v, grad, out, n, grad_bf16, lr, b1, b2, eps, wd, step, grad_scale,
                                       nullptr, 0.f, rng_key, rng_base, stream);
}

int pto_adamw_bf16state_clipped(float* master, uint16_t* m, uint16_t* v, const void* grad, void* out, long n,
                                int grad_bf16, float lr, float b1, float b2, float eps, float wd, int step,
                                float grad_scale, const float* sumsq, float max_norm, uint32_t rng_key,
                                uint64_t rng_base, void* stream) {
  if (!sumsq || ((uintptr_t)sumsq & 3u)) return -2;
  if (!(max_norm > 0.f)) return -1;
  return launch_adamw_bf16state<true>(master, m, v, grad, out, n, grad_bf16, lr, b1, b2, eps, wd, step, grad_scale,
                                      sumsq, max_norm, rng_key, rng_base, stream);
}

}  // extern "C"
