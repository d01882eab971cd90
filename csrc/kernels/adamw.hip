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

template <bool CLIP>
int launch_adamw(float* master, float* m, float* v, const void* grad, void* out, long n, int grad_bf16, float lr,
                 float b1, float b2, float eps, float wd, int step, float grad_scale, const float* sumsq,
                 float max_norm, void* stream) {
  if (n <= 0 || step < 1) return -1;
  if (!aligned16(master) || !aligned16(m) || !aligned16(v) || !aligned16(grad) || (out && !aligned16(out)))
    return -2;
  AdamArgs a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd; a.gscale = grad_scale;
  a.inv_bc1 = (float)(1.0 / (1.0 - pow((double)b1, step)));
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
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

}  // extern "C"
