// Global L2 norm of the gradient for clipping (max_grad_norm of the Llama worker), on device.
//
// Clipping by global norm needs sum(g^2) over every gradient before the first AdamW update: one
// extra streaming read of the gradient (2 or 4 B per element), nothing written but a few floats.
//
//   pto_grad_sumsq         one contiguous buffer -> one fp32 partial per block, plain stores into
//                          the buffer's own region of a workspace
//   pto_grad_sumsq_finish  one workgroup sums every partial of every region (in double, fixed
//                          order) -> out[0] = sum(g^2), out[1] = sqrt(out[0]) = the norm
//   pto_adamw_step_clipped (adamw.hip) reads out[0] on the device and folds
//                          min(1, max_norm / (norm + 1e-6)) into its gradient scale
//
// No float atomics anywhere: the grid, hence the number of partials and the order of every sum,
// is a function of n alone, so the norm is bitwise reproducible from run to run, independent of
// the buffer's address, and identical on every data-parallel replica.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte load: 8 bf16 or 4 fp32

constexpr int kT = 256;       // threads per block
constexpr int kU = 4;         // 16-byte loads in flight per lane (one fp32 accumulator each)
constexpr long kCap = 2048;   // blocks at most: 8 per CU, grid-stride beyond
constexpr int kF = 1024;      // threads of the one finish workgroup

// The grid, from n alone (no occupancy query: the partial count fixes the summation order).
long sumsq_blocks(long n, int bf16) {
  const long nv = n / (bf16 ? 8 : 4);
  long blocks = (nv + kT - 1) / kT;
  if (blocks < 1) blocks = 1;  // n below one vector: the scalar tail alone
  return blocks > kCap ? kCap : blocks;
}

__device__ __forceinline__ float sq_acc(float x, float scale, float acc) {
  x *= scale;
  return fmaf(x, x, acc);
}

template <bool BF16>
__global__ __launch_bounds__(kT) void grad_sumsq_kernel(const void* __restrict__ grad, long n, float scale,
                                                        float* __restrict__ partial) {
  constexpr int kE = BF16 ? 8 : 4;  // elements per 16-byte vector
  const long nv = n / kE;
  const long stride = (long)gridDim.x * kT;
  float acc[kU];
#pragma unroll
  for (int k = 0; k < kU; ++k) acc[k] = 0.f;
  const u32x4* __restrict__ gv = reinterpret_cast<const u32x4*>(grad);
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < nv; i += kU * stride) {
    u32x4 q[kU];
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      const long j = i + k * stride;
      // read once: nontemporal loads (measured 10 % faster than plain ones on 1 GiB buffers)
      q[k] = j < nv ? __builtin_nontemporal_load(&gv[j]) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < kU; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (BF16) {
          acc[k] = sq_acc(pto::bf_lo(q[k][c]), scale, acc[k]);
          acc[k] = sq_acc(pto::bf_hi(q[k][c]), scale, acc[k]);
        } else {
          acc[k] = sq_acc(__uint_as_float(q[k][c]), scale, acc[k]);
        }
      }
    }
  }
  // scalar tail (< one vector): one element per lane of block 0
  const long t = nv * kE + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float x = BF16 ? pto::bf2f(reinterpret_cast<const uint16_t*>(grad)[t])
                         : reinterpret_cast<const float*>(grad)[t];
    acc[0] = sq_acc(x, scale, acc[0]);
  }
  // fixed-shape sums from here on: accumulators pairwise, 6 wave steps, the waves pairwise
#pragma unroll
  for (int w = kU / 2; w >= 1; w >>= 1) {
#pragma unroll
    for (int k = 0; k < w; ++k) acc[k] += acc[k + w];
  }
  const float s = pto::wave_sum(acc[0]);
  __shared__ float part[kT / pto::kWave];
  if ((threadIdx.x & (pto::kWave - 1)) == 0) part[threadIdx.x / pto::kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
static_assert((kU & (kU - 1)) == 0 && kT / pto::kWave == 4, "pairwise sums: a power of two accumulators, 4 waves");

__global__ __launch_bounds__(kF) void grad_sumsq_finish_kernel(const float* __restrict__ partial, long count,
                                                               float* __restrict__ out) {
  // a few thousand non-negative partials: each thread a fixed strided subset, in double, then a
  // fixed tree -- one rounding (to fp32) in the whole kernel
  double s = 0.0;
  for (long i = threadIdx.x; i < count; i += kF) s += (double)partial[i];
  __shared__ double tree[kF];
  tree[threadIdx.x] = s;
  __syncthreads();
  for (int w = kF / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)tree[0];
    out[0] = total;
    out[1] = sqrtf(total);
  }
}

}  // namespace

extern "C" {

// Number of partials pto_grad_sumsq writes for a buffer of n elements (its workspace region).
long pto_grad_sumsq_parts(long n, int grad_bf16) { return n > 0 ? sumsq_blocks(n, grad_bf16) : 0; }

// partial[0 .. pto_grad_sumsq_parts(n)) = per-block sums of (scale * grad[i])^2.  `slots` is the
// room left in the workspace from `partial` on.
int pto_grad_sumsq(const void* grad, long n, int grad_bf16, float scale, float* partial, long slots, void* stream) {
  if (n <= 0 || !grad || !partial) return -1;
  if (((uintptr_t)grad & 15u) || ((uintptr_t)partial & 3u)) return -2;
  const long blocks = sumsq_blocks(n, grad_bf16);
  if (slots < blocks) return -3;
  const dim3 grid((unsigned)blocks), block(kT);
  hipStream_t s = (hipStream_t)stream;
  if (grad_bf16) hipLaunchKernelGGL(grad_sumsq_kernel<true>, grid, block, 0, s, grad, n, scale, partial);
  else hipLaunchKernelGGL(grad_sumsq_kernel<false>, grid, block, 0, s, grad, n, scale, partial);
  return (int)hipGetLastError();
}

// out[0] = sum of partial[0 .. count), out[1] = sqrt(out[0]).
int pto_grad_sumsq_finish(const float* partial, long count, float* out, void* stream) {
  if (count <= 0 || !partial || !out) return -1;
  if (((uintptr_t)partial & 3u) || ((uintptr_t)out & 3u)) return -2;
  hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(kF), 0, (hipStream_t)stream, partial, count, out);
  return (int)hipGetLastError();
}

}  // extern "C"
