// Gradient accumulation for the Llama worker (--grad-accum N): fold one micro-batch's gradient
// into a persistent fp32 accumulator.
//
// N micro-batches make one optimizer step.  Accumulating in the bf16 .grad (what autograd would do)
// drops every addend below half an ulp of the running sum; here the sum is fp32, one rounding per
// add, in micro-batch order:
//
//   first:  acc = g                (acc is NOT read: it need not be zero-filled, or even initialised)
//   else:   acc = acc + g          g is bf16 or fp32, widened to fp32
//   out:    out = bf16_rne(acc)    optional; the bf16 reduce-scatter of ZeRO-1 sends this
//
// Traffic per element with a bf16 g: 2 B read + 4 B written (first), + 4 B read otherwise, + 2 B
// written with out.  out may be the very buffer g is (a bf16 staging bucket reduced in place): the
// thread that writes an element is the one that read it, and it reads first.
//
// One thread owns each element: no LDS, no atomics, bitwise reproducible.  AdamW and the norm pass
// apply the 1/(N*W) through their gradient-scale arguments, so there is no scaling pass here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

constexpr int kT = 256;        // threads per block
constexpr int kE = 8;          // elements per thread and trip: one 16-byte bf16 access, two of fp32
constexpr long kCap = 8192;    // blocks at most (adamw.hip's cap); grid-stride beyond

// g and out carry no __restrict__: they may be one buffer.
template <typename G, bool FIRST, bool OUT>
__global__ __launch_bounds__(kT) void grad_accum_kernel(float* __restrict__ acc, const G* g, uint16_t* out, long n) {
  const long nv = n / kE;
  const long stride = (long)gridDim.x * kT;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < nv; i += stride) {
    float a[kE];
    pto::vload(g + kE * i, a);
    if (!FIRST) {
      float b[kE];
      pto::vload(acc + kE * i, b);
#pragma unroll
      for (int k = 0; k < kE; ++k) a[k] = b[k] + a[k];
    }
    pto::vstore(acc + kE * i, a);
    if (OUT) pto::vstore(out + kE * i, a);
  }
  // scalar tail (n % 8 elements): one per lane of block 0
  const long t = nv * kE + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float a = pto::load1(g + t);
    if (!FIRST) a = acc[t] + a;
    acc[t] = a;
    if (OUT) pto::store1(out + t, a);
  }
}

long accum_blocks(long n) {
  long blocks = (n / kE + kT - 1) / kT;
  if (blocks < 1) blocks = 1;  // n below one vector: the scalar tail alone
  return blocks > kCap ? kCap : blocks;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename G>
void launch(float* acc, const void* g, void* out, long n, int first, hipStream_t s) {
  const dim3 grid((unsigned)accum_blocks(n)), block(kT);
  const G* gp = reinterpret_cast<const G*>(g);
  uint16_t* op = reinterpret_cast<uint16_t*>(out);
  if (first && out) hipLaunchKernelGGL((grad_accum_kernel<G, true, true>), grid, block, 0, s, acc, gp, op, n);
  else if (first) hipLaunchKernelGGL((grad_accum_kernel<G, true, false>), grid, block, 0, s, acc, gp, op, n);
  else if (out) hipLaunchKernelGGL((grad_accum_kernel<G, false, true>), grid, block, 0, s, acc, gp, op, n);
  else hipLaunchKernelGGL((grad_accum_kernel<G, false, false>), grid, block, 0, s, acc, gp, op, n);
}

}  // namespace

extern "C" {

// Elements one sweep of the capped grid covers: a longer buffer takes a second loop trip.
long pto_grad_accum_sweep() { return kCap * kT * kE; }

// acc[i] = first ? g[i] : acc[i] + g[i] over n elements; out_bf16 (may be null, may be g when
// g_bf16) = bf16(acc[i]).  g_bf16: gradient dtype (1 = bf16, 0 = fp32).
int pto_grad_accum(float* acc, const void* g, void* out_bf16, long n, int g_bf16, int first, void* stream) {
  if (n <= 0) return -1;
  if (!acc || !g || !aligned16(acc) || !aligned16(g) || (out_bf16 && !aligned16(out_bf16))) return -2;
  if (g_bf16) launch<uint16_t>(acc, g, out_bf16, n, first, (hipStream_t)stream);
  else launch<float>(acc, g, out_bf16, n, first, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // extern "C"
