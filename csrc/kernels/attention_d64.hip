// The 4-wave flash-attention passes at head dim 64 (Llama-3.2 1B: dim 2048, 32 heads): the kernel
// text of attention_4wave.h compiled with D = 64, i.e. NDS = 4 k-steps per d-contraction, NDT = 2
// output tiles along d, CH = 8 chunks (128 bytes) per row in the D = 64 LDS image of
// attention_common.h.  K/V double buffers take 32 KB (forward, dQ) and the Q/dO ones 16 KB (dK/dV).
// Same tiles as D = 128 (128 query rows per forward / dQ workgroup, 64-key tiles, 128 keys per
// dK/dV workgroup), same properties: no atomics, deterministic, every dQ row finished in one
// workgroup, document bounds clamped to the block's causal range before they become tile indices,
// and with doc_start == 0 the document kernels run the plain kernels' operations in their order.
// There is no 8-wave forward and no pipelined backward at this head dim.
//
// Called by the entry points of attention.hip, which have checked the shapes and the alignment.
#define PTO_ATTN_D 64
#include "attention_4wave.h"

static_assert(D == 64 && NDS == 4 && NDT == 2 && CH == 8, "this file is the D = 64 instance");

extern "C" {

// doc_start == nullptr: the plain kernel (causal or full); otherwise the document kernel (causal)
int pto_attn_d64_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc_start, int B,
                     int S, int Hq, int Hkv, float c, int causal, void* stream) {
  const dim3 grid((S / BM) * B * Hq), block(NT);
  if (doc_start == nullptr)
    hipLaunchKernelGGL(ATTN_KERNEL(fwd), grid, block, 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, lse2, B, S, Hq, Hkv, c, causal);
  else
    hipLaunchKernelGGL(ATTN_KERNEL(doc_fwd), grid, block, 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, lse2, doc_start, B, S, Hq, Hkv, c);
  return (int)hipGetLastError();
}

// doc_start == nullptr: the plain dQ and dK/dV passes; otherwise the document passes (doc_end too)
int pto_attn_d64_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                     float* delta, void* dq, void* dk, void* dv, const int* doc_start, const int* doc_end, int B, int S,
                     int Hq, int Hkv, float c, float scale, int causal, void* stream) {
  const dim3 qgrid((S / BM) * B * Hq), kgrid((S / BK) * B * Hkv), block(NT);
  if (doc_start == nullptr) {
    hipLaunchKernelGGL(ATTN_KERNEL(bwd_dq), qgrid, block, 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)dout, lse2, delta, (bf16_t*)dq, B, S, Hq,
                       Hkv, c, scale, causal);
    hipLaunchKernelGGL(ATTN_KERNEL(bwd_dkdv), kgrid, block, 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse2, (const float*)delta,
                       (bf16_t*)dk, (bf16_t*)dv, B, S, Hq, Hkv, c, scale, causal);
  } else {
    hipLaunchKernelGGL(ATTN_KERNEL(doc_dq), qgrid, block, 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)dout, lse2, delta, (bf16_t*)dq, doc_start, B,
                       S, Hq, Hkv, c, scale);
    hipLaunchKernelGGL(ATTN_KERNEL(doc_dkdv), kgrid, block, 0, (hipStream_t)stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse2, (const float*)delta,
                       (bf16_t*)dk, (bf16_t*)dv, doc_end, B, S, Hq, Hkv, c, scale);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
