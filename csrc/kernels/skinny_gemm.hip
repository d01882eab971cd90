// Skinny bf16 GEMM for the Llama decode step: y[M, N] = x[M, K] . W[N, K]^T with 1 <= M <= 16 batch
// rows, x and W bf16 and K-contiguous (nn.Linear's weight as it lies in memory), fp32 accumulation,
// bf16 out.  Each weight byte is used M <= 16 times, so the kernel is a weight-streaming pipeline: it
// is laid out for bytes in flight, and the MFMA unit only keeps the arithmetic out of the way.
//
//   Operands  v_mfma_f32_16x16x32_bf16 with W as the A operand: 16 weight rows n are the 16 x 32 A
//             tile, x is the 32 x 16 B tile (batch row m = column, rows M..15 are zeros held in
//             registers, never read from memory), so D[n][m] = sum_k W[n][k] x[m][k].  A lane's A
//             fragment is 8 consecutive bf16 of one W row -- one 16-byte global load -- so W goes
//             HBM -> VGPR -> MFMA and never touches LDS.  x is at most 16 rows and stays in L2: each
//             lane loads its B fragment from global memory in the same way.
//   k order   The MFMA's k index is free as long as A and B agree.  A step is 64 k values = two
//             MFMAs: lane group g = lane / 16 takes the 16 consecutive values k0 + 16 g .. + 15 (32
//             bytes, two adjacent 16-byte loads), the first 8 for the step's first MFMA, the last 8
//             for its second.  The four groups of a row so read one whole 128-byte line per step.
//             K % 64 == 32 leaves one 32-wide half step in the plain order (group g: k0 + 8 g .. + 7).
//   Split     One workgroup per 16-row tile of W (epilogue 1: the gate tile n and the up tile F + n,
//             which share the B fragments), 4, 8 or 16 waves (the host picks from K).  The waves
//             split K: wave w owns the steps [w S / nw, (w + 1) S / nw) of the S = K / 64 steps, the
//             half step goes to wave 0 (the floor split gives it the fewest steps).  A wave keeps
//             kLoads = 8 W loads of 16 bytes per lane in flight (kLoads / 2 steps, or kLoads / 4 with
//             two tiles) before the first MFMA that consumes them; what is left of its slice after the
//             whole batches is one more batch whose absent steps are zeros.
//   Reduce    Every wave, one with an empty slice included (its accumulator is the exact zero it
//             started from), stores its 16 x 16 fp32 partial to LDS; after one barrier wave 0 adds the
//             partials in wave order 0, 1, ..., nw - 1.  No atomics, no second launch, no reduction
//             across workgroups: the same inputs give the same bits on every call.
//   Epilogue  0: round to bf16, store rows 0..M-1 (lane: batch row m = lane & 15, the 4 consecutive
//             n = n0 + 4 (lane / 16) .. + 3, one 8-byte store).  Accumulator columns M..15 are dropped.
//             1: packed SwiGLU over W = [W1 | W3] stacked on N = 2F: both sums are rounded to bf16 (as
//             the unfused path stores them between its two kernels), then silu(a) * b by the
//             expressions of llm_fused.hip's swiglu_packed_fwd_kernel, rounded to bf16 into y[M, F]:
//             bit-identical to epilogue 0 followed by that kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
using pto::f32x4;

constexpr int kRows = 16;       // W rows per tile, and the most batch rows (the MFMA's 16 x 16 output)
constexpr int kStep = 64;       // k values per step (two MFMAs)
constexpr int kLoads = 8;       // 16-byte W loads a lane has in flight
constexpr int kMaxWaves = 16;

// lane map (gfx950): A[i = lane & 15][k = 8 (lane >> 4) + e], B[k = 8 (lane >> 4) + e][j = lane & 15],
// D: j = lane & 15, i = 4 (lane >> 4) + reg.
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                 0, 0, 0);
}

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// llm_fused.hip's expressions, kept word for word: epilogue 1's bit-identity with that file's
// swiglu_packed_fwd_kernel rests on the compiler seeing the same arithmetic.
__device__ __forceinline__ float sigmoid(float a) { return 1.f / (1.f + __expf(-a)); }
__device__ __forceinline__ float swiglu_y(float a, float b) { return a * sigmoid(a) * b; }

// U steps from step s on: every load first, then the MFMAs.  GUARD: steps at or past s1 are zeros
// (s1 is the same for the whole wave, so the guards are scalar branches).
template <int TILES, int U, bool GUARD>
__device__ __forceinline__ void steps(const uint16_t* (&wp)[TILES], const uint16_t* xp, bool live, int s,
                                      int s1, f32x4 (&acc)[TILES]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 a[TILES][U][2], b[U][2];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long k = (long)(s + u) * kStep;
    const bool on = !GUARD || s + u < s1;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      a[t][u][0] = on ? ld16(wp[t] + k) : zero;
      a[t][u][1] = on ? ld16(wp[t] + k + 8) : zero;
    }
    b[u][0] = on && live ? ld16(xp + k) : zero;
    b[u][1] = on && live ? ld16(xp + k + 8) : zero;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) acc[t] = mfma(a[t][u][h], b[u][h], acc[t]);
    }
  }
}

// grid: one workgroup per tile (N / 16, or F / 16 with TILES == 2); nw * 64 threads.  `second` is the
// row distance from the first tile to the second (F).
template <int TILES>
__global__ __launch_bounds__(kMaxWaves * 64) void skinny_gemm_kernel(const uint16_t* __restrict__ x,
                                                                    const uint16_t* __restrict__ w,
                                                                    uint16_t* __restrict__ y, int M, int K,
                                                                    int ldy, int second) {
  constexpr int U = kLoads / (2 * TILES);
  __shared__ f32x4 red[TILES][kMaxWaves][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kRows;
  const bool live = r < M;  // as a B lane: batch row r exists; as a D lane: column r is stored

  const uint16_t* wrow[TILES];
  const uint16_t* wp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    wrow[t] = w + (long)(n0 + t * second + r) * K;
    wp[t] = wrow[t] + g * 16;
  }
  const uint16_t* xrow = x + (long)(live ? r : 0) * K;  // a dead lane never dereferences it
  const uint16_t* xp = xrow + g * 16;

  f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = pto::zero4();

  const int S = K / kStep;
  const int s0 = (int)((long)wv * S / nw), s1 = (int)((long)(wv + 1) * S / nw);
  int s = s0;
  for (; s + U <= s1; s += U) steps<TILES, U, false>(wp, xp, live, s, s1, acc);
  if (s < s1) steps<TILES, U, true>(wp, xp, live, s, s1, acc);
  if (wv == 0 && (K % kStep)) {  // the 32-wide half step, plain k order
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const long k = (long)S * kStep + g * 8;
    u32x4 a[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) a[t] = ld16(wrow[t] + k);
    const u32x4 b = live ? ld16(xrow + k) : zero;
#pragma unroll
    for (int t = 0; t < TILES; ++t) acc[t] = mfma(a[t], b, acc[t]);
  }

#pragma unroll
  for (int t = 0; t < TILES; ++t) red[t][wv][lane] = acc[t];
  __syncthreads();
  if (wv != 0 || !live) return;

  f32x4 sum[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    sum[t] = red[t][0][lane];
    for (int k = 1; k < nw; ++k) sum[t] += red[t][k][lane];
  }
  u32x2 out;
  if constexpr (TILES == 1) {
    out.x = pto::bf16_pack(sum[0][0], sum[0][1]);
    out.y = pto::bf16_pack(sum[0][2], sum[0][3]);
  } else {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[i] = swiglu_y(pto::bf2f(pto::bf16_rne(sum[0][i])), pto::bf2f(pto::bf16_rne(sum[1][i])));
    out.x = pto::bf16_pack(o[0], o[1]);
    out.y = pto::bf16_pack(o[2], o[3]);
  }
  *reinterpret_cast<u32x2*>(y + (long)r * ldy + n0 + g * 4) = out;
}

// Waves per workgroup.  A wave should have a whole batch of loads (kLoads / 2 steps) to issue, and a
// layer's projections should fill the machine: N / 16 tiles alone are 256 workgroups at N = 4096.
int waves_for(int K) { return K >= 2048 ? 16 : (K >= 1024 ? 8 : 4); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

long pto_skinny_max_rows() { return kRows; }

// The waves per workgroup pto_skinny_gemm launches at this K (tests and benchmarks report it).
long pto_skinny_waves(int K) { return waves_for(K); }

// x [M, K], w [N, K] bf16, contiguous, 16-byte aligned.  epilogue 0: y [M, N] = x . w^T in bf16.
// epilogue 1: w = [W1 | W3] stacked on N = 2F, y [M, F] = silu(x . W1^T) * (x . W3^T).
// -1: a shape outside the contract (1 <= M <= 16, N % 16 == 0 -- N % 32 == 0 with epilogue 1 --
// K % 32 == 0); -2: a misaligned pointer.
int pto_skinny_gemm(const void* x, const void* w, void* y, int M, int N, int K, int epilogue, void* stream) {
  if (epilogue < 0 || epilogue > 1 || M < 1 || M > kRows || N <= 0 || K <= 0 || K % 32 ||
      N % (kRows * (epilogue + 1)))
    return -1;
  if (!aligned16(x) || !aligned16(w) || !aligned16(y)) return -2;
  const dim3 block((unsigned)waves_for(K) * 64);
  if (epilogue == 0)
    hipLaunchKernelGGL(skinny_gemm_kernel<1>, dim3((unsigned)(N / kRows)), block, 0, (hipStream_t)stream,
                       (const uint16_t*)x, (const uint16_t*)w, (uint16_t*)y, M, K, N, 0);
  else
    hipLaunchKernelGGL(skinny_gemm_kernel<2>, dim3((unsigned)(N / 2 / kRows)), block, 0, (hipStream_t)stream,
                       (const uint16_t*)x, (const uint16_t*)w, (uint16_t*)y, M, K, N / 2, N / 2);
  return (int)hipGetLastError();
}

}  // extern "C"
