// Skinny GEMM on FP8 weights for the Llama decode step: y[M, N] = (x[M, K] . q[N, K]^T) * scale[N] with
// 1 <= M <= 16 batch rows, x bf16, q OCP e4m3 and K-contiguous with one fp32 power-of-two scale per output
// row (ops.skinny.quantize_rows), fp32 accumulation, bf16 out.  skinny_gemm.hip runs at the rate its weight
// bytes stream; this kernel streams half of them.  Activations are not quantised and the MFMA is the bf16
// one: e4m3 -> bf16 is exact, so the kernel computes the bf16 GEMM on the dequantised weights.
//
//   Operands  v_mfma_f32_16x16x32_bf16 with W as the A operand (16 weight rows n = the 16 x 32 A tile, x the
//             32 x 16 B tile, batch row m = column, rows M..15 zeros held in registers and never read from
//             memory), D[n][m] = sum_k q[n][k] x[m][k].  W goes HBM -> VGPR -> MFMA without LDS.
//   Widening  v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8): one VALU
//             instruction turns two e4m3 bytes (the low or the high half of a dword, by op_sel) into one
//             dword of two bf16, which is an MFMA operand dword as it stands: 4 instructions per A fragment.
//             The other candidate, v_cvt_pk_f32_fp8, gives two fp32 per instruction and then needs a
//             v_lshrrev_b32 and a v_and_or_b32 per output dword to take the upper halves: 3 per dword, 12
//             per fragment, in the generated ISA of both.  Both are exact over all 254 finite codes
//             (e4m3 has 3 mantissa bits and its subnormals are normal bf16 values).
//   k order   The MFMA's k index is free as long as A and B agree.  A step is 128 k values = four MFMAs: lane
//             group g = lane / 16 takes the 32 consecutive bytes k0 + 32 g .. + 31 of its W row (two adjacent
//             16-byte loads; the four groups of a row read one whole 128-byte line per step), bytes 8 j .. + 7
//             for the step's MFMA j.  The matching B fragment is the 32 consecutive bf16 k0 + 32 g .. + 31 of
//             the x row (four 16-byte loads), 8 per MFMA.  K % 128 == 64 leaves one 64-wide half step, two
//             MFMAs in the plain order (MFMA h, group g: k0 + 32 h + 8 g .. + 7; 8-byte W loads).
//   Tiles     A wave keeps T = 1, 2 or 4 accumulators: T tiles of 16 W rows that share every B fragment, so
//             x crosses L2 once per T tiles (at M = 16 and T = 1 that traffic is 2 x the weight bytes, with
//             T = 4 half of them).  A workgroup owns T consecutive tiles -- with epilogue 1, T / 2 consecutive
//             gate / up pairs at n and F + n -- and the last one may own fewer (a scalar guard: absent
//             tiles load zeros and store nothing).  The host picks T from (M, N): tiles_for().
//   Split     4, 8 or 16 waves per workgroup (from K, as skinny_gemm.hip).  The waves split K: wave w owns
//             the steps [w S / nw, (w + 1) S / nw) of the S = K / 128 steps, the half step goes to wave 0
//             (the floor split gives it the fewest steps).  A wave keeps kLoads = 8 W loads of 16 bytes per
//             lane in flight (kLoads / (2 T) steps) before the first conversion that consumes them; 16
//             waves are 4 per SIMD, 128 registers a lane: T = 1 holds 8 W + 16 x loads (96 registers) at
//             most, T = 4 8 W + 4 x loads and 16 accumulator registers.  What is left of a slice after the
//             whole batches is one more batch whose absent steps are zeros.
//   Reduce    Waves 1 .. nw - 1 (an empty slice included: its accumulator is the exact zero it started
//             from) store their 16 x 16 fp32 partials to LDS; after one barrier wave 0 adds them to its own
//             in wave order.  No atomics, no second launch, and the split depends on K alone: the same
//             inputs give the same bits on every call and for every T.
//   Epilogue  sum * scale[n] (exact: a power of two), then as skinny_gemm.hip.  0: round to bf16, store rows
//             0..M-1 (lane: batch row m = lane & 15, the 4 consecutive n = n0 + 4 (lane / 16) .. + 3, one
//             8-byte store).  1: packed SwiGLU over q = [W1 | W3] stacked on N = 2F: both scaled sums are
//             rounded to bf16, then silu(a) * b by the expressions of llm_fused.hip's swiglu_packed_fwd_kernel,
//             rounded to bf16 into y[M, F]: bit-identical to epilogue 0 followed by that kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
using pto::f32x4;

constexpr int kRows = 16;       // W rows per tile, and the most batch rows (the MFMA's 16 x 16 output)
constexpr int kStep = 128;      // k values per step (four MFMAs, one 128-byte line of a W row)
constexpr int kLoads = 8;       // 16-byte W loads a lane has in flight
constexpr int kMaxWaves = 16;
constexpr int kMaxTiles = 4;
constexpr int kCUs = 256;

// lane map (gfx950): A[i = lane & 15][k = 8 (lane >> 4) + e], B[k = 8 (lane >> 4) + e][j = lane & 15],
// D: j = lane & 15, i = 4 (lane >> 4) + reg.
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                 0, 0, 0);
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

__device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x2 ld8(const void* p) { return *reinterpret_cast<const u32x2*>(p); }

// llm_fused.hip's expressions, kept word for word: epilogue 1's bit-identity with that file's
// swiglu_packed_fwd_kernel rests on the compiler seeing the same arithmetic.
__device__ __forceinline__ float sigmoid(float a) { return 1.f / (1.f + __expf(-a)); }
__device__ __forceinline__ float swiglu_y(float a, float b) { return a * sigmoid(a) * b; }

// U steps from step s on: every load first, then the conversions and MFMAs.  GUARD: steps at or past s1 are
// zeros (s1 is the same for the whole wave, and nt for the whole workgroup, so the guards are scalar branches).
template <int T, int U, bool GUARD>
__device__ __forceinline__ void steps(const uint8_t* (&wp)[T], const uint16_t* xp, bool live, int nt, int s, int s1,
                                      f32x4 (&acc)[T]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 a[T][U][2], b[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long k = (long)(s + u) * kStep;
    const bool on = !GUARD || s + u < s1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      a[t][u][0] = on && t < nt ? ld16(wp[t] + k) : zero;
      a[t][u][1] = on && t < nt ? ld16(wp[t] + k + 16) : zero;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) b[u][j] = on && live ? ld16(xp + k + 8 * j) : zero;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = mfma(widen(a[t][u][j >> 1][2 * (j & 1)], a[t][u][j >> 1][2 * (j & 1) + 1]), b[u][j], acc[t]);
    }
  }
}

// grid: one workgroup per T tiles (SWIGLU: per T / 2 gate / up pairs); nw * 64 threads.  `tiles` is the
// number of tiles (pairs) in all, F the row distance from a gate tile to its up tile.
template <int T, bool SWIGLU>
__global__ __launch_bounds__(kMaxWaves * 64) void skinny_gemm_fp8_kernel(const uint16_t* __restrict__ x,
                                                                        const uint8_t* __restrict__ q,
                                                                        const float* __restrict__ scale,
                                                                        uint16_t* __restrict__ y, int M, int K,
                                                                        int ldy, int tiles, int F) {
  constexpr int U = kLoads / (2 * T) > 0 ? kLoads / (2 * T) : 1;
  constexpr int P = SWIGLU ? 2 : 1;  // accumulators per output tile
  static_assert(T % P == 0, "SwiGLU tiles come in pairs");
  __shared__ f32x4 red[T][kMaxWaves - 1][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int first = blockIdx.x * (T / P);          // this workgroup's first tile (pair)
  const int left = tiles - first;                  // >= 1
  const int nt = left < T / P ? left * P : T;      // accumulators in use
  const bool live = r < M;  // as a B lane: batch row r exists; as a D lane: column r is stored

  int n0[T];  // the first W row of accumulator t; an absent one keeps row 0 and is never dereferenced
  const uint8_t* wrow[T];
  const uint8_t* wp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    n0[t] = t < nt ? (first + t / P) * kRows + (t % P) * F : 0;
    wrow[t] = q + (long)(n0[t] + r) * K;
    wp[t] = wrow[t] + g * 32;
  }
  const uint16_t* xrow = x + (long)(live ? r : 0) * K;  // a dead lane never dereferences it
  const uint16_t* xp = xrow + g * 32;

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = pto::zero4();

  const int S = K / kStep;
  const int s0 = (int)((long)wv * S / nw), s1 = (int)((long)(wv + 1) * S / nw);
  int s = s0;
  for (; s + U <= s1; s += U) steps<T, U, false>(wp, xp, live, nt, s, s1, acc);
  if (s < s1) steps<T, U, true>(wp, xp, live, nt, s, s1, acc);
  if (wv == 0 && (K % kStep)) {  // the 64-wide half step, plain k order
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const u32x2 zero2 = {0u, 0u};
    const long k = (long)S * kStep + g * 8;
    u32x2 a[T][2];
    u32x4 b[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int t = 0; t < T; ++t) a[t][h] = t < nt ? ld8(wrow[t] + k + 32 * h) : zero2;
      b[h] = live ? ld16(xrow + k + 32 * h) : zero;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = mfma(widen(a[t][h][0], a[t][h][1]), b[h], acc[t]);
    }
  }

  if (wv != 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) red[t][wv - 1][lane] = acc[t];
  }
  __syncthreads();
  if (wv != 0 || !live) return;

#pragma unroll
  for (int t = 0; t < T; ++t) {
    for (int k = 1; k < nw; ++k) {
      const f32x4 p = red[t][k - 1][lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] += p[i];
    }
  }
#pragma unroll
  for (int t = 0; t < T; t += P) {
    if (t >= nt) break;
    float v[P][4];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[p][i] = acc[t + p][i] * scale[n0[t + p] + g * 4 + i];
    }
    u32x2 out;
    if constexpr (!SWIGLU) {
      out.x = pto::bf16_pack(v[0][0], v[0][1]);
      out.y = pto::bf16_pack(v[0][2], v[0][3]);
    } else {
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = swiglu_y(pto::bf2f(pto::bf16_rne(v[0][i])), pto::bf2f(pto::bf16_rne(v[1][i])));
      out.x = pto::bf16_pack(o[0], o[1]);
      out.y = pto::bf16_pack(o[2], o[3]);
    }
    *reinterpret_cast<u32x2*>(y + (long)r * ldy + n0[t] + g * 4) = out;
  }
}

// Waves per workgroup: skinny_gemm.hip's choice.  The bytes in flight come from the waves, and a layer's
// projections should fill the machine.
int waves_for(int K) { return K >= 2048 ? 16 : (K >= 1024 ? 8 : 4); }

// Accumulators per wave.  Sharing a B fragment among T tiles divides the x traffic and the number of
// workgroups by T; what it must not do is leave CUs idle.  With the workgroups dealt round over the CUs, the
// busiest CU streams per * ceil(workgroups / CUs) tiles: the choice is the per (tiles, or with epilogue 1
// gate / up pairs, per workgroup) that makes this least, and the largest such.  So N = 4096 (256 tiles) keeps
// one tile per workgroup, 6144 (384) takes two, the lm-head four.  M is part of the interface and does not
// enter: in profiles/skinny_fp8/linear.json the best T of a shape is the same at M = 1, 8 and 16.
int tiles_for(int M, int N, int epilogue) {
  (void)M;
  const int P = epilogue + 1, units = N / (kRows * P);
  int best = 1, load = 0;
  for (int per = 1; per <= kMaxTiles / P; per *= 2) {
    const int wgs = (units + per - 1) / per, l = per * ((wgs + kCUs - 1) / kCUs);
    if (per == 1 || l <= load) best = per, load = l;
  }
  return best * P;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int T, bool SWIGLU>
void launch(const void* x, const void* q, const void* scale, void* y, int M, int N, int K, hipStream_t stream) {
  const int P = SWIGLU ? 2 : 1, tiles = N / (kRows * P), per = T / P;
  hipLaunchKernelGGL((skinny_gemm_fp8_kernel<T, SWIGLU>), dim3((unsigned)((tiles + per - 1) / per)),
                     dim3((unsigned)waves_for(K) * 64), 0, stream, (const uint16_t*)x, (const uint8_t*)q,
                     (const float*)scale, (uint16_t*)y, M, K, N / P, tiles, SWIGLU ? N / 2 : 0);
}

}  // namespace

extern "C" {

// The waves per workgroup pto_skinny_fp8_gemm launches at this K (tests and benchmarks report it).
long pto_skinny_fp8_waves(int K) { return waves_for(K); }

// The accumulators per wave that tiles = 0 means at this shape.
long pto_skinny_fp8_tiles(int M, int N, int epilogue) { return tiles_for(M, N, epilogue); }

// x [M, K] bf16, q [N, K] e4m3, scale [N] fp32, contiguous; x, q and y 16-byte aligned, scale 4.  epilogue 0:
// y [M, N] = (x . q^T) * scale in bf16.  epilogue 1: q = [W1 | W3] stacked on N = 2F, y [M, F] =
// silu(a) * b of the two halves.  tiles: accumulators per wave, 1, 2 or 4, or 0 for tiles_for(); epilogue 1
// works in pairs and runs a request of 1 as 2.  The result does not depend on it.
// -1: outside the contract (1 <= M <= 16, N % 16 == 0 -- N % 32 == 0 with epilogue 1 --, K % 64 == 0,
// tiles in {0, 1, 2, 4}); -2: a misaligned pointer.
int pto_skinny_fp8_gemm(const void* x, const void* q, const void* scale, void* y, int M, int N, int K,
                        int epilogue, int tiles, void* stream) {
  if (epilogue < 0 || epilogue > 1 || M < 1 || M > kRows || N <= 0 || K <= 0 || K % 64 ||
      N % (kRows * (epilogue + 1)) || (tiles != 0 && tiles != 1 && tiles != 2 && tiles != 4))
    return -1;
  if (!aligned(x, 16) || !aligned(q, 16) || !aligned(y, 16) || !aligned(scale, 4)) return -2;
  if (tiles == 0) tiles = tiles_for(M, N, epilogue);
  hipStream_t st = (hipStream_t)stream;
  if (epilogue == 0) {
    if (tiles == 1) launch<1, false>(x, q, scale, y, M, N, K, st);
    else if (tiles == 2) launch<2, false>(x, q, scale, y, M, N, K, st);
    else launch<4, false>(x, q, scale, y, M, N, K, st);
  } else {
    if (tiles <= 2) launch<2, true>(x, q, scale, y, M, N, K, st);
    else launch<4, true>(x, q, scale, y, M, N, K, st);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
