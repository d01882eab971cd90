// Skinny GEMM on MXFP4 weights for the Llama decode step: y[M, N] = x[M, K] . w[N, K]^T with 1 <= M <= 16 batch
// rows, x bf16, w in OCP MXFP4 (ops.skinny.quantize_rows_fp4): q [N, K / 2] bytes, the e2m1 code of k = 2 j in the
// low nibble of byte j and of k = 2 j + 1 in the high one, and scale [N, K / 32] e8m0 bytes, 2^(b - 127) for the 32
// k values of a block.  fp32 accumulation, bf16 out.  skinny_gemm_fp8.hip streams a byte per weight; this kernel
// streams 17 / 32 of one.  An e2m1 value times a power of two is exact in bf16, so the kernel computes the bf16
// GEMM on the dequantised weights, as the e4m3 kernel does.
//
//   Operands  v_mfma_f32_16x16x32_bf16 with W as the A operand (16 weight rows n = the 16 x 32 A tile, x the
//             32 x 16 B tile, batch row m = column, rows M..15 zeros held in registers and never read from
//             memory), D[n][m] = sum_k w[n][k] x[m][k].  W goes HBM -> VGPR -> MFMA without LDS.
//             Not the scaled f8f6f4 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4): it takes its scales per 32 k of
//             both operands and would want x in an 8-bit or narrower format.  Activations stay bf16 and
//             unquantised here, so that the decode step runs the very model the prefill sees; the kernel is bound
//             by the bytes of W either way, and the bf16 MFMA at M <= 16 is far from the limit.
//   Widening  v_cvt_scalef32_pk_bf16_fp4 (__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dword, scale, byte_sel)): one
//             VALU instruction turns byte byte_sel of a dword, two codes, into one dword of two bf16, which is an
//             MFMA operand dword as it stands, and multiplies by the block's scale on the way: 4 instructions per
//             A fragment, none for the scale.  Measured on an MI355X over all 256 bytes x every scale byte in
//             [2, 252] x the four byte_sel: the LOW nibble lands in the LOW half of the dword (the k order of the
//             format, no permutation needed); the scale operand is an fp32 of which the instruction reads the
//             exponent field alone (126.0 and 127.0 scale alike), so the operand is the e8m0 byte << 23, one
//             shift per block; the product is exact, subnormal bf16 results included, code 0x0 gives +0 and 0x8
//             gives -0 at every scale (a zero either way once added to an accumulator).  Byte 255 gives NaN, as
//             e8m0 says; bytes 0 and 1 scale exactly too, the quantiser emits neither.
//   k order   The MFMA's k index is free as long as A and B agree.  A step is 256 k values = eight MFMAs: lane
//             group g = lane / 16 takes the 32 consecutive bytes 128 s + 32 g .. + 31 of its W row (two adjacent
//             16-byte loads; the four groups of a row read one whole 128-byte line per step), the dword j of
//             them for the step's MFMA j: k = 256 s + 64 g + 8 j .. + 7, ascending within the fragment.  MFMAs
//             0..3 lie in the lane's first scale block and 4..7 in its second: the two scale bytes are one
//             2-byte load per step.  The matching B fragment is the 64 consecutive bf16 256 s + 64 g .. + 63 of
//             the x row (eight 16-byte loads), 8 per MFMA.  K % 256 == 128 leaves one 128-wide half step: group
//             g takes the 16 bytes 128 S + 16 g .. + 15 (one load, four MFMAs, one scale block, one scale byte).
//   Tiles     A wave keeps T = 1, 2 or 4 accumulators: T tiles of 16 W rows that share every B fragment, so x
//             crosses L2 once per T tiles: at 4 bits a weight the x bytes of a tile are 4 M times the W bytes.
//             A workgroup owns T consecutive tiles -- with epilogue 1, T / 2 consecutive gate / up pairs at n and
//             F + n -- and the last one may own fewer (a scalar guard: absent tiles load zeros and store
//             nothing).  The host picks T from N: tiles_for(), the e4m3 kernel's rule.
//   Split     4, 8 or 16 waves per workgroup (from K, as skinny_gemm.hip).  The waves split K: wave w owns the
//             steps [w S / nw, (w + 1) S / nw) of the S = K / 256 steps, the half step goes to wave 0 (the floor
//             split gives it the fewest steps).
//   Depth     kLoads = 8 W loads of 16 bytes per lane in flight, the e4m3 kernel's count, which here covers
//             1024 k per tile where it covered 512 there.  The budget is 128 registers a lane (16 waves are 4
//             per SIMD), and at 4 bits it is x that fills them: a step's B fragments are 32 registers against 8
//             for a tile's W.  So a batch issues all its W and scale loads first (T = 1: 4 steps, T = 2: 2, T = 4:
//             1; 32 + 4 registers) and takes x, which comes from L2, one step at a time between them and the
//             MFMAs.  Two steps of x at once (64 registers) spilled at T = 1 and 2; as it stands no variant
//             spills (102, 102 and 119 registers at T = 1, 2, 4; 123 at 4 with epilogue 1), and the compiler is free to hoist the next
//             step's x loads into what is left.  What is left of a slice after the whole batches is one more
//             batch whose absent steps are zeros.
//   Reduce    Waves 1 .. nw - 1 (an empty slice included: its accumulator is the exact zero it started
//             from) store their 16 x 16 fp32 partials to LDS; after one barrier wave 0 adds them to its own
//             in wave order.  No atomics, no second launch, and the split depends on K alone: the same
//             inputs give the same bits on every call and for every T.  The adds are IEEE fp32 adds in a stated
//             order and there is no multiply after them, so the file needs no -packed-fp32-ops entry.
//   Epilogue  As skinny_gemm.hip.  0: round to bf16, store rows 0..M-1 (lane: batch row m = lane & 15, the 4
//             consecutive n = n0 + 4 (lane / 16) .. + 3, one 8-byte store).  1: packed SwiGLU over w = [W1 | W3]
//             stacked on N = 2F: both sums are rounded to bf16, then silu(a) * b by the expressions of
//             llm_fused.hip's swiglu_packed_fwd_kernel, rounded to bf16 into y[M, F]: bit-identical to epilogue 0
//             followed by that kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
using pto::f32x4;

constexpr int kRows = 16;       // W rows per tile, and the most batch rows (the MFMA's 16 x 16 output)
constexpr int kStep = 256;      // k values per step (eight MFMAs, one 128-byte line of a W row)
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

// The conversion's scale operand of an e8m0 byte: the fp32 whose exponent field it is.
__device__ __forceinline__ float scale_of(uint32_t e8m0) { return __builtin_bit_cast(float, e8m0 << 23); }

// Eight e2m1 codes (one dword, k ascending from the low nibble) times the block's scale -> eight bf16 (an A
// fragment), exactly.
__device__ __forceinline__ u32x4 widen(uint32_t d, float sc) {
  u32x4 a;
  a[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 0));
  a[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 1));
  a[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 2));
  a[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, sc, 3));
  return a;
}

__device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }

// llm_fused.hip's expressions, kept word for word: epilogue 1's bit-identity with that file's
// swiglu_packed_fwd_kernel rests on the compiler seeing the same arithmetic.
__device__ __forceinline__ float sigmoid(float a) { return 1.f / (1.f + __expf(-a)); }
__device__ __forceinline__ float swiglu_y(float a, float b) { return a * sigmoid(a) * b; }

// U steps from step s on: every W and scale load first, then step by step the x loads, the conversions and the
// MFMAs.  wo: the byte offset in q of the lane's 32 bytes of step 0; a lane's scale bytes lie at a sixteenth of its
// W offset (32 k are 16 bytes of codes and one of scale, and a row of q is a multiple of 64 bytes).  GUARD: steps
// at or past s1 are zeros (s1 is the same for the whole wave, and nt for the whole workgroup, so the guards are
// scalar branches).
template <int T, int U, bool GUARD>
__device__ __forceinline__ void steps(const uint8_t* q, const uint8_t* scale, const long (&wo)[T], const uint16_t* xp,
                                      bool live, int nt, int s, int s1, f32x4 (&acc)[T]) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 a[T][U][2];
  uint32_t e[T][U];  // the step's two scale bytes
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool on = !GUARD || s + u < s1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const bool have = on && t < nt;
      const long o = wo[t] + (long)(s + u) * (kStep / 2);
      a[t][u][0] = have ? ld16(q + o) : zero;
      a[t][u][1] = have ? ld16(q + o + 16) : zero;
      e[t][u] = have ? *reinterpret_cast<const uint16_t*>(scale + (o >> 4)) : 0u;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool on = (!GUARD || s + u < s1) && live;
    u32x4 b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = on ? ld16(xp + (long)(s + u) * kStep + 8 * j) : zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float sc = scale_of(j < 4 ? e[t][u] & 0xffu : e[t][u] >> 8);
        acc[t] = mfma(widen(a[t][u][j >> 2][j & 3], sc), b[j], acc[t]);
      }
    }
  }
}

// grid: one workgroup per T tiles (SWIGLU: per T / 2 gate / up pairs); nw * 64 threads.  `tiles` is the
// number of tiles (pairs) in all, F the row distance from a gate tile to its up tile.
template <int T, bool SWIGLU>
__global__ __launch_bounds__(kMaxWaves * 64) void skinny_gemm_fp4_kernel(const uint16_t* __restrict__ x,
                                                                        const uint8_t* __restrict__ q,
                                                                        const uint8_t* __restrict__ scale,
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
  long wo[T];  // the byte offset in q of the lane's first 32 bytes
#pragma unroll
  for (int t = 0; t < T; ++t) {
    n0[t] = t < nt ? (first + t / P) * kRows + (t % P) * F : 0;
    wo[t] = (long)(n0[t] + r) * (K / 2) + g * 32;
  }
  const uint16_t* xrow = x + (long)(live ? r : 0) * K;  // a dead lane never dereferences it
  const uint16_t* xp = xrow + g * 64;

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = pto::zero4();

  const int S = K / kStep;
  const int s0 = (int)((long)wv * S / nw), s1 = (int)((long)(wv + 1) * S / nw);
  int s = s0;
  for (; s + U <= s1; s += U) steps<T, U, false>(q, scale, wo, xp, live, nt, s, s1, acc);
  if (s < s1) steps<T, U, true>(q, scale, wo, xp, live, nt, s, s1, acc);
  if (wv == 0 && (K % kStep)) {  // the 128-wide half step: 16 bytes and one scale block per lane group
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 a[T], b[4];
    uint32_t e[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const long o = wo[t] + (long)S * (kStep / 2) - g * 16;  // the row's bytes 128 S + 16 g .. + 15
      a[t] = t < nt ? ld16(q + o) : zero;
      e[t] = t < nt ? scale[o >> 4] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = live ? ld16(xrow + (long)S * kStep + g * 32 + 8 * j) : zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = mfma(widen(a[t][j], scale_of(e[t])), b[j], acc[t]);
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
    u32x2 out;
    if constexpr (!SWIGLU) {
      out.x = pto::bf16_pack(acc[t][0], acc[t][1]);
      out.y = pto::bf16_pack(acc[t][2], acc[t][3]);
    } else {
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = swiglu_y(pto::bf2f(pto::bf16_rne(acc[t][i])), pto::bf2f(pto::bf16_rne(acc[t + 1][i])));
      out.x = pto::bf16_pack(o[0], o[1]);
      out.y = pto::bf16_pack(o[2], o[3]);
    }
    *reinterpret_cast<u32x2*>(y + (long)r * ldy + n0[t] + g * 4) = out;
  }
}

// Waves per workgroup: skinny_gemm.hip's choice.  The bytes in flight come from the waves, and a layer's
// projections should fill the machine.
int waves_for(int K) { return K >= 2048 ? 16 : (K >= 1024 ? 8 : 4); }

// Accumulators per wave: skinny_gemm_fp8.hip's rule.  With the workgroups dealt round over the CUs, the busiest CU
// streams per * ceil(workgroups / CUs) tiles: the choice is the per (tiles, or with epilogue 1 gate / up pairs,
// per workgroup) that makes this least, and the largest such.  M is part of the interface and does not enter.
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
  hipLaunchKernelGGL((skinny_gemm_fp4_kernel<T, SWIGLU>), dim3((unsigned)((tiles + per - 1) / per)),
                     dim3((unsigned)waves_for(K) * 64), 0, stream, (const uint16_t*)x, (const uint8_t*)q,
                     (const uint8_t*)scale, (uint16_t*)y, M, K, N / P, tiles, SWIGLU ? N / 2 : 0);
}

}  // namespace

extern "C" {

// The waves per workgroup pto_skinny_fp4_gemm launches at this K (tests and benchmarks report it).
long pto_skinny_fp4_waves(int K) { return waves_for(K); }

// The accumulators per wave that tiles = 0 means at this shape.
long pto_skinny_fp4_tiles(int M, int N, int epilogue) { return tiles_for(M, N, epilogue); }

// x [M, K] bf16, q [N, K / 2] bytes of two e2m1 codes, scale [N, K / 32] e8m0 bytes, contiguous; x, q and y
// 16-byte aligned, scale 2 (its rows are K / 32 bytes, a multiple of 4: every 2-byte load of a step's scales is
// aligned).  epilogue 0: y [M, N] = x . w^T in bf16.  epilogue 1: w = [W1 | W3] stacked on N = 2F, y [M, F] =
// silu(a) * b of the two halves.  tiles: accumulators per wave, 1, 2 or 4, or 0 for tiles_for(); epilogue 1 works
// in pairs and runs a request of 1 as 2.  The result does not depend on it.
// -1: outside the contract (1 <= M <= 16, N % 16 == 0 -- N % 32 == 0 with epilogue 1 --, K % 128 == 0,
// tiles in {0, 1, 2, 4}); -2: a misaligned pointer.
int pto_skinny_fp4_gemm(const void* x, const void* q, const void* scale, void* y, int M, int N, int K,
                        int epilogue, int tiles, void* stream) {
  if (epilogue < 0 || epilogue > 1 || M < 1 || M > kRows || N <= 0 || K <= 0 || K % 128 ||
      N % (kRows * (epilogue + 1)) || (tiles != 0 && tiles != 1 && tiles != 2 && tiles != 4))
    return -1;
  if (!aligned(x, 16) || !aligned(q, 16) || !aligned(y, 16) || !aligned(scale, 2)) return -2;
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
