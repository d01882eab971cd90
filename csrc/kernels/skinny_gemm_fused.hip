// The decode step's residual add and RMSNorm folded into the skinny GEMMs (skinny_gemm.hip on bf16 weights,
// skinny_gemm_fp8.hip on e4m3 weights with a power-of-two scale per row).  RMSNorm's row scale commutes with
// the projection after it, rstd[m] sum_k (h[m,k] g[k]) W[n,k] == sum_k (h[m,k] rstd[m] g[k]) W[n,k], so the
// norm between two projections needs no launch of its own:
//
//   Residual epilogue (wo, w2): the GEMM that produces a branch output adds the residual.  With d =
//             bf16_rne(acc) (times scale[n] first for e4m3: the bits the plain kernels store) and
//             hf = float(resid) + float(d) it writes the new stream h = hf (fp32 or bf16, the stream's dtype),
//             the next GEMM's operand a = bf16_rne(hf * gamma[n]), and ss[m][tile] = the sum of hf^2 over the
//             tile's 16 columns: a lane's four squares, each rounded, in column order, then the four lane
//             groups in order (one wave shuffle each), contraction off.  The order is the tile's alone: the
//             same inputs give the same bits for every wave and tile count.
//   Row-scale epilogue (wqkv, w13 + SwiGLU, lm-head): the GEMM that consumes a runs on it as the plain
//             kernels do and multiplies its accumulators by rstd[m] = rsqrtf(sum_t ss[m][t] / K + eps) before
//             the bf16 rounding (acc * scale[n] first for e4m3: exact).  SwiGLU then runs on the rounded pair
//             as the plain kernels' epilogue 1 does.
//   Partials  A row has K / 16 of them (256 at K = 4096).  They are summed in 16 chains: chain c adds
//             ss[m][c], ss[m][c + 16], ... in ascending order.  Lane (r, g) of wave w < 4 owns chain 4 w + g
//             of row r (the four groups of a row read 16 consecutive bytes per load), issues its loads before
//             its streaming loop, four at a time, and leaves the chain's sum in LDS; after the reduce's one
//             barrier every lane of wave 0 adds the 16 chains of its row in chain order.  Nothing here depends
//             on the waves or tiles of the launch, and nothing is loaded after the streaming loop.
//
// The operand path is the plain kernels', for both weight formats from one template: W is the A operand of
// v_mfma_f32_16x16x32_bf16 straight from 16-byte global loads (e4m3 widened by v_cvt_scalef32_pk_bf16_fp8),
// no LDS on the W path; a lane's slice of a step is 32 bytes of its W row in either format (16 bf16: a step is
// 64 k values and two MFMAs; 32 e4m3: 128 k values and four); the waves split the steps by the floor rule and
// wave 0 takes the half step (32 or 64 k values in the plain order); wave 0 adds the other waves' partials in
// wave order.  Every accumulator so sees the MFMAs of the plain kernel in the plain kernel's order, which is
// what makes d its bits.  e4m3 keeps 1, 2 or 4 tiles per wave sharing the x fragments; bf16 keeps one (two
// with SwiGLU).  Rows at or past M are neither read nor written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_vec.h"

extern "C" long pto_skinny_waves(int K);
extern "C" long pto_skinny_fp8_waves(int K);
extern "C" long pto_skinny_fp8_tiles(int M, int N, int epilogue);

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
using pto::f32x4;

constexpr int kRows = 16;       // W rows per tile, and the most batch rows (the MFMA's 16 x 16 output)
constexpr int kLoads = 8;       // 16-byte W loads a lane has in flight
constexpr int kMaxWaves = 16;
constexpr int kChains = 16;     // chains the K / 16 partials of a row are summed in
constexpr int kStepBytes = 128; // bytes of a W row per step, in either format

enum { kResid = 0, kScale = 1, kSwiglu = 2 };

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

// The A fragment of a step's MFMA j from the lane's two 16-byte loads.
template <bool FP8>
__device__ __forceinline__ u32x4 fragment(const u32x4 (&a)[2], int j) {
  if constexpr (FP8) return widen(a[j >> 1][2 * (j & 1)], a[j >> 1][2 * (j & 1) + 1]);
  else return a[j];
}

// llm_fused.hip's expressions, kept word for word: the SwiGLU epilogue's bit-identity with that file's
// swiglu_packed_fwd_kernel rests on the compiler seeing the same arithmetic.
__device__ __forceinline__ float sigmoid(float a) { return 1.f / (1.f + __expf(-a)); }
__device__ __forceinline__ float swiglu_y(float a, float b) { return a * sigmoid(a) * b; }

// The roundings of the epilogues, spelled out with the compiler's own contraction off (as rmsnorm.hip's).
__device__ __forceinline__ float add_rounded(float resid, float v) {
#pragma clang fp contract(off)
  return resid + pto::bf2f(pto::bf16_rne(v));
}
__device__ __forceinline__ float squares4(const float (&h)[4]) {
#pragma clang fp contract(off)
  float s = h[0] * h[0];
  s += h[1] * h[1];
  s += h[2] * h[2];
  s += h[3] * h[3];
  return s;
}
__device__ __forceinline__ float rstd_of(float total, int K, float eps) {
#pragma clang fp contract(off)
  return rsqrtf(total / (float)K + eps);
}

// U steps from step s on: every load first, then the conversions and MFMAs.  GUARD: steps at or past s1 are
// zeros (s1 is the same for the whole wave, and nt for the whole workgroup, so the guards are scalar branches).
template <bool FP8, int T, int U, bool GUARD>
__device__ __forceinline__ void steps(const uint8_t* (&wp)[T], const uint16_t* xp, bool live, int nt, int s, int s1,
                                      f32x4 (&acc)[T]) {
  constexpr int NM = FP8 ? 4 : 2;  // MFMAs per step
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 a[T][U][2], b[U][NM];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long kb = (long)(s + u) * kStepBytes, kx = (long)(s + u) * (NM * 32);
    const bool on = !GUARD || s + u < s1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      a[t][u][0] = on && t < nt ? ld16(wp[t] + kb) : zero;
      a[t][u][1] = on && t < nt ? ld16(wp[t] + kb + 16) : zero;
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) b[u][j] = on && live ? ld16(xp + kx + 8 * j) : zero;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = mfma(fragment<FP8>(a[t][u], j), b[u][j], acc[t]);
    }
  }
}

// What the epilogues read and write beside the GEMM's own operands.
struct Epilogue {
  const void* resid;    // kResid: [M, N], the stream's dtype
  const float* gamma;   // kResid: [N]
  void* h;              // kResid: [M, N], the stream's dtype
  uint16_t* a;          // kResid: [M, N] bf16
  float* ss_out;        // kResid: [M, N / 16]
  const float* ss_in;   // kScale, kSwiglu: [M, K / 16]
  float eps;
  uint16_t* y;          // kScale: [M, N]; kSwiglu: [M, N / 2]
};

// grid: one workgroup per T tiles (kSwiglu: per T / 2 gate / up pairs); nw * 64 threads.  `tiles` is the
// number of tiles (pairs) in all, F the row distance from a gate tile to its up tile, ldo the row length of
// the outputs.  TS: the stream's storage (float or bf16 bits), used by kResid alone.
template <bool FP8, int T, int EPI, typename TS>
__global__ __launch_bounds__(kMaxWaves * 64) void skinny_fused_kernel(const uint16_t* __restrict__ x,
                                                                     const uint8_t* __restrict__ w,
                                                                     const float* __restrict__ scale, int M, int K,
                                                                     int ldo, int tiles, int F, Epilogue e) {
  constexpr int ES = FP8 ? 1 : 2;                   // bytes per weight
  constexpr int kStep = kStepBytes / ES;            // k values per step
  constexpr int NH = FP8 ? 2 : 1;                   // MFMAs of the half step
  constexpr int U = kLoads / (2 * T) > 0 ? kLoads / (2 * T) : 1;
  constexpr int P = EPI == kSwiglu ? 2 : 1;         // accumulators per output tile
  static_assert(T % P == 0, "SwiGLU tiles come in pairs");
  __shared__ f32x4 red[T][kMaxWaves - 1][64];
  __shared__ float chain[EPI == kResid ? 1 : kChains][kRows];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int first = blockIdx.x * (T / P);          // this workgroup's first tile (pair)
  const int left = tiles - first;                  // >= 1
  const int nt = left < T / P ? left * P : T;      // accumulators in use
  const bool live = r < M;  // as a B lane: batch row r exists; as a D lane: column r is stored

  if constexpr (EPI != kResid) {
    if (wv < kChains / 4) {  // chain c of row r, before the streaming loop's loads
      const int c = 4 * wv + g, np = K / 16;
      float s = 0.f;
      if (live) {
        const float* p = e.ss_in + (long)r * np;
        int t = c;
        for (; t + 3 * kChains < np; t += 4 * kChains) {
          const float v0 = p[t], v1 = p[t + kChains], v2 = p[t + 2 * kChains], v3 = p[t + 3 * kChains];
          s += v0;
          s += v1;
          s += v2;
          s += v3;
        }
        for (; t < np; t += kChains) s += p[t];
      }
      chain[c][r] = s;
    }
  }

  int n0[T];  // the first W row of accumulator t; an absent one keeps row 0 and is never dereferenced
  const uint8_t* wrow[T];
  const uint8_t* wp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    n0[t] = t < nt ? (first + t / P) * kRows + (t % P) * F : 0;
    wrow[t] = w + (long)(n0[t] + r) * K * ES;
    wp[t] = wrow[t] + g * 32;
  }
  const uint16_t* xrow = x + (long)(live ? r : 0) * K;  // a dead lane never dereferences it
  const uint16_t* xp = xrow + g * (kStep / 4);

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = pto::zero4();

  const int S = K / kStep;
  const int s0 = (int)((long)wv * S / nw), s1 = (int)((long)(wv + 1) * S / nw);
  int s = s0;
  for (; s + U <= s1; s += U) steps<FP8, T, U, false>(wp, xp, live, nt, s, s1, acc);
  if (s < s1) steps<FP8, T, U, true>(wp, xp, live, nt, s, s1, acc);
  if (wv == 0 && (K % kStep)) {  // the half step, plain k order
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const long k = (long)S * kStep + g * 8;
    u32x4 a[T][NH], b[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (FP8) {
          const u32x2 q = t < nt ? ld8(wrow[t] + k + 32 * h) : u32x2{0u, 0u};
          a[t][h] = u32x4{q.x, q.y, 0u, 0u};
        } else {
          a[t][h] = ld16(wrow[t] + (k + 32 * h) * ES);
        }
      }
      b[h] = live ? ld16(xrow + k + 32 * h) : zero;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (FP8) acc[t] = mfma(widen(a[t][h][0], a[t][h][1]), b[h], acc[t]);
        else acc[t] = mfma(a[t][h], b[h], acc[t]);
      }
    }
  }

  if (wv != 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) red[t][wv - 1][lane] = acc[t];
  }
  __syncthreads();
  if (wv != 0) return;  // all 64 lanes of wave 0 stay: the ss shuffles below read dead lanes' zeros

#pragma unroll
  for (int t = 0; t < T; ++t) {
    for (int k = 1; k < nw; ++k) {
      const f32x4 p = red[t][k - 1][lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[t][i] += p[i];
    }
  }
  float rstd = 0.f;
  if constexpr (EPI != kResid) {
    float total = chain[0][r];
#pragma unroll
    for (int c = 1; c < kChains; ++c) total += chain[c][r];
    rstd = rstd_of(total, K, e.eps);
  }
#pragma unroll
  for (int t = 0; t < T; t += P) {
    if (t >= nt) break;  // the same for the whole wave
    float v[P][4];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[p][i] = acc[t + p][i];
        if constexpr (FP8) v[p][i] *= scale[n0[t + p] + g * 4 + i];
        if constexpr (EPI != kResid) v[p][i] *= rstd;
      }
    }
    const long o = (long)r * ldo + n0[t] + g * 4;
    if constexpr (EPI == kResid) {
      float hf[4] = {0.f, 0.f, 0.f, 0.f};
      if (live) pto::vload(static_cast<const TS*>(e.resid) + o, hf);
#pragma unroll
      for (int i = 0; i < 4; ++i) hf[i] = add_rounded(hf[i], v[0][i]);
      if (live) {
        pto::vstore(static_cast<TS*>(e.h) + o, hf);
        const float* gm = e.gamma + n0[t] + g * 4;
        u32x2 out;
        out.x = pto::bf16_pack(hf[0] * gm[0], hf[1] * gm[1]);
        out.y = pto::bf16_pack(hf[2] * gm[2], hf[3] * gm[3]);
        *reinterpret_cast<u32x2*>(e.a + o) = out;
      }
      const float q0 = squares4(hf);
      const float q1 = __shfl(q0, r + 16, 64), q2 = __shfl(q0, r + 32, 64), q3 = __shfl(q0, r + 48, 64);
      if (live && g == 0) e.ss_out[(long)r * (ldo / kRows) + n0[t] / kRows] = ((q0 + q1) + q2) + q3;
    } else if (live) {
      u32x2 out;
      if constexpr (EPI == kScale) {
        out.x = pto::bf16_pack(v[0][0], v[0][1]);
        out.y = pto::bf16_pack(v[0][2], v[0][3]);
      } else {
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          y[i] = swiglu_y(pto::bf2f(pto::bf16_rne(v[0][i])), pto::bf2f(pto::bf16_rne(v[1][i])));
        out.x = pto::bf16_pack(y[0], y[1]);
        out.y = pto::bf16_pack(y[2], y[3]);
      }
      *reinterpret_cast<u32x2*>(e.y + o) = out;
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <bool FP8, int T, int EPI, typename TS>
void launch(const void* x, const void* w, const void* scale, int M, int N, int K, const Epilogue& e, hipStream_t st) {
  const int P = EPI == kSwiglu ? 2 : 1, tiles = N / (kRows * P), per = T / P;
  const long nw = FP8 ? pto_skinny_fp8_waves(K) : pto_skinny_waves(K);
  hipLaunchKernelGGL((skinny_fused_kernel<FP8, T, EPI, TS>), dim3((unsigned)((tiles + per - 1) / per)),
                     dim3((unsigned)nw * 64), 0, st, (const uint16_t*)x, (const uint8_t*)w, (const float*)scale, M, K,
                     N / P, tiles, EPI == kSwiglu ? N / 2 : 0, e);
}

// T of the e4m3 form: the caller's 1, 2 or 4 (SwiGLU works in pairs and runs 1 as 2), or the plain kernel's choice.
template <int EPI, typename TS>
void launch_fp8(int tiles, const void* x, const void* q, const void* scale, int M, int N, int K, const Epilogue& e,
                hipStream_t st) {
  if (tiles == 0) tiles = (int)pto_skinny_fp8_tiles(M, N, EPI == kSwiglu);
  if constexpr (EPI != kSwiglu) {
    if (tiles == 1) return launch<true, 1, EPI, TS>(x, q, scale, M, N, K, e, st);
  }
  if (tiles <= 2) launch<true, 2, EPI, TS>(x, q, scale, M, N, K, e, st);
  else launch<true, 4, EPI, TS>(x, q, scale, M, N, K, e, st);
}

// Both weight formats: scale == nullptr is bf16 weights.  The -1 / -2 contract of the plain kernels, K % 32 == 0
// for bf16 and K % 64 == 0 for e4m3, tiles in {0, 1, 2, 4} (0 alone for bf16).
int check(const void* scale, int M, int N, int K, int swiglu, int tiles) {
  const bool fp8 = scale != nullptr;
  if (M < 1 || M > kRows || N <= 0 || K <= 0 || K % (fp8 ? 64 : 32) || N % (kRows * (swiglu + 1))) return -1;
  if (fp8 ? (tiles != 0 && tiles != 1 && tiles != 2 && tiles != 4) : tiles != 0) return -1;
  return 0;
}

int add_norm(const void* x, const void* w, const void* scale, const void* resid, const void* gamma, void* h, void* a,
             void* ss, int M, int N, int K, int stream_bf16, int tiles, void* stream) {
  if (check(scale, M, N, K, 0, tiles) || stream_bf16 < 0 || stream_bf16 > 1) return -1;
  if (!aligned(x, 16) || !aligned(w, 16) || !aligned(resid, 16) || !aligned(h, 16) || !aligned(a, 16) ||
      !aligned(gamma, 4) || !aligned(ss, 4) || !aligned(scale, 4))
    return -2;
  const Epilogue e = {resid, (const float*)gamma, h, (uint16_t*)a, (float*)ss, nullptr, 0.f, nullptr};
  hipStream_t st = (hipStream_t)stream;
  if (scale == nullptr) {
    if (stream_bf16) launch<false, 1, kResid, uint16_t>(x, w, scale, M, N, K, e, st);
    else launch<false, 1, kResid, float>(x, w, scale, M, N, K, e, st);
  } else {
    if (stream_bf16) launch_fp8<kResid, uint16_t>(tiles, x, w, scale, M, N, K, e, st);
    else launch_fp8<kResid, float>(tiles, x, w, scale, M, N, K, e, st);
  }
  return (int)hipGetLastError();
}

int scaled(const void* a, const void* w, const void* scale, const void* ss, float eps, void* y, int M, int N, int K,
           int epilogue, int tiles, void* stream) {
  if (epilogue < 0 || epilogue > 1 || check(scale, M, N, K, epilogue, tiles)) return -1;
  if (!aligned(a, 16) || !aligned(w, 16) || !aligned(y, 16) || !aligned(ss, 4) || !aligned(scale, 4)) return -2;
  const Epilogue e = {nullptr, nullptr, nullptr, nullptr, nullptr, (const float*)ss, eps, (uint16_t*)y};
  hipStream_t st = (hipStream_t)stream;
  if (scale == nullptr) {
    if (epilogue == 0) launch<false, 1, kScale, float>(a, w, scale, M, N, K, e, st);
    else launch<false, 2, kSwiglu, float>(a, w, scale, M, N, K, e, st);
  } else {
    if (epilogue == 0) launch_fp8<kScale, float>(tiles, a, w, scale, M, N, K, e, st);
    else launch_fp8<kSwiglu, float>(tiles, a, w, scale, M, N, K, e, st);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// The chains the row-scale epilogue sums a row's partials in (tests derive their bound from it).
long pto_skinny_fused_chains() { return kChains; }

// Residual epilogue.  x [M, K] bf16, w [N, K] bf16, resid and h [M, N] fp32 (stream_bf16 = 0) or bf16 (1), gamma
// [N] fp32, a [M, N] bf16, ss [M, N / 16] fp32, all contiguous; x, w, resid, h and a 16-byte aligned.
// h = resid + bf16(x . w^T), a = bf16(h * gamma), ss = the sums of h^2 per 16 columns.
// -1: a shape outside the contract (1 <= M <= 16, N % 16 == 0, K % 32 == 0); -2: a misaligned pointer.
int pto_skinny_add_norm(const void* x, const void* w, const void* resid, const void* gamma, void* h, void* a, void* ss,
                        int M, int N, int K, int stream_bf16, void* stream) {
  return add_norm(x, w, nullptr, resid, gamma, h, a, ss, M, N, K, stream_bf16, 0, stream);
}

// The same on q [N, K] e4m3 with scale [N] fp32: K % 64 == 0, tiles as pto_skinny_fp8_gemm's.
int pto_skinny_fp8_add_norm(const void* x, const void* q, const void* scale, const void* resid, const void* gamma,
                            void* h, void* a, void* ss, int M, int N, int K, int stream_bf16, int tiles,
                            void* stream) {
  if (scale == nullptr) return -2;
  return add_norm(x, q, scale, resid, gamma, h, a, ss, M, N, K, stream_bf16, tiles, stream);
}

// Row-scale epilogue.  a [M, K] bf16, w [N, K] bf16, ss [M, K / 16] fp32.  epilogue 0: y [M, N] =
// bf16(rstd[m] * (a . w^T)), rstd[m] = rsqrt(sum_t ss[m][t] / K + eps); epilogue 1: w = [W1 | W3], y [M, N / 2] =
// the packed SwiGLU of the rounded pair.  Returns as pto_skinny_gemm.
int pto_skinny_scaled(const void* a, const void* w, const void* ss, float eps, void* y, int M, int N, int K,
                      int epilogue, void* stream) {
  return scaled(a, w, nullptr, ss, eps, y, M, N, K, epilogue, 0, stream);
}

// The same on q [N, K] e4m3 with scale [N] fp32.  Returns as pto_skinny_fp8_gemm.
int pto_skinny_fp8_scaled(const void* a, const void* q, const void* scale, const void* ss, float eps, void* y, int M,
                          int N, int K, int epilogue, int tiles, void* stream) {
  if (scale == nullptr) return -2;
  return scaled(a, q, scale, ss, eps, y, M, N, K, epilogue, tiles, stream);
}

}  // extern "C"
