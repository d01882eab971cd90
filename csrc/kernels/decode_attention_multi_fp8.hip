// A decode step over S tokens per sequence on the e4m3 KV cache (decode_attention_fp8.hip has the format):
// decode_attention_multi.hip's two steps with half the cache bytes, both products on the matrix unit.
//
//   rope_append_multi_fp8  qkv [B, S, (Hq + 2 Hkv) D] bf16 -> q [B, S, Hq, D] rotated at pos[b] + s (64-bit sum);
//             the rotated k and the copied v are rounded to bf16, quantised per (token, kv head) by
//             decode_fp8.h's head_quantize and stored with their scales at cache row pos[b] + s.
//             rope_append_fp8_kernel with the token index split into (b, s): the same text, so q, codes and
//             scales equal S calls of it byte for byte.  A row outside [0, max_len) stores nothing to the cache
//             or the scales, token by token.  head_quantize's lane group: a token's groups come in multiples
//             of D / 8, B S of them too, and the grid stride is a multiple of 256, so the D / 8 threads of a
//             head are an aligned lane group of one wave; (b, s), the head and with them the early exit are
//             the same for all of them, so the group is whole whenever it reaches the quantiser.
//   decode_attn_multi_fp8  q, o [B, S, Hq, D] bf16; query s of sequence b sees the keys j < n_s,
//             n_s = min(lens[b], max_keys) - (S - 1 - s); n_s <= 0 gives a zero row.  R = S G <= 16 query rows
//             per kv head (row r = s G + g), G and S run-time arguments.
//     grid    (chunks of kChunk keys, Hkv, B), 256 threads; wave w owns keys 64 w .. 64 w + 63; a workgroup
//             whose chunk starts at or past n = min(lens[b], max_keys) leaves before its first load.
//     scores  S^T = K . q^T on v_mfma_f32_16x16x32_bf16: decode_attn_fp8_kernel's path (HBM -> VGPR, widened
//             exactly by v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, its k permutation) with q's R rows as the B
//             columns; columns at or past R are zeros that are never loaded.  All K loads of the wave's four
//             tiles are issued before the first conversion.  Accumulator lane (r = lane & 15, g = lane >> 4)
//             holds keys 4 g .. 4 g + 3 of each tile for row r and multiplies by k_scale[key] (exact: a power
//             of two) and 1 / sqrt(D): one aligned 16-byte load of the four scales where all four keys are
//             valid, by selection otherwise.
//     masks   by selection: a key slot at or past the chunk's valid count re-reads the last valid row; a score
//             whose key is at or past its row's n_s - c0 is -inf and its p an exact 0; a tile wholly past the
//             count is skipped by the whole wave.  Code rows and scales at or past the count are never read.
//     softmax per chunk and row in fp32 on the accumulators: 16 values per lane, xor 16 and 32 across the lane
//             groups, then the four waves through LDS in wave order.  l is the sum of the fp32 p.
//     P . V   O^T = V^T . P^T on the same MFMA.  p' = p v_scale[key] on the accumulators (exact: a power of
//             two, and bf16 has fp32's exponent range), split hi = bf16(p'), lo = bf16(p' - hi) and fed as two
//             MFMAs on one V fragment: P's relative error stays 2^-16.  V is staged in LDS as the e4m3 bytes
//             it is: the wave's 64 rows by 16-byte loads (issued before the softmax) into its own region, rows
//             D + 16 bytes apart, each 16-row tile a further 128 bytes on, so that the sixteen rows two lane
//             groups read together start at sixteen different 16-byte slots of the 256 bytes the banks span.
//             ds_read_b64_tr_b8 (map below) then returns, for d column lane & 15 of a 16-wide d tile, keys
//             4 g .. 4 g + 3 of tile t in one dword and of tile t + 1 in the other: k = 8 g + e <-> key
//             4 g + (e & 3) of tile t + (e >> 2), the accumulators' own order.  widen() makes them the A fragment.
//             The LDS image is half the bf16 kernel's (38 KiB against 72.5 at D = 128).
//     reduce  each wave writes its 16 x D fp32 partial over its own V region; after a barrier the workgroup
//             adds the four in wave order.  No atomics, no scratch; the same bits on every call.
//     partials decode_common.h's layout with S Hq heads, merged by decode_multi.h's decode_combine_multi_kernel
//             (one text for both caches).
//
//   ds_read_b64_tr_b8, as measured on gfx950 with a known tile: each lane of a 16-lane group names 8 bytes,
//             lane l16 the bytes 8 (l16 & 1) .. + 7 of row l16 >> 1 of an 8-row x 16-byte block whose rows may
//             lie anywhere (addresses are per lane); it receives byte l16 of the eight rows, rows 0 .. 3 in the
//             first dword and 4 .. 7 in the second, ascending.
#include "decode_fp8.h"
#include "decode_multi.h"

namespace {

typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int kPadB = 16;    // bytes between the V rows of a tile in the LDS image
constexpr int kSkewB = 128;  // bytes between the 16-row tiles, past their rows

using V8 = pto::Vec<8>;
using pto::vload;
using pto::vstore;

// ---------------------------------------------------------------------------- rope_append_multi_fp8
// One thread per 8-element group of a token's packed row; heads [0, Hq) -> q, [Hq, Hq+Hkv) -> k cache,
// the rest -> v cache.  Token (b, s) sits at position pos[b] + s.
__global__ __launch_bounds__(kT) void rope_append_multi_fp8_kernel(
    const uint16_t* __restrict__ pk, uint16_t* __restrict__ q, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    float* __restrict__ ks, float* __restrict__ vs, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ pos, long B, int S, int max_len, int sstride, int table_rows, int Hq, int Hkv, int D) {
  const int W = (Hq + 2 * Hkv) * D, gpr = W / 8, lpg = D / 8;
  const long groups = B * S * gpr;
  for (long gi = (long)blockIdx.x * kT + threadIdx.x; gi < groups; gi += (long)gridDim.x * kT) {
    const long tok = gi / gpr;
    const int c = (int)(gi - tok * gpr) * 8;
    const int hh = c / D, d0 = c - hh * D;
    const long b = tok / S;
    const long p = (long)pos[b] + (tok - b * S);  // 64-bit: pos near INT_MAX must not wrap into the cache
    const bool in_cache = p >= 0 && p < max_len;
    if (hh >= Hq && !in_cache) continue;  // the cache has no such row (the head's whole lane group leaves)
    const bool rot = hh < Hq + Hkv;
    const V8 in = vload<8>(pk + tok * W + c);
    V8 out = in;
    if (rot) {
      const int s = p < 0 ? 0 : (p >= table_rows ? table_rows - 1 : (int)p);
      // sign and the sign * sin products mirror rope_qkv_kernel's expressions (its dir argument): exact,
      // and kept so that the compiler sees the same arithmetic -- the bit-identity with that kernel rests on it
      const float sign = 1.f;
      const float4 cv = *reinterpret_cast<const float4*>(cosb + (long)s * (D / 2) + d0 / 2);
      const float4 sv = *reinterpret_cast<const float4*>(sinb + (long)s * (D / 2) + d0 / 2);
      const float cs[4] = {cv.x, cv.y, cv.z, cv.w}, sn[4] = {sign * sv.x, sign * sv.y, sign * sv.z, sign * sv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x0 = in.v[2 * i], x1 = in.v[2 * i + 1];
        out.v[2 * i] = x0 * cs[i] - x1 * sn[i];
        out.v[2 * i + 1] = x0 * sn[i] + x1 * cs[i];
      }
    }
    if (hh < Hq) {
      vstore(q + (tok * Hq + hh) * D + d0, out);
      continue;
    }
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = pto::bf2f(pto::bf16_rne(out.v[i]));  // the row the bf16 cache would hold
    const bool isk = hh < Hq + Hkv;
    const int h = isk ? hh - Hq : hh - Hq - Hkv;
    const long row = b * max_len + p;
    head_quantize(x, lpg, d0 == 0, (isk ? kc : vc) + (row * Hkv + h) * D + d0,
                  (isk ? ks : vs) + (b * Hkv + h) * sstride + p);
  }
}

// ---------------------------------------------------------------------------- decode_attn_multi_fp8
__device__ __forceinline__ i32x2 tr_read8(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(p));
}

// The four scales of keys key .. key + 3 of the chunk; a key at or past nloc gives 0 and is never read.
__device__ __forceinline__ void scales4(const float* __restrict__ sc, int key, int nloc, float (&s)[4]) {
  if (key + 3 < nloc) {
    const float4 v4 = *reinterpret_cast<const float4*>(sc + key);
    s[0] = v4.x; s[1] = v4.y; s[2] = v4.z; s[3] = v4.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = key + i < nloc ? sc[key + i] : 0.f;
  }
}

template <int D>
__global__ __launch_bounds__(kT) void decode_attn_multi_fp8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ ks, const float* __restrict__ vs, const int* __restrict__ lens, float* __restrict__ po,
    float* __restrict__ pm, float* __restrict__ pl, int max_len, int sstride, int max_keys, int Hkv, int G, int S,
    int nchunks, float scale) {
  constexpr int NM = D / 32;            // score MFMAs per key tile
  constexpr int NL = D / 64;            // 16-byte K loads per lane and tile
  constexpr int ND = D / 16;            // 16-wide output tiles along d
  constexpr int RS = D + kPadB;         // V row stride in LDS, bytes
  constexpr int TS = 16 * RS + kSkewB;  // V tile stride in LDS, bytes
  constexpr int CPR = D / 16;           // 16-byte chunks per V row
  constexpr int NV = kWaveKeys * CPR / 64;  // 16-byte V loads per lane
  constexpr int RPI = 64 / CPR;         // V rows per wave load instruction
  static_assert(kTiles * 16 * (kT / 64) == kChunk, "the waves' key tiles cover the chunk");
  static_assert(kMaxRows * D * 4 <= kTiles * TS, "a wave's fp32 partial fits its V region");
  static_assert(RS % 32 == 16 && TS % 256 == 128, "rows of a tile pair start at sixteen different 16-byte slots");
  __shared__ __align__(16) uint8_t vt[kT / 64][kTiles * TS];  // per wave: V rows (e4m3), then its fp32 partial
  __shared__ float wred[2][kT / 64][kMaxRows];                // per-wave max, per-wave sum

  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const int c0 = chunk * kChunk;
  if (c0 >= n) return;  // whole block: nothing of this chunk is valid for any row (n <= 0 included)
  const int nloc = (n - c0) < kChunk ? (n - c0) : kChunk;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int Hq = Hkv * G, R = S * G;
  const long row0 = (long)b * max_len + c0;  // first cache row of the chunk
  const long rstride = (long)Hkv * D;        // bytes
  const float* ksc = ks + ((long)b * Hkv + kvh) * sstride + c0;
  const float* vsc = vs + ((long)b * Hkv + kvh) * sstride + c0;
  const int w0 = w * kWaveKeys;              // the wave's first key of the chunk
  const bool live = w0 < nloc;               // the same for the whole wave
  // this lane's query row: sequence position sq, head kvh G + gq; it sees the chunk's keys below lim
  const int sq = r / G, gq = r - sq * G;
  const int lim = r < R ? n - (S - 1 - sq) - c0 : 0;
  const long qrow = ((long)b * S + sq) * Hq + kvh * G + gq;  // also the row of the partials

  // ---- scores: 16-key tiles through the MFMA
  f32x4 sc[kTiles];
  {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 qb[NM];  // B fragments: row r, elements (D / 4) g + 8 j .. + 7
#pragma unroll
    for (int j = 0; j < NM; ++j)
      qb[j] = r < R ? *reinterpret_cast<const u32x4*>(q + qrow * D + (D / 4) * g + 8 * j) : zero;
    const uint8_t* kbase = kc + (row0 * Hkv + kvh) * D + (D / 4) * g;
    u32x4 a[kTiles][NL];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = w0 + 16 * t;
      if (k0 < nloc) {  // the same for the whole wave
        const int j = k0 + r;
        const uint8_t* p = kbase + (j < nloc ? j : nloc - 1) * rstride;
#pragma unroll
        for (int l = 0; l < NL; ++l) a[t][l] = *reinterpret_cast<const u32x4*>(p + 16 * l);
      }
    }
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = w0 + 16 * t, key = k0 + 4 * g;  // this lane's accumulator keys: key .. key + 3
      sc[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (k0 < nloc) {
        f32x4 acc = pto::zero4();
#pragma unroll
        for (int j = 0; j < NM; ++j)
          acc = mfma(widen(a[t][j >> 1][2 * (j & 1)], a[t][j >> 1][2 * (j & 1) + 1]), qb[j], acc);
        float sk[4];
        scales4(ksc, key, nloc, sk);
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[t][i] = key + i < lim ? acc[i] * sk[i] * scale : -INFINITY;
      }
    }
  }

  // ---- V of the wave's 64 keys: 16-byte loads in flight during the softmax
  u32x4 vr[NV];
  if (live) {
    const uint8_t* vbase = vc + (row0 * Hkv + kvh) * D + (lane % CPR) * 16;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = w0 + i * RPI + lane / CPR;
      vr[i] = *reinterpret_cast<const u32x4*>(vbase + (j < nloc ? j : nloc - 1) * rstride);
    }
  }

  // ---- max, exp, sum per row: lane, lane groups (xor 16, 32), waves (LDS, in order)
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, sc[t][i]);
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (g == 0) wred[0][w][r] = m;
  __syncthreads();
  m = wred[0][0][r];
#pragma unroll
  for (int k = 1; k < kT / 64; ++k) m = fmaxf(m, wred[0][k][r]);
  const float mref = m == -INFINITY ? 0.f : m;  // a row without a key in this chunk: every p is 0 by selection
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
    if (w0 + 16 * t < nloc) scales4(vsc, w0 + 16 * t + 4 * g, nloc, sv);  // the same for the whole wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = sc[t][i] == -INFINITY ? 0.f : __expf(sc[t][i] - mref);
      sc[t][i] = p * sv[i];  // p': exact, a power of two
      l += p;
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (g == 0) wred[1][w][r] = l;

  // ---- P . V as O^T = V^T . P^T
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = pto::zero4();
  uint8_t* mine = vt[w];
  if (live) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int jl = i * RPI + lane / CPR;  // the row among the wave's 64
      *reinterpret_cast<u32x4*>(mine + (jl >> 4) * TS + (jl & 15) * RS + (lane % CPR) * 16) = vr[i];
    }
    // the wave reads what its own lanes wrote: LDS operations of one wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // source address of the transposed reads: of the group's eight rows this lane names row r >> 1, that is key
    // 4 g + ((r >> 1) & 3) of tile t + (r >> 3), bytes 8 (r & 1) .. + 7 of a 16-wide d tile
    const uint8_t* src = mine + (r >> 3) * TS + (4 * g + ((r >> 1) & 3)) * RS + 8 * (r & 1);
#pragma unroll
    for (int t = 0; t < kTiles; t += 2) {
      if (w0 + 16 * t < nloc) {  // the same for the whole wave; a pair wholly past the count has p = 0 throughout
        const HiLo s0 = split2(sc[t][0], sc[t][1]), s1 = split2(sc[t][2], sc[t][3]);
        const HiLo s2 = split2(sc[t + 1][0], sc[t + 1][1]), s3 = split2(sc[t + 1][2], sc[t + 1][3]);
        const u32x4 hi = {s0.hi, s1.hi, s2.hi, s3.hi}, lo = {s0.lo, s1.lo, s2.lo, s3.lo};
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const i32x2 v = tr_read8(src + t * TS + 16 * dt);
          const u32x4 vf = widen((uint32_t)v[0], (uint32_t)v[1]);
          o[dt] = mfma(vf, hi, o[dt]);
          o[dt] = mfma(vf, lo, o[dt]);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // the wave's partial [row r][d] over its own V region: lane (r, g) holds d = 16 dt + 4 g .. + 3
  float* part = reinterpret_cast<float*>(mine);
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<f32x4*>(part + r * D + 16 * dt + 4 * g) = o[dt];
  __syncthreads();

  // ---- the four waves in order, out to the partials of (b, s, head)
  for (int e = tid; e < R * D; e += kT) {
    const int rr = e / D, d = e - rr * D;
    float t = reinterpret_cast<const float*>(vt[0])[e];
#pragma unroll
    for (int k = 1; k < kT / 64; ++k) t += reinterpret_cast<const float*>(vt[k])[e];
    const int s2 = rr / G;
    const long prow = ((long)b * S + s2) * Hq + kvh * G + (rr - s2 * G);
    po[(prow * nchunks + chunk) * D + d] = t;
  }
  if (tid < R) {  // wave 0, g == 0: r == tid, and m is the row's maximum over the chunk
    float t = wred[1][0][tid];
#pragma unroll
    for (int k = 1; k < kT / 64; ++k) t += wred[1][k][tid];
    pm[qrow * nchunks + chunk] = m;
    pl[qrow * nchunks + chunk] = t;
  }
}

template <int D>
int launch_multi_fp8(const void* q, const void* kc, const void* vc, const float* ks, const float* vs, int sstride,
                     const int* lens, float* po, float* pm, float* pl, void* o, int B, int S, int max_len,
                     int max_keys, int Hq, int Hkv, int nchunks, hipStream_t st) {
  hipLaunchKernelGGL((decode_attn_multi_fp8_kernel<D>), dim3((unsigned)nchunks, (unsigned)Hkv, (unsigned)B), dim3(kT),
                     0, st, (const uint16_t*)q, (const uint8_t*)kc, (const uint8_t*)vc, ks, vs, lens, po, pm, pl,
                     max_len, sstride, max_keys, Hkv, Hq / Hkv, S, nchunks, 1.f / sqrtf((float)D));
  hipLaunchKernelGGL((decode_combine_multi_kernel<D>), dim3((unsigned)(S * Hq), (unsigned)B), dim3(D), 0, st, po, pm,
                     pl, lens, (uint16_t*)o, max_keys, Hq, S, nchunks);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// pto_rope_append_multi on an e4m3 cache: qkv [B, S, (Hq + 2 Hkv) D], q bf16 (dtype must be 1); k_cache, v_cache
// [B, max_len, Hkv, D] e4m3; k_scale, v_scale fp32 [B, Hkv, sstride]; pos int32 [B] on the device: token s of
// sequence b goes to position pos[b] + s.  D in {64, 128}.
int pto_rope_append_multi_fp8(const void* qkv, void* q, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                              int sstride, const float* cosb, const float* sinb, const int* pos, long B, int S,
                              int max_len, int table_rows, int Hq, int Hkv, int D, int dtype, void* stream) {
  if (B <= 0 || S <= 0 || max_len <= 0 || table_rows <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 128) ||
      dtype != 1 || (long)B * max_len > 0x7fffffffL || (long)B * S > 0x7fffffffL)
    return -1;
  if (!aligned16(qkv) || !aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(cosb) ||
      !aligned16(sinb) || ((uintptr_t)pos & 3u) || !scales_ok(k_scale, v_scale, sstride, max_len))
    return -2;
  const long groups = B * S * ((Hq + 2 * Hkv) * D / 8);
  hipLaunchKernelGGL(rope_append_multi_fp8_kernel, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                     (const uint16_t*)qkv, (uint16_t*)q, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, cosb,
                     sinb, pos, B, S, max_len, sstride, table_rows, Hq, Hkv, D);
  return (int)hipGetLastError();
}

// q, o [B, S, Hq, D] bf16; k_cache, v_cache [B, max_len, Hkv, D] e4m3; k_scale, v_scale fp32 [B, Hkv, sstride];
// lens int32 [B] on the device (valid rows after the append); po, pm, pl and nchunks as pto_decode_attn_multi's.
// 1 <= S and S * Hq / Hkv <= 16.
int pto_decode_attn_multi_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale,
                              const float* v_scale, int sstride, const int* lens, void* o, float* po, float* pm,
                              float* pl, int B, int S, int max_len, int max_keys, int Hq, int Hkv, int D, int nchunks,
                              void* stream) {
  if (B <= 0 || B > 65535 || S <= 0 || max_len <= 0 || max_keys <= 0 || max_keys > max_len || Hq <= 0 || Hkv <= 0 ||
      Hkv > 65535 || Hq % Hkv || (long)S * (Hq / Hkv) > kMaxRows || (D != 64 && D != 128) ||
      nchunks != (max_keys + kChunk - 1) / kChunk || (long)B * max_len > 0x7fffffffL || (long)B * S > 0x7fffffffL)
    return -1;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(o) || !aligned16(po) ||
      ((uintptr_t)pm & 3u) || ((uintptr_t)pl & 3u) || ((uintptr_t)lens & 3u) ||
      !scales_ok(k_scale, v_scale, sstride, max_len))
    return -2;
  if (D == 128)
    return launch_multi_fp8<128>(q, k_cache, v_cache, k_scale, v_scale, sstride, lens, po, pm, pl, o, B, S, max_len,
                                 max_keys, Hq, Hkv, nchunks, (hipStream_t)stream);
  return launch_multi_fp8<64>(q, k_cache, v_cache, k_scale, v_scale, sstride, lens, po, pm, pl, o, B, S, max_len,
                              max_keys, Hq, Hkv, nchunks, (hipStream_t)stream);
}

}  // extern "C"
