// A decode step over S tokens per sequence (the verification step of speculative decoding, or a few
// tokens appended to an existing cache): append S rows to the bf16 KV cache and attend S queries per
// sequence over it, each with its own causal length.
//
//   rope_append_multi  qkv [B, S, (Hq + 2 Hkv) D] -> q [B, S, Hq, D] rotated at pos[b] + s, the rotated k and
//             the copied v stored at cache row pos[b] + s.  decode_attention.hip's rope_append_kernel with the
//             token index split into (b, s): the rotation is the same text, so a row equals rope_append's at
//             the same position bit for bit.  A row outside [0, max_len) stores nothing, token by token.
//   decode_attn_multi  q, o [B, S, Hq, D]; query s of sequence b sees the keys j < n_s,
//             n_s = min(lens[b], max_keys) - (S - 1 - s); n_s <= 0 gives a zero row.  R = S G <= 16 query
//             rows per kv head (row r = s G + g) fill the 16 columns of v_mfma_f32_16x16x32_bf16.
//     grid    (chunks of kChunk keys, Hkv, B), 256 threads, as decode_attention.hip: K and V of a chunk
//             are read once for all R rows; a workgroup whose chunk starts at or past
//             n = min(lens[b], max_keys) leaves before its first load.  Wave w owns keys 64 w .. 64 w + 63.
//     scores  S^T = K . q^T: a 16-key tile of K is the A operand straight from HBM (16-byte loads into
//             registers, no LDS), q the B operand (column r; columns at or past R are zeros that are never
//             loaded).  The k index is permuted alike on both sides, as decode_attention_fp8.hip does: lane
//             group g = lane >> 4 takes elements (D / 4) g .. + D / 4 - 1 of its key's row, MFMA j eats
//             (D / 4) g + 8 j .. + 7.  All K loads of the wave's four tiles are issued before the first MFMA.
//             Accumulator lane (r = lane & 15, g) holds keys 4 g .. 4 g + 3 of each tile for row r.
//     masks   by selection: a key slot at or past the chunk's valid count re-reads the last valid row; a
//             score whose key is at or past its row's n_s is -inf and its p an exact 0; a tile wholly past
//             the count is skipped by the whole wave.  Rows at or past n are never read.
//     softmax per chunk and row in fp32 on the accumulators: 16 values per lane, xor 16 and 32 across the
//             lane groups, then the four waves through LDS in wave order.
//     P . V   O^T = V^T . P^T on the same MFMA.  The accumulators of tiles t and t + 1 are a B fragment as
//             they stand (k = 8 g + e <-> key 4 g + (e & 3) of tile t + (e >> 2)); P is split
//             hi = bf16(p), lo = bf16(p - hi) and fed as two MFMAs on one V fragment: P's relative error
//             is 2^-16.  V^T is the A operand: the wave's 64 V rows go to its own LDS region (rows
//             padded by 32 bytes: the four rows of a transposed read fall on disjoint banks) and
//             ds_read_b64_tr_b16 returns, per 16-lane group, column lane & 15 of four rows.  The V loads are
//             issued before the softmax.  l is the sum of the fp32 p.
//     reduce  each wave writes its 16 x D fp32 partial over its own V region; after a barrier the workgroup
//             adds the four in wave order.  No atomics.
//     partials po [B, S Hq, nchunks, D], pm, pl [B, S Hq, nchunks]: decode_common.h's layout with S Hq
//             heads.  A row whose n_s ends before this chunk gets (0, -inf, 0); decode_combine_multi counts
//             a row's chunks from the row's own n_s, so it reads neither those nor anything stale.
#include "decode_multi.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
constexpr int kPad = 16;     // bf16 elements (32 bytes) between the V rows of the LDS image

using V8 = pto::Vec<8>;
using pto::vload;
using pto::vstore;

// ---------------------------------------------------------------------------- rope_append_multi
// One thread per 8-element group of a token's packed row; heads [0, Hq) -> q, [Hq, Hq+Hkv) -> k cache,
// the rest -> v cache.  Token (b, s) sits at position pos[b] + s.
template <typename T>
__global__ __launch_bounds__(kT) void rope_append_multi_kernel(const T* __restrict__ pk, T* __restrict__ q,
                                                               T* __restrict__ kc, T* __restrict__ vc,
                                                               const float* __restrict__ cosb,
                                                               const float* __restrict__ sinb,
                                                               const int* __restrict__ pos, long B, int S,
                                                               int max_len, int table_rows, int Hq, int Hkv, int D) {
  const int W = (Hq + 2 * Hkv) * D, gpr = W / 8;
  const long groups = B * S * gpr;
  for (long gi = (long)blockIdx.x * kT + threadIdx.x; gi < groups; gi += (long)gridDim.x * kT) {
    const long tok = gi / gpr;
    const int c = (int)(gi - tok * gpr) * 8;
    const int hh = c / D, d0 = c - hh * D;
    const long b = tok / S;
    const long pl = (long)pos[b] + (tok - b * S);  // 64-bit: pos near INT_MAX must not wrap into the cache
    const bool in_cache = pl >= 0 && pl < max_len;
    T* other;
    bool rot = true;
    if (hh < Hq) {
      other = q + (tok * Hq + hh) * D + d0;
    } else {
      if (!in_cache) continue;  // the cache has no such row
      const long row = b * max_len + pl;
      if (hh < Hq + Hkv) {
        other = kc + (row * Hkv + (hh - Hq)) * D + d0;
      } else {
        other = vc + (row * Hkv + (hh - Hq - Hkv)) * D + d0;
        rot = false;
      }
    }
    const V8 in = vload<8>(pk + tok * W + c);
    V8 out = in;
    if (rot) {
      const int s = pl < 0 ? 0 : (pl >= table_rows ? table_rows - 1 : (int)pl);
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
    vstore(other, out);
  }
}

// ---------------------------------------------------------------------------- decode_attn_multi
// decode_multi.h has the MFMA and its lane map, split2 and decode_combine_multi_kernel.
// ds_read_b64_tr_b16: each lane of a 16-lane group names 8 bytes (row q = l16 >> 2, columns 4 (l16 & 3) .. + 3
// of a 4 x 16 block) and receives column l16 of the block's four rows.
__device__ __forceinline__ s16x4 tr_read(const uint16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

template <int D>
__global__ __launch_bounds__(kT) void decode_attn_multi_kernel(const uint16_t* __restrict__ q,
                                                               const uint16_t* __restrict__ kc,
                                                               const uint16_t* __restrict__ vc,
                                                               const int* __restrict__ lens, float* __restrict__ po,
                                                               float* __restrict__ pm, float* __restrict__ pl,
                                                               int max_len, int max_keys, int Hkv, int G, int S,
                                                               int nchunks, float scale) {
  constexpr int NM = D / 32;          // score MFMAs (and 16-byte K loads per lane) per key tile
  constexpr int ND = D / 16;          // 16-wide output tiles along d
  constexpr int RS = D + kPad;        // V row stride in LDS, elements
  constexpr int CPR = D / 8;          // 16-byte chunks per V row
  constexpr int NV = kWaveKeys * CPR / 64;  // 16-byte V loads per lane
  constexpr int RPI = 64 / CPR;       // V rows per wave load instruction
  static_assert(kTiles * 16 * (kT / 64) == kChunk, "the waves' key tiles cover the chunk");
  static_assert(kMaxRows * D * 4 <= kWaveKeys * RS * 2, "a wave's fp32 partial fits its V region");
  __shared__ __align__(16) uint16_t vt[kT / 64][kWaveKeys * RS];  // per wave: V rows, then its fp32 partial
  __shared__ float wred[2][kT / 64][kMaxRows];                    // per-wave max, per-wave sum

  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const int c0 = chunk * kChunk;
  if (c0 >= n) return;  // whole block: nothing of this chunk is valid for any row (n <= 0 included)
  const int nloc = (n - c0) < kChunk ? (n - c0) : kChunk;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int Hq = Hkv * G, R = S * G;
  const long row0 = (long)b * max_len + c0;  // first cache row of the chunk
  const long rstride = (long)Hkv * D;
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
    const uint16_t* kbase = kc + (row0 * Hkv + kvh) * D + (D / 4) * g;
    u32x4 a[kTiles][NM];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = w0 + 16 * t;
      if (k0 < nloc) {  // the same for the whole wave
        const int j = k0 + r;
        const uint16_t* p = kbase + (j < nloc ? j : nloc - 1) * rstride;
#pragma unroll
        for (int l = 0; l < NM; ++l) a[t][l] = *reinterpret_cast<const u32x4*>(p + 8 * l);
      }
    }
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = w0 + 16 * t, key = k0 + 4 * g;  // this lane's accumulator keys: key .. key + 3
      f32x4 acc = pto::zero4();
      if (k0 < nloc) {
#pragma unroll
        for (int j = 0; j < NM; ++j) acc = mfma(a[t][j], qb[j], acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[t][i] = (k0 < nloc && key + i < lim) ? acc[i] * scale : -INFINITY;
    }
  }

  // ---- V of the wave's 64 keys: 16-byte loads in flight during the softmax
  u32x4 vr[NV];
  if (live) {
    const uint16_t* vbase = vc + (row0 * Hkv + kvh) * D + (lane % CPR) * 8;
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = sc[t][i] == -INFINITY ? 0.f : __expf(sc[t][i] - mref);
      sc[t][i] = p;
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
  uint16_t* mine = vt[w];
  if (live) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      *reinterpret_cast<u32x4*>(mine + (i * RPI + lane / CPR) * RS + (lane % CPR) * 8) = vr[i];
    // the wave reads what its own lanes wrote: LDS operations of one wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // source address of the transposed reads: row 4 g + (r >> 2) of a tile, columns 4 (r & 3) .. + 3 of a d tile
    const uint16_t* src = mine + (4 * g + (r >> 2)) * RS + 4 * (r & 3);
#pragma unroll
    for (int t = 0; t < kTiles; t += 2) {
      if (w0 + 16 * t < nloc) {  // the same for the whole wave; a pair wholly past the count has p = 0 throughout
        const HiLo s0 = split2(sc[t][0], sc[t][1]), s1 = split2(sc[t][2], sc[t][3]);
        const HiLo s2 = split2(sc[t + 1][0], sc[t + 1][1]), s3 = split2(sc[t + 1][2], sc[t + 1][3]);
        const u32x4 hi = {s0.hi, s1.hi, s2.hi, s3.hi}, lo = {s0.lo, s1.lo, s2.lo, s3.lo};
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          s16x8 v;
          v.lo = tr_read(src + (16 * t) * RS + 16 * dt);
          v.hi = tr_read(src + (16 * t + 16) * RS + 16 * dt);
          const u32x4 vf = __builtin_bit_cast(u32x4, v);
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
int launch_multi(const void* q, const void* kc, const void* vc, const int* lens, float* po, float* pm, float* pl,
                 void* o, int B, int S, int max_len, int max_keys, int Hq, int Hkv, int nchunks, hipStream_t st) {
  hipLaunchKernelGGL((decode_attn_multi_kernel<D>), dim3((unsigned)nchunks, (unsigned)Hkv, (unsigned)B), dim3(kT), 0,
                     st, (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, po, pm, pl, max_len,
                     max_keys, Hkv, Hq / Hkv, S, nchunks, 1.f / sqrtf((float)D));
  hipLaunchKernelGGL((decode_combine_multi_kernel<D>), dim3((unsigned)(S * Hq), (unsigned)B), dim3(D), 0, st, po, pm,
                     pl, lens, (uint16_t*)o, max_keys, Hq, S, nchunks);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Query rows one kv head can carry: S * (Hq / Hkv) <= this.
long pto_decode_multi_rows() { return kMaxRows; }

// dtype: 0 = fp32, 1 = bf16 (qkv, q and the caches share it).  qkv [B, S, (Hq + 2 Hkv) D]; pos int32 [B] on the
// device: token s of sequence b goes to position pos[b] + s.
int pto_rope_append_multi(const void* qkv, void* q, void* k_cache, void* v_cache, const float* cosb,
                          const float* sinb, const int* pos, long B, int S, int max_len, int table_rows, int Hq,
                          int Hkv, int D, int dtype, void* stream) {
  if (B <= 0 || S <= 0 || max_len <= 0 || table_rows <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0 || D % 8 || dtype < 0 ||
      dtype > 1 || (long)B * max_len > 0x7fffffffL || (long)B * S > 0x7fffffffL)
    return -1;
  if (!aligned16(qkv) || !aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(cosb) ||
      !aligned16(sinb) || ((uintptr_t)pos & 3u))
    return -2;
  const long groups = B * S * ((Hq + 2 * Hkv) * D / 8);
  if (dtype == 0)
    hipLaunchKernelGGL(rope_append_multi_kernel<float>, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                       (const float*)qkv, (float*)q, (float*)k_cache, (float*)v_cache, cosb, sinb, pos, B, S, max_len,
                       table_rows, Hq, Hkv, D);
  else
    hipLaunchKernelGGL(rope_append_multi_kernel<uint16_t>, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                       (const uint16_t*)qkv, (uint16_t*)q, (uint16_t*)k_cache, (uint16_t*)v_cache, cosb, sinb, pos,
                       B, S, max_len, table_rows, Hq, Hkv, D);
  return (int)hipGetLastError();
}

// q, o [B, S, Hq, D] bf16; k_cache, v_cache [B, max_len, Hkv, D] bf16; lens int32 [B] on the device (valid rows
// after the append); po [B, S Hq, nchunks, D], pm, pl [B, S Hq, nchunks] fp32 workspace,
// nchunks = ceil(max_keys / chunk).  1 <= S and S * Hq / Hkv <= 16.
int pto_decode_attn_multi(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o,
                          float* po, float* pm, float* pl, int B, int S, int max_len, int max_keys, int Hq, int Hkv,
                          int D, int nchunks, void* stream) {
  if (B <= 0 || B > 65535 || S <= 0 || max_len <= 0 || max_keys <= 0 || max_keys > max_len || Hq <= 0 || Hkv <= 0 ||
      Hkv > 65535 || Hq % Hkv || (long)S * (Hq / Hkv) > kMaxRows || (D != 64 && D != 128) ||
      nchunks != (max_keys + kChunk - 1) / kChunk || (long)B * max_len > 0x7fffffffL)
    return -1;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(o) || !aligned16(po) ||
      ((uintptr_t)pm & 3u) || ((uintptr_t)pl & 3u) || ((uintptr_t)lens & 3u))
    return -2;
  if (D == 128)
    return launch_multi<128>(q, k_cache, v_cache, lens, po, pm, pl, o, B, S, max_len, max_keys, Hq, Hkv, nchunks,
                             (hipStream_t)stream);
  return launch_multi<64>(q, k_cache, v_cache, lens, po, pm, pl, o, B, S, max_len, max_keys, Hq, Hkv, nchunks,
                          (hipStream_t)stream);
}

}  // extern "C"
