// Decode step of the Llama worker: append one token's k / v to a KV cache and run single-query
// attention over the cache.
//
//   rope_append: the decode step's packed projection qkv [B, (Hq + 2 Hkv) * D] (one token per batch
//            row) -> q [B, Hq, D] rotated at position pos[b], the rotated k and the copied v stored
//            at row pos[b] of one layer's cache k_cache / v_cache [B, max_len, Hkv, D].  One launch,
//            one pass; the rotation is rope_qkv_kernel's (llm_fused.hip), expression for
//            expression, so a row is bit-identical to that kernel's at the same position.  pos is
//            read on the device: a row with pos outside [0, max_len) stores nothing to the cache
//            (its q is still written, rotated at the nearest table row).
//   decode_attn: o [B, Hq, D] = softmax(q . K[:n]^T / sqrt(D)) . V[:n], n = min(lens[b], max_keys),
//            bf16 in and out, fp32 inside.  The key axis is cut into chunks of kChunk keys; one
//            workgroup serves the G = Hq / Hkv query heads of one (batch row, kv head, chunk), so
//            every K and V row is read once.  The grid depends on max_keys alone (lens stays on the
//            device); a workgroup whose chunk starts at or past n leaves without a load or a store.
//            Inside a workgroup D / 8 lanes share one key (16 bytes of the row per lane, straight
//            into registers): the G dot products are VALU FMAs over the lane's 8 elements and a
//            cross-lane sum over the D / 8 lanes.  The scores of the chunk go to LDS, the block
//            takes the max and the sum per head, and the same lane layout accumulates p . V.  Rows
//            at or past n are never loaded, and their score is -inf by selection.
//            Each chunk writes fp32 partials (unnormalised o, max, sum); decode_combine merges the
//            ceil(n / kChunk) partials of a row in chunk order -- it reads lens itself, so partials
//            that an earlier call left in the workspace beyond that count are never read.  No
//            atomics anywhere: the same inputs and max_keys give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pto_vec.h"

namespace {

constexpr int kT = 256;
constexpr int kChunk = 256;  // keys per workgroup
constexpr int kU = 4;        // cache rows a lane has in flight (16-byte loads issued before the first use)

using V8 = pto::Vec<8>;
using pto::vload;
using pto::vstore;

// ---------------------------------------------------------------------------- rope_append
// One thread per 8-element group of the packed row; heads [0, Hq) -> q, [Hq, Hq+Hkv) -> k cache,
// the rest -> v cache.
template <typename T>
__global__ __launch_bounds__(kT) void rope_append_kernel(const T* __restrict__ pk, T* __restrict__ q,
                                                         T* __restrict__ kc, T* __restrict__ vc,
                                                         const float* __restrict__ cosb,
                                                         const float* __restrict__ sinb,
                                                         const int* __restrict__ pos, long B, int max_len,
                                                         int table_rows, int Hq, int Hkv, int D) {
  const int W = (Hq + 2 * Hkv) * D, gpr = W / 8;
  const long groups = B * gpr;
  for (long gi = (long)blockIdx.x * kT + threadIdx.x; gi < groups; gi += (long)gridDim.x * kT) {
    const long tok = gi / gpr;
    const int c = (int)(gi - tok * gpr) * 8;
    const int hh = c / D, d0 = c - hh * D;
    const int p = pos[tok];
    const bool in_cache = p >= 0 && p < max_len;
    T* other;
    bool rot = true;
    if (hh < Hq) {
      other = q + (tok * Hq + hh) * D + d0;
    } else {
      if (!in_cache) continue;  // the cache has no such row
      const long row = tok * max_len + p;
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
      const int s = p < 0 ? 0 : (p >= table_rows ? table_rows - 1 : p);
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

// ---------------------------------------------------------------------------- decode_attn
// grid (chunks, Hkv, B), kT threads.  Lane layout: LPK = D / 8 lanes per key, KPW = 64 / LPK keys
// per wave and pass, KPB = 4 * KPW keys per workgroup and pass.
template <int D, int G>
__global__ __launch_bounds__(kT) void decode_attn_kernel(const uint16_t* __restrict__ q,
                                                         const uint16_t* __restrict__ kc,
                                                         const uint16_t* __restrict__ vc,
                                                         const int* __restrict__ lens, float* __restrict__ po,
                                                         float* __restrict__ pm, float* __restrict__ pl,
                                                         int max_len, int max_keys, int Hkv, int nchunks,
                                                         float scale) {
  constexpr int LPK = D / 8, KPW = 64 / LPK, KPB = (kT / 64) * KPW, NIT = kChunk / KPB;
  static_assert(NIT % kU == 0, "the passes over the chunk come in groups of kU");
  __shared__ float sc[G][kChunk];        // scores, then probabilities, of the chunk
  __shared__ float red[kT / 64][G][D];   // per-wave partial p.V
  __shared__ float wred[kT / 64][G];     // per-wave max / sum
  __shared__ float stat[2][G];           // block max, block sum

  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const int c0 = chunk * kChunk;
  if (c0 >= n) return;  // whole block: nothing of this chunk is valid (n <= 0 included)
  const int nloc = (n - c0) < kChunk ? (n - c0) : kChunk;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, sub = lane / LPK, dl = lane % LPK, d0 = dl * 8;
  const int Hq = Hkv * G;
  const long row0 = (long)b * max_len + c0;  // first cache row of the chunk
  const long rstride = (long)Hkv * D;
  const uint16_t* kbase = kc + (row0 * Hkv + kvh) * D + d0;
  const uint16_t* vbase = vc + (row0 * Hkv + kvh) * D + d0;

  // ---- scores
  {
    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) vload(q + ((long)b * Hq + kvh * G + g) * D + d0, qf[g]);
    // kU rows in flight per lane.  A slot at or past nloc re-reads the chunk's last valid row (never a
    // row past n) and its score is replaced by -inf below.
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += kU) {
      float kf[kU][8];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int j = (it0 + u) * KPB + w * KPW + sub;
        vload(kbase + (j < nloc ? j : nloc - 1) * rstride, kf[u]);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int j = (it0 + u) * KPB + w * KPW + sub;
        float s[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float a = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) a = fmaf(qf[g][i], kf[u][i], a);
          s[g] = a;
        }
        // the LPK lanes of a key are consecutive lanes: xor offsets below LPK stay inside the group
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
          for (int o = LPK / 2; o >= 1; o >>= 1) s[g] += __shfl_xor(s[g], o, 64);
        }
        if (dl == 0) {
#pragma unroll
          for (int g = 0; g < G; ++g) sc[g][j] = j < nloc ? s[g] * scale : -INFINITY;
        }
      }
    }
  }
  __syncthreads();

  // ---- max, exp, sum over the chunk: thread t owns key t of every head
  float sv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    sv[g] = sc[g][tid];
    const float m = pto::wave_max(sv[g]);
    if (lane == 0) wred[w][g] = m;
  }
  __syncthreads();
  if (tid < G) {
    float m = wred[0][tid];
#pragma unroll
    for (int k = 1; k < kT / 64; ++k) m = fmaxf(m, wred[k][tid]);
    stat[0][tid] = m;  // finite: key c0 is valid
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float p = tid < nloc ? __expf(sv[g] - stat[0][g]) : 0.f;
    sc[g][tid] = p;
    const float t = pto::wave_sum(p);
    if (lane == 0) wred[w][g] = t;
  }
  __syncthreads();
  if (tid < G) {
    float t = wred[0][tid];
#pragma unroll
    for (int k = 1; k < kT / 64; ++k) t += wred[k][tid];
    stat[1][tid] = t;
  }

  // ---- p . V
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
  }
  // as above: a slot at or past nloc re-reads the last valid row, and its p is the exact 0 stored above
#pragma unroll
  for (int it0 = 0; it0 < NIT; it0 += kU) {
    float vf[kU][8];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = (it0 + u) * KPB + w * KPW + sub;
      vload(vbase + (j < nloc ? j : nloc - 1) * rstride, vf[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = (it0 + u) * KPB + w * KPW + sub;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = sc[g][j];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = fmaf(p, vf[u][i], acc[g][i]);
      }
    }
  }
  // the KPW key slots of a wave hold the same d-slice LPK lanes apart
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int o = 32; o >= LPK; o >>= 1) acc[g][i] += __shfl_xor(acc[g][i], o, 64);
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[w][g][d0 + i] = acc[g][i];
    }
  }
  __syncthreads();
  const long pbase = ((long)b * Hq + kvh * G) * nchunks;  // + g * nchunks + chunk
  for (int e = tid; e < G * D; e += kT) {
    const int g = e / D, d = e - g * D;
    float t = red[0][g][d];
#pragma unroll
    for (int k = 1; k < kT / 64; ++k) t += red[k][g][d];
    po[(pbase + (long)g * nchunks + chunk) * D + d] = t;
  }
  if (tid < G) {
    pm[pbase + (long)tid * nchunks + chunk] = stat[0][tid];
    pl[pbase + (long)tid * nchunks + chunk] = stat[1][tid];
  }
}

// One workgroup of D threads per (batch row, query head): merge the row's valid partials in order.
template <int D>
__global__ __launch_bounds__(D) void decode_combine_kernel(const float* __restrict__ po,
                                                           const float* __restrict__ pm,
                                                           const float* __restrict__ pl,
                                                           const int* __restrict__ lens, uint16_t* __restrict__ o,
                                                           int max_keys, int Hq, int nchunks) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const long r = (long)b * Hq + h;
  float out = 0.f;
  if (n > 0) {
    const int nc = (n + kChunk - 1) / kChunk;  // <= nchunks, as n <= max_keys
    const float* m = pm + r * nchunks;
    const float* l = pl + r * nchunks;
    float M = m[0];
    for (int c = 1; c < nc; ++c) M = fmaxf(M, m[c]);
    float num = 0.f, den = 0.f;
    for (int c = 0; c < nc; ++c) {
      const float f = __expf(m[c] - M);
      num = fmaf(f, po[(r * nchunks + c) * D + d], num);
      den = fmaf(f, l[c], den);
    }
    out = num / den;
  }
  pto::store1(o + r * D + d, out);
}

unsigned grid_for(long work) {
  const long b = (work + kT - 1) / kT;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int D, int G>
void launch_decode(const void* q, const void* kc, const void* vc, const int* lens, float* po, float* pm, float* pl,
                   void* o, int B, int max_len, int max_keys, int Hkv, int nchunks, hipStream_t st) {
  hipLaunchKernelGGL((decode_attn_kernel<D, G>), dim3((unsigned)nchunks, (unsigned)Hkv, (unsigned)B), dim3(kT), 0,
                     st, (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc, lens, po, pm, pl, max_len,
                     max_keys, Hkv, nchunks, 1.f / sqrtf((float)D));
  hipLaunchKernelGGL((decode_combine_kernel<D>), dim3((unsigned)(Hkv * G), (unsigned)B), dim3(D), 0, st, po, pm, pl,
                     lens, (uint16_t*)o, max_keys, Hkv * G, nchunks);
}

template <int D>
int launch_decode_g(int G, const void* q, const void* kc, const void* vc, const int* lens, float* po, float* pm,
                    float* pl, void* o, int B, int max_len, int max_keys, int Hkv, int nchunks, hipStream_t st) {
  switch (G) {
    case 1: launch_decode<D, 1>(q, kc, vc, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks, st); break;
    case 2: launch_decode<D, 2>(q, kc, vc, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks, st); break;
    case 4: launch_decode<D, 4>(q, kc, vc, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks, st); break;
    case 8: launch_decode<D, 8>(q, kc, vc, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks, st); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Keys per workgroup: the wrapper sizes the partial workspace by ceil(max_keys / chunk).
long pto_decode_chunk() { return kChunk; }

// dtype: 0 = fp32, 1 = bf16 (qkv, q and the caches share it).  pos: int32 [B] on the device.
int pto_rope_append(const void* qkv, void* q, void* k_cache, void* v_cache, const float* cosb, const float* sinb,
                    const int* pos, long B, int max_len, int table_rows, int Hq, int Hkv, int D, int dtype,
                    void* stream) {
  if (B <= 0 || max_len <= 0 || table_rows <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0 || D % 8 || dtype < 0 ||
      dtype > 1 || (long)B * max_len > 0x7fffffffL)
    return -1;
  if (!aligned16(qkv) || !aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(cosb) ||
      !aligned16(sinb) || ((uintptr_t)pos & 3u))
    return -2;
  const long groups = B * ((Hq + 2 * Hkv) * D / 8);
  if (dtype == 0)
    hipLaunchKernelGGL(rope_append_kernel<float>, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                       (const float*)qkv, (float*)q, (float*)k_cache, (float*)v_cache, cosb, sinb, pos, B, max_len,
                       table_rows, Hq, Hkv, D);
  else
    hipLaunchKernelGGL(rope_append_kernel<uint16_t>, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                       (const uint16_t*)qkv, (uint16_t*)q, (uint16_t*)k_cache, (uint16_t*)v_cache, cosb, sinb, pos,
                       B, max_len, table_rows, Hq, Hkv, D);
  return (int)hipGetLastError();
}

// q, o [B, Hq, D] bf16; k_cache, v_cache [B, max_len, Hkv, D] bf16; lens int32 [B] on the device;
// po [B, Hq, nchunks, D], pm, pl [B, Hq, nchunks] fp32 workspace, nchunks = ceil(max_keys / chunk).
int pto_decode_attn(const void* q, const void* k_cache, const void* v_cache, const int* lens, void* o, float* po,
                    float* pm, float* pl, int B, int max_len, int max_keys, int Hq, int Hkv, int D, int nchunks,
                    void* stream) {
  if (B <= 0 || B > 65535 || max_len <= 0 || max_keys <= 0 || max_keys > max_len || Hq <= 0 || Hkv <= 0 ||
      Hkv > 65535 || Hq % Hkv || (D != 64 && D != 128) || nchunks != (max_keys + kChunk - 1) / kChunk)
    return -1;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(o) || !aligned16(po) ||
      ((uintptr_t)pm & 3u) || ((uintptr_t)pl & 3u) || ((uintptr_t)lens & 3u))
    return -2;
  const int G = Hq / Hkv;
  if (D == 128)
    return launch_decode_g<128>(G, q, k_cache, v_cache, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks,
                                (hipStream_t)stream);
  return launch_decode_g<64>(G, q, k_cache, v_cache, lens, po, pm, pl, o, B, max_len, max_keys, Hkv, nchunks,
                             (hipStream_t)stream);
}

}  // extern "C"
