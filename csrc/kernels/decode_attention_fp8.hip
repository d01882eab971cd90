// The decode step on an FP8 KV cache: OCP e4m3 keys and values with one fp32 power-of-two scale per
// (token, kv head), half the bytes of the bf16 cache that decode_attention.hip serves.
//
//   Format    k, v [B, max_len, Hkv, D] e4m3, the bf16 cache's layout; k_scale, v_scale fp32
//             [B, Hkv, sstride], sstride >= max_len and a multiple of 4 (the scales of a chunk are
//             contiguous and 16-byte aligned).  A row is ops.skinny.quantize_rows of the bf16 row the
//             bf16 cache would hold: scale = 2^ceil(log2(amax / 448)) (exponent at least -126; 1 for a
//             zero row), q = row / scale rounded to nearest even.  With amax = m 2^e, m in [1, 2), the
//             exponent is e - 8 for m <= 1.75 and e - 7 above: head_quantize reads it off amax's bits.
//             scale * q is exact in bf16, so the kernels below compute the bf16 attention on the
//             dequantised cache.
//   rope_append_fp8  decode_attention.hip's rope_append with the quantiser behind it: one thread per 8
//             elements of the packed row, q written as there (bit-identical), the rotated k / copied v
//             rounded to bf16 and quantised per head.  The D / 8 threads of a head are an aligned lane
//             group of one wave (a token's groups come in multiples of D / 8 and the grid stride is a
//             multiple of 256): amax by xor steps inside the group, v_cvt_pk_fp8_f32, 8 bytes stored per
//             thread and the scale by the group's first lane.  pos outside [0, max_len): no store to
//             the cache or the scales.
//   kv_quantize  the prefill's copy: rows [0, n) of k, v [B, S, Hkv, D] bf16 through the same head_quantize.
//   decode_attn_fp8  grid (chunks of kChunk keys, Hkv, B), 256 threads, fp32 partials as decode_common.h
//             lays them out; decode_combine_kernel merges them.  No atomics.
//     scores  on the matrix unit, v_mfma_f32_16x16x32_bf16 with a 16-key tile of K as the A operand
//             (HBM -> VGPR -> MFMA, no LDS) widened exactly by v_cvt_scalef32_pk_bf16_fp8 at scale 1.0,
//             and q as the B operand: column = query head lane & 15 (columns at or past G are zeros that
//             are never loaded), held in registers for the whole chunk.  The k index is permuted the
//             same way on both sides, as skinny_gemm_fp8.hip does: at D = 128 lane group g = lane >> 4
//             takes bytes 32 g .. + 31 of its key's row (two 16-byte loads, four MFMAs: MFMA j eats bytes
//             32 g + 8 j .. + 7 against q[32 g + 8 j .. + 7]); at D = 64 bytes 16 g .. + 15 (one load, two
//             MFMAs).  Wave w owns the key tiles 4 w .. 4 w + 3 and issues all their loads before the
//             first conversion.  The accumulator lane (head lane & 15, keys 4 (lane >> 4) + r of the
//             tile) multiplies by k_scale[key] (exact) and 1 / sqrt(D) and stores to LDS when its head
//             is below G: no cross-lane tree.
//     lengths a lane whose key is at or past the chunk's valid count re-reads the chunk's last valid row
//             and its score is -inf by selection; a tile wholly past the count is skipped by the whole
//             wave; rows and scales at or past n are never read.
//     softmax as decode_attention.hip: thread t owns key t; P stays fp32.  p * v_scale[key] is formed
//             there, once per key (exact), and is what P . V reads from LDS; the sum l is of p itself.
//     P . V   on the VALU (V's contraction runs across rows; an MFMA form would need a transpose and a
//             bf16 P).  D / E lanes share a key, E bytes of the row per lane, widened in registers with
//             v_cvt_pk_f32_fp8, G x E accumulators per lane.  E = 16 (16-byte loads) for G <= 4 and E = 8
//             for G = 8: in the compiler's resource report 16-byte loads at G = 8 take 256 registers (128
//             of them accumulators), one workgroup per CU; with E = 8 every instance has no scratch, at
//             most 140 registers and three workgroups per CU (profiles/decode_fp8/README.md has the table).
//             Two head passes at G = 8 were not built.
#include "decode_fp8.h"  // head_quantize, widen, scales_ok

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
using pto::f32x4;

constexpr int kU = 4;      // V rows a lane has in flight
constexpr int kTiles = 4;  // 16-key tiles per wave: kChunk / 16 / (kT / 64)

using V8 = pto::Vec<8>;
using pto::vload;
using pto::vstore;

// ---------------------------------------------------------------------------- rope_append_fp8
// One thread per 8-element group of the packed row; heads [0, Hq) -> q, [Hq, Hq+Hkv) -> k cache,
// the rest -> v cache.
__global__ __launch_bounds__(kT) void rope_append_fp8_kernel(const uint16_t* __restrict__ pk, uint16_t* __restrict__ q,
                                                             uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                             float* __restrict__ ks, float* __restrict__ vs,
                                                             const float* __restrict__ cosb,
                                                             const float* __restrict__ sinb,
                                                             const int* __restrict__ pos, long B, int max_len,
                                                             int sstride, int table_rows, int Hq, int Hkv, int D) {
  const int W = (Hq + 2 * Hkv) * D, gpr = W / 8, lpg = D / 8;
  const long groups = B * gpr;
  for (long gi = (long)blockIdx.x * kT + threadIdx.x; gi < groups; gi += (long)gridDim.x * kT) {
    const long tok = gi / gpr;
    const int c = (int)(gi - tok * gpr) * 8;
    const int hh = c / D, d0 = c - hh * D;
    const int p = pos[tok];
    const bool in_cache = p >= 0 && p < max_len;
    if (hh >= Hq && !in_cache) continue;  // the cache has no such row (the head's whole lane group leaves)
    const bool rot = hh < Hq + Hkv;
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
    if (hh < Hq) {
      vstore(q + (tok * Hq + hh) * D + d0, out);
      continue;
    }
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = pto::bf2f(pto::bf16_rne(out.v[i]));  // the row the bf16 cache would hold
    const bool isk = hh < Hq + Hkv;
    const int h = isk ? hh - Hq : hh - Hq - Hkv;
    const long row = tok * max_len + p;
    head_quantize(x, lpg, d0 == 0, (isk ? kc : vc) + (row * Hkv + h) * D + d0,
                  (isk ? ks : vs) + (tok * Hkv + h) * sstride + p);
  }
}

// ---------------------------------------------------------------------------- kv_quantize
// One thread per 8 elements of rows [0, n) of k and of v [B, S, Hkv, D].
__global__ __launch_bounds__(kT) void kv_quantize_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                         uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                         float* __restrict__ ks, float* __restrict__ vs, long B, int S,
                                                         int n, int max_len, int sstride, int Hkv, int D) {
  const int lpg = D / 8;
  const long per = B * n * Hkv * lpg;  // groups of k; as many of v
  for (long gi = (long)blockIdx.x * kT + threadIdx.x; gi < 2 * per; gi += (long)gridDim.x * kT) {
    const bool isk = gi < per;
    long r = isk ? gi : gi - per;
    const int d0 = (int)(r % lpg) * 8;
    r /= lpg;
    const int h = (int)(r % Hkv);
    r /= Hkv;
    const int s = (int)(r % n);
    const long b = r / n;
    float x[8];
    vload((isk ? k : v) + ((b * S + s) * Hkv + h) * D + d0, x);
    head_quantize(x, lpg, d0 == 0, (isk ? kc : vc) + ((b * max_len + s) * Hkv + h) * D + d0,
                  (isk ? ks : vs) + (b * Hkv + h) * sstride + s);
  }
}

// ---------------------------------------------------------------------------- decode_attn_fp8
// lane map (gfx950): A[i = lane & 15][k = 8 (lane >> 4) + e], B[k = 8 (lane >> 4) + e][j = lane & 15],
// D: j = lane & 15, i = 4 (lane >> 4) + reg.
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                 0, 0, 0);
}

// W dwords of e4m3 (4 bytes each, ascending) -> 4 W floats.
template <int W>
__device__ __forceinline__ void widen_f32(const uint32_t (&w)[W], float (&f)[4 * W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = a[0]; f[4 * i + 1] = a[1]; f[4 * i + 2] = b[0]; f[4 * i + 3] = b[1];
  }
}

// E: bytes (elements) of a V row per lane in P . V.
template <int D, int G, int E>
__global__ __launch_bounds__(kT) void decode_attn_fp8_kernel(const uint16_t* __restrict__ q,
                                                             const uint8_t* __restrict__ kc,
                                                             const uint8_t* __restrict__ vc,
                                                             const float* __restrict__ ks,
                                                             const float* __restrict__ vs,
                                                             const int* __restrict__ lens, float* __restrict__ po,
                                                             float* __restrict__ pm, float* __restrict__ pl,
                                                             int max_len, int sstride, int max_keys, int Hkv,
                                                             int nchunks, float scale) {
  constexpr int LPK = D / E, KPW = 64 / LPK, KPB = (kT / 64) * KPW, NIT = kChunk / KPB;
  constexpr int NM = D / 32;   // MFMAs per key tile
  constexpr int NL = D / 64;   // 16-byte K loads per lane and tile
  static_assert(NIT % kU == 0, "the passes over the chunk come in groups of kU");
  static_assert(kTiles * 16 * (kT / 64) == kChunk, "the waves' key tiles cover the chunk");
  __shared__ __align__(16) float sc[G][kChunk];  // scores, then p * v_scale, of the chunk (16-byte stores)
  __shared__ float red[kT / 64][G][D];   // per-wave partial p.V
  __shared__ float wred[kT / 64][G];     // per-wave max / sum
  __shared__ float stat[2][G];           // block max, block sum

  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  int n = lens[b];
  n = n < max_keys ? n : max_keys;
  const int c0 = chunk * kChunk;
  if (c0 >= n) return;  // whole block: nothing of this chunk is valid (n <= 0 included)
  const int nloc = (n - c0) < kChunk ? (n - c0) : kChunk;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int Hq = Hkv * G;
  const long row0 = (long)b * max_len + c0;  // first cache row of the chunk
  const long rstride = (long)Hkv * D;        // bytes
  const float* ksc = ks + ((long)b * Hkv + kvh) * sstride + c0;
  const float* vsc = vs + ((long)b * Hkv + kvh) * sstride + c0;

  // ---- scores: 16-key tiles through the MFMA
  {
    const int r = lane & 15, g = lane >> 4;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 qb[NM];  // B fragments: head r, k values (D / 4) g + 8 j .. + 7
#pragma unroll
    for (int j = 0; j < NM; ++j)
      qb[j] = r < G ? *reinterpret_cast<const u32x4*>(q + ((long)b * Hq + kvh * G + r) * D + (D / 4) * g + 8 * j) : zero;
    const uint8_t* kbase = kc + (row0 * Hkv + kvh) * D + (D / 4) * g;
    u32x4 a[kTiles][NL];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = (w * kTiles + t) * 16;
      if (k0 < nloc) {  // the same for the whole wave
        const int j = k0 + r;
        const uint8_t* p = kbase + (j < nloc ? j : nloc - 1) * rstride;
#pragma unroll
        for (int l = 0; l < NL; ++l) a[t][l] = *reinterpret_cast<const u32x4*>(p + 16 * l);
      }
    }
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      const int k0 = (w * kTiles + t) * 16, key = k0 + 4 * g;  // this lane's accumulator keys: key .. key + 3
      float s[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (k0 < nloc) {
        f32x4 acc = pto::zero4();
#pragma unroll
        for (int j = 0; j < NM; ++j)
          acc = mfma(widen(a[t][j >> 1][2 * (j & 1)], a[t][j >> 1][2 * (j & 1) + 1]), qb[j], acc);
        float sk[4];
        if (key + 3 < nloc) {
          const float4 v4 = *reinterpret_cast<const float4*>(ksc + key);
          sk[0] = v4.x; sk[1] = v4.y; sk[2] = v4.z; sk[3] = v4.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) sk[i] = key + i < nloc ? ksc[key + i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = key + i < nloc ? acc[i] * sk[i] * scale : -INFINITY;
      }
      if (r < G) *reinterpret_cast<float4*>(&sc[r][key]) = make_float4(s[0], s[1], s[2], s[3]);
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
  const float vscale = tid < nloc ? vsc[tid] : 0.f;
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
    sc[g][tid] = p * vscale;  // exact: a power of two
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

  // ---- p . V: LPK lanes share a key, E bytes of its row each
  const int sub = lane / LPK, dl = lane % LPK, d0 = dl * E;
  const uint8_t* vbase = vc + (row0 * Hkv + kvh) * D + d0;
  float acc[G][E];
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < E; ++i) acc[g][i] = 0.f;
  }
  // a slot at or past nloc re-reads the last valid row, and its p * v_scale is the exact 0 stored above
#pragma unroll
  for (int it0 = 0; it0 < NIT; it0 += kU) {
    uint32_t vw[kU][E / 4];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = (it0 + u) * KPB + w * KPW + sub;
      pto::load_words(vbase + (j < nloc ? j : nloc - 1) * rstride, vw[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = (it0 + u) * KPB + w * KPW + sub;
      float vf[E];
      widen_f32(vw[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = sc[g][j];
#pragma unroll
        for (int i = 0; i < E; ++i) acc[g][i] = fmaf(p, vf[i], acc[g][i]);
      }
    }
  }
  // the KPW key slots of a wave hold the same d-slice LPK lanes apart
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
#pragma unroll
      for (int o = 32; o >= LPK; o >>= 1) acc[g][i] += __shfl_xor(acc[g][i], o, 64);
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < E; ++i) red[w][g][d0 + i] = acc[g][i];
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

struct AttnArgs {
  const void *q, *kc, *vc;
  const float *ks, *vs;
  const int* lens;
  float *po, *pm, *pl;
  void* o;
  int B, max_len, sstride, max_keys, Hkv, nchunks;
  hipStream_t st;
};

template <int D, int G>
void launch_decode(const AttnArgs& a) {
  constexpr int E = G <= 4 ? 16 : 8;
  hipLaunchKernelGGL((decode_attn_fp8_kernel<D, G, E>), dim3((unsigned)a.nchunks, (unsigned)a.Hkv, (unsigned)a.B),
                     dim3(kT), 0, a.st, (const uint16_t*)a.q, (const uint8_t*)a.kc, (const uint8_t*)a.vc, a.ks, a.vs,
                     a.lens, a.po, a.pm, a.pl, a.max_len, a.sstride, a.max_keys, a.Hkv, a.nchunks,
                     1.f / sqrtf((float)D));
  hipLaunchKernelGGL((decode_combine_kernel<D>), dim3((unsigned)(a.Hkv * G), (unsigned)a.B), dim3(D), 0, a.st, a.po,
                     a.pm, a.pl, a.lens, (uint16_t*)a.o, a.max_keys, a.Hkv * G, a.nchunks);
}

template <int D>
int launch_decode_g(int G, const AttnArgs& a) {
  switch (G) {
    case 1: launch_decode<D, 1>(a); break;
    case 2: launch_decode<D, 2>(a); break;
    case 4: launch_decode<D, 4>(a); break;
    case 8: launch_decode<D, 8>(a); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// pto_rope_append on an e4m3 cache: qkv, q bf16 (dtype must be 1); k_cache, v_cache [B, max_len, Hkv, D]
// e4m3; k_scale, v_scale fp32 [B, Hkv, sstride].  D in {64, 128}.
int pto_rope_append_fp8(const void* qkv, void* q, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                        int sstride, const float* cosb, const float* sinb, const int* pos, long B, int max_len,
                        int table_rows, int Hq, int Hkv, int D, int dtype, void* stream) {
  if (B <= 0 || max_len <= 0 || table_rows <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 128) || dtype != 1 ||
      (long)B * max_len > 0x7fffffffL)
    return -1;
  if (!aligned16(qkv) || !aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(cosb) ||
      !aligned16(sinb) || ((uintptr_t)pos & 3u) || !scales_ok(k_scale, v_scale, sstride, max_len))
    return -2;
  const long groups = B * ((Hq + 2 * Hkv) * D / 8);
  hipLaunchKernelGGL(rope_append_fp8_kernel, dim3(grid_for(groups)), dim3(kT), 0, (hipStream_t)stream,
                     (const uint16_t*)qkv, (uint16_t*)q, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, cosb,
                     sinb, pos, B, max_len, sstride, table_rows, Hq, Hkv, D);
  return (int)hipGetLastError();
}

// k, v [B, S, Hkv, D] bf16 contiguous -> rows [0, min(S, max_len)) of the e4m3 cache layer and its scales.
int pto_kv_quantize(const void* k, const void* v, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                    int sstride, long B, int S, int max_len, int Hkv, int D, void* stream) {
  if (B <= 0 || S <= 0 || max_len <= 0 || Hkv <= 0 || (D != 64 && D != 128) || (long)B * max_len > 0x7fffffffL ||
      (long)B * S > 0x7fffffffL)
    return -1;
  if (!aligned16(k) || !aligned16(v) || !aligned16(k_cache) || !aligned16(v_cache) ||
      !scales_ok(k_scale, v_scale, sstride, max_len))
    return -2;
  const int n = S < max_len ? S : max_len;
  hipLaunchKernelGGL(kv_quantize_kernel, dim3(grid_for(2 * B * n * Hkv * (D / 8))), dim3(kT), 0, (hipStream_t)stream,
                     (const uint16_t*)k, (const uint16_t*)v, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, B,
                     S, n, max_len, sstride, Hkv, D);
  return (int)hipGetLastError();
}

// q, o [B, Hq, D] bf16; k_cache, v_cache [B, max_len, Hkv, D] e4m3; k_scale, v_scale fp32 [B, Hkv, sstride];
// lens int32 [B] on the device; po, pm, pl and nchunks as pto_decode_attn's.
int pto_decode_attn_fp8(const void* q, const void* k_cache, const void* v_cache, const float* k_scale,
                        const float* v_scale, int sstride, const int* lens, void* o, float* po, float* pm, float* pl,
                        int B, int max_len, int max_keys, int Hq, int Hkv, int D, int nchunks, void* stream) {
  if (B <= 0 || B > 65535 || max_len <= 0 || max_keys <= 0 || max_keys > max_len || Hq <= 0 || Hkv <= 0 ||
      Hkv > 65535 || Hq % Hkv || (D != 64 && D != 128) || nchunks != (max_keys + kChunk - 1) / kChunk)
    return -1;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(o) || !aligned16(po) ||
      ((uintptr_t)pm & 3u) || ((uintptr_t)pl & 3u) || ((uintptr_t)lens & 3u) ||
      !scales_ok(k_scale, v_scale, sstride, max_len))
    return -2;
  const AttnArgs a = {q, k_cache, v_cache, k_scale, v_scale, lens, po, pm, pl, o,
                      B, max_len, sstride, max_keys, Hkv, nchunks, (hipStream_t)stream};
  return D == 128 ? launch_decode_g<128>(Hq / Hkv, a) : launch_decode_g<64>(Hq / Hkv, a);
}

}  // extern "C"
