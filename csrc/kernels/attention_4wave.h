// The 4-wave flash-attention kernels -- plain and document-masked forward, dQ pass, dK/dV pass --
// written once in terms of D, NDS, NDT and CH (attention_common.h) and compiled per head dim: by
// attention.hip at D = 128 and by attention_d64.hip (which defines PTO_ATTN_D 64 first) at D = 64.
// attention.hip's header has the layout, the MFMA plan and the document mask.  A per-file macro
// rather than a template parameter: the D = 128 kernels keep their symbol names and compile to
// the instructions they had before the second head dim existed (profiles/attn_d64/README.md).
#pragma once
#include "attention_common.h"

// Kernel symbols: attn_<stem>_kernel at D = 128, attn_<stem>_d64_kernel at D = 64 (tools/isa_dump.py
// and the resource tests find kernels by symbol name; no D = 64 name contains a D = 128 one).
#define ATTN_KERNEL_CAT_(stem, d) attn_##stem##_d##d##_kernel
#define ATTN_KERNEL_CAT(stem, d) ATTN_KERNEL_CAT_(stem, d)
#if PTO_ATTN_D == 128
#define ATTN_KERNEL(stem) attn_##stem##_kernel
#else
#define ATTN_KERNEL(stem) ATTN_KERNEL_CAT(stem, PTO_ATTN_D)
#endif

namespace {

// ------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(NT, 2) void ATTN_KERNEL(fwd)(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                         const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                         float* __restrict__ lse2, int B, int S, int Hq, int Hkv,
                                                         float c, int causal) {
  __shared__ u32x4 smem[4 * BN * CH];  // K0 V0 K1 V1 (64 KB; 32 KB at D = 64)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  int qblk, b, hq, hk;
  block_coords(S, B, Hq, Hkv, causal, qblk, b, hq, hk);
  const int q0w = qblk * BM + w * 32;
  const size_t qstride = (size_t)Hq * D, kvstride = (size_t)Hkv * D;

  bf16x8 qf[NDS];
  {
    const bf16_t* qrow = q + ((size_t)b * S + q0w + r) * qstride + (size_t)hq * D + 8 * h;
#pragma unroll
    for (int s = 0; s < NDS; ++s) qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qrow + 16 * s));
  }
  const bf16_t* kb = k + (size_t)b * S * kvstride + (size_t)hk * D;
  const bf16_t* vb = v + (size_t)b * S * kvstride + (size_t)hk * D;
  const int ntiles = causal ? (qblk * BM + BM) / BN : S / BN;

  Stage<BN> ks, vs;
  ks.load(kb, kvstride, tid);
  vs.load(vb, kvstride, tid);
  ks.store(smem, tid);
  vs.store(smem + BN * CH, tid);
  __syncthreads();

  f32x16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = zero16();
  float m2 = -INFINITY, l = 0.f;
  const int qme = q0w + r;

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const u32x4* Ks = smem + cur * 2 * BN * CH;
    const u32x4* Vs = Ks + BN * CH;
    const int kv0 = t * BN;
    const bool more = t + 1 < ntiles;
    // No per-wave skip of tiles wholly above the diagonal (a wave's last tile at most): a
    // branch around the accumulators makes the compiler shuttle them through AGPRs.  Such a
    // tile gives p = 0 everywhere (never the first tile, so the running max stays finite).
    f32x16 sacc[2];
    {
      // S^T = K . Q^T: all 16 K row operands in flight, then two independent MFMA chains
      bf16x8 a0[NDS], a1[NDS];
#pragma unroll
      for (int s = 0; s < NDS; ++s) {
        a0[s] = row_frag(Ks, r, 2 * s + h);
        a1[s] = row_frag(Ks, 32 + r, 2 * s + h);
      }
      __builtin_amdgcn_sched_barrier(0);
      sacc[0] = zero16();
      sacc[1] = zero16();
#pragma unroll
      for (int s = 0; s < NDS; ++s) {
        sacc[0] = mfma(a0[s], qf[s], sacc[0]);
        sacc[1] = mfma(a1[s], qf[s], sacc[1]);
      }
    }
    if (more) {  // next tile's global loads fly under the softmax and P.V
      ks.load(kb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
      vs.load(vb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
    }
    {
      if (causal && kv0 + BN - 1 > q0w) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (kv0 + kt * 32 + acc_row(i, h) > qme) sacc[kt][i] = -INFINITY;
      }
      float mx = sacc[0][0];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kt][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(m2, mx * c);
      const float alpha = __builtin_amdgcn_exp2f(m2 - mnew);
      m2 = mnew;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kt][i], c, -mnew));
          sacc[kt][i] = p;
          rs += p;
        }
      l = fmaf(l, alpha, rs);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) oacc[dt] *= alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        bf16x8 pb[2], vv[2][NDT];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) vv[s2][dt] = tr_frag(Vs, kt * 32 + 16 * s2, dt * 32, lane);
        pb[0] = acc_frag(sacc[kt], 0);
        pb[1] = acc_frag(sacc[kt], 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) oacc[dt] = mfma(vv[s2][dt], pb[s2], oacc[dt]);
      }
    }
    if (more) {
      u32x4* nk = smem + (cur ^ 1) * 2 * BN * CH;
      ks.store(nk, tid);
      vs.store(nk + BN * CH, tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32);
  const float inv = 1.f / l;
  store_rows_T(oacc, inv, smem + w * 32 * CH, lane, o + ((size_t)b * S + q0w) * qstride + (size_t)hq * D, qstride);
  if (h == 0) lse2[((size_t)b * Hq + hq) * S + qme] = m2 + log2f(l);
}

// ------------------------------------------------------- forward, document mask
// attn_fwd_kernel with the bounds (see the top of the file for why it is not one body with it).
// Differences: the tile loop starts at t0, the `kv0 < lomax` mask, the `msub` guard, and K / V
// operands fetched one half / one k-step at a time.
__global__ __launch_bounds__(NT, 2) void ATTN_KERNEL(doc_fwd)(const bf16_t* __restrict__ q,
                                                             const bf16_t* __restrict__ k,
                                                             const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                             float* __restrict__ lse2,
                                                             const int* __restrict__ doc_start, int B, int S, int Hq,
                                                             int Hkv, float c) {
  __shared__ u32x4 smem[4 * BN * CH];  // K0 V0 K1 V1 (64 KB; 32 KB at D = 64)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  int qblk, b, hq, hk;
  block_coords(S, B, Hq, Hkv, 1, qblk, b, hq, hk);
  const int q0w = qblk * BM + w * 32;
  const size_t qstride = (size_t)Hq * D, kvstride = (size_t)Hkv * D;

  bf16x8 qf[NDS];
  {
    const bf16_t* qrow = q + ((size_t)b * S + q0w + r) * qstride + (size_t)hq * D + 8 * h;
#pragma unroll
    for (int s = 0; s < NDS; ++s) qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qrow + 16 * s));
  }
  const bf16_t* kb = k + (size_t)b * S * kvstride + (size_t)hk * D;
  const bf16_t* vb = v + (size_t)b * S * kvstride + (size_t)hk * D;
  const int qme = q0w + r;
  const int* ds = doc_start + (size_t)b * S;
  const int lome = ds[qme];                  // first visible key of this lane's query
  const int lomax = uniform(ds[q0w + 31]);   // the wave's largest bound (its last row's)
  // first tile any row of the block sees, clamped into the block's causal range
  const int t0 = min(max(uniform(ds[qblk * BM]), 0), qblk * BM) / BN;
  const int ntiles = (qblk * BM + BM) / BN;

  Stage<BN> ks, vs;
  ks.load(kb + (size_t)t0 * BN * kvstride, kvstride, tid);
  vs.load(vb + (size_t)t0 * BN * kvstride, kvstride, tid);
  ks.store(smem, tid);
  vs.store(smem + BN * CH, tid);
  __syncthreads();

  f32x16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = zero16();
  float m2 = -INFINITY, l = 0.f;

  for (int t = t0; t < ntiles; ++t) {
    const int cur = (t - t0) & 1;
    const u32x4* Ks = smem + cur * 2 * BN * CH;
    const u32x4* Vs = Ks + BN * CH;
    const int kv0 = t * BN;
    const bool more = t + 1 < ntiles;
    // No per-wave skip of wholly masked tiles (above the diagonal, or before every document of
    // the wave): a branch around the accumulators makes the compiler shuttle them through AGPRs.
    f32x16 sacc[2];
    {
      // S^T = K . Q^T, one 32-key half at a time (the plain forward keeps all 16 K row operands
      // in flight; with the bounds live as well that spills at two workgroups per CU).  Each
      // half's MFMA chain runs in the plain forward's order.
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        bf16x8 a[NDS];
#pragma unroll
        for (int s = 0; s < NDS; ++s) a[s] = row_frag(Ks, 32 * kt + r, 2 * s + h);
        __builtin_amdgcn_sched_barrier(0);
        sacc[kt] = zero16();
#pragma unroll
        for (int s = 0; s < NDS; ++s) sacc[kt] = mfma(a[s], qf[s], sacc[kt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) {  // next tile's global loads fly under the softmax and P.V
      ks.load(kb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
      vs.load(vb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
    }
    {
      if (kv0 + BN - 1 > q0w) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (kv0 + kt * 32 + acc_row(i, h) > qme) sacc[kt][i] = -INFINITY;
      }
      if (kv0 < lomax) {  // some row of the wave starts its document after this tile's first key
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (kv0 + kt * 32 + acc_row(i, h) < lome) sacc[kt][i] = -INFINITY;
      }
      float mx = sacc[0][0];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kt][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(m2, mx * c);
      // The plain forward relies on a wholly masked tile never being a row's first tile, so that
      // its running max is finite.  Here a wave's later rows can belong to a document that starts
      // after the block's first processed tile: their first tiles are all -inf, m2 = mnew = -inf,
      // and exp2(m2 - mnew) would be NaN.  Subtract 0 instead of -inf in both exponentials (a
      // select, no branch around the accumulators): alpha = exp2(-inf) = 0 and p = exp2(-inf) = 0,
      // so a row with no visible key yet keeps m2 = -inf, l = 0 and O = 0.  With a finite max the
      // values are the plain forward's.
      const float msub = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = __builtin_amdgcn_exp2f(m2 - msub);
      m2 = mnew;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kt][i], c, -msub));
          sacc[kt][i] = p;
          rs += p;
        }
      l = fmaf(l, alpha, rs);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) oacc[dt] *= alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {  // one k-step's V operands at a time (registers)
          bf16x8 vv[NDT];
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) vv[dt] = tr_frag(Vs, kt * 32 + 16 * s2, dt * 32, lane);
          const bf16x8 pb = acc_frag(sacc[kt], s2);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) oacc[dt] = mfma(vv[dt], pb, oacc[dt]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (more) {
      u32x4* nk = smem + (cur ^ 1) * 2 * BN * CH;
      ks.store(nk, tid);
      vs.store(nk + BN * CH, tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32);
  const float inv = 1.f / l;
  store_rows_T(oacc, inv, smem + w * 32 * CH, lane, o + ((size_t)b * S + q0w) * qstride + (size_t)hq * D, qstride);
  if (h == 0) lse2[((size_t)b * Hq + hq) * S + qme] = m2 + log2f(l);
}

// ------------------------------------------------------------------- backward pass 1: dQ
template <bool kDoc>
__device__ __forceinline__ void dq_pass(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                        const bf16_t* __restrict__ v, const bf16_t* __restrict__ o,
                                        const bf16_t* __restrict__ dout, const float* __restrict__ lse2,
                                        float* __restrict__ delta, bf16_t* __restrict__ dq,
                                        const int* __restrict__ doc_start, int B, int S, int Hq, int Hkv, float c,
                                        float scale, int causal, u32x4* smem) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  int qblk, b, hq, hk;
  block_coords(S, B, Hq, Hkv, causal, qblk, b, hq, hk);
  const int q0w = qblk * BM + w * 32, qme = q0w + r;
  const size_t qstride = (size_t)Hq * D, kvstride = (size_t)Hkv * D;

  bf16x8 qf[NDS], df[NDS];
  float dl;
  {
    const size_t off = ((size_t)b * S + qme) * qstride + (size_t)hq * D + 8 * h;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < NDS; ++s) {
      const u32x4 qq = *reinterpret_cast<const u32x4*>(q + off + 16 * s);
      const u32x4 dd = *reinterpret_cast<const u32x4*>(dout + off + 16 * s);
      const u32x4 oo = *reinterpret_cast<const u32x4*>(o + off + 16 * s);
      qf[s] = __builtin_bit_cast(bf16x8, qq);
      df[s] = __builtin_bit_cast(bf16x8, dd);
      const uint32_t dw[4] = {dd.x, dd.y, dd.z, dd.w}, ow[4] = {oo.x, oo.y, oo.z, oo.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part = fmaf(bf2f(dw[e] & 0xffffu), bf2f(ow[e] & 0xffffu), part);
        part = fmaf(bf2f(dw[e] >> 16), bf2f(ow[e] >> 16), part);
      }
    }
    dl = part + __shfl_xor(part, 32);
  }
  const size_t srow = ((size_t)b * Hq + hq) * S + qme;
  const float lq = lse2[srow];
  if (h == 0) delta[srow] = dl;

  const bf16_t* kb = k + (size_t)b * S * kvstride + (size_t)hk * D;
  const bf16_t* vb = v + (size_t)b * S * kvstride + (size_t)hk * D;
  const int* ds = kDoc ? doc_start + (size_t)b * S : nullptr;  // the forward's bounds
  const int lome = kDoc ? ds[qme] : 0;
  const int lomax = kDoc ? uniform(ds[q0w + 31]) : 0;
  const int t0 = kDoc ? min(max(uniform(ds[qblk * BM]), 0), qblk * BM) / BN : 0;
  const int ntiles = causal ? (qblk * BM + BM) / BN : S / BN;
  Stage<BN> ks, vs;
  ks.load(kb + (size_t)t0 * BN * kvstride, kvstride, tid);
  vs.load(vb + (size_t)t0 * BN * kvstride, kvstride, tid);
  ks.store(smem, tid);
  vs.store(smem + BN * CH, tid);
  __syncthreads();

  f32x16 dacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dacc[dt] = zero16();

  for (int t = t0; t < ntiles; ++t) {
    const int cur = (t - t0) & 1;
    const u32x4* Ks = smem + cur * 2 * BN * CH;
    const u32x4* Vs = Ks + BN * CH;
    const int kv0 = t * BN;
    const bool more = t + 1 < ntiles;
    {  // no per-wave skip of masked tiles (see the forward)
      const bool diag = causal && kv0 + BN - 1 > q0w;
      const bool edge = kDoc && kv0 < lomax;  // a document of the wave starts after this tile's first key
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x16 sa = zero16(), pa = zero16();
        {
          bf16x8 ka[NDS], va[NDS];
#pragma unroll
          for (int s = 0; s < NDS; ++s) {
            ka[s] = row_frag(Ks, kt * 32 + r, 2 * s + h);
            va[s] = row_frag(Vs, kt * 32 + r, 2 * s + h);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < NDS; ++s) {
            sa = mfma(ka[s], qf[s], sa);
            pa = mfma(va[s], df[s], pa);
          }
        }
        if (kt == 0 && more) {  // next tile's global loads fly under the rest of this one
          ks.load(kb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
          vs.load(vb + (size_t)(t + 1) * BN * kvstride, kvstride, tid);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float p = __builtin_amdgcn_exp2f(fmaf(sa[i], c, -lq));
          if (diag && kv0 + kt * 32 + acc_row(i, h) > qme) p = 0.f;
          if (edge && kv0 + kt * 32 + acc_row(i, h) < lome) p = 0.f;  // the saved lse2 excludes it
          sa[i] = p * (pa[i] - dl);
        }
        bf16x8 db[2], kk[2][NDT];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) kk[s2][dt] = tr_frag(Ks, kt * 32 + 16 * s2, dt * 32, lane);
        db[0] = acc_frag(sa, 0);
        db[1] = acc_frag(sa, 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) dacc[dt] = mfma(kk[s2][dt], db[s2], dacc[dt]);
      }
    }
    if (more) {
      u32x4* nk = smem + (cur ^ 1) * 2 * BN * CH;
      ks.store(nk, tid);
      vs.store(nk + BN * CH, tid);
    }
    __syncthreads();
  }
  store_rows_T(dacc, scale, smem + w * 32 * CH, lane, dq + ((size_t)b * S + q0w) * qstride + (size_t)hq * D, qstride);
}

__global__ __launch_bounds__(NT, 1) void ATTN_KERNEL(bwd_dq)(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, const float* __restrict__ lse2,
    float* __restrict__ delta, bf16_t* __restrict__ dq, int B, int S, int Hq, int Hkv, float c, float scale,
    int causal) {
  __shared__ u32x4 smem[4 * BN * CH];  // K0 V0 K1 V1 (64 KB; 32 KB at D = 64)
  dq_pass<false>(q, k, v, o, dout, lse2, delta, dq, nullptr, B, S, Hq, Hkv, c, scale, causal, smem);
}

__global__ __launch_bounds__(NT, 1) void ATTN_KERNEL(doc_dq)(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, const float* __restrict__ lse2,
    float* __restrict__ delta, bf16_t* __restrict__ dq, const int* __restrict__ doc_start, int B, int S, int Hq,
    int Hkv, float c, float scale) {
  __shared__ u32x4 smem[4 * BN * CH];  // K0 V0 K1 V1 (64 KB; 32 KB at D = 64)
  dq_pass<true>(q, k, v, o, dout, lse2, delta, dq, doc_start, B, S, Hq, Hkv, c, scale, 1, smem);
}

// -------------------------------------------------------------- backward pass 2: dK, dV
template <bool kDoc>
__device__ __forceinline__ void dkdv_pass(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                          const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
                                          const float* __restrict__ lse2, const float* __restrict__ delta,
                                          bf16_t* __restrict__ dk, bf16_t* __restrict__ dv,
                                          const int* __restrict__ doc_end, int B, int S, int Hq, int Hkv, float c,
                                          float scale, int causal, u32x4* smem, float4 (*stat)[2][QT / 4]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  // key block slowest in the launch order: under the causal mask kblk 0 (the most query tiles)
  // is dispatched first, so the light blocks fill in behind the heavy ones (with documents a
  // block's weight depends on where its last key's document ends, not on kblk alone)
  const int kblk = (int)blockIdx.x / (B * Hkv), bh = (int)blockIdx.x % (B * Hkv);
  const int b = bh / Hkv, hk = bh % Hkv, G = Hq / Hkv;
  const int k0w = kblk * BK + w * 32, kme = k0w + r;
  const size_t qstride = (size_t)Hq * D, kvstride = (size_t)Hkv * D;

  bf16x8 kf[NDS], vf[NDS];
  {
    const size_t off = ((size_t)b * S + kme) * kvstride + (size_t)hk * D + 8 * h;
#pragma unroll
    for (int s = 0; s < NDS; ++s) {
      kf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(k + off + 16 * s));
      vf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(v + off + 16 * s));
    }
  }
  const int* de = kDoc ? doc_end + (size_t)b * S : nullptr;
  const int hime = kDoc ? de[kme] : 0;            // one past the last query that sees this lane's key
  const int himin = kDoc ? uniform(de[k0w]) : 0;  // the wave's smallest bound (its first key's)
  const int qt0 = causal ? (kblk * BK) / QT : 0;
  // one past the last query tile any key of the block is seen from, clamped to [qt0 + 1, S / QT]
  const int qtend = kDoc ? min(max((uniform(de[kblk * BK + BK - 1]) + QT - 1) / QT, qt0 + 1), S / QT) : S / QT;
  const int nqt = qtend - qt0;  // query tiles per head
  const int ntiles = G * nqt;

  auto tile_ptrs = [&](int t, const bf16_t*& qp, const bf16_t*& dp, size_t& srow) {
    const int g = t / nqt, qt = qt0 + t % nqt, hq = hk * G + g;
    const size_t off = ((size_t)b * S + (size_t)qt * QT) * qstride + (size_t)hq * D;
    qp = q + off;
    dp = dout + off;
    srow = ((size_t)b * Hq + hq) * S + (size_t)qt * QT;
  };
  Stage<QT> qs, ds;
  float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load = [&](int t) {
    const bf16_t *qp, *dp;
    size_t srow;
    tile_ptrs(t, qp, dp, srow);
    qs.load(qp, qstride, tid);
    ds.load(dp, qstride, tid);
    if (tid < 16) st = reinterpret_cast<const float4*>((tid < 8 ? lse2 : delta) + srow)[tid & 7];
  };
  auto store = [&](int buf) {
    qs.store(smem + buf * 2 * QT * CH, tid);
    ds.store(smem + buf * 2 * QT * CH + QT * CH, tid);
    if (tid < 16) stat[buf][tid >> 3][tid & 7] = st;
  };
  load(0);
  store(0);
  __syncthreads();

  f32x16 dka[NDT], dva[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    dka[dt] = zero16();
    dva[dt] = zero16();
  }
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const u32x4* Qs = smem + cur * 2 * QT * CH;
    const u32x4* Ds = Qs + QT * CH;
    const int q0 = (qt0 + t % nqt) * QT;
    const bool more = t + 1 < ntiles;
    f32x16 sa = zero16(), pa = zero16();
    {  // no per-wave skip of masked tiles (see the forward)
      bf16x8 qa[NDS], da[NDS];
#pragma unroll
      for (int s = 0; s < NDS; ++s) {
        qa[s] = row_frag(Qs, r, 2 * s + h);
        da[s] = row_frag(Ds, r, 2 * s + h);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < NDS; ++s) {
        sa = mfma(qa[s], kf[s], sa);
        pa = mfma(da[s], vf[s], pa);
      }
    }
    if (more) load(t + 1);
    {
      const bool diag = causal && k0w + 31 > q0;
      const bool edge = kDoc && q0 + QT > himin;  // a document of the wave ends before this tile's last query
      // rows (queries) of register group g: 8g + 4h + 0..3 -> one float4 of lse2 / delta
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 L4 = stat[cur][0][2 * g + h];
        const float4 D4 = stat[cur][1][2 * g + h];
        const float Lv[4] = {L4.x, L4.y, L4.z, L4.w}, Dv[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          float p = __builtin_amdgcn_exp2f(fmaf(sa[i], c, -Lv[e]));
          if (diag && kme > q0 + 8 * g + 4 * h + e) p = 0.f;
          if (edge && q0 + 8 * g + 4 * h + e >= hime) p = 0.f;  // a query of a later document
          sa[i] = p;
          pa[i] = p * (pa[i] - Dv[e]);
        }
      }
      bf16x8 pb[2], db[2], td[2][NDT], tq[2][NDT];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          td[s2][dt] = tr_frag(Ds, 16 * s2, dt * 32, lane);
          tq[s2][dt] = tr_frag(Qs, 16 * s2, dt * 32, lane);
        }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        pb[s2] = acc_frag(sa, s2);
        db[s2] = acc_frag(pa, s2);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          dva[dt] = mfma(td[s2][dt], pb[s2], dva[dt]);
          dka[dt] = mfma(tq[s2][dt], db[s2], dka[dt]);
        }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
  }
  const size_t off = ((size_t)b * S + k0w) * kvstride + (size_t)hk * D;
  store_rows_T(dva, 1.f, smem + w * 32 * CH, lane, dv + off, kvstride);
  __syncthreads();
  store_rows_T(dka, scale, smem + w * 32 * CH, lane, dk + off, kvstride);
}

__global__ __launch_bounds__(NT, 1) void ATTN_KERNEL(bwd_dkdv)(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse2, const float* __restrict__ delta,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int B, int S, int Hq, int Hkv, float c, float scale,
    int causal) {
  __shared__ u32x4 smem[4 * QT * CH];  // Q0 dO0 Q1 dO1 (32 KB; 16 KB at D = 64); reused for the dK/dV epilogue
  __shared__ float4 stat[2][2][QT / 4];  // [buf][lse2 | delta][32 rows]
  dkdv_pass<false>(q, k, v, dout, lse2, delta, dk, dv, nullptr, B, S, Hq, Hkv, c, scale, causal, smem, stat);
}

__global__ __launch_bounds__(NT, 1) void ATTN_KERNEL(doc_dkdv)(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse2, const float* __restrict__ delta,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, const int* __restrict__ doc_end, int B, int S, int Hq,
    int Hkv, float c, float scale) {
  __shared__ u32x4 smem[4 * QT * CH];  // Q0 dO0 Q1 dO1 (32 KB; 16 KB at D = 64); reused for the dK/dV epilogue
  __shared__ float4 stat[2][2][QT / 4];  // [buf][lse2 | delta][32 rows]
  dkdv_pass<true>(q, k, v, dout, lse2, delta, dk, dv, doc_end, B, S, Hq, Hkv, c, scale, 1, smem, stat);
}

}  // namespace
