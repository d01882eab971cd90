// Causal / full GQA flash attention, forward and backward, bf16 in / bf16 out, for the Llama
// DDP worker (BASELINE "Llama-3 8B DDP bf16").  Replaces scaled_dot_product_attention (whose
// ROCm kernels ran at 328 TF/s forward and 156 TF/s backward on the 8B step,
// profiles/r1_llama3_8b_kernel_stats_master_adamw.md) and the [B,S,H,D] <-> [B,H,S,D]
// transposes around it: q/k/v/o/dq/dk/dv are read and written in the projections' own
// token-major layout [B, S, H, D].
//
// Layout and MFMA plan (v_mfma_f32_32x32x16_bf16; D = 128 = 8 k-steps / 4 output tiles):
//   * every kernel keeps one index "on the lane" (MFMA column = lane & 31) so that the
//     softmax statistics are per-lane scalars and an accumulator tile feeds the next MFMA
//     as its B operand with no data movement (the accumulator-as-operand k permutation:
//     registers 8s..8s+7 are k-step s; the other operand is read in the matching order);
//   * K/V (forward, dQ pass) and Q/dO (dK/dV pass) tiles are staged global -> registers ->
//     LDS once per tile (loads of tile t+1 in flight under the MFMAs of tile t, one
//     barrier per tile) in an XOR-swizzled 256-byte-row image that serves BOTH the row
//     reads (ds_read_b128) and the hardware-transposed reads (ds_read_b64_tr_b16)
//     conflict-free;
//   * forward: 4 waves x 32 queries per workgroup, 64-key tiles; S^T = K.Q^T (query on the
//     lane), online softmax in exp2 units, O^T += V^T.P^T; O is staged through LDS and
//     stored as whole rows; lse2 = m + log2(l) (log2 units) is kept for the backward;
//   * backward, pass 1 (dQ): same shape as the forward; recomputes S^T and dP^T = V.dO^T,
//     dS = P*(dP - delta), dQ^T += K^T.dS^T; computes delta = rowsum(dO*O) itself and
//     writes it for pass 2.  Every dQ row is finished inside one workgroup: no atomics;
//   * backward, pass 2 (dK, dV): 4 waves x 32 keys per workgroup (key on the lane), sweeps
//     the Hq/Hkv query heads of its kv head and every query tile at or after its keys;
//     S = Q.K^T, dP = dO.V^T, dV^T += dO^T.P, dK^T += Q^T.dS.  Deterministic, no atomics.
//   Causal workgroups run heaviest-first (the block index is the slowest grid index).
//
// Document mask for packed-sequence training (pto_attn_doc_fwd / pto_attn_doc_bwd).  The two
// 4-wave backward passes are written once, as bodies templated on kDoc (dq_pass, dkdv_pass); the
// plain and the document kernels are thin wrappers around them.  Without kDoc every bound below is
// a compile-time 0 / false; the document kernels are always causal (`causal` is the literal 1).
// The wrappers declare the LDS arrays and hand them in: as static arrays of the inlined body they
// cost the document dK/dV kernel two more registers (one more allocation granule).
// The two forward kernels stay separate texts.  Merged the same way (the operand schedule as one
// more template parameter) the document forward kept its registers and instruction counts but ran
// 2 % slower at S = 8192, and the plain one 0.8 % (profiles/attn_merge/README.md); as kernels of
// their own both compile to the instructions they had.  An edit to one forward's MFMA chains, mask
// or softmax has to be made in the other: tests/test_attention_doc_gpu.py holds them bit-identical
// with one document.
// Mask: query i sees key j iff doc_start[b, i] <= j <= i, equivalently j <= i < doc_end[b, j].
// doc_start [B, S] int32 is the index of the first token of token i's document, doc_end [B, S]
// one past its last token; both are non-decreasing along S.  So
//   * a wave's smallest / largest bound are the values at its first / last row (two wave-uniform
//     loads), and the per-element bound is a per-lane scalar: doc_start[query on the lane] in the
//     forward and dQ passes, doc_end[key on the lane] in the dK/dV pass;
//   * the bound is applied only on tiles that straddle a boundary for the wave (wave-uniform
//     test, like `diag` for the causal mask);
//   * tiles no row of the workgroup can see are never loaded: a forward / dQ query block starts
//     at key tile doc_start[first row of the block] / BN, and a dK/dV key block stops at query
//     tile ceil(doc_end[last key of the block] / QT).
// With doc_start == 0 (doc_end == S) every document kernel runs the plain kernel's operations in
// its order: bit-identical outputs.  The bounds are clamped to the block's causal range before
// they become tile indices, so no value in doc_start / doc_end can move a load out of the tensors.
//
// Head dim.  The 4-wave kernels (plain and document forward, dQ pass, dK/dV pass) live in
// attention_4wave.h and are compiled twice: here at D = 128 and in attention_d64.hip at D = 64
// (Llama-3.2 1B: 4 k-steps / 2 output tiles, 128-byte rows in their own LDS image, half the LDS).
// The entry points below check Dh and hand D = 64 calls to that file's launchers.  The 8-wave
// forward below and the pipelined backward (attention_bwd_pipe.hip) exist at D = 128 only, so the
// variant setters and PTO_ATTN_* select nothing at D = 64.
#include "attention_4wave.h"

extern "C" int pto_attn_dq_pipe(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                const float* lse2, float* delta, void* dq, int B, int S, int Hq, int Hkv, float c,
                                float scale, int causal, void* stream);
extern "C" int pto_attn_dkdv_pipe(const void* q, const void* k, const void* v, const void* dout, const float* lse2,
                                  const float* delta, void* dk, void* dv, int B, int S, int Hq, int Hkv, float c,
                                  float scale, int causal, int variant, void* stream);
// attention_d64.hip: the 4-wave passes at head dim 64 (shapes and alignment are checked here)
extern "C" int pto_attn_d64_fwd(const void* q, const void* k, const void* v, void* o, float* lse2,
                                const int* doc_start, int B, int S, int Hq, int Hkv, float c, int causal,
                                void* stream);
extern "C" int pto_attn_d64_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                                const float* lse2, float* delta, void* dq, void* dk, void* dv, const int* doc_start,
                                const int* doc_end, int B, int S, int Hq, int Hkv, float c, float scale, int causal,
                                void* stream);
// experiments/attention_variants.hip (experiment builds only; null in the default library)
extern "C" __attribute__((weak)) int pto_attn_exp_fwd(int variant, const void* q, const void* k, const void* v,
                                                      void* o, float* lse2, int B, int S, int Hq, int Hkv, float c,
                                                      int causal, void* stream);
extern "C" __attribute__((weak)) int pto_attn_exp_dq(int variant, const void* q, const void* k, const void* v,
                                                     const void* o, const void* dout, const float* lse2, float* delta,
                                                     void* dq, int B, int S, int Hq, int Hkv, float c, float scale,
                                                     int causal, void* stream);
extern "C" __attribute__((weak)) int pto_attn_exp_dkdv(int variant, const void* q, const void* k, const void* v,
                                                       const void* dout, const float* lse2, const float* delta,
                                                       void* dk, void* dv, int B, int S, int Hq, int Hkv, float c,
                                                       float scale, int causal, void* stream);

namespace {

// ------------------------------------------------------------- forward, 8-wave workgroup
// 8 waves x 32 queries (BM8 = 256 rows) share each staged K/V tile: half the LDS writes and
// the L2 -> CU tile traffic per FLOP of the 4-wave kernel (attention_4wave.h) at the same occupancy (one
// workgroup per CU = two waves per SIMD).  Differences besides the shape:
//   * workgroup -> (q block, b, q head in group, kv head) with the kv head FASTEST: block i
//     runs on XCD i % 8, so at Hkv = 8 every workgroup that reads one (b, kv head)'s K/V sits
//     on one XCD and its L2 holds them (K/V leave HBM once, not once per XCD);
//   * deferred rescale (defer-max): the running max only moves, and O / l are only rescaled,
//     when some row of the wave sees a tile max more than DEFER (log2 units) above it, so
//     p = exp2(s*c - m) stays <= 2^DEFER; most tiles after the first few skip the O-wide
//     multiply pass;
//   * wave-uniform skip of tiles wholly above a wave's diagonal (the last ones of its block);
//   * the younger half (waves 4-7) runs at priority 1 from the start (static form of
//     s_setprio: it otherwise loses VALU arbitration to the older half on every segment).
__global__ __launch_bounds__(NT8, 1) void attn_fwd8_kernel(const bf16_t* __restrict__ q,
                                                          const bf16_t* __restrict__ k,
                                                          const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                          float* __restrict__ lse2, int B, int S, int Hq, int Hkv,
                                                          float c, int causal) {
  __shared__ u32x4 smem[4 * BN * CH];  // K0 V0 K1 V1 (64 KB); the O staging image after the loop
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r = lane & 31;
  if (__builtin_amdgcn_readfirstlane(tid) >= NT8 / 2) __builtin_amdgcn_s_setprio(1);
  const int G = Hq / Hkv, nqb = S / BM8;
  int bi = (int)blockIdx.x;
  const int hk = bi % Hkv;
  bi /= Hkv;
  const int hq = hk * G + bi % G;
  bi /= G;
  const int b = bi % B, qi = bi / B;
  const int qblk = causal ? nqb - 1 - qi : qi;
  const int q0w = qblk * BM8 + w * 32, qme = q0w + r;
  const size_t qstride = (size_t)Hq * D, kvstride = (size_t)Hkv * D;

  bf16x8 qf[NDS];
  {
    const bf16_t* qrow = q + ((size_t)b * S + qme) * qstride + (size_t)hq * D + 8 * h;
#pragma unroll
    for (int s = 0; s < NDS; ++s) qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qrow + 16 * s));
  }
  const bf16_t* kb = k + (size_t)b * S * kvstride + (size_t)hk * D;
  const bf16_t* vb = v + (size_t)b * S * kvstride + (size_t)hk * D;
  const int ntiles = causal ? (qblk * BM8 + BM8) / BN : S / BN;
  // tiles this wave needs: under the mask the ones starting at or before its last row
  const int wtiles = causal ? (q0w + 31) / BN + 1 : ntiles;

  // K/V tiles by LDS-DMA issued from asm (no staging registers, no store pass; the next tile
  // lands under this tile's MFMAs).  Round 4: 187 vs 189 us against register staging, bit-identical
  // (profiles/r4_attn_fwd_dma_ab.json; that form is in git history, 3eed2ef).
  glds_tile_asm<BN, NT8>(kb, kvstride, smem, tid);
  glds_tile_asm<BN, NT8>(vb, kvstride, smem + BN * CH, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x16 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = zero16();
  float m2 = -INFINITY, l = 0.f;

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const u32x4* Ks = smem + cur * 2 * BN * CH;
    const u32x4* Vs = Ks + BN * CH;
    const int kv0 = t * BN;
    const bool more = t + 1 < ntiles;
    if (more) {  // next tile's DMA flies under this tile's MFMAs, into the buffer tile t-1 left
      u32x4* nk = smem + (cur ^ 1) * 2 * BN * CH;
      glds_tile_asm<BN, NT8>(kb + (size_t)(t + 1) * BN * kvstride, kvstride, nk, tid);
      glds_tile_asm<BN, NT8>(vb + (size_t)(t + 1) * BN * kvstride, kvstride, nk + BN * CH, tid);
    }
    if (t < wtiles) {  // wave-uniform
      f32x16 sacc[2];
      {
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
      if (causal && kv0 + BN - 1 > q0w) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          // key kv0 + 32kt + acc_row(i, h) > qme  <=>  (i&3) + 8(i>>2) > lim
          const int lim = qme - kv0 - kt * 32 - 4 * h;
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if ((i & 3) + 8 * (i >> 2) > lim) sacc[kt][i] = -INFINITY;
        }
      }
      // max3 chain in asm: plain fmaxf on MFMA results gets a canonicalising v_max per operand
      float mx = max3(sacc[0][0], sacc[0][1], sacc[0][2]);
#pragma unroll
      for (int i = 3; i < 15; i += 2) mx = max3(mx, sacc[0][i], sacc[0][i + 1]);
      mx = max3(mx, sacc[0][15], sacc[1][0]);
#pragma unroll
      for (int i = 1; i < 15; i += 2) mx = max3(mx, sacc[1][i], sacc[1][i + 1]);
      mx = max3(mx, sacc[1][15], sacc[1][15]);
      mx = half_max(mx);
      const float mt = mx * c;
      if (__builtin_amdgcn_ballot_w64(mt > m2 + DEFER) != 0) {  // wave-uniform: rescale
        const float mnew = fmaxf(m2, mt);
        const float alpha = __builtin_amdgcn_exp2f(m2 - mnew);
        m2 = mnew;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) oacc[dt] *= alpha;
      }
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sacc[kt][i], c, -m2));
          sacc[kt][i] = p;
          rs += p;
        }
      l += rs;
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t + 1 landed
    __syncthreads();
  }
  l = half_sum(l);
  const float inv = 1.f / l;
  store_rows_T(oacc, inv, smem + w * 32 * CH, lane, o + ((size_t)b * S + q0w) * qstride + (size_t)hq * D, qstride);
  if (h == 0) lse2[((size_t)b * Hq + hq) * S + qme] = m2 + log2f(l);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
bool aligned4(const void* p) { return p != nullptr && ((uintptr_t)p & 3u) == 0; }  // doc_start / doc_end

// Pass selection.  Default build: forward 10 (the 8-wave forward with LDS-DMA K/V staging, S % 256
// == 0; the 4-wave attn_fwd_kernel otherwise), dQ 9 and dK/dV 8 (the software-pipelined passes of
// attention_bwd_pipe.hip, every S % 128 == 0 shape).  The plain 4-wave passes stay as references
// and fallbacks: forward 4, dQ 4 (attn_bwd_dq_kernel) and dK/dV 1 (attn_bwd_dkdv_kernel), which the
// pipelined dK/dV pass matches bit for bit.  Other numbers are the rejected variants of
// experiments/attention_variants.hip, reachable only in experiment builds that link it (weak
// symbols below are null in the default library).  PTO_ATTN_FWD / PTO_ATTN_DQ / PTO_ATTN_DKDV in
// the environment, or pto_attn_set_*_variant() (tests, A/B runs).
int env_or(const char* name, int dflt) {
  const char* e = getenv(name);
  return e != nullptr ? atoi(e) : dflt;
}
int g_fwd_variant = -1, g_dq_variant = -1, g_dkdv_variant = -1;
int fwd_variant() { return g_fwd_variant < 0 ? (g_fwd_variant = env_or("PTO_ATTN_FWD", 10)) : g_fwd_variant; }
int dq_variant() { return g_dq_variant < 0 ? (g_dq_variant = env_or("PTO_ATTN_DQ", 9)) : g_dq_variant; }
int dkdv_variant() { return g_dkdv_variant < 0 ? (g_dkdv_variant = env_or("PTO_ATTN_DKDV", 8)) : g_dkdv_variant; }

int check_shapes(int B, int S, int Hq, int Hkv, int Dh) {
  if (B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || (Dh != 64 && Dh != 128)) return -1;
  if (S % BM || S % BK || Hq % Hkv) return -1;
  if ((long)(S / BM) * B * Hq > (1L << 30)) return -1;
  return 0;
}

}  // namespace

extern "C" {

int pto_attn_set_dq_variant(int v) {
  const int old = dq_variant();
  if (v == 4 || v == 9 || (v == 8 && pto_attn_exp_dq != nullptr)) g_dq_variant = v;
  return old;
}

int pto_attn_set_dkdv_variant(int v) {
  const int old = dkdv_variant();
  if (v == 1 || v == 8 || ((v >= 2 && v <= 4) || v == 6 || v == 7) && pto_attn_exp_dkdv != nullptr) g_dkdv_variant = v;
  return old;
}

int pto_attn_set_variant(int fwd) {
  const int old = fwd_variant();
  if (fwd == 4 || fwd == 10 || (fwd == 9 && pto_attn_exp_fwd != nullptr)) g_fwd_variant = fwd;
  return old;
}

// q [B,S,Hq,Dh], k/v [B,S,Hkv,Dh] bf16 contiguous; o [B,S,Hq,Dh] bf16; lse2 [B,Hq,S] f32
// (log2 units of the scaled scores).  Dh 64 or 128, S a multiple of 128, Hq a multiple of Hkv.
int pto_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, int B, int S, int Hq, int Hkv,
                 int Dh, float scale, int causal, void* stream) {
  if (check_shapes(B, S, Hq, Hkv, Dh)) return -1;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse2)) return -2;
  const float c = scale * 1.4426950408889634f;
  if (Dh == 64) return pto_attn_d64_fwd(q, k, v, o, lse2, nullptr, B, S, Hq, Hkv, c, causal, stream);
  const int fv = fwd_variant();
  if (fv != 4 && fv != 10 && pto_attn_exp_fwd != nullptr &&
      pto_attn_exp_fwd(fv, q, k, v, o, lse2, B, S, Hq, Hkv, c, causal, stream) == 0)
    return 0;
  if (fv != 4 && S % BM8 == 0)
    hipLaunchKernelGGL(attn_fwd8_kernel, dim3((S / BM8) * B * Hq), dim3(NT8), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse2, B, S, Hq, Hkv, c,
                       causal);
  else
    hipLaunchKernelGGL(attn_fwd_kernel, dim3((S / BM) * B * Hq), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse2, B, S, Hq, Hkv, c,
                       causal);
  return (int)hipGetLastError();
}

// dq [B,S,Hq,Dh], dk/dv [B,S,Hkv,Dh] bf16; delta [B,Hq,S] f32 scratch (rowsum(dO * O)).
int pto_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                 float* delta, void* dq, void* dk, void* dv, int B, int S, int Hq, int Hkv, int Dh, float scale,
                 int causal, void* stream) {
  if (check_shapes(B, S, Hq, Hkv, Dh)) return -1;
  const void* ps[] = {q, k, v, o, dout, lse2, delta, dq, dk, dv};
  for (const void* p : ps)
    if (!aligned16(p)) return -2;
  const float c = scale * 1.4426950408889634f;
  if (Dh == 64)
    return pto_attn_d64_bwd(q, k, v, o, dout, lse2, delta, dq, dk, dv, nullptr, nullptr, B, S, Hq, Hkv, c, scale,
                            causal, stream);
  const int qv = dq_variant(), kv = dkdv_variant();
  bool done = false;
  if (qv == 9) {
    const int rc = pto_attn_dq_pipe(q, k, v, o, dout, lse2, delta, dq, B, S, Hq, Hkv, c, scale, causal, stream);
    if (rc != 0) return rc;
    done = true;
  } else if (qv != 4 && pto_attn_exp_dq != nullptr) {
    done = pto_attn_exp_dq(qv, q, k, v, o, dout, lse2, delta, dq, B, S, Hq, Hkv, c, scale, causal, stream) == 0;
  }
  if (!done)
    hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3((S / BM) * B * Hq), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o,
                       (const bf16_t*)dout, lse2, delta, (bf16_t*)dq, B, S, Hq, Hkv, c, scale, causal);
  done = false;
  if (kv == 8) {
    const int rc = pto_attn_dkdv_pipe(q, k, v, dout, lse2, delta, dk, dv, B, S, Hq, Hkv, c, scale, causal, kv, stream);
    if (rc != 0) return rc;
    done = true;
  } else if (kv != 1 && pto_attn_exp_dkdv != nullptr) {
    done = pto_attn_exp_dkdv(kv, q, k, v, dout, lse2, delta, dk, dv, B, S, Hq, Hkv, c, scale, causal, stream) == 0;
  }
  if (!done)
    hipLaunchKernelGGL(attn_bwd_dkdv_kernel, dim3((S / BK) * B * Hkv), dim3(NT), 0, (hipStream_t)stream,
                       (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse2,
                       (const float*)delta, (bf16_t*)dk, (bf16_t*)dv, B, S, Hq, Hkv, c, scale, causal);
  return (int)hipGetLastError();
}

// pto_attn_fwd under the document mask: the same tensors (q [B,S,Hq,Dh], k/v [B,S,Hkv,Dh], o
// [B,S,Hq,Dh] bf16 contiguous; lse2 [B,Hq,S] f32, log2 units; S a multiple of 128, Hq a multiple
// of Hkv) plus doc_start [B,S] int32.  Always causal, always the 4-wave document kernel.
int pto_attn_doc_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int* doc_start, int B,
                     int S, int Hq, int Hkv, int Dh, float scale, void* stream) {
  if (check_shapes(B, S, Hq, Hkv, Dh)) return -1;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse2) || !aligned4(doc_start))
    return -2;
  const float c = scale * 1.4426950408889634f;
  if (Dh == 64) return pto_attn_d64_fwd(q, k, v, o, lse2, doc_start, B, S, Hq, Hkv, c, 1, stream);
  hipLaunchKernelGGL(attn_doc_fwd_kernel, dim3((S / BM) * B * Hq), dim3(NT), 0, (hipStream_t)stream,
                     (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse2, doc_start, B, S, Hq, Hkv,
                     c);
  return (int)hipGetLastError();
}

// pto_attn_bwd under the document mask: the same tensors (dq [B,S,Hq,Dh], dk/dv [B,S,Hkv,Dh]
// bf16; delta [B,Hq,S] f32 scratch, rowsum(dO * O)) plus doc_start / doc_end [B,S] int32.  Two
// launches, deterministic, no atomics.
int pto_attn_doc_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse2,
                     float* delta, void* dq, void* dk, void* dv, const int* doc_start, const int* doc_end, int B,
                     int S, int Hq, int Hkv, int Dh, float scale, void* stream) {
  if (check_shapes(B, S, Hq, Hkv, Dh)) return -1;
  const void* ps[] = {q, k, v, o, dout, lse2, delta, dq, dk, dv};
  for (const void* p : ps)
    if (!aligned16(p)) return -2;
  if (!aligned4(doc_start) || !aligned4(doc_end)) return -2;
  const float c = scale * 1.4426950408889634f;
  if (Dh == 64)
    return pto_attn_d64_bwd(q, k, v, o, dout, lse2, delta, dq, dk, dv, doc_start, doc_end, B, S, Hq, Hkv, c, scale, 1,
                            stream);
  hipLaunchKernelGGL(attn_doc_dq_kernel, dim3((S / BM) * B * Hq), dim3(NT), 0, (hipStream_t)stream,
                     (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)dout,
                     lse2, delta, (bf16_t*)dq, doc_start, B, S, Hq, Hkv, c, scale);
  hipLaunchKernelGGL(attn_doc_dkdv_kernel, dim3((S / BK) * B * Hkv), dim3(NT), 0, (hipStream_t)stream,
                     (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout, lse2,
                     (const float*)delta, (bf16_t*)dk, (bf16_t*)dv, doc_end, B, S, Hq, Hkv, c, scale);
  return (int)hipGetLastError();
}

}  // extern "C"
