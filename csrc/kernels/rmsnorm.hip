// Fused RMSNorm forward/backward for the Llama path (fp32 or bf16 activations, fp32
// weight, fp32 statistics).  y = x * rsqrt(mean(x^2) + eps) * w.
//
// Forward: one workgroup per row, the row held in registers, sum of squares reduced
// wave-then-LDS, rstd saved for the backward.
// Backward: a workgroup owns R consecutive rows; per row it recomputes the row dot
// product sum_j dy_j w_j x_j, writes dx, and accumulates dw_j += dy_j x_j rstd for its
// columns in registers; the per-workgroup dw partials are reduced column-wise by a
// second tiny launch in fixed order (deterministic, no atomics).
//
// One kernel per direction, <TX, TY, W, P>: a lane moves W consecutive elements per access
// (W = 4: 16 B fp32 / 8 B bf16, when D % 4 == 0 and every pointer is 16-byte aligned; W = 1
// otherwise) and makes P accesses per row, at columns j = W * (threadIdx.x + k * kT), k < P.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "pto_vec.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxPer = 32;  // D <= kT * kMaxPer = 8192
static_assert(kT == pto::kBlockSumThreads, "pto::block_sum sums 256 threads");

// The roundings of the forward's sum of squares are spelled out, with the compiler's own contraction
// off, so rstd is a property of this code.  W = 4 rounds every square and adds them in order (in the
// load loop of the kernel).  W = 1, here, rounds x1^2, fuses x0^2 into it and then every further
// square in order: the rounding of the first one-element kernels, which a compiler's choice of
// operand order had fixed.  The one exception is P = 1: a lone square is still the compiler's to
// fuse into the first add of block_sum, as it always has been.
template <int P>
__device__ __forceinline__ float sum_squares(const pto::Vec<1> (&v)[P]) {
  if constexpr (P == 1) {
    return v[0].v[0] * v[0].v[0];
  } else {
#pragma clang fp contract(off)
    float ss = fmaf(v[0].v[0], v[0].v[0], v[1].v[0] * v[1].v[0]);
#pragma unroll
    for (int k = 2; k < P; ++k) ss = fmaf(v[k].v[0], v[k].v[0], ss);
    return ss;
  }
}

// TX: activation dtype of x / dx (the residual stream, fp32 or bf16).  TY: dtype of y / dy
// (bf16 when the norm feeds autocast bf16 matmuls: writing bf16 here removes the separate
// fp32->bf16 cast kernel in the forward and the bf16->fp32 dy cast in the backward).
// Fused residual form (delta != nullptr, W = 4 only): s = x + delta is written to s_out (the
// residual stream, dtype TX) and normalised, so the block's residual add costs no separate pass.
template <typename TX, typename TY, int W, int P>
__global__ __launch_bounds__(kT) void rmsnorm_fwd_kernel(const TX* __restrict__ x, const float* __restrict__ w,
                                                         TY* __restrict__ y, float* __restrict__ rstd, int D,
                                                         float eps, const TY* __restrict__ delta,
                                                         TX* __restrict__ s_out) {
  __shared__ float sh[kT / 64];
  const long row = blockIdx.x;
  pto::Vec<W> v[P];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int j = W * (threadIdx.x + k * kT);
    v[k] = j < D ? pto::vload<W>(x + row * D + j) : pto::Vec<W>{};
    if (W == 4 && delta != nullptr && j < D) {
      const pto::Vec<W> dd = pto::vload<W>(delta + row * D + j);
#pragma unroll
      for (int e = 0; e < W; ++e) v[k].v[e] += dd.v[e];
      pto::vstore(s_out + row * D + j, v[k]);
    }
    if constexpr (W == 4) {
#pragma clang fp contract(off)
#pragma unroll
      for (int e = 0; e < W; ++e) ss += v[k].v[e] * v[k].v[e];
    }
  }
  if constexpr (W == 1) ss = sum_squares(v);
  const float r = rsqrtf(pto::block_sum(ss, sh) / (float)D + eps);
  if (threadIdx.x == 0) rstd[row] = r;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int j = W * (threadIdx.x + k * kT);
    if (j < D) {
      const pto::Vec<W> wv = pto::vload<W>(w + j);
      pto::Vec<W> o;
#pragma unroll
      for (int e = 0; e < W; ++e) o.v[e] = v[k].v[e] * r * wv.v[e];
      pto::vstore(y + row * D + j, o);
    }
  }
}

// The W = 1 backward's roundings, spelled out with the compiler's own contraction off so that they
// are a property of this code and not of a build: the row dot product and dw fuse each product into
// the running sum; dx rounds r * w * g and x * c and subtracts.  FUSED_DX is the one historical
// exception, kept so that no result changes: bf16 x and dy at P = 1 (D <= 256) has always formed
// dx = fma(g, r * w, -(x * c)).  (W = 4 keeps the compiler's contraction: its kernels are checked
// instruction by instruction against the build they replace, profiles/kernel_helpers.)
struct Bwd1 {
  static __device__ __forceinline__ float dot(float g, float w, float x, float acc) {
#pragma clang fp contract(off)
    return fmaf(g * w, x, acc);
  }
  template <bool FUSED_DX>
  static __device__ __forceinline__ float dx(float r, float w, float g, float x, float c) {
#pragma clang fp contract(off)
    if constexpr (FUSED_DX) return fmaf(g, r * w, -(x * c));
    else return r * w * g - x * c;
  }
  static __device__ __forceinline__ float dw(float g, float x, float r, float acc) {
#pragma clang fp contract(off)
    return fmaf(g * x, r, acc);
  }
};

// Backward, software-pipelined: the next row's x / dy loads are issued before this row's
// block reduction, so HBM latency overlaps the two LDS barriers of block_sum.
// Fused residual form (gres != nullptr, W = 4 only): dx = gres + d(norm)/dx -- the residual
// stream's gradient is summed here instead of by a separate add; with dbranch != nullptr the same
// value is also written in the branch dtype TY (the gradient of the block's bf16 output).
template <typename TX, typename TY, int W, int P>
__global__ __launch_bounds__(kT) void rmsnorm_bwd_kernel(const TY* __restrict__ dy, const TX* __restrict__ x,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ rstd, TX* __restrict__ dx,
                                                         float* __restrict__ dw_part, long rows, int D,
                                                         int rows_per_block, const TX* __restrict__ gres,
                                                         TY* __restrict__ dbranch) {
  __shared__ float sh[kT / 64];
  using V = pto::Vec<W>;
  V wv[P], dwa[P], xv[P], gv[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int j = W * (threadIdx.x + k * kT);
    wv[k] = j < D ? pto::vload<W>(w + j) : V{};
    dwa[k] = V{};
  }
  const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  auto load_row = [&](long row, V* xo, V* go) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int j = W * (threadIdx.x + k * kT);
      xo[k] = j < D ? pto::vload<W>(x + row * D + j) : V{};
      go[k] = j < D ? pto::vload<W>(dy + row * D + j) : V{};
    }
  };
  if (r0 < r1) load_row(r0, xv, gv);
  for (long row = r0; row < r1; ++row) {
    V xn[P], gn[P];
    if (row + 1 < r1) load_row(row + 1, xn, gn);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < P; ++k)
#pragma unroll
      for (int e = 0; e < W; ++e) {
        if constexpr (W == 1) dot = Bwd1::dot(gv[k].v[e], wv[k].v[e], xv[k].v[e], dot);
        else dot += gv[k].v[e] * wv[k].v[e] * xv[k].v[e];
      }
    const float r = rstd[row];
    const float c = pto::block_sum(dot, sh) * r * r * r / (float)D;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int j = W * (threadIdx.x + k * kT);
      if (j < D) {
        V o;
#pragma unroll
        for (int e = 0; e < W; ++e) {
          if constexpr (W == 1) {
            o.v[e] = Bwd1::dx<P == 1 && sizeof(TX) == 2>(r, wv[k].v[e], gv[k].v[e], xv[k].v[e], c);
            dwa[k].v[e] = Bwd1::dw(gv[k].v[e], xv[k].v[e], r, dwa[k].v[e]);
          } else {
            o.v[e] = r * wv[k].v[e] * gv[k].v[e] - xv[k].v[e] * c;
            dwa[k].v[e] += gv[k].v[e] * xv[k].v[e] * r;
          }
        }
        if (W == 4 && gres != nullptr) {
          const V gr = pto::vload<W>(gres + row * D + j);
#pragma unroll
          for (int e = 0; e < W; ++e) o.v[e] += gr.v[e];
        }
        if (W == 4 && dbranch != nullptr) pto::vstore(dbranch + row * D + j, o);
        pto::vstore(dx + row * D + j, o);
      }
    }
    if (row + 1 < r1) {
#pragma unroll
      for (int k = 0; k < P; ++k) {
        xv[k] = xn[k];
        gv[k] = gn[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int j = W * (threadIdx.x + k * kT);
    if (j < D) pto::vstore(dw_part + (long)blockIdx.x * D + j, dwa[k]);
  }
}

// Column sums of dw_part [nparts, D] in a fixed order (deterministic).  A workgroup owns
// kColsPerWg columns: kCLanes lanes per row slice read them as float4 and kSlices slices
// walk disjoint row ranges with all loads of a slice issued back to back, then the slices
// are added in slice order through LDS.  D=4096, 512 parts: 128 workgroups x 256 lanes
// with 32 float4 loads in flight each, instead of 16 workgroups each walking 512 rows one
// dependent load at a time (123 us -> a few us, see docs/kernels.md).
constexpr int kCLanes = 8;                   // float4 lanes per slice -> 32 columns
constexpr int kColsPerWg = kCLanes * 4;
constexpr int kSlices = kT / kCLanes;        // 32 row slices
__global__ __launch_bounds__(kT) void colsum_kernel(const float* __restrict__ part, int nparts, int D,
                                                    float* __restrict__ out) {
  __shared__ float4 sh[kSlices][kCLanes];
  const int lane = threadIdx.x % kCLanes, slice = threadIdx.x / kCLanes;
  const int j = blockIdx.x * kColsPerWg + lane * 4;
  const int per = (nparts + kSlices - 1) / kSlices;
  const int p0 = slice * per, p1 = min(nparts, p0 + per);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j + 3 < D && (D & 3) == 0) {
#pragma unroll 8
    for (int p = p0; p < p1; ++p) {
      const float4 v = *reinterpret_cast<const float4*>(part + (long)p * D + j);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  } else {
    for (int p = p0; p < p1; ++p) {
      const float* r = part + (long)p * D;
      if (j < D) s.x += r[j];
      if (j + 1 < D) s.y += r[j + 1];
      if (j + 2 < D) s.z += r[j + 2];
      if (j + 3 < D) s.w += r[j + 3];
    }
  }
  sh[slice][lane] = s;
  __syncthreads();
  if (slice == 0) {
    float4 t = sh[0][lane];
    for (int k = 1; k < kSlices; ++k) {
      const float4 v = sh[k][lane];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    if (j < D) out[j] = t.x;
    if (j + 1 < D) out[j + 1] = t.y;
    if (j + 2 < D) out[j + 2] = t.z;
    if (j + 3 < D) out[j + 3] = t.w;
  }
}

bool vec_ok(int D, std::initializer_list<const void*> ptrs) {
  if (D % 4) return false;
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15u) return false;
  return true;
}

// Calls f with P as a std::integral_constant: the accesses per lane that cover D, rounded up to
// a power of two.  W = 4 takes P in {1, 2, 4, 8}, W = 1 in {1, .., 32} (D <= kT * kMaxPer).
template <int N>
using Int = std::integral_constant<int, N>;
template <int W, typename F>
void with_p(int D, F f) {
  const int p = (D + W * kT - 1) / (W * kT);
  if (p <= 1) f(Int<1>{});
  else if (p <= 2) f(Int<2>{});
  else if (p <= 4) f(Int<4>{});
  else if (W == 4 || p <= 8) f(Int<8>{});
  else if constexpr (W == 1) {
    if (p <= 16) f(Int<16>{});
    else f(Int<32>{});
  }
}

template <typename TX, typename TY, int W>
void fwd_launch(const void* x, const float* w, void* y, float* rstd, long rows, int D, float eps, void* stream,
                const void* delta, void* s_out) {
  with_p<W>(D, [&](auto p) {
    hipLaunchKernelGGL((rmsnorm_fwd_kernel<TX, TY, W, decltype(p)::value>), dim3(rows), dim3(kT), 0,
                       (hipStream_t)stream, (const TX*)x, w, (TY*)y, rstd, D, eps, (const TY*)delta, (TX*)s_out);
  });
}

template <typename TX, typename TY>
int fwd_dispatch(const void* x, const float* w, void* y, float* rstd, long rows, int D, float eps, void* stream,
                 const void* delta, void* s_out) {
  if (vec_ok(D, {x, w, y}) && (delta == nullptr || vec_ok(D, {delta, s_out})))
    fwd_launch<TX, TY, 4>(x, w, y, rstd, rows, D, eps, stream, delta, s_out);
  else if (delta != nullptr)
    return -3;  // the fused residual form needs W = 4
  else
    fwd_launch<TX, TY, 1>(x, w, y, rstd, rows, D, eps, stream, nullptr, nullptr);
  return (int)hipGetLastError();
}

template <typename TX, typename TY, int W>
void bwd_launch(const void* dy, const void* x, const float* w, const float* rstd, void* dx, float* dw_part,
                long rows, int D, int rpb, long nb, void* stream, const void* gres, void* dbranch) {
  with_p<W>(D, [&](auto p) {
    hipLaunchKernelGGL((rmsnorm_bwd_kernel<TX, TY, W, decltype(p)::value>), dim3(nb), dim3(kT), 0,
                       (hipStream_t)stream, (const TY*)dy, (const TX*)x, w, rstd, (TX*)dx, dw_part, rows, D, rpb,
                       (const TX*)gres, (TY*)dbranch);
  });
}

template <typename TX, typename TY>
int bwd_dispatch(const void* dy, const void* x, const float* w, const float* rstd, void* dx, float* dw_part,
                 long rows, int D, int rpb, long nb, void* stream, const void* gres, void* dbranch) {
  if (vec_ok(D, {dy, x, w, dx, dw_part}) && (gres == nullptr || vec_ok(D, {gres})) &&
      (dbranch == nullptr || vec_ok(D, {dbranch})))
    bwd_launch<TX, TY, 4>(dy, x, w, rstd, dx, dw_part, rows, D, rpb, nb, stream, gres, dbranch);
  else if (gres != nullptr || dbranch != nullptr)
    return -3;
  else
    bwd_launch<TX, TY, 1>(dy, x, w, rstd, dx, dw_part, rows, D, rpb, nb, stream, nullptr, nullptr);
  return 0;
}

// dtype pair code: 0 = (x fp32, y fp32), 1 = (bf16, bf16), 2 = (x fp32, y bf16).  Calls f with a
// value of each type.
bool valid_pair(int code) { return code >= 0 && code <= 2; }
template <typename F>
int with_pair(int code, F f) {
  if (code == 0) return f(float{}, float{});
  if (code == 1) return f(__hip_bfloat16{}, __hip_bfloat16{});
  return f(float{}, __hip_bfloat16{});
}

int fwd_any(const void* x, const void* delta, const float* w, void* y, void* s_out, float* rstd, long rows, int D,
            float eps, int dtype, void* stream) {
  if (D <= 0 || D > kT * kMaxPer || rows <= 0 || !valid_pair(dtype)) return -1;
  return with_pair(dtype, [&](auto tx, auto ty) {
    return fwd_dispatch<decltype(tx), decltype(ty)>(x, w, y, rstd, rows, D, eps, stream, delta, s_out);
  });
}

}  // namespace

extern "C" {

int pto_rmsnorm_fwd(const void* x, const float* w, void* y, float* rstd, long rows, int D, float eps, int dtype,
                    void* stream) {
  return fwd_any(x, nullptr, w, y, nullptr, rstd, rows, D, eps, dtype, stream);
}

// Number of workgroups (= rows of dw_part) the backward uses for `rows` rows.
long pto_rmsnorm_bwd_parts(long rows, int rows_per_block) { return (rows + rows_per_block - 1) / rows_per_block; }

// Residual-fused forms.  fwd: s = x + delta (written to s_out), y = rmsnorm(s).  bwd: x is s,
// gres the residual stream's incoming gradient; dx = gres + d(norm), dbranch = the same in
// the y dtype (nullable).  W = 4 only (D % 4 == 0, 16-byte aligned): -3 otherwise.
int pto_add_rmsnorm_fwd(const void* x, const void* delta, const float* w, void* y, void* s_out, float* rstd,
                        long rows, int D, float eps, int dtype, void* stream) {
  if (delta == nullptr || s_out == nullptr) return -1;
  return fwd_any(x, delta, w, y, s_out, rstd, rows, D, eps, dtype, stream);
}

int pto_add_rmsnorm_bwd(const void* dy, const void* x, const float* w, const float* rstd, const void* gres,
                        void* dx, void* dbranch, float* dw, float* dw_part, long rows, int D, int rows_per_block,
                        int dtype, void* stream) {
  if (D <= 0 || D > kT * kMaxPer || rows <= 0 || rows_per_block <= 0 || !valid_pair(dtype)) return -1;
  const long nb = (rows + rows_per_block - 1) / rows_per_block;
  if (nb > (1L << 30)) return -1;
  const int rc = with_pair(dtype, [&](auto tx, auto ty) {
    return bwd_dispatch<decltype(tx), decltype(ty)>(dy, x, w, rstd, dx, dw_part, rows, D, rows_per_block, nb, stream,
                                                    gres, dbranch);
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(colsum_kernel, dim3((D + kColsPerWg - 1) / kColsPerWg), dim3(kT), 0, (hipStream_t)stream,
                     dw_part, (int)nb, D, dw);
  return (int)hipGetLastError();
}

int pto_rmsnorm_bwd(const void* dy, const void* x, const float* w, const float* rstd, void* dx, float* dw,
                    float* dw_part, long rows, int D, int rows_per_block, int dtype, void* stream) {
  return pto_add_rmsnorm_bwd(dy, x, w, rstd, nullptr, dx, nullptr, dw, dw_part, rows, D, rows_per_block, dtype,
                             stream);
}

}  // extern "C"
