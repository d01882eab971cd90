// bf16 -> scaled OCP FP8 (e4m3fn / e5m2) operands for the Llama projections' FP8 GEMMs.
//
// Per-tensor scaling computed just in time from the tensor itself, two launches per tensor:
//
//   pto_fp8_amax   max |x| over the finite elements -> one fp32 partial per workgroup, plain
//                  stores into a caller-supplied workspace (the form of pto_grad_sumsq: 16-byte
//                  nontemporal loads, several in flight per lane, wave reduce, block reduce)
//   pto_fp8_cast   every workgroup reduces the partials (at most 4 KB, L2-resident) to amax,
//                  forms scale = fmax / amax (1 when amax == 0) and, for its 2x2 block of 64x64 tiles, writes
//                  q = rne(clamp(float(x) * scale, -fmax, fmax)) as [R, C] and/or its transpose
//                  [C, R] (through LDS) from one read of the source; workgroup 0 also writes
//                  scale_inv = amax / fmax (1 when amax == 0), the dequantisation factor the GEMM
//                  takes as a device tensor
//
// No float atomics, no memset, no host read: the grids are functions of the shape alone, max is
// order-independent, so the bytes are reproducible from run to run.
//
// The clamp is required: amax * (fmax / amax) can round above fmax.  Non-finite inputs are not
// hidden: they are left out of amax (the finite elements keep a usable scale) and come out as
// the NaN code 0x7f in either format.
//
// gfx950 FP8 is OCP: e4m3fn (max 448, no Inf) and e5m2 (max 57344), not the MI300 fnuz forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pto_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte access

constexpr int kT = 256;          // threads per block, both kernels
constexpr int kU = 4;            // amax: 16-byte loads in flight per lane
constexpr long kAmaxCap = 1024;  // amax: blocks (= partials) at most, grid-stride beyond
constexpr int kTile = 64;        // cast: tile edge
constexpr uint32_t kNaN8 = 0x7fu;

long amax_blocks(long n) {
  long blocks = (n / 8 + kT - 1) / kT;
  if (blocks < 1) blocks = 1;
  return blocks > kAmaxCap ? kAmaxCap : blocks;
}

// |x| of one bf16 as its 15 magnitude bits (monotonic in |x|); 0 for Inf / NaN.
__device__ __forceinline__ uint32_t finite_mag(uint32_t h) {
  h &= 0x7fffu;
  return h >= 0x7f80u ? 0u : h;
}

__global__ __launch_bounds__(kT) void fp8_amax_kernel(const u32x4* __restrict__ xv, long nv,
                                                      float* __restrict__ partial) {
  const long stride = (long)gridDim.x * kT;
  uint32_t m[kU];
#pragma unroll
  for (int k = 0; k < kU; ++k) m[k] = 0u;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < nv; i += kU * stride) {
    u32x4 q[kU];
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      const long j = i + k * stride;
      q[k] = j < nv ? __builtin_nontemporal_load(&xv[j]) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < kU; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        m[k] = max(m[k], finite_mag(q[k][c]));
        m[k] = max(m[k], finite_mag(q[k][c] >> 16));
      }
    }
  }
#pragma unroll
  for (int k = 1; k < kU; ++k) m[0] = max(m[0], m[k]);
  const float s = pto::wave_max(__uint_as_float(m[0] << 16));
  __shared__ float part[kT / pto::kWave];
  if ((threadIdx.x & (pto::kWave - 1)) == 0) part[threadIdx.x / pto::kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// Two floats -> two FP8 codes in the low (hi = false) or high half of `old`, round to nearest even.
template <bool E5M2, bool HI>
__device__ __forceinline__ uint32_t cvt_pk(float a, float b, uint32_t old) {
  if (E5M2) return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, (int)old, HI);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, HI);
}

// Four bf16 (two dwords) -> four FP8 codes in one dword, element order kept.
template <bool E5M2>
__device__ __forceinline__ uint32_t quant4(uint32_t w0, uint32_t w1, float scale, float fmax) {
  const uint32_t h[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
  float v[4];
  uint32_t nan_mask = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = fminf(fmaxf(__uint_as_float(h[i] << 16) * scale, -fmax), fmax);
    if ((h[i] & 0x7f80u) == 0x7f80u) nan_mask |= 0xffu << (8 * i);
  }
  uint32_t p = cvt_pk<E5M2, false>(v[0], v[1], 0u);
  p = cvt_pk<E5M2, true>(v[2], v[3], p);
  return (p & ~nan_mask) | ((kNaN8 * 0x01010101u) & nan_mask);
}

// LDS image of the transposed tile: byte (c, r) of a [64 c][64 r] tile, the four 16-byte slots of
// each row rotated by the row's 16-group so that the byte writes of one wave (16 tile rows r, four
// 16-column groups) land on 16 different banks; the 16-byte row reads stay one slot each.
__device__ __forceinline__ int lds_at(int c, int r) {
  return c * kTile + ((((r >> 4) ^ (c >> 4)) & 3) << 4) + (r & 15);
}

template <bool E5M2>
__global__ __launch_bounds__(kT) void fp8_cast_kernel(const uint16_t* __restrict__ x, long rows, long cols,
                                                      float fmax, const float* __restrict__ partial, int nparts,
                                                      const float* __restrict__ fixed_scale,
                                                      uint8_t* __restrict__ q, uint8_t* __restrict__ qT,
                                                      float* __restrict__ scale_inv) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[2][kTile * kTile];
  __shared__ float part[kT / pto::kWave];
  const int tid = threadIdx.x;
  const int r = tid >> 2, c0 = (tid & 3) * 16;  // this lane's 16 elements of the tile: row r, columns c0..
  const long tiles_r = rows / kTile, tiles_c = cols / kTile;

  // One 2x2 block of neighbouring tiles per workgroup, tile after tile.  A tile row of q and of qT
  // is 64 bytes, half a cache line: the block writes both halves of every line from the same CU
  // one after the other, where its L2 can merge them (3-5 % on the largest tensors against tiles
  // in linear order, profiles/fp8/README.md).  Odd tile counts leave 1-wide blocks at the edge:
  // `on`, the same for the whole workgroup.
  const long sup_r = (tiles_r + 1) / 2;
  const long tr0 = 2 * (blockIdx.x % sup_r), tc0 = 2 * (blockIdx.x / sup_r);
  auto locate = [&](int k, long& r0, long& cb, bool& on) -> bool {  // false: past the fourth tile
    const long tr = tr0 + (k >> 1), tc = tc0 + (k & 1);
    on = tr < tiles_r && tc < tiles_c;
    r0 = tr * kTile, cb = tc * kTile;
    return k < 4;
  };
  auto load = [&](long r0, long cb, u32x4& a, u32x4& b) {
    const u32x4* src = reinterpret_cast<const u32x4*>(x + (r0 + r) * cols + cb + c0);
    a = __builtin_nontemporal_load(src), b = __builtin_nontemporal_load(src + 1);
  };

  // the first tile's loads go out before the partials are read: one memory latency, not two
  int k = 0;
  long r0 = 0, cb = 0;
  bool on = false, more = locate(0, r0, cb, on);
  u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (more && on) load(r0, cb, a, b);

  float scale, inv;
  if (fixed_scale) {
    scale = fixed_scale[0];
    inv = 1.f / scale;
  } else {
    float p[4];  // nparts <= 1024: four independent loads per lane, in flight together
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = tid + i * kT < nparts ? partial[tid + i * kT] : 0.f;
    const float m = pto::wave_max(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])));
    if ((tid & (pto::kWave - 1)) == 0) part[tid / pto::kWave] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    scale = amax > 0.f ? fmax / amax : 1.f;
    inv = amax > 0.f ? amax / fmax : 1.f;
  }
  if (blockIdx.x == 0 && tid == 0) scale_inv[0] = inv;

  int buf = 0;
  while (more) {
    // the next tile's loads before this tile's work
    long nr0 = 0, ncb = 0;
    bool non = false;
    const bool nmore = locate(++k, nr0, ncb, non);
    u32x4 na = {0u, 0u, 0u, 0u}, nb = {0u, 0u, 0u, 0u};
    if (nmore && non) load(nr0, ncb, na, nb);
    if (on) {  // the same for the whole workgroup
      u32x4 o;
      o[0] = quant4<E5M2>(a[0], a[1], scale, fmax);
      o[1] = quant4<E5M2>(a[2], a[3], scale, fmax);
      o[2] = quant4<E5M2>(b[0], b[1], scale, fmax);
      o[3] = quant4<E5M2>(b[2], b[3], scale, fmax);
      if (q) *reinterpret_cast<u32x4*>(q + (r0 + r) * cols + cb + c0) = o;
      if (qT) {
        uint8_t* tl = tile[buf];
#pragma unroll
        for (int i = 0; i < 16; ++i) tl[lds_at(c0 + i, r)] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
        // one barrier per tile: the buffer written two tiles on was last read before the next
        // tile's barrier
        __syncthreads();
        // lane -> transposed row tid >> 2 (an input column), input rows 16 (tid & 3) ..
        const u32x4 w = *reinterpret_cast<const u32x4*>(tl + lds_at(r, c0));
        *reinterpret_cast<u32x4*>(qT + (cb + r) * rows + r0 + c0) = w;
        buf ^= 1;
      }
    }
    a = na, b = nb, r0 = nr0, cb = ncb, on = non, more = nmore;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

// Number of partials pto_fp8_amax writes for a matrix of n elements.
long pto_fp8_amax_parts(long n) { return n > 0 ? amax_blocks(n) : 0; }

// partial[0 .. pto_fp8_amax_parts(rows * cols)) = per-block max |x| over the finite elements of the
// contiguous bf16 matrix x [rows, cols]; `slots` is the room in `partial`.
int pto_fp8_amax(const void* x, long rows, long cols, float* partial, long slots, void* stream) {
  if (!x || !partial || rows <= 0 || cols <= 0 || rows % kTile || cols % kTile) return -1;
  if (!aligned16(x) || ((uintptr_t)partial & 3u)) return -2;
  const long n = rows * cols, blocks = amax_blocks(n);
  if (slots < blocks) return -3;
  hipLaunchKernelGGL(fp8_amax_kernel, dim3((unsigned)blocks), dim3(kT), 0, (hipStream_t)stream,
                     (const u32x4*)x, n / 8, partial);
  return (int)hipGetLastError();
}

// x [rows, cols] bf16 -> q [rows, cols] and / or qT [cols, rows] FP8 bytes (null skips one), and
// scale_inv[0].  format: 0 = e4m3fn, 1 = e5m2.  The scale comes from `partial[0 .. nparts)` (what
// pto_fp8_amax wrote for this matrix) or, when `fixed_scale` is not null, from fixed_scale[0].
int pto_fp8_cast(const void* x, long rows, long cols, int format, const float* partial, long nparts,
                 const float* fixed_scale, void* q, void* qT, float* scale_inv, void* stream) {
  if (!x || !scale_inv || (!q && !qT) || rows <= 0 || cols <= 0 || rows % kTile || cols % kTile ||
      format < 0 || format > 1)
    return -1;
  if (!fixed_scale && (!partial || nparts <= 0 || nparts > kAmaxCap)) return -1;
  if (!aligned16(x) || !aligned16(q) || !aligned16(qT) || ((uintptr_t)partial & 3u) ||
      ((uintptr_t)fixed_scale & 3u) || ((uintptr_t)scale_inv & 3u))
    return -2;
  const long blocks = ((rows / kTile + 1) / 2) * ((cols / kTile + 1) / 2);  // 2x2 tiles each
  if (blocks > 0x7fffffffL) return -1;
  const dim3 grid((unsigned)blocks), block(kT);
  hipStream_t s = (hipStream_t)stream;
  if (format == 0)
    hipLaunchKernelGGL(fp8_cast_kernel<false>, grid, block, 0, s, (const uint16_t*)x, rows, cols, 448.f, partial,
                       (int)nparts, fixed_scale, (uint8_t*)q, (uint8_t*)qT, scale_inv);
  else
    hipLaunchKernelGGL(fp8_cast_kernel<true>, grid, block, 0, s, (const uint16_t*)x, rows, cols, 57344.f, partial,
                       (int)nparts, fixed_scale, (uint8_t*)q, (uint8_t*)qT, scale_inv);
  return (int)hipGetLastError();
}

}  // extern "C"
