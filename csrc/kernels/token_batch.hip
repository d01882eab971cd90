// Token-file batches for the Llama worker (--data): expand the narrow tokens of one micro-batch
// into everything the step needs, in one launch.
//
//   src    uint16 / uint32 tokens; row b is tok[b * row_stride + 0 .. S] (S + 1 tokens: the last
//          one is only the final target).  row_stride = S: the rows overlap by one token (one
//          contiguous slice of the stream); row_stride = S + 1: separately gathered rows.
//   x      int64 [B, S]   x[b, i] = tok[i], an id >= vocab written as vocab - 1 (and counted)
//   y      int64 [B, S]   tok[i + 1], or -100 where x[b, i] == eos (that target would be the next
//                         document's first token)
//   doc_start, doc_end    int32 [B, S], with eos >= 0 only: the first token of i's document and one
//                         past its last.  Position j starts a document iff j == 0 or x[j - 1] ==
//                         eos; doc_start[i] = the last start <= i, doc_end[i] = the first start > i
//                         (or S) -- ops.attention.doc_starts_from_tokens / doc_ends.
//   stats  int64 [3]      += targets that are not ignored, document starts, ids >= vocab (counted
//                         over the S + 1 tokens of every row).  The caller zeroes it.
//
// grid = (ceil(S / 1024), B): a block owns 1024 positions of one row, a thread 4 consecutive ones.
// Every block walks its whole row's narrow tokens once (<= 4 * (S + 1) bytes, L2-resident after the
// first block): the walk stages the chunk (and one token either side) into LDS and finds the two
// carries, the last document start before the chunk and the first one after it, so no block waits
// for another.  Inside the chunk the running max / min are thread, wave (__shfl) and block (LDS)
// scans.  The walk reads aligned 16-byte granules; a granule that is not wholly inside the row (row
// bases are only token-aligned) is read token by token, so nothing outside the row is touched.
// Integer results: the three atomics per block commute.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kT = 256;           // threads per block
constexpr int kE = 4;             // positions per thread
constexpr int kChunk = kT * kE;   // positions per block
constexpr int kWaves = kT / 64;

template <typename T>
__device__ __forceinline__ void load_granule(const uint8_t* gp, uint32_t (&t)[16 / sizeof(T)]) {
  const uint4 q = *reinterpret_cast<const uint4*>(gp);
  if constexpr (sizeof(T) == 4) {
    t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
  } else {
    t[0] = q.x & 0xffffu; t[1] = q.x >> 16; t[2] = q.y & 0xffffu; t[3] = q.y >> 16;
    t[4] = q.z & 0xffffu; t[5] = q.z >> 16; t[6] = q.w & 0xffffu; t[7] = q.w >> 16;
  }
}

template <typename T, bool EOS>
__global__ __launch_bounds__(kT) void token_batch_kernel(const T* __restrict__ src, long row_stride, int S,
                                                         uint32_t vocab, int eos, long long* __restrict__ x,
                                                         long long* __restrict__ y, int* __restrict__ doc_start,
                                                         int* __restrict__ doc_end,
                                                         unsigned long long* __restrict__ stats) {
  constexpr int kG = 16 / sizeof(T);  // tokens per 16-byte granule
  __shared__ uint32_t s_tok[kChunk + 2];  // clamped tokens of positions c0 - 1 .. c0 + kChunk
  __shared__ int s_red[4][kWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * kChunk;
  const int c1 = min(c0 + kChunk, S);
  const T* row = src + (long)b * row_stride;

  // ---- the walk over the row's S + 1 tokens ----
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(row);
  const uintptr_t g0 = a0 >> 4, g1 = (a0 + (uintptr_t)(S + 1) * sizeof(T) - 1) >> 4;
  int cin = 0, cout = S, oob = 0;
  for (uintptr_t g = g0 + tid; g <= g1; g += kT) {
    const uint8_t* gp = reinterpret_cast<const uint8_t*>(g << 4);
    // position of the granule's first token in the row (negative in the head granule)
    const long q0 = ((long)(g << 4) - (long)a0) / (long)sizeof(T);
    uint32_t t[kG];
    if (q0 >= 0 && q0 + kG - 1 <= S) {
      load_granule<T>(gp, t);
    } else {
#pragma unroll
      for (int k = 0; k < kG; ++k) {
        const long q = q0 + k;
        t[k] = (q >= 0 && q <= S) ? (uint32_t)row[q] : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < kG; ++k) {
      const long ql = q0 + k;
      if (ql < 0 || ql > S) continue;
      const int q = (int)ql;
      uint32_t v = t[k];
      const bool bad = v >= vocab;
      if (bad) v = vocab - 1;
      if (q >= c0 - 1 && q <= c1) s_tok[q - (c0 - 1)] = v;
      if (bad && ((q >= c0 && q < c1) || (q == S && c1 == S))) ++oob;
      if (EOS && (int)v == eos && q <= S - 2) {
        const int st = q + 1;  // a document starts after this token
        if (st < c0) cin = max(cin, st);
        if (st >= c1) cout = min(cout, st);
      }
    }
  }
  if (EOS) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      cin = max(cin, __shfl_xor(cin, d));
      cout = min(cout, __shfl_xor(cout, d));
    }
    if (lane == 0) { s_red[0][wave] = cin; s_red[1][wave] = cout; }
  }
  __syncthreads();  // s_tok and the waves' carries are written
  if (EOS) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      cin = max(cin, s_red[0][w]);
      cout = min(cout, s_red[1][w]);
    }
  }

  // ---- this thread's 4 positions ----
  const int p0 = c0 + tid * kE;
  uint32_t tk[kE + 2];  // tokens p0 - 1 .. p0 + kE
#pragma unroll
  for (int j = 0; j < kE + 2; ++j) tk[j] = (p0 + j - 1 <= c1) ? s_tok[tid * kE + j] : 0u;

  bool first[kE];
  int fwd[kE], bwd[kE];  // inclusive running max of starts; exclusive reverse running min
  int nstart = 0, nvalid = 0;
  if (EOS) {
    int run = -1;
#pragma unroll
    for (int j = 0; j < kE; ++j) {
      const int p = p0 + j;
      first[j] = p < c1 && (p == 0 || (int)tk[j] == eos);  // tk[j] is token p - 1
      if (first[j]) { run = p; ++nstart; }
      fwd[j] = run;
    }
    int rmin = S;
#pragma unroll
    for (int j = kE - 1; j >= 0; --j) {
      bwd[j] = rmin;
      if (first[j]) rmin = p0 + j;
    }
    // wave scans of the threads' totals: inclusive max from the left, inclusive min from the right
    int wmax = run, wmin = rmin;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(wmax, d), v = __shfl_down(wmin, d);
      if (lane >= d) wmax = max(wmax, u);
      if (lane + d < 64) wmin = min(wmin, v);
    }
    if (lane == 63) s_red[2][wave] = wmax;
    if (lane == 0) s_red[3][wave] = wmin;
    // exclusive: what the threads before (after) this one in the wave found
    int pre = __shfl_up(wmax, 1), post = __shfl_down(wmin, 1);
    if (lane == 0) pre = -1;
    if (lane == 63) post = S;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) pre = max(pre, s_red[2][w]);
      if (w > wave) post = min(post, s_red[3][w]);
    }
    pre = max(pre, cin);     // c0 == 0: position 0 is a start, the carry is never the answer
    post = min(post, cout);
#pragma unroll
    for (int j = 0; j < kE; ++j) {
      fwd[j] = max(fwd[j], pre);
      bwd[j] = min(bwd[j], post);
    }
  } else if (p0 == 0 && c1 > 0) {
    nstart = 1;  // one document per row
  }

  const long obase = (long)b * S;
#pragma unroll
  for (int j = 0; j < kE; ++j) {
    const int p = p0 + j;
    if (p >= c1) break;
    const uint32_t xv = tk[j + 1];
    const bool ignore = EOS && (int)xv == eos;
    x[obase + p] = (long long)xv;
    y[obase + p] = ignore ? -100ll : (long long)tk[j + 2];
    if (!ignore) ++nvalid;
    if (EOS) {
      doc_start[obase + p] = fwd[j];
      doc_end[obase + p] = bwd[j];
    }
  }

  // ---- stats: wave sums, then one atomic per wave and counter that has something to add ----
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    nvalid += __shfl_xor(nvalid, d);
    nstart += __shfl_xor(nstart, d);
    oob += __shfl_xor(oob, d);
  }
  if (lane == 0) {
    if (nvalid) atomicAdd(&stats[0], (unsigned long long)nvalid);
    if (nstart) atomicAdd(&stats[1], (unsigned long long)nstart);
    if (oob) atomicAdd(&stats[2], (unsigned long long)oob);
  }
}

template <typename T>
void launch(const void* src, long row_stride, int B, int S, uint32_t vocab, int eos, void* x, void* y, void* ds,
            void* de, void* stats, hipStream_t s) {
  const dim3 grid((unsigned)((S + kChunk - 1) / kChunk), (unsigned)B), block(kT);
  const T* sp = reinterpret_cast<const T*>(src);
  long long* xp = reinterpret_cast<long long*>(x);
  long long* yp = reinterpret_cast<long long*>(y);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
  if (eos >= 0)
    hipLaunchKernelGGL((token_batch_kernel<T, true>), grid, block, 0, s, sp, row_stride, S, vocab, eos, xp, yp,
                       reinterpret_cast<int*>(ds), reinterpret_cast<int*>(de), st);
  else
    hipLaunchKernelGGL((token_batch_kernel<T, false>), grid, block, 0, s, sp, row_stride, S, vocab, eos, xp, yp,
                       (int*)nullptr, (int*)nullptr, st);
}

}  // namespace

extern "C" {

// Positions one block owns: a row longer than this is split over several blocks.
long pto_token_batch_chunk() { return kChunk; }

// width_bytes: 2 (uint16) or 4 (uint32) tokens.  row_stride (tokens) >= S.  eos < 0: no document
// outputs (doc_start and doc_end must be null); eos >= 0: both required.  stats is zeroed by the caller.
int pto_token_batch(const void* src, int width_bytes, long row_stride, int B, int S, long vocab, int eos, void* x,
                    void* y, void* doc_start, void* doc_end, void* stats, void* stream) {
  if (B <= 0 || S <= 0 || B > 65535 || row_stride < S || vocab <= 0 || vocab > 0x7fffffffL) return -1;
  if (!src || !x || !y || !stats || (width_bytes != 2 && width_bytes != 4)) return -2;
  if (((uintptr_t)src % (uintptr_t)width_bytes) || ((uintptr_t)x & 7u) || ((uintptr_t)y & 7u) ||
      ((uintptr_t)stats & 7u))
    return -2;
  if (eos >= 0 ? (!doc_start || !doc_end || ((uintptr_t)doc_start & 3u) || ((uintptr_t)doc_end & 3u) || eos >= vocab)
               : (doc_start || doc_end))
    return -3;
  if (width_bytes == 2)
    launch<uint16_t>(src, row_stride, B, S, (uint32_t)vocab, eos, x, y, doc_start, doc_end, stats, (hipStream_t)stream);
  else
    launch<uint32_t>(src, row_stride, B, S, (uint32_t)vocab, eos, x, y, doc_start, doc_end, stats, (hipStream_t)stream);
  return (int)hipGetLastError();
}

}  // extern "C"
