// Kernels over the optimiser's flat fp32 buffers (optim.hip, consolidate.hip, agem.hip; the loss heads' scalar folds in loss.hip):
// the single definition of the partition of a deterministic reduction, of the refold of its partial sums, and of the elementwise
// grid ("one partition, one refold").  Every result bit of these kernels depends on what is written here.
#pragma once
#include "cxrk_common.h"

namespace cxrk {

// Every kernel on these helpers is launched with 256 threads, and the helpers' own loops step by the constant: blockDim.x read in a
// helper that also reads blockIdx.x is compiled to a per-lane load of the work-group size (the compiler folds it to a scalar load
// only where the kernel itself reads it).  flat_reduce still pays that load once per thread, through block_sum's blockDim.x.
constexpr int FLAT_THREADS = 256;
constexpr int FLAT_UNROLL = 4;        // groups in flight per thread, one accumulator each
constexpr long FLAT_MAX_PARTS = 1024;

// Number of blocks, and of partial sums per sum, of a reduction over n elements: a function of n alone, never of the device.
static inline long flat_nparts(long n) {
  const long nb = (n / 4 + (long)FLAT_THREADS * FLAT_UNROLL - 1) / ((long)FLAT_THREADS * FLAT_UNROLL);
  return nb < 1 ? 1 : (nb > FLAT_MAX_PARTS ? FLAT_MAX_PARTS : nb);
}

// Grid of an elementwise kernel (flat_for_each) over n elements.
static inline unsigned flat_blocks(long n) {
  const long nb = (n / 4 + FLAT_THREADS - 1) / FLAT_THREADS;
  return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
}

// The refold: the sum of part[0..n) in one fixed order (thread t takes partials t, t + 256, ..., then the block sum), so that
// every block, every run and every data-parallel rank derives the same bits.  `sh` as for block_sum; all threads get the result.
__device__ __forceinline__ float block_fold(const float* __restrict__ part, long n, float* sh) {
  float t = 0.f;
  for (long i = threadIdx.x; i < n; i += FLAT_THREADS) t += part[i];
  return block_sum(t, sh);
}
// Two refolds, a of part[0..n) and b of part[n..2n): the bits of two block_fold calls, with the loads of both in flight before the
// first block sum (every block of agem_project waits for them before it starts its share of the buffer).
__device__ __forceinline__ void block_fold2(const float* __restrict__ part, long n, float* sh, float& a, float& b) {
  float ta = 0.f, tb = 0.f;
  for (long i = threadIdx.x; i < n; i += FLAT_THREADS) { ta += part[i]; tb += part[n + i]; }
  a = block_sum(ta, sh);                                         // block_sum syncs before it writes sh again
  b = block_sum(tb, sh);
}

// The partition walker: NSUM sums of per-element terms over n elements, as gridDim.x = flat_nparts(n) partial sums each;
// part[s * gridDim.x + blockIdx.x] takes block blockIdx.x's share of sum s.  Block b's thread t takes the float4 groups
// (b * 256 + t) + j * gridDim.x * 256, j = 0, 1, ...: FLAT_UNROLL of them are loaded before any arithmetic and go to one accumulator
// each (a group past the end is read as zeros), the accumulators are combined as (a0 + a1) + (a2 + a3), and the n % 4 elements behind
// the last whole group go to accumulator 0 of block 0's thread 0.  `in`: NIN arrays that are only read; `rw` (RW): one array that is
// read, handed to `elem` and written back.  elem(const float (&v)[NIN], float& w, float (&s)[NSUM]) holds the kernel's own arithmetic
// for one element: v[a] = in[a][i], w = rw[i] (a dummy without RW), s = the accumulators the element's terms are added to.
template <int NIN, bool RW, int NSUM, class Elem>
__device__ __forceinline__ void flat_reduce(const float* const* in, float* rw, long n, float* part, Elem elem) {
  static_assert(FLAT_UNROLL == 4, "the combine below is written for four accumulators");
  __shared__ float sh[16];
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * FLAT_THREADS;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  float acc[FLAT_UNROLL][NSUM];
#pragma unroll
  for (int k = 0; k < FLAT_UNROLL; ++k)
#pragma unroll
    for (int s = 0; s < NSUM; ++s) acc[k][s] = 0.f;
  for (long i = (long)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n4; i += FLAT_UNROLL * stride) {
    f32x4 x[FLAT_UNROLL][NIN], w[FLAT_UNROLL];
#pragma unroll
    for (int k = 0; k < FLAT_UNROLL; ++k) {
      const long q = i + k * stride;
      const bool inside = q < n4;
#pragma unroll
      for (int a = 0; a < NIN; ++a) x[k][a] = inside ? reinterpret_cast<const f32x4*>(in[a])[q] : zero;
      w[k] = (RW && inside) ? reinterpret_cast<const f32x4*>(rw)[q] : zero;
    }
#pragma unroll
    for (int k = 0; k < FLAT_UNROLL; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float v[NIN], wc = w[k][c];
#pragma unroll
        for (int a = 0; a < NIN; ++a) v[a] = x[k][a][c];
        elem(v, wc, acc[k]);
        w[k][c] = wc;
      }
    if (RW) {
#pragma unroll
      for (int k = 0; k < FLAT_UNROLL; ++k)
        if (i + k * stride < n4) reinterpret_cast<f32x4*>(rw)[i + k * stride] = w[k];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long j = n4 * 4; j < n; ++j) {
      float v[NIN], wj = RW ? rw[j] : 0.f;
#pragma unroll
      for (int a = 0; a < NIN; ++a) v[a] = in[a][j];
      elem(v, wj, acc[0]);
      if (RW) rw[j] = wj;
    }
#pragma unroll
  for (int s = 0; s < NSUM; ++s) {
    const float t = block_sum((acc[0][s] + acc[1][s]) + (acc[2][s] + acc[3][s]), sh);   // block_sum syncs before it writes sh again
    if (threadIdx.x == 0) part[(long)s * gridDim.x + blockIdx.x] = t;
  }
}

// The elementwise walk on flat_blocks(n)'s grid: Elem::apply<T>(i, args...) once per whole group of four elements at i with
// T = f32x4, and once per element behind the last whole group with T = float, so that a kernel writes its formula once, over
// `at<T>(ptr, i)`.  The kernel's pointers and scalars travel as plain arguments (a capturing lambda's closure was kept in LDS).
template <class Elem, class... Args>
__device__ __forceinline__ void flat_for_each(long n, Args... args) {
  const long stride = (long)gridDim.x * FLAT_THREADS * 4;
  for (long i = ((long)blockIdx.x * FLAT_THREADS + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      Elem::template apply<f32x4>(i, args...);
    } else {
      for (long j = i; j < n; ++j) Elem::template apply<float>(j, args...);
    }
  }
}
template <class T> __device__ __forceinline__ T& at(float* p, long i) { return *reinterpret_cast<T*>(p + i); }
template <class T> __device__ __forceinline__ const T& at(const float* p, long i) { return *reinterpret_cast<const T*>(p + i); }
// fmaf on one element or on each of four; a kernel's scalar argument w enters as T(w), which for f32x4 is w in all four lanes
template <class T> __device__ __forceinline__ T fma_each(T a, T b, T c) { return __builtin_elementwise_fma(a, b, c); }

}  // namespace cxrk
