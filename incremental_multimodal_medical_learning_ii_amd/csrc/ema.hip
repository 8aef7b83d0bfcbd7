// Exponential moving average of the parameters over the flat fp32 buffers (include/cxrk.h, "ema_update" / "flat_swap"): two HBM-bound
// elementwise passes on flat_buffers.h's walker.  No workspace, no atomics, no LDS.
//  * ema_update: avg += (1 - decay) * (p - avg), 8 B read + 4 B written per parameter
//  * flat_swap:  a <-> b, 8 B read + 8 B written per parameter, nothing of the size of the buffers in between
#include "cxrk.h"
#include "cxrk_common.h"
#include "flat_buffers.h"

using namespace cxrk;

namespace {

// The roundings are spelled out: d = p - avg (one), r = fma(c, d, avg) (one), nothing contracted beyond the fused multiply-add written
// below, so that the error bound of the tests (tests/ema_ref.py) counts the same operations.  The lerp form is the contract: d = 0
// gives r = avg, and so does c = 0 with a finite d.  Where r equals avg as a number, avg keeps its own bits: the addition alone would
// turn avg = -0 into +0, and models do hold negative zeros.
__device__ __forceinline__ float keep_equal(float r, float a) { return r == a ? a : r; }      // a NaN r compares unequal and stays
__device__ __forceinline__ f32x4 keep_equal(f32x4 r, f32x4 a) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = keep_equal(r[k], a[k]);
  return o;
}

struct EmaElem {
  template <class T>
  static __device__ __forceinline__ void apply(long i, float* avg, const float* p, float c) {
#pragma clang fp contract(off)
    const T a = at<T>(avg, i);
    const T d = at<T>(p, i) - a;
    at<T>(avg, i) = keep_equal(fma_each(T(c), d, a), a);
  }
};
__global__ __launch_bounds__(256) void ema_update_kernel(float* avg, const float* p, long n, float c) {
  flat_for_each<EmaElem>(n, avg, p, c);
}

// moves only: every bit pattern (NaN payloads included) arrives as it left
struct SwapElem {
  template <class T>
  static __device__ __forceinline__ void apply(long i, float* __restrict__ a, float* __restrict__ b) {
    const T x = at<T>(a, i);
    const T y = at<T>(b, i);
    at<T>(a, i) = y;
    at<T>(b, i) = x;
  }
};
__global__ __launch_bounds__(256) void flat_swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
  flat_for_each<SwapElem>(n, a, b);
}

}  // namespace

extern "C" int cxrk_ema_update(float* avg, const float* p, long n, float decay, hipStream_t stream) {
  CXRK_CHECK_ARG(avg && p && n > 0);
  CXRK_CHECK_ARG(aligned16(avg) && aligned16(p));
  CXRK_CHECK_ARG(decay >= 0.f && decay <= 1.f);                  // a NaN decay fails both comparisons
  const float c = 1.f - decay;                                   // formed once, in fp32: exact for decay >= 0.5
  hipLaunchKernelGGL(ema_update_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, avg, p, n, c);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_flat_swap(float* a, float* b, long n, hipStream_t stream) {
  CXRK_CHECK_ARG(a && b && n > 0);
  CXRK_CHECK_ARG(aligned16(a) && aligned16(b));
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  CXRK_CHECK_ARG(ua + bytes <= ub || ub + bytes <= ua);          // a == b and every overlap of the two ranges
  hipLaunchKernelGGL(flat_swap_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, a, b, n);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
