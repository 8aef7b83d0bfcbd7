// Elastic weight consolidation over the flat fp32 buffers (include/cxrk.h, "fisher_accumulate" / "ewc_consolidate" / "ewc_penalty"):
// HBM-bound elementwise work and one reduction on flat_buffers.h's walkers.
//  * fisher_accumulate: acc += w * g^2, 8 B read + 4 B written per parameter
//  * ewc_consolidate:   F = gamma * F + scale * acc and anchor = p in one pass, 12 B read + 8 B written (4 + 4 with the identity Fisher)
//  * ewc_penalty:       g += strength * F * (p - anchor) and per-block partial sums of F * (p - anchor)^2,
//                       16 B read + 4 B written per parameter (12 + 4 with the identity Fisher)
#include "cxrk.h"
#include "cxrk_common.h"
#include "flat_buffers.h"

using namespace cxrk;

namespace {

// The roundings are spelled out in every kernel of this file: no contraction beyond the fused multiply-adds written below, so that
// the host emulation and the error bounds of the tests (tests/ewc_ref.py) count the same operations.

struct FisherElem {
  template <class T>
  static __device__ __forceinline__ void apply(long i, float* __restrict__ acc, const float* __restrict__ g, float w) {
#pragma clang fp contract(off)
    const T gv = at<T>(g, i);
    at<T>(acc, i) = fma_each(T(w), gv * gv, at<T>(acc, i));
  }
};
__global__ __launch_bounds__(256) void fisher_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, float w) {
  flat_for_each<FisherElem>(n, acc, g, w);
}

template <bool HAS_F>
struct ConsolidateElem {
  template <class T>
  static __device__ __forceinline__ void apply(long i, float* __restrict__ F, const float* __restrict__ acc, float* __restrict__ anchor,
                                               const float* __restrict__ p, float gamma, float scale) {
#pragma clang fp contract(off)
    at<T>(anchor, i) = at<T>(p, i);
    if (HAS_F) at<T>(F, i) = fma_each(T(gamma), at<T>(F, i), T(scale) * at<T>(acc, i));
  }
};
template <bool HAS_F>
__global__ __launch_bounds__(256) void ewc_consolidate_kernel(float* __restrict__ F, const float* __restrict__ acc,
                                                              float* __restrict__ anchor, const float* __restrict__ p, long n,
                                                              float gamma, float scale) {
  flat_for_each<ConsolidateElem<HAS_F>>(n, F, acc, anchor, p, gamma, scale);
}

// one element: d = p - a;  t = F * d (t = d with the identity Fisher: 1 * d is d bit for bit);  g += strength * t;  sum += t * d
template <bool HAS_F>
__device__ __forceinline__ void penalty_elem(float& g, float p, float a, float f, float strength, float& sum) {
#pragma clang fp contract(off)
  const float d = p - a;
  const float t = HAS_F ? f * d : d;
  g = fmaf(strength, t, g);
  sum = fmaf(t, d, sum);
}

// a group past the end contributes d = 0, t = 0: +0 into its accumulator
template <bool HAS_F>
__global__ __launch_bounds__(FLAT_THREADS) void ewc_penalty_kernel(float* __restrict__ g, const float* __restrict__ p,
                                                                   const float* __restrict__ anchor, const float* __restrict__ F, long n,
                                                                   float strength, float* __restrict__ part) {
  constexpr int NIN = HAS_F ? 3 : 2;
  const float* const in[3] = {p, anchor, F};
  flat_reduce<NIN, true, 1>(in, g, n, part, [=](const float (&v)[NIN], float& gi, float (&s)[1]) {
    penalty_elem<HAS_F>(gi, v[0], v[1], v[NIN - 1], strength, s[0]);   // (without F the last argument is not used)
  });
}

}  // namespace

extern "C" int cxrk_fisher_accumulate(float* acc, const float* g, long n, float w, hipStream_t stream) {
  CXRK_CHECK_ARG(acc && g && n > 0);
  CXRK_CHECK_ARG(aligned16(acc) && aligned16(g));
  hipLaunchKernelGGL(fisher_accumulate_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, acc, g, n, w);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_ewc_consolidate(float* F, const float* acc, float* anchor, const float* p, long n, float gamma, float scale,
                                    hipStream_t stream) {
  CXRK_CHECK_ARG(anchor && p && n > 0);
  CXRK_CHECK_ARG((F == nullptr) == (acc == nullptr));            // the identity Fisher has neither
  CXRK_CHECK_ARG(aligned16(anchor) && aligned16(p) && aligned16(F) && aligned16(acc));
  if (F != nullptr)
    hipLaunchKernelGGL(ewc_consolidate_kernel<true>, dim3(flat_blocks(n)), dim3(256), 0, stream, F, acc, anchor, p, n, gamma, scale);
  else
    hipLaunchKernelGGL(ewc_consolidate_kernel<false>, dim3(flat_blocks(n)), dim3(256), 0, stream, F, acc, anchor, p, n, gamma, scale);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" size_t cxrk_ewc_penalty_partials_bytes(long n) { return n > 0 ? (size_t)flat_nparts(n) * sizeof(float) : 0; }

extern "C" int cxrk_ewc_penalty(float* g, const float* p, const float* anchor, const float* F, long n, float strength, float* partials,
                                size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(g && p && anchor && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(p) && aligned16(anchor) && aligned16(F));
  const long nb = flat_nparts(n);
  if (partials == nullptr || ws_bytes < (size_t)nb * sizeof(float)) return CXRK_ERR_WS;
  if (F != nullptr)
    hipLaunchKernelGGL(ewc_penalty_kernel<true>, dim3((unsigned)nb), dim3(FLAT_THREADS), 0, stream, g, p, anchor, F, n, strength, partials);
  else
    hipLaunchKernelGGL(ewc_penalty_kernel<false>, dim3((unsigned)nb), dim3(FLAT_THREADS), 0, stream, g, p, anchor, F, n, strength, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
