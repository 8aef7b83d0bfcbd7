// A-GEM gradient projection over the flat fp32 buffers (include/cxrk.h, "agem_dots" / "agem_project"): one HBM-bound reduction and one
// conditional axpy on flat_buffers.h's walkers.
//  * agem_dots:    per-block partial sums of g * gref and of gref * gref, 8 B read per parameter
//  * agem_project: every block re-derives dot and rr from the partials; iff !(dot >= 0): g -= (dot / rr) * gref, 8 B read + 4 B
//                  written per parameter.  With dot >= 0 every block returns behind the partials: g and gref are not touched.
#include "cxrk.h"
#include "cxrk_common.h"
#include "flat_buffers.h"

using namespace cxrk;

namespace {

// The roundings are spelled out in both kernels: no contraction beyond the fused multiply-adds written below, so that the host
// emulation and the error bounds of the tests (tests/agem_ref.py) count the same operations.

__global__ __launch_bounds__(FLAT_THREADS) void agem_dots_kernel(const float* __restrict__ g, const float* __restrict__ r, long n,
                                                                 float* __restrict__ part) {
  const float* const in[2] = {g, r};
  flat_reduce<2, false, 2>(in, nullptr, n, part, [](const float (&v)[2], float&, float (&s)[2]) {
    s[0] = fmaf(v[0], v[1], s[0]);
    s[1] = fmaf(v[1], v[1], s[1]);
  });
}

struct AxpyElem {   // g += a * r, one fused multiply-add
  template <class T>
  static __device__ __forceinline__ void apply(long i, float* __restrict__ g, const float* __restrict__ r, float a) {
    at<T>(g, i) = fma_each(T(a), at<T>(r, i), at<T>(g, i));
  }
};

// Every block re-derives both sums from the partials (block_fold2), so all blocks, all runs and all data-parallel ranks decide alike.
// stats[3] counts the projected calls on the device.
__global__ __launch_bounds__(256) void agem_project_kernel(float* __restrict__ g, const float* __restrict__ r, long n,
                                                           const float* __restrict__ part, int nparts, float* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  float dot, rr;
  block_fold2(part, nparts, sh, dot, rr);
  const bool project = !(dot >= 0.f);                            // a NaN dot projects, and makes every element NaN
  const float coef = project ? dot / rr : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = dot; stats[1] = rr; stats[2] = coef;
    if (project) stats[3] = stats[3] + 1.f;
  }
  if (!project) return;
  flat_for_each<AxpyElem>(n, g, r, -coef);
}

}  // namespace

extern "C" size_t cxrk_agem_dots_partials_bytes(long n) { return n > 0 ? 2 * (size_t)flat_nparts(n) * sizeof(float) : 0; }

extern "C" int cxrk_agem_dots(const float* g, const float* gref, long n, float* partials, size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(g && gref && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(gref));
  const long nb = flat_nparts(n);
  if (partials == nullptr || ws_bytes < 2 * (size_t)nb * sizeof(float)) return CXRK_ERR_WS;
  hipLaunchKernelGGL(agem_dots_kernel, dim3((unsigned)nb), dim3(FLAT_THREADS), 0, stream, g, gref, n, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_agem_project(float* g, const float* gref, long n, const float* partials, float* stats, hipStream_t stream) {
  CXRK_CHECK_ARG(g && gref && partials && stats && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(gref));
  hipLaunchKernelGGL(agem_project_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, g, gref, n, partials, (int)flat_nparts(n), stats);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
