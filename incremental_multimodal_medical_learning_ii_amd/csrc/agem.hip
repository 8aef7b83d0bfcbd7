// A-GEM gradient projection over the flat fp32 buffers (include/cxrk.h, "agem_dots" / "agem_project"): one HBM-bound reduction and one
// conditional axpy, beside optim.hip's grad_sqnorm / adamw_clipped and consolidate.hip's ewc_penalty, and in their style.
//  * agem_dots:    per-block partial sums of g * gref and of gref * gref in grad_sqnorm's partition, 8 B read per parameter
//  * agem_project: every block re-derives dot and rr from the partials; iff !(dot >= 0): g -= (dot / rr) * gref, 8 B read + 4 B
//                  written per parameter.  With dot >= 0 every block returns behind the partials: g and gref are not touched.
#include "cxrk.h"
#include "cxrk_common.h"

using namespace cxrk;

namespace {

// The roundings are spelled out in both kernels: no contraction beyond the fmaf()s written below, so that the host emulation and the
// error bounds of the tests (tests/agem_ref.py) count the same operations.

// grad_sqnorm's partition (optim.hip): a function of n alone, nparts blocks of 256 threads, block b's thread t takes the float4 groups
// (b * 256 + t) + j * nparts * 256, j = 0, 1, ..., four of them in flight in four accumulators per sum; the n % 4 tail in block 0.
constexpr int DOT_THREADS = 256;
constexpr int DOT_UNROLL = 4;

__global__ __launch_bounds__(DOT_THREADS) void agem_dots_kernel(const float* __restrict__ g, const float* __restrict__ r, long n,
                                                                float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * DOT_THREADS;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float ad[DOT_UNROLL], ar[DOT_UNROLL];
#pragma unroll
  for (int k = 0; k < DOT_UNROLL; ++k) { ad[k] = 0.f; ar[k] = 0.f; }
  for (long i = (long)blockIdx.x * DOT_THREADS + threadIdx.x; i < n4; i += DOT_UNROLL * stride) {
    float4 gv[DOT_UNROLL], rv[DOT_UNROLL];
#pragma unroll
    for (int k = 0; k < DOT_UNROLL; ++k) {
      const long q = i + k * stride;
      const bool in = q < n4;                       // a group past the end contributes +0 to both accumulators
      gv[k] = in ? reinterpret_cast<const float4*>(g)[q] : zero;
      rv[k] = in ? reinterpret_cast<const float4*>(r)[q] : zero;
    }
#pragma unroll
    for (int k = 0; k < DOT_UNROLL; ++k) {
      ad[k] = fmaf(gv[k].x, rv[k].x, ad[k]); ad[k] = fmaf(gv[k].y, rv[k].y, ad[k]);
      ad[k] = fmaf(gv[k].z, rv[k].z, ad[k]); ad[k] = fmaf(gv[k].w, rv[k].w, ad[k]);
      ar[k] = fmaf(rv[k].x, rv[k].x, ar[k]); ar[k] = fmaf(rv[k].y, rv[k].y, ar[k]);
      ar[k] = fmaf(rv[k].z, rv[k].z, ar[k]); ar[k] = fmaf(rv[k].w, rv[k].w, ar[k]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)                       // the n % 4 elements behind the last whole group
    for (long j = n4 * 4; j < n; ++j) { ad[0] = fmaf(g[j], r[j], ad[0]); ar[0] = fmaf(r[j], r[j], ar[0]); }
  const float sd = block_sum((ad[0] + ad[1]) + (ad[2] + ad[3]), sh);
  const float sr = block_sum((ar[0] + ar[1]) + (ar[2] + ar[3]), sh);
  if (threadIdx.x == 0) { part[blockIdx.x] = sd; part[gridDim.x + blockIdx.x] = sr; }
}

// Every block re-derives both sums from the partials in adamw_clipped's fixed order (thread t takes partials t, t + 256, ..., then the
// block sum), so all blocks, all runs and all data-parallel ranks decide alike.  stats[3] counts the projected calls on the device.
__global__ __launch_bounds__(256) void agem_project_kernel(float* __restrict__ g, const float* __restrict__ r, long n,
                                                           const float* __restrict__ part, int nparts, float* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ float sh[16];
  float td = 0.f, tr = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) { td += part[i]; tr += part[nparts + i]; }
  const float dot = block_sum(td, sh);                           // block_sum syncs before it writes sh again
  const float rr = block_sum(tr, sh);
  const bool project = !(dot >= 0.f);                            // a NaN dot projects, and makes every element NaN
  const float coef = project ? dot / rr : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = dot; stats[1] = rr; stats[2] = coef;
    if (project) stats[3] = stats[3] + 1.f;
  }
  if (!project) return;
  const float nc = -coef;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 gv = *reinterpret_cast<float4*>(g + i);
      const float4 rv = *reinterpret_cast<const float4*>(r + i);
      gv.x = fmaf(nc, rv.x, gv.x); gv.y = fmaf(nc, rv.y, gv.y);
      gv.z = fmaf(nc, rv.z, gv.z); gv.w = fmaf(nc, rv.w, gv.w);
      *reinterpret_cast<float4*>(g + i) = gv;
    } else {
      for (long j = i; j < n; ++j) g[j] = fmaf(nc, r[j], g[j]);
    }
  }
}

static inline unsigned flat_blocks(long n) {
  long nb = (n / 4 + 255) / 256;
  return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
}

}  // namespace

extern "C" size_t cxrk_agem_dots_partials_bytes(long n) { return 2 * cxrk_grad_sqnorm_partials_bytes(n); }

extern "C" int cxrk_agem_dots(const float* g, const float* gref, long n, float* partials, size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(g && gref && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(gref));
  const long nb = (long)(cxrk_grad_sqnorm_partials_bytes(n) / sizeof(float));   // one partition for every flat reduction
  if (partials == nullptr || ws_bytes < 2 * (size_t)nb * sizeof(float)) return CXRK_ERR_WS;
  hipLaunchKernelGGL(agem_dots_kernel, dim3((unsigned)nb), dim3(DOT_THREADS), 0, stream, g, gref, n, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_agem_project(float* g, const float* gref, long n, const float* partials, float* stats, hipStream_t stream) {
  CXRK_CHECK_ARG(g && gref && partials && stats && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(gref));
  const long np = (long)(cxrk_grad_sqnorm_partials_bytes(n) / sizeof(float));
  hipLaunchKernelGGL(agem_project_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, g, gref, n, partials, (int)np, stats);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
