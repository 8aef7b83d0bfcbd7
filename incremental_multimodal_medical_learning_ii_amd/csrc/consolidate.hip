// Elastic weight consolidation over the flat fp32 buffers (include/cxrk.h, "fisher_accumulate" / "ewc_consolidate" / "ewc_penalty"):
// HBM-bound elementwise work and one reduction, beside optim.hip's grad_sqnorm / adamw_clipped and in their style.
//  * fisher_accumulate: acc += w * g^2, 8 B read + 4 B written per parameter
//  * ewc_consolidate:   F = gamma * F + scale * acc and anchor = p in one pass, 12 B read + 8 B written (4 + 4 with the identity Fisher)
//  * ewc_penalty:       g += strength * F * (p - anchor) and per-block partial sums of F * (p - anchor)^2 in grad_sqnorm's partition,
//                       16 B read + 4 B written per parameter (12 + 4 with the identity Fisher)
#include "cxrk.h"
#include "cxrk_common.h"

using namespace cxrk;

namespace {

// The roundings are spelled out in every kernel of this file: no contraction beyond the fmaf()s written below, so that the host
// emulation and the error bounds of the tests (tests/ewc_ref.py) count the same operations.

__global__ __launch_bounds__(256) void fisher_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, float w) {
#pragma clang fp contract(off)
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 av = *reinterpret_cast<float4*>(acc + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      av.x = fmaf(w, gv.x * gv.x, av.x); av.y = fmaf(w, gv.y * gv.y, av.y);
      av.z = fmaf(w, gv.z * gv.z, av.z); av.w = fmaf(w, gv.w * gv.w, av.w);
      *reinterpret_cast<float4*>(acc + i) = av;
    } else {
      for (long j = i; j < n; ++j) acc[j] = fmaf(w, g[j] * g[j], acc[j]);
    }
  }
}

template <bool HAS_F>
__global__ __launch_bounds__(256) void ewc_consolidate_kernel(float* __restrict__ F, const float* __restrict__ acc,
                                                              float* __restrict__ anchor, const float* __restrict__ p, long n,
                                                              float gamma, float scale) {
#pragma clang fp contract(off)
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      *reinterpret_cast<float4*>(anchor + i) = *reinterpret_cast<const float4*>(p + i);
      if (HAS_F) {
        float4 fv = *reinterpret_cast<float4*>(F + i);
        const float4 av = *reinterpret_cast<const float4*>(acc + i);
        fv.x = fmaf(gamma, fv.x, scale * av.x); fv.y = fmaf(gamma, fv.y, scale * av.y);
        fv.z = fmaf(gamma, fv.z, scale * av.z); fv.w = fmaf(gamma, fv.w, scale * av.w);
        *reinterpret_cast<float4*>(F + i) = fv;
      }
    } else {
      for (long j = i; j < n; ++j) {
        anchor[j] = p[j];
        if (HAS_F) F[j] = fmaf(gamma, F[j], scale * acc[j]);
      }
    }
  }
}

// grad_sqnorm's partition (optim.hip): a function of n alone, nparts blocks of 256 threads, block b's thread t takes the float4 groups
// (b * 256 + t) + j * nparts * 256, j = 0, 1, ..., four of them in flight in four accumulators; the n % 4 tail in block 0.
constexpr int PEN_THREADS = 256;
constexpr int PEN_UNROLL = 4;

// one element: d = p - a;  t = F * d (t = d with the identity Fisher: 1 * d is d bit for bit);  g += strength * t;  sum += t * d
template <bool HAS_F>
__device__ __forceinline__ void penalty_elem(float& g, float p, float a, float f, float strength, float& sum) {
#pragma clang fp contract(off)
  const float d = p - a;
  const float t = HAS_F ? f * d : d;
  g = fmaf(strength, t, g);
  sum = fmaf(t, d, sum);
}

template <bool HAS_F>
__global__ __launch_bounds__(PEN_THREADS) void ewc_penalty_kernel(float* __restrict__ g, const float* __restrict__ p,
                                                                  const float* __restrict__ anchor, const float* __restrict__ F, long n,
                                                                  float strength, float* __restrict__ part) {
  __shared__ float sh[16];
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * PEN_THREADS;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float acc[PEN_UNROLL];
#pragma unroll
  for (int k = 0; k < PEN_UNROLL; ++k) acc[k] = 0.f;
  for (long i = (long)blockIdx.x * PEN_THREADS + threadIdx.x; i < n4; i += PEN_UNROLL * stride) {
    float4 gv[PEN_UNROLL], pv[PEN_UNROLL], av[PEN_UNROLL], fv[PEN_UNROLL];
#pragma unroll
    for (int k = 0; k < PEN_UNROLL; ++k) {
      const long q = i + k * stride;
      const bool in = q < n4;                       // a group past the end contributes d = 0, t = 0: +0 into its accumulator
      gv[k] = in ? reinterpret_cast<const float4*>(g)[q] : zero;
      pv[k] = in ? reinterpret_cast<const float4*>(p)[q] : zero;
      av[k] = in ? reinterpret_cast<const float4*>(anchor)[q] : zero;
      fv[k] = (HAS_F && in) ? reinterpret_cast<const float4*>(F)[q] : zero;
    }
#pragma unroll
    for (int k = 0; k < PEN_UNROLL; ++k) {
      penalty_elem<HAS_F>(gv[k].x, pv[k].x, av[k].x, fv[k].x, strength, acc[k]);
      penalty_elem<HAS_F>(gv[k].y, pv[k].y, av[k].y, fv[k].y, strength, acc[k]);
      penalty_elem<HAS_F>(gv[k].z, pv[k].z, av[k].z, fv[k].z, strength, acc[k]);
      penalty_elem<HAS_F>(gv[k].w, pv[k].w, av[k].w, fv[k].w, strength, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < PEN_UNROLL; ++k)
      if (i + k * stride < n4) reinterpret_cast<float4*>(g)[i + k * stride] = gv[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)                       // the n % 4 elements behind the last whole group
    for (long j = n4 * 4; j < n; ++j) {
      float gj = g[j];
      penalty_elem<HAS_F>(gj, p[j], anchor[j], HAS_F ? F[j] : 0.f, strength, acc[0]);
      g[j] = gj;
    }
  const float s = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

static inline unsigned flat_blocks(long n) {
  long nb = (n / 4 + 255) / 256;
  return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
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

extern "C" size_t cxrk_ewc_penalty_partials_bytes(long n) { return cxrk_grad_sqnorm_partials_bytes(n); }

extern "C" int cxrk_ewc_penalty(float* g, const float* p, const float* anchor, const float* F, long n, float strength, float* partials,
                                size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(g && p && anchor && n > 0);
  CXRK_CHECK_ARG(aligned16(g) && aligned16(p) && aligned16(anchor) && aligned16(F));
  const long nb = (long)(cxrk_grad_sqnorm_partials_bytes(n) / sizeof(float));   // one partition for both reductions
  if (partials == nullptr || ws_bytes < (size_t)nb * sizeof(float)) return CXRK_ERR_WS;
  if (F != nullptr)
    hipLaunchKernelGGL(ewc_penalty_kernel<true>, dim3((unsigned)nb), dim3(PEN_THREADS), 0, stream, g, p, anchor, F, n, strength, partials);
  else
    hipLaunchKernelGGL(ewc_penalty_kernel<false>, dim3((unsigned)nb), dim3(PEN_THREADS), 0, stream, g, p, anchor, F, n, strength, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
