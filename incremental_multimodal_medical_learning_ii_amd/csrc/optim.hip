// Optimiser + continual-learning weight-reset kernels (HBM-bound elementwise / reduction work).
//  * fused Adam, torch.optim.Adam defaults (Trainer.py:172-178): 16 B read + 12 B written per parameter
//  * SGD (Trainer.py:176-178)
//  * global gradient norm (per-block partial sums of g^2, 4 B read per parameter) + AdamW with decoupled masked decay and clipping
//    (torch.optim.AdamW behind torch.nn.utils.clip_grad_norm_): 16.25 B read + 12 B written per parameter
//  * Trainer.myIncremental (Trainer.py:1556-1587): per-tensor min/max of |new-old|, thresholded restore + counters
#include "cxrk.h"
#include "cxrk_common.h"
#include "flat_buffers.h"

using namespace cxrk;

namespace {

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float weight_decay, float bc1, float bc2_sqrt, float grad_scale) {
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gg = gp[k] * grad_scale;
        if (weight_decay != 0.f) gg += weight_decay * pp[k];
        mp[k] = mp[k] + (gg - mp[k]) * (1.f - b1);            // exp_avg.lerp_(grad, 1-beta1)
        vp[k] = vp[k] * b2 + (1.f - b2) * gg * gg;            // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
        const float denom = sqrtf(vp[k]) / bc2_sqrt + eps;
        pp[k] = pp[k] - (lr / bc1) * (mp[k] / denom);         // param.addcdiv_(exp_avg, denom, value=-step_size)
      }
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
    } else {
      for (long j = i; j < n; ++j) {
        float gg = g[j] * grad_scale;
        if (weight_decay != 0.f) gg += weight_decay * p[j];
        const float mm = m[j] + (gg - m[j]) * (1.f - b1);
        const float vv = v[j] * b2 + (1.f - b2) * gg * gg;
        m[j] = mm; v[j] = vv;
        p[j] = p[j] - (lr / bc1) * (mm / (sqrtf(vv) / bc2_sqrt + eps));
      }
    }
  }
}

// ---- global gradient norm + clipped, masked AdamW (include/cxrk.h, "grad_sqnorm" / "adamw_clipped") -------------------
__global__ __launch_bounds__(FLAT_THREADS) void grad_sqnorm_kernel(const float* __restrict__ g, long n, float* __restrict__ part) {
  const float* const in[1] = {g};
  flat_reduce<1, false, 1>(in, nullptr, n, part, [](const float (&v)[1], float&, float (&s)[1]) { s[0] = fmaf(v[0], v[0], s[0]); });
}

// One launch over the flat buffers; adam_kernel's moment / parameter lines in adam_kernel's order, so that with coef = 1 and no
// decay the result is adam_kernel's (weight_decay = 0) bit for bit.  Every block re-derives the squared norm from the partials
// (block_fold), as weight_reset_kernel re-derives its threshold.
__global__ __launch_bounds__(256) void adamw_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const unsigned char* __restrict__ mask, long n,
                                                            float lr, float b1, float b2, float eps, float decay_factor, int decays,
                                                            float bc1, float bc2_sqrt, float grad_scale, float max_norm,
                                                            const float* __restrict__ part, int nparts, float* __restrict__ stats) {
  // The roundings are spelled out: no contraction beyond the fmaf()s below, which are the fused operations of adam_kernel's code
  // (a gradient product fused into gg - m would round differently from adam_kernel, where the L2 branch keeps gg a value of its own).
#pragma clang fp contract(off)
  __shared__ float sh[16];
  float norm = 0.f, coef = 1.f;
  if (part != nullptr) {
    norm = fabsf(grad_scale) * sqrtf(block_fold(part, nparts, sh));
    if (max_norm > 0.f) coef = min_keep_nan(max_norm / (norm + 1e-6f), 1.f);   // clip_grad_norm_'s constants; NaN norm -> NaN
  }
  if (stats != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = norm; stats[1] = coef; }
  const float gs = grad_scale * coef;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    const bool dec = decays && (mask == nullptr || mask[i >> 2] != 0);
    if (i + 3 < n) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = gp[k] * gs;
        if (dec) pp[k] = pp[k] * decay_factor;                    // param.mul_(1 - lr * weight_decay)
        mp[k] = fmaf(1.f - b1, gg - mp[k], mp[k]);
        vp[k] = fmaf(gg, (1.f - b2) * gg, vp[k] * b2);
        const float denom = sqrtf(vp[k]) / bc2_sqrt + eps;
        pp[k] = fmaf(-(lr / bc1), mp[k] / denom, pp[k]);
      }
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
    } else {
      // adam_kernel's tail as it is compiled: its loop runs two elements at a time in the fused forms of the body, and an odd last
      // element with the products of m and v rounded on their own
      const long fused_end = i + ((n - i) & ~1L);
      for (long j = i; j < n; ++j) {
        const float gg = g[j] * gs;
        const float p0 = dec ? p[j] * decay_factor : p[j];
        const float d = gg - m[j], sq = (1.f - b2) * gg;
        const float mm = j < fused_end ? fmaf(1.f - b1, d, m[j]) : m[j] + d * (1.f - b1);
        const float vv = j < fused_end ? fmaf(gg, sq, v[j] * b2) : v[j] * b2 + sq * gg;
        m[j] = mm; v[j] = vv;
        p[j] = fmaf(-(lr / bc1), mm / (sqrtf(vv) / bc2_sqrt + eps), p0);
      }
    }
  }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, long n, float lr, float weight_decay, float grad_scale) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float gg = g[i] * grad_scale;
    if (weight_decay != 0.f) gg += weight_decay * p[i];
    p[i] -= lr * gg;
  }
}

// stage 1: per-block min/max of |a-b|.  A NaN difference makes both NaN, as torch's min() / max() (fminf / fmaxf would skip it):
// the threshold of stage 2 is then NaN, no element is below it, and nothing is restored (Trainer.myIncremental on the same input).
__global__ __launch_bounds__(256) void absdiff_minmax_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                             float* __restrict__ part) {
  __shared__ float sh[16];
  float mn = INFINITY, mx = -INFINITY;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = fabsf(a[i] - b[i]);
    mn = min_keep_nan(mn, d); mx = max_keep_nan(mx, d);
  }
  const int bad = __syncthreads_or(mn != mn);
  mn = block_min(mn, sh); mx = block_max(mx, sh);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = bad ? NAN : mn; part[2 * blockIdx.x + 1] = bad ? NAN : mx; }
}
// stage 2: every block re-derives the threshold from the partials, restores, counts.
__global__ __launch_bounds__(256) void weight_reset_kernel(float* __restrict__ pnew, const float* __restrict__ pold, long n,
                                                           const float* __restrict__ part, int nparts, float threshold,
                                                           unsigned long long* __restrict__ counters) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < nparts; ++i) { mn = min_keep_nan(mn, part[2 * i]); mx = max_keep_nan(mx, part[2 * i + 1]); }
  const float to_reset = mn + threshold * (mx - mn);
  unsigned int cnt = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float o = pold[i];
    const float d = fabsf(pnew[i] - o);
    if (d < to_reset) { pnew[i] = o; ++cnt; }
  }
  __shared__ float sh[16];
  const float tot = block_sum((float)cnt, sh);  // exact below 2^24 per block
  if (threadIdx.x == 0) {
    atomicAdd(&counters[0], (unsigned long long)(tot + 0.5f));
  }
}

}  // namespace

extern "C" int cxrk_adam_fused(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, float grad_scale, hipStream_t stream) {
  CXRK_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
  CXRK_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v));
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                     (float)bc1, (float)sqrt(bc2), grad_scale);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" size_t cxrk_grad_sqnorm_partials_bytes(long n) { return n > 0 ? (size_t)flat_nparts(n) * sizeof(float) : 0; }

extern "C" int cxrk_grad_sqnorm(const float* g, long n, float* partials, size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(g && n > 0 && aligned16(g));
  const long nb = flat_nparts(n);
  if (partials == nullptr || ws_bytes < (size_t)nb * sizeof(float)) return CXRK_ERR_WS;
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nb), dim3(FLAT_THREADS), 0, stream, g, n, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_adamw_clipped(float* p, const float* g, float* m, float* v, const unsigned char* decay_mask, long n, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                  float max_norm, const float* partials, size_t ws_bytes, float* stats, hipStream_t stream) {
  CXRK_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
  CXRK_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v));
  CXRK_CHECK_ARG(partials != nullptr || !(max_norm > 0.f));     // clipping (or monitoring, max_norm = inf) needs the partial sums
  const long np = flat_nparts(n);
  if (partials != nullptr && ws_bytes < (size_t)np * sizeof(float)) return CXRK_ERR_WS;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float decay_factor = (float)(1.0 - (double)lr * (double)weight_decay);
  hipLaunchKernelGGL(adamw_clipped_kernel, dim3(flat_blocks(n)), dim3(256), 0, stream, p, g, m, v, decay_mask, n, lr, beta1, beta2, eps,
                     decay_factor, (int)(weight_decay != 0.f), (float)bc1, (float)sqrt(bc2), grad_scale, max_norm, partials, (int)np,
                     stats);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_sgd(float* p, const float* g, long n, float lr, float weight_decay, float grad_scale, hipStream_t stream) {
  CXRK_CHECK_ARG(p && g && n > 0);
  long nb = (n + 255) / 256; if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)nb), dim3(256), 0, stream, p, g, n, lr, weight_decay, grad_scale);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" size_t cxrk_weight_reset_ws_bytes(void) { return 2 * 256 * sizeof(float); }

// counters[0] += number of restored elements (caller derives updated = n - reset).
extern "C" int cxrk_weight_reset(float* pnew, const float* pold, long n, float threshold, unsigned long long* counters,
                                 float* ws, size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(pnew && pold && counters && n > 0);
  CXRK_CHECK_WS(ws, ws_bytes, 2 * 256 * sizeof(float));
  long nb = (n + 255) / 256; if (nb > 256) nb = 256;
  hipLaunchKernelGGL(absdiff_minmax_kernel, dim3((unsigned)nb), dim3(256), 0, stream, pnew, pold, n, ws);
  CXRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(weight_reset_kernel, dim3((unsigned)nb), dim3(256), 0, stream, pnew, pold, n, ws, (int)nb, threshold, counters);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
