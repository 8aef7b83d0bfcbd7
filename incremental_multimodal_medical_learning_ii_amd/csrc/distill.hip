// Similarity distillation head: on a student logits block S[rows][cols] and the frozen teacher's block St of the same
// shape,
//  * row statistics: lse of both rows and KL(softmax(St_i) || softmax(S_i)) in ONE pass over the two rows, + the fixed-order loss sum
//  * the in-place gradient transform  S <- (softmax_row(S) - softmax_row(St)) + (softmax_col(S) - softmax_col(St))
// Exact fp32 (no GEMM here), one 256-thread block per row, no scratch memory, no atomics.
#include "cxrk.h"
#include "cxrk_common.h"

using namespace cxrk;

namespace {

// Per-thread running (max, sum of exp(x - max)) of a strided part of one row: RowAcc of loss.hip without the positives.  The student's
// and the teacher's row go through THIS code, so bit-identical rows give bit-identical sums, maxima and log-sum-exps.
struct LseAcc {
  float m = -INFINITY, s = 0.f;
  // raise the running maximum to mx >= m; returns the factor the sums taken against the old maximum shrink by.  (m = -inf: s is 0
  // and stays 0.)  A NaN takes the maximum over and stays, as in RowAcc::rescale: torch.logsumexp gives NaN for such a row.
  __device__ __forceinline__ float rescale(float mx) {
    if (mx > m || mx != mx) { const float f = expf(m - mx); s *= f; m = mx; return f; }
    return 1.f;
  }
  __device__ __forceinline__ float add(float x) { const float e = expf(x - m); s += e; return e; }
};

// block-wide merge in a fixed order: block maximum, then the sums rescaled to it -> the log-sum-exp; `scale` = the factor that
// carries this thread's sums to the block maximum
__device__ __forceinline__ float merge_lse(const LseAcc& a, float* sh, float& scale, float& total) {
  const float M = block_max(a.m, sh);
  scale = a.m == -INFINITY ? 0.f : expf(a.m - M);
  total = block_sum(a.m == -INFINITY ? 0.f : a.s * scale, sh);
  return M + logf(total);
}

// lse[i], lse_t[i] and kl[i] = sum_j pt_ij (St_ij - S_ij) + (lse_i - lse_t_i), pt = softmax of the teacher's row.  The weighted sum is
// carried against the teacher's running maximum next to its sum of exponentials, so each row is read once.  Every summand holds the
// factor (St_ij - S_ij) and the tail is a difference of two log-sum-exps formed by the same code: bit-identical rows give exactly 0.
// VEC: 16-byte loads (ld % 4 == 0, ldt % 4 == 0, both bases 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void distill_row_stats_kernel(const float* __restrict__ S, long ld, const float* __restrict__ St,
                                                                long ldt, int cols, float* __restrict__ lse,
                                                                float* __restrict__ lse_t, float* __restrict__ kl) {
  __shared__ float sh[16];
  const long row = blockIdx.x;
  const float* s = S + row * ld;
  const float* t = St + row * ldt;
  LseAcc a, b;       // student, teacher
  float w = 0.f;     // sum of exp(St - b.m) * (St - S)
  int tail = 0;
  if (VEC) {
    tail = cols & ~3;
    for (int j = threadIdx.x * 4; j < tail; j += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(s + j);
      const f32x4 u = *reinterpret_cast<const f32x4*>(t + j);
      a.rescale(max_keep_nan(max_keep_nan(v[0], v[1]), max_keep_nan(v[2], v[3])));   // fmaxf would skip a NaN lane
      w *= b.rescale(max_keep_nan(max_keep_nan(u[0], u[1]), max_keep_nan(u[2], u[3])));
#pragma unroll
      for (int q = 0; q < 4; ++q) { a.add(v[q]); w += b.add(u[q]) * (u[q] - v[q]); }
    }
  }
  for (int j = tail + threadIdx.x; j < cols; j += 256) {
    const float x = s[j], y = t[j];
    a.rescale(x);
    w *= b.rescale(y);
    a.add(x);
    w += b.add(y) * (y - x);
  }
  float fa, fb, sum_a, sum_b;
  const float la = merge_lse(a, sh, fa, sum_a);
  const float lb = merge_lse(b, sh, fb, sum_b);
  const float W = block_sum(b.m == -INFINITY ? 0.f : w * fb, sh);
  if (threadIdx.x == 0) { lse[row] = la; lse_t[row] = lb; kl[row] = W / sum_b + (la - lb); }
}

// out[0] (+)= scale * sum kl[0..n); single block, fixed order.
__global__ __launch_bounds__(256) void distill_loss_kernel(const float* __restrict__ kl, int n, float scale, float* __restrict__ out,
                                                           int accumulate) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += kl[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}

// one element of the gradient block: student - teacher per direction, so bit-identical inputs give exactly 0
__device__ __forceinline__ float distill_grad(float x, float y, float lr, float ltr, float lc, float ltc) {
  return (expf(x - lr) - expf(y - ltr)) + (expf(x - lc) - expf(y - ltc));
}

// In place on S; St is read only.  One block per row, a thread owns groups of 4 consecutive columns 1024 apart.
template <bool VEC>
__global__ __launch_bounds__(256) void distill_grad_kernel(float* __restrict__ S, long ld, const float* __restrict__ St, long ldt,
                                                           int cols, const float* __restrict__ lse_row,
                                                           const float* __restrict__ lse_col, const float* __restrict__ lse_t_row,
                                                           const float* __restrict__ lse_t_col) {
  const long i = blockIdx.x;
  float* s = S + i * ld;
  const float* t = St + i * ldt;
  const float lr = lse_row[i], ltr = lse_t_row[i];
  int tail = 0;
  if (VEC) {
    tail = cols & ~3;
    for (int j = threadIdx.x * 4; j < tail; j += 1024) {
      f32x4 v = *reinterpret_cast<const f32x4*>(s + j);
      const f32x4 u = *reinterpret_cast<const f32x4*>(t + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = distill_grad(v[q], u[q], lr, ltr, lse_col[j + q], lse_t_col[j + q]);
      *reinterpret_cast<f32x4*>(s + j) = v;
    }
  }
  for (int j = tail + threadIdx.x; j < cols; j += 256) s[j] = distill_grad(s[j], t[j], lr, ltr, lse_col[j], lse_t_col[j]);
}

}  // namespace

extern "C" int cxrk_distill_row_stats(const float* S, long ld, const float* St, long ldt, int rows, int cols, float* lse, float* lse_t,
                                      float* kl, float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream) {
  CXRK_CHECK_ARG(S && St && lse && lse_t && kl && rows > 0 && cols > 0 && ld >= cols && ldt >= cols);
  if (ld % 4 == 0 && ldt % 4 == 0 && aligned16(S) && aligned16(St))
    hipLaunchKernelGGL(distill_row_stats_kernel<true>, dim3(rows), dim3(256), 0, stream, S, ld, St, ldt, cols, lse, lse_t, kl);
  else
    hipLaunchKernelGGL(distill_row_stats_kernel<false>, dim3(rows), dim3(256), 0, stream, S, ld, St, ldt, cols, lse, lse_t, kl);
  CXRK_LAUNCH_CHECK();
  if (loss_out) {
    hipLaunchKernelGGL(distill_loss_kernel, dim3(1), dim3(256), 0, stream, kl, rows, loss_scale, loss_out, loss_accumulate);
    CXRK_LAUNCH_CHECK();
  }
  return CXRK_OK;
}

extern "C" int cxrk_distill_grad_inplace(float* S, long ld, const float* St, long ldt, int rows, int cols, const float* lse_row,
                                         const float* lse_col, const float* lse_t_row, const float* lse_t_col, hipStream_t stream) {
  CXRK_CHECK_ARG(S && St && S != St && lse_row && lse_col && lse_t_row && lse_t_col && rows > 0 && cols > 0 && ld >= cols && ldt >= cols);
  if (ld % 4 == 0 && ldt % 4 == 0 && aligned16(S) && aligned16(St))
    hipLaunchKernelGGL(distill_grad_kernel<true>, dim3(rows), dim3(256), 0, stream, S, ld, St, ldt, cols, lse_row, lse_col, lse_t_row,
                       lse_t_col);
  else
    hipLaunchKernelGGL(distill_grad_kernel<false>, dim3(rows), dim3(256), 0, stream, S, ld, St, ldt, cols, lse_row, lse_col, lse_t_row,
                       lse_t_col);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
