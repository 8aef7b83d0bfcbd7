// Similarity + loss heads.
//  * L2 row normalisation fwd/bwd (F.normalize semantics, eps on the norm)
//  * InfoNCE pieces on a materialised logits block S[B][Bg] (the logits GEMMs run on the shared MFMA mainloop):
//    row log-sum-exp + diagonal pick, and the in-place softmax-gradient transform; their multi-positive (keyed) forms; and the
//    forms with a learnable temperature (device logit scale, fused d theta partial sums)
//  * pairwise sigmoid loss on the same block: forward, gradient and the partial sums of loss / d theta / d b in one pass
//  * torchmetrics-style pairwise cosine fwd/bwd (reference Trainer.myCosineSimilarity, Trainer.py:1682-1704)
//  * pos-neg logits + BCE-with-logits(mean) fwd+bwd in one pass (Trainer.py:575-583, ZERO_JOINT_BOUNDS.py:36)
//  * eval scoring (Trainer.py:797-837)
#include "cxrk.h"
#include "cxrk_common.h"
#include "flat_buffers.h"

using namespace cxrk;

namespace {

// one wave per row; D <= 64*8
constexpr int NV = 8;

__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, long rows, int D, float eps,
                                                         float* __restrict__ xhat, long ldh, float* __restrict__ norm) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float v[NV]; float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const int c = lane + i * 64; v[i] = c < D ? x[row * D + c] : 0.f; q += v[i] * v[i]; }
  const float n_raw = sqrtf(wave_sum(q));
  const float n = n_raw < eps ? eps : n_raw;   // clamp_min by comparison: a NaN norm stays NaN (fmaxf would return eps), as F.normalize
  const float inv = 1.0f / n;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const int c = lane + i * 64; if (c < D) xhat[row * ldh + c] = v[i] * inv; }
  if (lane == 0 && norm) norm[row] = n;
}

// dx = (dxhat - xhat * <xhat, dxhat>) / norm
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dxhat, const float* __restrict__ xhat, long ldh,
                                                         const float* __restrict__ norm, long rows, int D,
                                                         float* __restrict__ dx) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float g[NV], h[NV]; float dot = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + i * 64;
    g[i] = c < D ? dxhat[row * D + c] : 0.f; h[i] = c < D ? xhat[row * ldh + c] : 0.f; dot += g[i] * h[i];
  }
  dot = wave_sum(dot);
  const float inv = 1.0f / norm[row];
#pragma unroll
  for (int i = 0; i < NV; ++i) { const int c = lane + i * 64; if (c < D) dx[row * D + c] = (g[i] - h[i] * dot) * inv; }
}

// lse[i] = log sum_j exp(S[i][j]); diag[i] = S[i][diag_off + i]; one 256-thread block per row.
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ S, long ld, int cols, int diag_off,
                                                      float* __restrict__ lse, float* __restrict__ diag) {
  __shared__ float sh[16];
  const long row = blockIdx.x;
  const float* s = S + row * ld;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < cols; j += 256) m = fmaxf(m, s[j]);
  m = block_max(m, sh);
  float sum = 0.f;
  for (int j = threadIdx.x; j < cols; j += 256) sum += expf(s[j] - m);
  sum = block_sum(sum, sh);
  if (threadIdx.x == 0) { lse[row] = m + logf(sum); diag[row] = s[diag_off + row]; }
}

// G[i][j] = exp(S[i][j]-lse_row[i]) + exp(S[i][j]-lse_col[j]) - 2*[j == diag_off+i], in place.
__global__ void infonce_grad_kernel(float* __restrict__ S, long ld, long rows, int cols, int diag_off,
                                    const float* __restrict__ lse_row, const float* __restrict__ lse_col) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * cols) return;
  const long i = t / cols; const int j = (int)(t - i * cols);
  const float s = S[i * ld + j];
  float g = expf(s - lse_row[i]) + expf(s - lse_col[j]);
  if (j == diag_off + (int)i) g -= 2.f;
  S[i * ld + j] = g;
}

// sum_i (lse[i] - diag[i]) * scale  -> out[0] (+= when accumulate); single block.
__global__ void lse_loss_kernel(const float* __restrict__ lse, const float* __restrict__ diag, int n, float scale,
                                float* __restrict__ out, int accumulate) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += lse[i] - diag[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}

// ---------------------------------------------------------------------------------------------------------------
// multi-positive InfoNCE: the positives of row i are the columns whose 64-bit key equals the row's.
// ---------------------------------------------------------------------------------------------------------------
// Per-thread running (max, sum of exp(x - max)) over a strided part of one row, with the matching columns' sum and count.
struct RowAcc {
  float m = -INFINITY, s = 0.f, pos = 0.f; int n = 0;
  __device__ __forceinline__ void rescale(float mx) {   // raise the running maximum to mx >= m
    // (m = -inf: s is 0 and stays 0.)  A NaN takes the maximum over and stays: a thread whose only elements are NaN would otherwise
    // keep m = -inf, and the merge below drops the sums of such threads (torch.logsumexp gives NaN for the row).
    if (mx > m || mx != mx) { s *= expf(m - mx); m = mx; }
  }
  __device__ __forceinline__ void add(float x, bool match) {
    s += expf(x - m);
    if (match) { pos += x; ++n; }
  }
};

// lse[i] = log sum_j exp(S[i][j]); posmean[i] = mean of S[i][j] over keys_col[j] == keys_row[i]; npos[i] = their number.
// One 256-thread block per row, ONE pass over the row; VEC: 16-byte loads of S (ld % 4 == 0, base 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void multipos_row_stats_kernel(const float* __restrict__ S, long ld, int cols,
                                                                 const long long* __restrict__ keys_row,
                                                                 const long long* __restrict__ keys_col, float* __restrict__ lse,
                                                                 float* __restrict__ posmean, float* __restrict__ npos) {
  __shared__ float sh[16];
  __shared__ int shn[4];
  const long row = blockIdx.x;
  const float* s = S + row * ld;
  const long long kr = keys_row[row];
  RowAcc a;
  int tail = 0;
  if (VEC) {
    tail = cols & ~3;
    for (int j = threadIdx.x * 4; j < tail; j += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(s + j);
      a.rescale(max_keep_nan(max_keep_nan(v[0], v[1]), max_keep_nan(v[2], v[3])));   // fmaxf would skip a NaN lane: see RowAcc::rescale
#pragma unroll
      for (int q = 0; q < 4; ++q) a.add(v[q], keys_col[j + q] == kr);
    }
  }
  for (int j = tail + threadIdx.x; j < cols; j += 256) { const float x = s[j]; a.rescale(x); a.add(x, keys_col[j] == kr); }
  // merge in a fixed order: block maximum, then the sums rescaled to it
  const float M = block_max(a.m, sh);
  const float sum = block_sum(a.m == -INFINITY ? 0.f : a.s * expf(a.m - M), sh);
  const float pos = block_sum(a.pos, sh);
  int n = a.n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) shn[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    n = (shn[0] + shn[1]) + (shn[2] + shn[3]);
    lse[row] = M + logf(sum);
    posmean[row] = n > 0 ? pos / (float)n : 0.f;
    npos[row] = (float)n;
  }
}

// G[i][j] = exp(S[i][j]-lse_row[i]) + exp(S[i][j]-lse_col[j]) - 2*[keys_row[i] == keys_col[j]] / n_row[i], in place.
// grid (rows, ceil(cols / 1024)); a thread owns 4 consecutive columns: one 16-byte load / store where VEC allows, else scalar.
template <bool VEC>
__global__ __launch_bounds__(256) void multipos_grad_kernel(float* __restrict__ S, long ld, int cols,
                                                            const long long* __restrict__ keys_row,
                                                            const long long* __restrict__ keys_col, const float* __restrict__ n_row,
                                                            const float* __restrict__ lse_row, const float* __restrict__ lse_col) {
  const long i = blockIdx.x;
  const int j0 = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (j0 >= cols) return;
  float* s = S + i * ld;
  const long long kr = keys_row[i];
  const float lr = lse_row[i], w = 2.f / n_row[i];
  if (VEC && j0 + 4 <= cols) {
    f32x4 v = *reinterpret_cast<const f32x4*>(s + j0);
    const f32x4 lc = *reinterpret_cast<const f32x4*>(lse_col + j0);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = expf(v[q] - lr) + expf(v[q] - lc[q]) - (keys_col[j0 + q] == kr ? w : 0.f);
    *reinterpret_cast<f32x4*>(s + j0) = v;
  } else {
    const int j1 = min(j0 + 4, cols);
    for (int j = j0; j < j1; ++j) { const float x = s[j]; s[j] = expf(x - lr) + expf(x - lse_col[j]) - (keys_col[j] == kr ? w : 0.f); }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// learnable temperature: the block holds the unscaled cosines C, the logits are x = s * c with s = exp(theta), theta on the device.
// ---------------------------------------------------------------------------------------------------------------
// RowAcc in cosine space: s > 0, so the row maximum of x is s * (the maximum of c).  M = fl(s * mc) is the offset every exponent of the
// row is taken against with ONE rounding, fma(s, c, -M); M's own rounding cancels in lse = M + log(sum).
struct ScaledRowAcc {
  float mc = -INFINITY, M = -INFINITY, s = 0.f, pos = 0.f; int n = 0;
  __device__ __forceinline__ void rescale(float c, float sc) {
    if (c > mc || c != c) { const float Mn = sc * c; s *= expf(M - Mn); mc = c; M = Mn; }   // (M = -inf: s is 0 and stays 0; NaN as in RowAcc)
  }
  __device__ __forceinline__ void add(float c, float sc, bool match) {
    s += expf(fmaf(sc, c, -M));
    if (match) { pos += sc * c; ++n; }
  }
};

// multipos_row_stats_kernel on x = exp(*log_scale) * C.  KEYED: positives by key; else the one positive of row i is column
// diag_off + i (posmean = the diagonal logit, npos unused).  One pass over the row in both forms.
template <bool VEC, bool KEYED>
__global__ __launch_bounds__(256) void scaled_row_stats_kernel(const float* __restrict__ C, long ld, int cols, int diag_off,
                                                               const long long* __restrict__ keys_row,
                                                               const long long* __restrict__ keys_col,
                                                               const float* __restrict__ log_scale, float* __restrict__ lse,
                                                               float* __restrict__ posmean, float* __restrict__ npos) {
  __shared__ float sh[16];
  __shared__ int shn[4];
  const long row = blockIdx.x;
  const float* c = C + row * ld;
  const float sc = expf(log_scale[0]);
  const long long kr = KEYED ? keys_row[row] : 0;
  const int dcol = diag_off + (int)row;
  ScaledRowAcc a;
  int tail = 0;
  if (VEC) {
    tail = cols & ~3;
    for (int j = threadIdx.x * 4; j < tail; j += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(c + j);
      a.rescale(max_keep_nan(max_keep_nan(v[0], v[1]), max_keep_nan(v[2], v[3])), sc);
#pragma unroll
      for (int q = 0; q < 4; ++q) a.add(v[q], sc, KEYED ? keys_col[j + q] == kr : j + q == dcol);
    }
  }
  for (int j = tail + threadIdx.x; j < cols; j += 256) {
    const float x = c[j];
    a.rescale(x, sc);
    a.add(x, sc, KEYED ? keys_col[j] == kr : j == dcol);
  }
  // merge in a fixed order: block maximum, then the sums rescaled to it
  const float M = block_max(a.M, sh);
  const float sum = block_sum(a.M == -INFINITY ? 0.f : a.s * expf(a.M - M), sh);
  const float pos = block_sum(a.pos, sh);
  int n = a.n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) shn[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    n = (shn[0] + shn[1]) + (shn[2] + shn[3]);
    lse[row] = M + logf(sum);
    posmean[row] = n > 0 ? pos / (float)n : 0.f;
    if (KEYED) npos[row] = (float)n;
  }
}

// In place on C, with x = s * c:  g = exp(x-lse_row[i]) + exp(x-lse_col[j]) - 2*[positive(i,j)] / n_i;  C[i][j] <- s * g, and
// part[i * gridDim.y + chunk] = sum over the chunk's columns of g * x (block_sum: fixed order).  grid (rows, ceil(cols / 1024)), a
// thread owns 4 consecutive columns as in multipos_grad_kernel.  No thread leaves before the block sum.
template <bool VEC, bool KEYED>
__global__ __launch_bounds__(256) void scaled_grad_kernel(float* __restrict__ C, long ld, int cols, int diag_off,
                                                          const long long* __restrict__ keys_row,
                                                          const long long* __restrict__ keys_col, const float* __restrict__ n_row,
                                                          const float* __restrict__ lse_row, const float* __restrict__ lse_col,
                                                          const float* __restrict__ log_scale, float* __restrict__ part) {
  __shared__ float sh[16];
  const long i = blockIdx.x;
  const int j0 = (blockIdx.y * 256 + threadIdx.x) * 4;
  float* c = C + i * ld;
  const float sc = expf(log_scale[0]);
  const long long kr = KEYED ? keys_row[i] : 0;
  const int dcol = diag_off + (int)i;
  const float lr = lse_row[i], w = KEYED ? 2.f / n_row[i] : 2.f;
  float acc = 0.f;
  if (VEC && j0 + 4 <= cols) {
    f32x4 v = *reinterpret_cast<const f32x4*>(c + j0);
    const f32x4 lc = *reinterpret_cast<const f32x4*>(lse_col + j0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool match = KEYED ? keys_col[j0 + q] == kr : j0 + q == dcol;
      const float g = expf(fmaf(sc, v[q], -lr)) + expf(fmaf(sc, v[q], -lc[q])) - (match ? w : 0.f);
      acc += g * (sc * v[q]);
      v[q] = sc * g;
    }
    *reinterpret_cast<f32x4*>(c + j0) = v;
  } else if (j0 < cols) {
    const int j1 = min(j0 + 4, cols);
    for (int j = j0; j < j1; ++j) {
      const float x = c[j];
      const bool match = KEYED ? keys_col[j] == kr : j == dcol;
      const float g = expf(fmaf(sc, x, -lr)) + expf(fmaf(sc, x, -lse_col[j])) - (match ? w : 0.f);
      acc += g * (sc * x);
      c[j] = sc * g;
    }
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) part[i * gridDim.y + blockIdx.y] = acc;
}

// dtheta[0] (+)= upstream[0] * scale * (sum part1 + sum part2); single block, fixed order.
__global__ __launch_bounds__(256) void logit_scale_grad_kernel(const float* __restrict__ part1, long n1,
                                                               const float* __restrict__ part2, long n2,
                                                               const float* __restrict__ upstream, float scale,
                                                               float* __restrict__ dtheta, int accumulate) {
  __shared__ float sh[16];
  const float s1 = block_fold(part1, n1, sh);
  const float s = s1 + block_fold(part2, n2, sh);
  if (threadIdx.x == 0) { const float v = upstream[0] * scale * s; dtheta[0] = accumulate ? dtheta[0] + v : v; }
}

// ---------------------------------------------------------------------------------------------------------------
// pairwise sigmoid loss: every (row, column) pair is a binary problem on x = fma(t, c, b), t = exp(theta); theta and b on the device.
// ---------------------------------------------------------------------------------------------------------------
// One element: l = softplus(-x) for a positive pair, softplus(x) otherwise; g = dl/dx = -sigmoid(-x) or sigmoid(x).  With
// e = exp(-|x|) and r = 1 / (1 + e):  softplus(y) = max(y, 0) + log1p(e),  sigmoid(x) = x >= 0 ? r : e * r.  The positive branch is
// -sigmoid(-x), never sigmoid(x) - 1 (which cancels to 0 from x ~ 17 on).  A NaN x makes e, and so l and g, NaN.
template <bool SUMS>
__device__ __forceinline__ float sigmoid_pair(float t, float cv, float b, bool pos, float& sl, float& sgx, float& sg) {
  const float x = fmaf(t, cv, b);
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  const float er = e * r;
  const float g = pos ? -(x >= 0.f ? er : r) : (x >= 0.f ? r : er);
  if (SUMS) {
    const float y = pos ? -x : x;
    sl += (y > 0.f ? y : 0.f) + log1pf(e);
    sgx += g * (t * cv);
    sg += g;
  }
  return t * g;
}

// In place on C: C[i][j] <- t * g_ij.  grid (rows, ceil(cols / 1024)), a thread owns 4 consecutive columns as in scaled_grad_kernel.
// SUMS: part holds three planes of gridDim.x * gridDim.y floats (sum l, sum g * (t c), sum g); entry [i * gridDim.y + chunk] of each is
// the block_sum (fixed order) over the chunk's columns of row i.  No thread leaves before the block sums.
template <bool VEC, bool KEYED, bool SUMS>
__global__ __launch_bounds__(256) void sigmoid_pairs_kernel(float* __restrict__ C, long ld, int cols, int diag_off,
                                                            const long long* __restrict__ keys_row,
                                                            const long long* __restrict__ keys_col,
                                                            const float* __restrict__ log_scale, const float* __restrict__ bias,
                                                            float* __restrict__ part) {
  __shared__ float sh[16];
  const long i = blockIdx.x;
  const int j0 = (blockIdx.y * 256 + threadIdx.x) * 4;
  float* c = C + i * ld;
  const float t = expf(log_scale[0]), b = bias[0];
  const long long kr = KEYED ? keys_row[i] : 0;
  const int dcol = diag_off + (int)i;
  float sl = 0.f, sgx = 0.f, sg = 0.f;
  if (VEC && j0 + 4 <= cols) {
    f32x4 v = *reinterpret_cast<const f32x4*>(c + j0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[q] = sigmoid_pair<SUMS>(t, v[q], b, KEYED ? keys_col[j0 + q] == kr : j0 + q == dcol, sl, sgx, sg);
    *reinterpret_cast<f32x4*>(c + j0) = v;
  } else if (j0 < cols) {
    const int j1 = min(j0 + 4, cols);
    for (int j = j0; j < j1; ++j) c[j] = sigmoid_pair<SUMS>(t, c[j], b, KEYED ? keys_col[j] == kr : j == dcol, sl, sgx, sg);
  }
  if (SUMS) {
    const long plane = (long)gridDim.x * gridDim.y, at = i * gridDim.y + blockIdx.y;
    sl = block_sum(sl, sh);
    sgx = block_sum(sgx, sh);
    sg = block_sum(sg, sh);
    if (threadIdx.x == 0) { part[at] = sl; part[plane + at] = sgx; part[2 * plane + at] = sg; }
  }
}

// out[0] (+)= scale * sum part[0..n); single block, fixed order.  The last launch of the sigmoid loss and of the BCE loss.
__global__ __launch_bounds__(256) void scaled_fold_kernel(const float* __restrict__ part, long n, float scale,
                                                          float* __restrict__ out, int accumulate) {
  __shared__ float sh[16];
  const float s = block_fold(part, n, sh);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}

// x <- min(max(x, lo), hi) by comparisons, which are false for a NaN: a NaN stays a NaN (fminf / fmaxf would return the bound).
__global__ void clamp_kernel(float* __restrict__ x, long n, float lo, float hi) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  x[i] = v < lo ? lo : (v > hi ? hi : v);
}

// ---------------------------------------------------------------------------------------------------------------
// pairwise cosine: cos[i][p] = <x_i, y_p> / (|x_i| |y_p|)  (no epsilon: torchmetrics semantics)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pairwise_cosine_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  long B, int P, int D, float* __restrict__ cosv,
                                                                  float* __restrict__ xnorm, float* __restrict__ ynorm, int Pg,
                                                                  float* __restrict__ maxv, float* __restrict__ meanv,
                                                                  int* __restrict__ argmax) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int lane = threadIdx.x & 63;
  float v[NV]; float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const int c = lane + i * 64; v[i] = c < D ? x[row * D + c] : 0.f; q += v[i] * v[i]; }
  const float xn = sqrtf(wave_sum(q));
  if (lane == 0) xnorm[row] = xn;
  float gmax = 0.f, gsum = 0.f; int gidx = 0;
  for (int p = 0; p < P; ++p) {
    float d = 0.f, yy = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + i * 64;
      const float w = c < D ? y[(long)p * D + c] : 0.f;
      d += v[i] * w; yy += w * w;
    }
    d = wave_sum(d); yy = sqrtf(wave_sum(yy));
    const float c = (d / xn) / yy;
    if (lane == 0) { cosv[row * P + p] = c; if (row == 0) ynorm[p] = yy; }
    if (Pg > 0) {   // max (first winner, torch.max on ties) and mean over the Pg prompts of group p / Pg  (Trainer.py:1691-1693)
      const int j = p % Pg;
      if (j == 0) { gmax = c; gsum = c; gidx = 0; }
      else { gsum += c; if (c > gmax || (c != c && gmax == gmax)) { gmax = c; gidx = j; } }
      if (j == Pg - 1 && lane == 0) {
        const long o = row * (P / Pg) + p / Pg;
        maxv[o] = gmax; meanv[o] = gsum / (float)Pg; argmax[o] = gidx;
      }
    }
  }
}

// sim[r] = <patch_r, text>: the patch-wise similarity GEMV of vlp/inference_engine.py:104 (one wave per patch row).
__global__ __launch_bounds__(256) void rows_dot_kernel(const float* __restrict__ x, const float* __restrict__ t, long R, int D,
                                                       float* __restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  float d = 0.f;
  for (int c = lane; c < D; c += 64) d += x[row * D + c] * t[c];
  d = wave_sum(d);
  if (lane == 0) out[row] = d;
}

// dx_i = sum_p dc[i][p] * (yhat_p - cos*xhat_i)/|x_i| ; dy partial[blk][p] = sum_{i in blk} dc * (xhat_i - cos*yhat_p)/|y_p|
// One launch covers the prompt columns [p0, p0 + Pc) of the P (the LDS accumulators hold Pc x D per wave; the host walks P in
// chunks that fit): cosv / dcos rows are P wide, y / ynorm are indexed by the global prompt, dy_part is [blocks][Pc][D], and a
// launch with p0 > 0 adds its part of dx to what the earlier chunks wrote.
__global__ __launch_bounds__(256) void pairwise_cosine_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ cosv, const float* __restrict__ dcos,
                                                                  const float* __restrict__ xnorm, const float* __restrict__ ynorm,
                                                                  long B, int P, int p0, int Pc, int D, int rows_per,
                                                                  float* __restrict__ dx, float* __restrict__ dy_part, int Pg,
                                                                  const int* __restrict__ argmax) {
  extern __shared__ float sm[];  // [4 waves][Pc][D]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* mine = sm + (long)w * Pc * D;
  for (int i = lane; i < Pc * D; i += 64) mine[i] = 0.f;
  const long r0 = (long)blockIdx.x * rows_per, r1 = min(B, r0 + rows_per);
  for (long row = r0 + w; row < r1; row += 4) {
    float xh[NV], acc[NV];
    const float ixn = 1.0f / xnorm[row];
#pragma unroll
    for (int i = 0; i < NV; ++i) { const int c = lane + i * 64; xh[i] = c < D ? x[row * D + c] * ixn : 0.f; acc[i] = 0.f; }
    for (int pl = 0; pl < Pc; ++pl) {
      const int p = p0 + pl;
      float dc;   // Pg > 0: dcos is [B, P / Pg], the gradient of the group maximum, routed to the winner only
      if (Pg > 0) { const long o = row * (P / Pg) + p / Pg; dc = argmax[o] == p % Pg ? dcos[o] : 0.f; }
      else dc = dcos[row * P + p];
      const float cs = cosv[row * P + p];
      const float iyn = 1.0f / ynorm[p];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + i * 64;
        if (c < D) {
          const float yh = y[(long)p * D + c] * iyn;
          acc[i] += dc * (yh - cs * xh[i]);
          mine[pl * D + c] += dc * (xh[i] - cs * yh) * iyn;
        }
      }
    }
    if (dx) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + i * 64;
        if (c < D) dx[row * D + c] = (p0 > 0 ? dx[row * D + c] : 0.f) + acc[i] * ixn;
      }
    }
  }
  __syncthreads();
  const long n = (long)Pc * D;
  for (int i = threadIdx.x; i < n; i += 256)
    dy_part[(long)blockIdx.x * n + i] = (sm[i] + sm[n + i]) + (sm[2 * n + i] + sm[3 * n + i]);
}
__global__ void partial_reduce_kernel(const float* __restrict__ part, int nparts, long n, float* __restrict__ out, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < nparts; ++p) s += part[(long)p * n + i];
  out[i] = accumulate ? out[i] + s : s;
}

// logits[i][c] = cos[i][2c] - cos[i][2c+1] (diff) or cos[i][2c]; loss = mean BCEWithLogits; dcos = dloss/dcos.
// Single-pass: per-block partial loss sums, finished by lse-style final kernel.
__global__ __launch_bounds__(256) void bce_posneg_kernel(const float* __restrict__ cosv, const float* __restrict__ labels,
                                                         long B, int C, int ldlab, int diff, float* __restrict__ logits,
                                                         float* __restrict__ dcos, float* __restrict__ part) {
  __shared__ float sh[16];
  const long n = B * C;
  const float invn = 1.0f / (float)n;
  float ls = 0.f;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
    const long i = t / C; const int c = (int)(t - i * C);
    const float cp = cosv[i * 2 * C + 2 * c], cn = cosv[i * 2 * C + 2 * c + 1];
    const float z = diff ? cp - cn : cp;
    const float yv = labels[i * ldlab + c];
    // max(z,0) - z*y + log1p(exp(-|z|))
    ls += fmaxf(z, 0.f) - z * yv + log1pf(expf(-fabsf(z)));
    if (logits) logits[t] = z;
    if (dcos) {
      const float sg = 1.0f / (1.0f + expf(-z));
      const float dz = (sg - yv) * invn;
      dcos[i * 2 * C + 2 * c] = dz;
      dcos[i * 2 * C + 2 * c + 1] = diff ? -dz : 0.f;
    }
  }
  ls = block_sum(ls, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = ls;
}

// Trainer.val scoring: score = (pos+1)/2 or (pos-neg+2)/4; pred = argmax([neg,pos]) ; logit diff kept for the BCE log.
__global__ void eval_score_kernel(const float* __restrict__ cosv, long B, int C, int pred_diff, float* __restrict__ score,
                                  float* __restrict__ pred) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * C) return;
  const long i = t / C; const int c = (int)(t - i * C);
  const float cp = cosv[i * 2 * C + 2 * c], cn = cosv[i * 2 * C + 2 * c + 1];
  score[t] = pred_diff ? (cp - cn + 2.f) * 0.25f : (cp + 1.f) * 0.5f;
  pred[t] = cp > cn ? 1.f : 0.f;
}

// prompt-group mean: out[g][d] = mean_n in[g][n][d]  and its backward
__global__ void group_mean_fwd_kernel(const float* __restrict__ in, int G, int n, int D, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G * D) return;
  const int g = t / D, d = t - g * D;
  float s = 0.f;
  for (int k = 0; k < n; ++k) s += in[((long)g * n + k) * D + d];
  out[t] = s / (float)n;
}
__global__ void group_mean_bwd_kernel(const float* __restrict__ dout, int G, int n, int D, float* __restrict__ din) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G * n * D) return;
  const int d = t % D; const int g = t / (n * D);
  din[t] = dout[g * D + d] / (float)n;
}

// out = alpha * (alpha_dev ? *alpha_dev : 1) * x * (mask_src ? mask_src > 0 : 1)
__global__ void scale_mask_kernel(const float* __restrict__ x, const float* __restrict__ mask_src,
                                  const float* __restrict__ alpha_dev, float alpha, long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = alpha_dev ? alpha * alpha_dev[0] : alpha;
  float v = a * x[i];
  if (mask_src) v = mask_src[i] > 0.f ? v : 0.f;
  out[i] = v;
}

}  // namespace

extern "C" int cxrk_scale_mask(const float* x, const float* mask_src, const float* alpha_dev, float alpha, long n,
                               float* out, hipStream_t stream) {
  CXRK_CHECK_ARG(x && out && n > 0);
  hipLaunchKernelGGL(scale_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, mask_src, alpha_dev, alpha, n, out);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_l2norm_fwd(const float* x, long rows, int D, float eps, float* xhat, long ldxhat, float* norm, hipStream_t stream) {
  CXRK_CHECK_ARG(x && xhat && rows > 0 && D > 0 && D <= 64 * NV && ldxhat >= D);
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, rows, D, eps, xhat, ldxhat, norm);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
extern "C" int cxrk_l2norm_bwd(const float* dxhat, const float* xhat, long ldxhat, const float* norm, long rows, int D, float* dx,
                               hipStream_t stream) {
  CXRK_CHECK_ARG(dxhat && xhat && norm && dx && rows > 0 && D > 0 && D <= 64 * NV && ldxhat >= D);
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, dxhat, xhat, ldxhat, norm, rows, D, dx);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_infonce_row_lse(const float* S, long ld, int rows, int cols, int diag_off, float* lse, float* diag,
                                    float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream) {
  CXRK_CHECK_ARG(S && lse && diag && rows > 0 && cols > 0 && diag_off >= 0 && diag_off + rows <= cols);
  hipLaunchKernelGGL(row_lse_kernel, dim3(rows), dim3(256), 0, stream, S, ld, cols, diag_off, lse, diag);
  CXRK_LAUNCH_CHECK();
  if (loss_out) {
    hipLaunchKernelGGL(lse_loss_kernel, dim3(1), dim3(256), 0, stream, lse, diag, rows, loss_scale, loss_out, loss_accumulate);
    CXRK_LAUNCH_CHECK();
  }
  return CXRK_OK;
}

extern "C" int cxrk_infonce_grad_inplace(float* S, long ld, int rows, int cols, int diag_off, const float* lse_row,
                                         const float* lse_col, hipStream_t stream) {
  CXRK_CHECK_ARG(S && lse_row && lse_col && rows > 0 && cols > 0);
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(infonce_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, S, ld, (long)rows, cols,
                     diag_off, lse_row, lse_col);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_multipos_row_stats(const float* S, long ld, int rows, int cols, const long long* keys_row,
                                       const long long* keys_col, float* lse, float* posmean, float* npos, float* loss_out,
                                       float loss_scale, int loss_accumulate, hipStream_t stream) {
  CXRK_CHECK_ARG(S && keys_row && keys_col && lse && posmean && npos && rows > 0 && cols > 0 && ld >= cols);
  if (ld % 4 == 0 && aligned16(S))
    hipLaunchKernelGGL(multipos_row_stats_kernel<true>, dim3(rows), dim3(256), 0, stream, S, ld, cols, keys_row, keys_col, lse, posmean, npos);
  else
    hipLaunchKernelGGL(multipos_row_stats_kernel<false>, dim3(rows), dim3(256), 0, stream, S, ld, cols, keys_row, keys_col, lse, posmean, npos);
  CXRK_LAUNCH_CHECK();
  if (loss_out) {   // sum_i (lse[i] - posmean[i]) * scale, one block, fixed order
    hipLaunchKernelGGL(lse_loss_kernel, dim3(1), dim3(256), 0, stream, lse, posmean, rows, loss_scale, loss_out, loss_accumulate);
    CXRK_LAUNCH_CHECK();
  }
  return CXRK_OK;
}

extern "C" int cxrk_multipos_grad_inplace(float* S, long ld, int rows, int cols, const long long* keys_row,
                                          const long long* keys_col, const float* n_row, const float* lse_row,
                                          const float* lse_col, hipStream_t stream) {
  CXRK_CHECK_ARG(S && keys_row && keys_col && n_row && lse_row && lse_col && rows > 0 && cols > 0 && ld >= cols);
  const dim3 grid(rows, (unsigned)((cols + 1023) / 1024));
  if (ld % 4 == 0 && aligned16(S) && aligned16(lse_col))
    hipLaunchKernelGGL(multipos_grad_kernel<true>, grid, dim3(256), 0, stream, S, ld, cols, keys_row, keys_col, n_row, lse_row, lse_col);
  else
    hipLaunchKernelGGL(multipos_grad_kernel<false>, grid, dim3(256), 0, stream, S, ld, cols, keys_row, keys_col, n_row, lse_row, lse_col);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

// learnable temperature: one templated pair of kernels serves the plain (KEYED = false) and the keyed entry points
template <bool KEYED>
static int scaled_row_stats(const float* C, long ld, int rows, int cols, int diag_off, const long long* keys_row,
                            const long long* keys_col, const float* log_scale, float* lse, float* posmean, float* npos,
                            float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream) {
  if (ld % 4 == 0 && aligned16(C))
    hipLaunchKernelGGL((scaled_row_stats_kernel<true, KEYED>), dim3(rows), dim3(256), 0, stream, C, ld, cols, diag_off, keys_row,
                       keys_col, log_scale, lse, posmean, npos);
  else
    hipLaunchKernelGGL((scaled_row_stats_kernel<false, KEYED>), dim3(rows), dim3(256), 0, stream, C, ld, cols, diag_off, keys_row,
                       keys_col, log_scale, lse, posmean, npos);
  CXRK_LAUNCH_CHECK();
  if (loss_out) {   // sum_i (lse[i] - posmean[i]) * scale, one block, fixed order
    hipLaunchKernelGGL(lse_loss_kernel, dim3(1), dim3(256), 0, stream, lse, posmean, rows, loss_scale, loss_out, loss_accumulate);
    CXRK_LAUNCH_CHECK();
  }
  return CXRK_OK;
}

template <bool KEYED>
static int scaled_grad(float* C, long ld, int rows, int cols, int diag_off, const long long* keys_row, const long long* keys_col,
                       const float* n_row, const float* lse_row, const float* lse_col, const float* log_scale, float* partials,
                       hipStream_t stream) {
  const dim3 grid(rows, (unsigned)((cols + 1023) / 1024));
  if (ld % 4 == 0 && aligned16(C) && aligned16(lse_col))
    hipLaunchKernelGGL((scaled_grad_kernel<true, KEYED>), grid, dim3(256), 0, stream, C, ld, cols, diag_off, keys_row, keys_col, n_row,
                       lse_row, lse_col, log_scale, partials);
  else
    hipLaunchKernelGGL((scaled_grad_kernel<false, KEYED>), grid, dim3(256), 0, stream, C, ld, cols, diag_off, keys_row, keys_col, n_row,
                       lse_row, lse_col, log_scale, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_infonce_row_lse_scaled(const float* C, long ld, int rows, int cols, int diag_off, const float* log_scale,
                                           float* lse, float* diag, float* loss_out, float loss_scale, int loss_accumulate,
                                           hipStream_t stream) {
  CXRK_CHECK_ARG(C && log_scale && lse && diag && rows > 0 && cols > 0 && ld >= cols && diag_off >= 0 && diag_off + rows <= cols);
  return scaled_row_stats<false>(C, ld, rows, cols, diag_off, nullptr, nullptr, log_scale, lse, diag, nullptr, loss_out, loss_scale,
                                 loss_accumulate, stream);
}

extern "C" int cxrk_infonce_grad_scaled_inplace(float* C, long ld, int rows, int cols, int diag_off, const float* lse_row,
                                                const float* lse_col, const float* log_scale, float* partials, hipStream_t stream) {
  CXRK_CHECK_ARG(C && lse_row && lse_col && log_scale && partials && rows > 0 && cols > 0 && ld >= cols && diag_off >= 0 &&
                 diag_off + rows <= cols);
  return scaled_grad<false>(C, ld, rows, cols, diag_off, nullptr, nullptr, nullptr, lse_row, lse_col, log_scale, partials, stream);
}

extern "C" int cxrk_multipos_row_stats_scaled(const float* C, long ld, int rows, int cols, const long long* keys_row,
                                              const long long* keys_col, const float* log_scale, float* lse, float* posmean,
                                              float* npos, float* loss_out, float loss_scale, int loss_accumulate,
                                              hipStream_t stream) {
  CXRK_CHECK_ARG(C && keys_row && keys_col && log_scale && lse && posmean && npos && rows > 0 && cols > 0 && ld >= cols);
  return scaled_row_stats<true>(C, ld, rows, cols, 0, keys_row, keys_col, log_scale, lse, posmean, npos, loss_out, loss_scale,
                                loss_accumulate, stream);
}

extern "C" int cxrk_multipos_grad_scaled_inplace(float* C, long ld, int rows, int cols, const long long* keys_row,
                                                 const long long* keys_col, const float* n_row, const float* lse_row,
                                                 const float* lse_col, const float* log_scale, float* partials,
                                                 hipStream_t stream) {
  CXRK_CHECK_ARG(C && keys_row && keys_col && n_row && lse_row && lse_col && log_scale && partials && rows > 0 && cols > 0 &&
                 ld >= cols);
  return scaled_grad<true>(C, ld, rows, cols, 0, keys_row, keys_col, n_row, lse_row, lse_col, log_scale, partials, stream);
}

extern "C" int cxrk_logit_scale_grad(const float* partials1, long n1, const float* partials2, long n2, const float* upstream,
                                     float scale, float* dtheta, int accumulate, hipStream_t stream) {
  CXRK_CHECK_ARG(partials1 && n1 > 0 && n2 >= 0 && (partials2 || n2 == 0) && upstream && dtheta);
  hipLaunchKernelGGL(logit_scale_grad_kernel, dim3(1), dim3(256), 0, stream, partials1, n1, partials2, n2, upstream, scale, dtheta,
                     accumulate);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

template <bool KEYED, bool SUMS>
static int sigmoid_pairs(float* C, long ld, int rows, int cols, int diag_off, const long long* keys_row, const long long* keys_col,
                         const float* log_scale, const float* bias, float* partials, hipStream_t stream) {
  const dim3 grid(rows, (unsigned)((cols + 1023) / 1024));
  if (ld % 4 == 0 && aligned16(C))
    hipLaunchKernelGGL((sigmoid_pairs_kernel<true, KEYED, SUMS>), grid, dim3(256), 0, stream, C, ld, cols, diag_off, keys_row, keys_col,
                       log_scale, bias, partials);
  else
    hipLaunchKernelGGL((sigmoid_pairs_kernel<false, KEYED, SUMS>), grid, dim3(256), 0, stream, C, ld, cols, diag_off, keys_row, keys_col,
                       log_scale, bias, partials);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_sigmoid_pairs_fwd_bwd_inplace(float* C, long ld, int rows, int cols, int diag_off, const long long* keys_row,
                                                  const long long* keys_col, const float* log_scale, const float* bias,
                                                  float* partials, hipStream_t stream) {
  CXRK_CHECK_ARG(C && log_scale && bias && rows > 0 && cols > 0 && ld >= cols && (keys_row == nullptr) == (keys_col == nullptr));
  if (keys_row) {
    return partials ? sigmoid_pairs<true, true>(C, ld, rows, cols, 0, keys_row, keys_col, log_scale, bias, partials, stream)
                    : sigmoid_pairs<true, false>(C, ld, rows, cols, 0, keys_row, keys_col, log_scale, bias, nullptr, stream);
  }
  CXRK_CHECK_ARG(diag_off >= 0 && diag_off + rows <= cols);
  return partials ? sigmoid_pairs<false, true>(C, ld, rows, cols, diag_off, nullptr, nullptr, log_scale, bias, partials, stream)
                  : sigmoid_pairs<false, false>(C, ld, rows, cols, diag_off, nullptr, nullptr, log_scale, bias, nullptr, stream);
}

extern "C" int cxrk_sigmoid_pairs_loss(const float* partials, long n, float scale, float* loss_out, int accumulate,
                                       hipStream_t stream) {
  CXRK_CHECK_ARG(partials && n > 0 && loss_out);
  hipLaunchKernelGGL(scaled_fold_kernel, dim3(1), dim3(256), 0, stream, partials, n, scale, loss_out, accumulate);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_clamp_inplace(float* x, long n, float lo, float hi, hipStream_t stream) {
  CXRK_CHECK_ARG(x && n > 0 && lo <= hi);   // (a NaN bound fails lo <= hi)
  hipLaunchKernelGGL(clamp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, lo, hi);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_pairwise_cosine_fwd(const float* x, const float* y, long B, int P, int D, float* cosv, float* xnorm,
                                        float* ynorm, hipStream_t stream) {
  CXRK_CHECK_ARG(x && y && cosv && xnorm && ynorm && B > 0 && P > 0 && D > 0 && D <= 64 * NV);
  hipLaunchKernelGGL(pairwise_cosine_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, x, y, B, P, D, cosv, xnorm, ynorm,
                     0, nullptr, nullptr, nullptr);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_patch_similarity(const float* patches, const float* text, long R, int D, float* sim, hipStream_t stream) {
  CXRK_CHECK_ARG(patches && text && sim && R > 0 && D > 0);
  hipLaunchKernelGGL(rows_dot_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, patches, text, R, D, sim);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_pairwise_cosine_max_fwd(const float* x, const float* y, long B, int G, int Pg, int D, float* cosv, float* xnorm,
                                            float* ynorm, float* maxv, float* meanv, int* argmax, hipStream_t stream) {
  CXRK_CHECK_ARG(x && y && cosv && xnorm && ynorm && maxv && meanv && argmax && B > 0 && G > 0 && Pg > 0 && D > 0 && D <= 64 * NV);
  hipLaunchKernelGGL(pairwise_cosine_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, x, y, B, G * Pg, D, cosv, xnorm,
                     ynorm, Pg, maxv, meanv, argmax);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

static int cos_bwd_blocks(long B) { long nb = (B + 63) / 64; if (nb > 512) nb = 512; if (nb < 1) nb = 1; return (int)nb; }
extern "C" size_t cxrk_pairwise_cosine_bwd_ws_bytes(long B, int P, int D) { return (size_t)cos_bwd_blocks(B) * P * D * sizeof(float); }

static int cosine_bwd(const float* x, const float* y, const float* cosv, const float* dcos, const float* xnorm, const float* ynorm, long B,
                      int P, int D, float* dx, float* dy, int accumulate_dy, float* ws, size_t ws_bytes, int Pg, const int* argmax,
                      hipStream_t stream) {
  CXRK_CHECK_ARG(x && y && cosv && dcos && xnorm && ynorm && dy && B > 0 && P > 0 && D > 0 && D <= 64 * NV);
  // one [Pc][D] accumulator per wave in LDS: P is walked in chunks of at most 64 KiB / (4 waves x D x 4 B) prompts (32 at D = 128;
  // NEW_PROMPTS with positive-only logits stacks 5 classes x 2 x 10 = 100 prompt rows into one call, Trainer.py:1691-1693)
  int pc_max = (int)((64 * 1024) / ((size_t)4 * D * sizeof(float)));
  if (pc_max < 1) return CXRK_ERR_UNSUPPORTED;
  int nb = cos_bwd_blocks(B);
  CXRK_CHECK_WS(ws, ws_bytes, (size_t)nb * P * D * sizeof(float));
  const int rows_per = (int)((B + nb - 1) / nb);
  nb = (int)((B + rows_per - 1) / rows_per);
  for (int p0 = 0; p0 < P; p0 += pc_max) {
    const int Pc = P - p0 < pc_max ? P - p0 : pc_max;
    const size_t sh = (size_t)4 * Pc * D * sizeof(float);
    hipLaunchKernelGGL(pairwise_cosine_bwd_kernel, dim3(nb), dim3(256), sh, stream, x, y, cosv, dcos, xnorm, ynorm, B, P, p0, Pc, D,
                       rows_per, dx, ws, Pg, argmax);
    CXRK_LAUNCH_CHECK();
    const long n = (long)Pc * D;   // (the chunk's partials are consumed before the next launch overwrites them: same stream)
    hipLaunchKernelGGL(partial_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, nb, n, dy + (long)p0 * D,
                       accumulate_dy);
    CXRK_LAUNCH_CHECK();
  }
  return CXRK_OK;
}

extern "C" int cxrk_pairwise_cosine_bwd(const float* x, const float* y, const float* cosv, const float* dcos,
                                        const float* xnorm, const float* ynorm, long B, int P, int D, float* dx, float* dy,
                                        int accumulate_dy, float* ws, size_t ws_bytes, hipStream_t stream) {
  return cosine_bwd(x, y, cosv, dcos, xnorm, ynorm, B, P, D, dx, dy, accumulate_dy, ws, ws_bytes, 0, nullptr, stream);
}

extern "C" int cxrk_pairwise_cosine_max_bwd(const float* x, const float* y, const float* cosv, const float* dmax, const int* argmax,
                                            const float* xnorm, const float* ynorm, long B, int G, int Pg, int D, float* dx, float* dy,
                                            int accumulate_dy, float* ws, size_t ws_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(argmax && G > 0 && Pg > 0);
  return cosine_bwd(x, y, cosv, dmax, xnorm, ynorm, B, G * Pg, D, dx, dy, accumulate_dy, ws, ws_bytes, Pg, argmax, stream);
}

extern "C" size_t cxrk_bce_posneg_ws_bytes(void) { return 256 * sizeof(float); }

extern "C" int cxrk_bce_posneg_fwd_bwd(const float* cosv, const float* labels, long B, int C, int ldlab, int diff,
                                       float* logits, float* dcos, float* loss, float* ws, size_t ws_bytes,
                                       hipStream_t stream) {
  CXRK_CHECK_ARG(cosv && labels && loss && B > 0 && C > 0 && ldlab >= C);
  CXRK_CHECK_WS(ws, ws_bytes, 256 * sizeof(float));
  long nb = (B * C + 255) / 256; if (nb > 256) nb = 256;
  hipLaunchKernelGGL(bce_posneg_kernel, dim3((unsigned)nb), dim3(256), 0, stream, cosv, labels, B, C, ldlab, diff, logits, dcos, ws);
  CXRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(scaled_fold_kernel, dim3(1), dim3(256), 0, stream, ws, nb, 1.0f / (float)(B * C), loss, 0);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_eval_score(const float* cosv, long B, int C, int pred_diff, float* score, float* pred, hipStream_t stream) {
  CXRK_CHECK_ARG(cosv && score && pred && B > 0 && C > 0);
  const long n = B * C;
  hipLaunchKernelGGL(eval_score_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cosv, B, C, pred_diff, score, pred);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_group_mean_fwd(const float* in, int G, int n, int D, float* out, hipStream_t stream) {
  CXRK_CHECK_ARG(in && out && G > 0 && n > 0 && D > 0);
  hipLaunchKernelGGL(group_mean_fwd_kernel, dim3((unsigned)((G * D + 255) / 256)), dim3(256), 0, stream, in, G, n, D, out);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
extern "C" int cxrk_group_mean_bwd(const float* dout, int G, int n, int D, float* din, hipStream_t stream) {
  CXRK_CHECK_ARG(dout && din && G > 0 && n > 0 && D > 0);
  hipLaunchKernelGGL(group_mean_bwd_kernel, dim3((unsigned)((G * n * D + 255) / 256)), dim3(256), 0, stream, dout, G, n, D, din);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
