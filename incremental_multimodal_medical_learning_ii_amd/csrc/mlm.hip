// Masked-language-modelling auxiliary loss of the joint step (include/cxrk.h, "mlm"):
//  * token masking on the device: HF DataCollatorForLanguageModeling's rule drawn with the counter-based Philox of dropout.h, and the
//    selected tokens compacted in ascending token order (per-block counts, then a fixed-order prefix: no atomic decides an order)
//  * gather of the selected rows of the last hidden state / scatter of their gradient back (plain stores: no token is listed twice)
//  * the vocabulary cross-entropy over a logits block that only ever holds a CHUNK of the vocabulary: per-(row, lane) running
//    (max, sum-exp, argmax) folded chunk by chunk, a finishing pass, and the gradient transform of a recomputed chunk
// Row-reduction and element-wise kernels: exact fp32, one wave per row for the statistics, 16-byte accesses, no scratch memory, no
// atomics.  Every kernel reads the number of rows that count (`kept`) from device memory.
#include "cxrk.h"
#include "cxrk_common.h"
#include "dropout.h"

using namespace cxrk;

namespace {

constexpr unsigned MLM_T80 = 3435973837u;   // ceil(0.8 * 2^32): word 1 below it -> the mask token
constexpr unsigned MLM_T90 = 3865470567u;   // ceil(0.9 * 2^32): word 1 below it -> a random id; else the token keeps its id

struct MlmKey {
  unsigned k0, k1, c3;              // seed low / high word; (call counter & 0xffffff) << 8 | 0xF4
  unsigned long long sel_thresh;    // selected iff word 0 < round(p * 2^32)  (2^32 at p = 1)
  long row_offset;                  // global sequence index of the call's first sequence
  int L;
  long V, mask_id;
  int nspecial;
  long special[8];
};

// the draw of token i of the call (sequence i / L, token i % L): selected?  `newid` = what the encoder reads at that position
__device__ __forceinline__ bool mlm_draw(const MlmKey& k, long i, long id, bool attended, long& newid) {
  newid = id;
  bool cand = attended;
#pragma unroll
  for (int q = 0; q < 8; ++q) cand = cand && !(q < k.nspecial && id == k.special[q]);
  if (!cand) return false;
  const unsigned n = (unsigned)(k.row_offset + i / k.L), t = (unsigned)(i % k.L);
  const uint4 r = philox4x32_10(make_uint4(0u, n, t, k.c3), k.k0, k.k1);
  if ((unsigned long long)r.x >= k.sel_thresh) return false;
  if (r.y < MLM_T80) newid = k.mask_id;
  else if (r.y < MLM_T90) newid = (long)(((unsigned long long)r.z * (unsigned long long)k.V) >> 32);
  return true;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block_counts[b] = selected tokens among tokens [256 b, 256 (b + 1))
__global__ __launch_bounds__(256) void mlm_count_kernel(const long* __restrict__ ids, const long* __restrict__ mask, long T, MlmKey key,
                                                        int* __restrict__ block_counts) {
  __shared__ int sh[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool s = false;
  if (i < T) { long nid; s = mlm_draw(key, i, ids[i], mask ? mask[i] != 0 : true, nid); }
  const int c = __popcll(__ballot(s));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// ids_out, and the compact list: the k-th selected token in token order goes to slot k while k < cap.  The last block also writes
// stats = {kept, selected}, count_f = float(kept), and -1 into the unused slots [kept, cap).
__global__ __launch_bounds__(256) void mlm_place_kernel(const long* __restrict__ ids, const long* __restrict__ mask, long T, MlmKey key,
                                                        const int* __restrict__ block_counts, int cap, long* __restrict__ ids_out,
                                                        int* __restrict__ sel, int* __restrict__ tgt, int* __restrict__ stats,
                                                        float* __restrict__ count_f) {
  __shared__ int sh[4], shw[4];
  int part = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) part += block_counts[b];
  part = wave_sum_i(part);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = part;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool s = false;
  long id = 0, nid = 0;
  if (i < T) { id = ids[i]; s = mlm_draw(key, i, id, mask ? mask[i] != 0 : true, nid); ids_out[i] = nid; }
  const unsigned long long bal = __ballot(s);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) shw[w] = __popcll(bal);
  __syncthreads();
  const int base = sh[0] + sh[1] + sh[2] + sh[3];
  int woff = 0;
  for (int q = 0; q < w; ++q) woff += shw[q];
  const int pos = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
  if (s && pos < cap) { sel[pos] = (int)i; tgt[pos] = (int)id; }
  if (blockIdx.x == gridDim.x - 1) {
    const int total = base + shw[0] + shw[1] + shw[2] + shw[3];
    const int kept = total < cap ? total : cap;
    if (threadIdx.x == 0) { stats[0] = kept; stats[1] = total; count_f[0] = (float)kept; }
    for (int q = kept + threadIdx.x; q < cap; q += 256) { sel[q] = -1; tgt[q] = -1; }
  }
}

__device__ __forceinline__ int kept_rows(const int* stats, int rows) {
  const int k = stats[0];
  return k < 0 ? 0 : (k > rows ? rows : k);
}

// out[r] = last[sel[r]] for r < kept, zero otherwise; one wave per row.  PL: the output is a planes tensor.
template <bool PL>
__global__ __launch_bounds__(256) void mlm_gather_kernel(const float* __restrict__ last, long T, int H, const int* __restrict__ sel,
                                                         const int* __restrict__ stats, int cap, void* __restrict__ out, long plane) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= cap) return;
  const int kept = kept_rows(stats, cap);
  const long t = r < kept ? sel[r] : -1;
  const bool live = t >= 0 && t < T;
  const float* src = last + (live ? t : 0) * (long)H;
  if (PL) {
    unsigned short* o = static_cast<unsigned short*>(out);
    for (int j = lane * 8; j < H; j += 512) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + j), b = *reinterpret_cast<const f32x4*>(src + j + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
      }
      planes_store8(o, plane, (long)r * H + j, v);
    }
  } else {
    float* o = static_cast<float*>(out) + (long)r * H;
    for (int j = lane * 4; j < H; j += 256) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (live) a = *reinterpret_cast<const f32x4*>(src + j);
      *reinterpret_cast<f32x4*>(o + j) = a;
    }
  }
}

// dlast[sel[r]] = dx[r] for r < kept (dlast zeroed by the caller; sel holds no token twice: plain stores); one wave per row
__global__ __launch_bounds__(256) void mlm_scatter_kernel(const float* __restrict__ dx, const int* __restrict__ sel,
                                                          const int* __restrict__ stats, int cap, long T, int H, float* __restrict__ dlast) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= kept_rows(stats, cap)) return;
  const long t = sel[r];
  if (t < 0 || t >= T) return;
  const float* s = dx + (long)r * H;
  float* d = dlast + t * (long)H;
  for (int j = lane * 4; j < H; j += 256) *reinterpret_cast<f32x4*>(d + j) = *reinterpret_cast<const f32x4*>(s + j);
}

// Running statistics of one (row, lane): online (max, sum of exp(x - max)) as LseAcc of distill.hip, and the first maximum.
struct LaneAcc {
  float m, s, bv;
  int bi;
  __device__ __forceinline__ void rescale(float mx) {       // a NaN takes the maximum over and stays
    if (mx > m || mx != mx) { s *= expf(m - mx); m = mx; }
  }
  __device__ __forceinline__ void add(float x, int col) {
    s += expf(x - m);
    if (bi < 0 || x > bv || (x != x && bv == bv)) { bv = x; bi = col; }   // strict >: the first maximum; a NaN wins once
  }
};

// One wave per row, rows >= kept untouched.  The block holds columns [v0, v0 + cols) of the vocabulary, of which the first `skip`
// are not counted (they belong to the chunk before).  Lane l folds, in ascending order, the groups of four columns whose ABSOLUTE
// group index (column / 4) is congruent to l mod 64 into state[.][row][l]: the sequence a lane sees does not depend on where the
// chunk boundaries lie (as long as they are multiples of 4), so neither do its sums.  VEC = false: column by column, lane =
// absolute column mod 64 (the unaligned tail chunk).  x = S + bias[column]; the target's logit goes to tl[row].
template <bool VEC>
__global__ __launch_bounds__(256) void mlm_xent_stats_kernel(const float* __restrict__ S, long ld, int rows, int cols, int skip, int v0,
                                                             const float* __restrict__ bias, const int* __restrict__ tgt,
                                                             const int* __restrict__ stats, float* __restrict__ state,
                                                             float* __restrict__ tl, int first) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= kept_rows(stats, rows)) return;
  const long plane = (long)rows * 64, at = (long)r * 64 + lane;
  LaneAcc a;
  if (first) { a.m = -INFINITY; a.s = 0.f; a.bv = -INFINITY; a.bi = -1; }
  else { a.m = state[at]; a.s = state[plane + at]; a.bv = state[2 * plane + at]; a.bi = __builtin_bit_cast(int, state[3 * plane + at]); }
  const float* s = S + (long)r * ld;
  const int target = tgt[r];
  if (VEC) {
    const int g0 = (lane - ((v0 >> 2) & 63) + 64) & 63;
    for (int j = g0 * 4; j < cols; j += 256) {
      f32x4 v = *reinterpret_cast<const f32x4*>(s + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += bias[v0 + j + q];
      a.rescale(max_keep_nan(max_keep_nan(v[0], v[1]), max_keep_nan(v[2], v[3])));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a.add(v[q], v0 + j + q);
        if (v0 + j + q == target) tl[r] = v[q];
      }
    }
  } else {
    const int j0 = skip + ((lane - ((v0 + skip) & 63) + 64) & 63);
    for (int j = j0; j < cols; j += 64) {
      const float x = s[j] + bias[v0 + j];
      a.rescale(x);
      a.add(x, v0 + j);
      if (v0 + j == target) tl[r] = x;
    }
  }
  state[at] = a.m; state[plane + at] = a.s; state[2 * plane + at] = a.bv; state[3 * plane + at] = __builtin_bit_cast(float, a.bi);
}

// Per row: the 64 lanes merged in a fixed butterfly -> lse, lse - target logit, argmax == target; rows >= kept get zeros.
__global__ __launch_bounds__(256) void mlm_xent_rows_kernel(const float* __restrict__ state, const float* __restrict__ tl,
                                                            const int* __restrict__ tgt, const int* __restrict__ stats, int rows,
                                                            float* __restrict__ lse, float* __restrict__ rowloss, int* __restrict__ hit) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  if (r >= kept_rows(stats, rows)) {
    if (lane == 0) { lse[r] = 0.f; rowloss[r] = 0.f; hit[r] = 0; }
    return;
  }
  const long plane = (long)rows * 64, at = (long)r * 64 + lane;
  const float m = state[at], s = state[plane + at];
  float bv = state[2 * plane + at];
  int bi = __builtin_bit_cast(int, state[3 * plane + at]);
  float M = m;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = max_keep_nan(M, __shfl_xor(M, o, 64));
  const float total = wave_sum(m == -INFINITY ? 0.f : s * expf(m - M));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    bool take;       // is the other lane's candidate the better one?  (symmetric: both lanes of a pair decide alike)
    if (oi < 0) take = false;
    else if (bi < 0) take = true;
    else if (ov != ov || bv != bv) take = (ov != ov) && (bv == bv || oi < bi);
    else take = ov > bv || (ov == bv && oi < bi);
    if (take) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
    const float l = M + logf(total);
    lse[r] = l;
    rowloss[r] = l - tl[r];
    hit[r] = bi == tgt[r] ? 1 : 0;
  }
}

// loss_out = (sum of rowloss[0..kept)) * scale[0], correct_out = sum of hit[0..kept); one block, fixed order
__global__ __launch_bounds__(256) void mlm_xent_loss_kernel(const float* __restrict__ rowloss, const int* __restrict__ hit,
                                                            const int* __restrict__ stats, int rows, const float* __restrict__ scale,
                                                            float* __restrict__ loss_out, int* __restrict__ correct_out) {
  __shared__ float sh[16];
  __shared__ int shi[4];
  const int kept = kept_rows(stats, rows);
  float s = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < kept; i += 256) { s += rowloss[i]; c += hit[i]; }
  s = block_sum(s, sh);
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) { loss_out[0] = s * scale[0]; correct_out[0] = shi[0] + shi[1] + shi[2] + shi[3]; }
}

// The recomputed chunk -> its gradient: g = (exp(x - lse[r]) - [column == tgt[r]]) * f for r < kept and column >= skip, else 0, with
// x = S + bias[column] and f = upstream[0] * scale[0] * alpha.  PL: written as planes to G (ldg, gplane); otherwise in place.
// Block (r, y) takes columns [4096 y, 4096 (y + 1)) of row r in groups of 8.
template <bool PL>
__global__ __launch_bounds__(256) void mlm_xent_grad_kernel(float* __restrict__ S, long ld, unsigned short* __restrict__ G, long ldg,
                                                            long gplane, int rows, int cols, int skip, int v0,
                                                            const float* __restrict__ bias, const int* __restrict__ tgt,
                                                            const int* __restrict__ stats, const float* __restrict__ lse,
                                                            const float* __restrict__ upstream, const float* __restrict__ scale,
                                                            float alpha) {
  const int r = blockIdx.x;
  const bool live = r < kept_rows(stats, rows);
  const float f = upstream[0] * scale[0] * alpha;
  const float l = live ? lse[r] : 0.f;
  const int target = live ? tgt[r] : -1;
  float* s = S + (long)r * ld;
  const int hi = min(cols, ((int)blockIdx.y + 1) * 4096);
  for (int j = blockIdx.y * 4096 + threadIdx.x * 8; j < hi; j += 2048) {
    float v[8];
    if (live) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(s + j), b = *reinterpret_cast<const f32x4*>(s + j + 4);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float x = (q < 4 ? a[q & 3] : b[q & 3]) + bias[v0 + j + q];
        v[q] = j + q < skip ? 0.f : (expf(x - l) - (v0 + j + q == target ? 1.f : 0.f)) * f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = 0.f;
    }
    if (PL) {
      planes_store8(G, gplane, (long)r * ldg + j, v);
    } else {
      *reinterpret_cast<f32x4*>(s + j) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(s + j + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
  }
}

}  // namespace

extern "C" int cxrk_mlm_mask_tokens(const long* ids, const long* mask, int N, int L, long row_offset, unsigned long long seed,
                                    unsigned counter, double p, long V, long mask_id, const long* special, int nspecial, int cap,
                                    long* ids_out, int* sel, int* tgt, int* stats, float* count_f, int* block_counts,
                                    hipStream_t stream) {
  CXRK_CHECK_ARG(ids && ids_out && sel && tgt && stats && count_f && block_counts && N > 0 && L > 0 && cap > 0 && row_offset >= 0);
  CXRK_CHECK_ARG(p >= 0.0 && p <= 1.0 && V > 0 && V < (1L << 31) && mask_id >= 0 && mask_id < V && nspecial >= 0 && nspecial <= 8 &&
                 (nspecial == 0 || special));
  const long T = (long)N * L;
  CXRK_CHECK_ARG(T < (1L << 31) && cap <= T);
  MlmKey key;
  key.k0 = (unsigned)(seed & 0xffffffffull); key.k1 = (unsigned)(seed >> 32);
  key.c3 = ((counter & 0xffffffu) << 8) | 0xF4u;
  key.sel_thresh = (unsigned long long)(p * 4294967296.0 + 0.5);
  key.row_offset = row_offset; key.L = L; key.V = V; key.mask_id = mask_id; key.nspecial = nspecial;
  for (int q = 0; q < 8; ++q) key.special[q] = q < nspecial ? special[q] : -1;
  const unsigned nb = (unsigned)((T + 255) / 256);
  hipLaunchKernelGGL(mlm_count_kernel, dim3(nb), dim3(256), 0, stream, ids, mask, T, key, block_counts);
  CXRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(mlm_place_kernel, dim3(nb), dim3(256), 0, stream, ids, mask, T, key, block_counts, cap, ids_out, sel, tgt, stats,
                     count_f);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_mlm_gather_rows(const float* last, long T, int H, const int* sel, const int* stats, int cap, void* out, long plane,
                                    hipStream_t stream) {
  CXRK_CHECK_ARG(last && sel && stats && out && T > 0 && H > 0 && cap > 0 && plane >= 0 && aligned16(last) && aligned16(out));
  CXRK_CHECK_ARG(plane > 0 ? (H % 8 == 0 && plane % 8 == 0 && plane >= (long)cap * H) : H % 4 == 0);
  if (plane > 0)
    hipLaunchKernelGGL(mlm_gather_kernel<true>, dim3(ceil_div(cap, 4)), dim3(256), 0, stream, last, T, H, sel, stats, cap, out, plane);
  else
    hipLaunchKernelGGL(mlm_gather_kernel<false>, dim3(ceil_div(cap, 4)), dim3(256), 0, stream, last, T, H, sel, stats, cap, out, plane);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_mlm_scatter_rows(const float* dx, const int* sel, const int* stats, int cap, long T, int H, float* dlast,
                                     hipStream_t stream) {
  CXRK_CHECK_ARG(dx && sel && stats && dlast && cap > 0 && T > 0 && H > 0 && H % 4 == 0 && aligned16(dx) && aligned16(dlast));
  hipLaunchKernelGGL(mlm_scatter_kernel, dim3(ceil_div(cap, 4)), dim3(256), 0, stream, dx, sel, stats, cap, T, H, dlast);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_mlm_xent_stats(const float* S, long ld, int rows, int cols, int skip, int v0, const float* bias, const int* tgt,
                                   const int* stats, float* state, float* target_logit, int first, hipStream_t stream) {
  CXRK_CHECK_ARG(S && bias && tgt && stats && state && target_logit && rows > 0 && cols > 0 && ld >= cols && skip >= 0 && skip < cols &&
                 v0 >= 0 && (long)v0 + cols < (1L << 31));
  if (skip == 0 && ld % 4 == 0 && cols % 4 == 0 && v0 % 4 == 0 && aligned16(S))
    hipLaunchKernelGGL(mlm_xent_stats_kernel<true>, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, S, ld, rows, cols, skip, v0, bias,
                       tgt, stats, state, target_logit, first);
  else
    hipLaunchKernelGGL(mlm_xent_stats_kernel<false>, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, S, ld, rows, cols, skip, v0, bias,
                       tgt, stats, state, target_logit, first);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_mlm_xent_finish(const float* state, const float* target_logit, const int* tgt, const int* stats, int rows,
                                    const float* scale, float* lse, float* rowloss, int* hit, float* loss_out, int* correct_out,
                                    hipStream_t stream) {
  CXRK_CHECK_ARG(state && target_logit && tgt && stats && scale && lse && rowloss && hit && loss_out && correct_out && rows > 0);
  hipLaunchKernelGGL(mlm_xent_rows_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, state, target_logit, tgt, stats, rows, lse,
                     rowloss, hit);
  CXRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(mlm_xent_loss_kernel, dim3(1), dim3(256), 0, stream, rowloss, hit, stats, rows, scale, loss_out, correct_out);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_mlm_xent_grad(float* S, long ld, void* G, long ldg, long gplane, int rows, int cols, int skip, int v0,
                                  const float* bias, const int* tgt, const int* stats, const float* lse, const float* upstream,
                                  const float* scale, float alpha, hipStream_t stream) {
  CXRK_CHECK_ARG(S && bias && tgt && stats && lse && upstream && scale && rows > 0 && cols > 0 && cols % 8 == 0 && ld >= cols &&
                 ld % 4 == 0 && aligned16(S) && skip >= 0 && skip < cols && v0 >= 0 && (long)v0 + cols < (1L << 31));
  const dim3 grid(rows, ceil_div(cols, 4096));
  if (G) {
    CXRK_CHECK_ARG(ldg >= cols && ldg % 8 == 0 && gplane % 8 == 0 && gplane >= (long)(rows - 1) * ldg + cols && aligned16(G));
    hipLaunchKernelGGL(mlm_xent_grad_kernel<true>, grid, dim3(256), 0, stream, S, ld, static_cast<unsigned short*>(G), ldg, gplane, rows,
                       cols, skip, v0, bias, tgt, stats, lse, upstream, scale, alpha);
  } else {
    hipLaunchKernelGGL(mlm_xent_grad_kernel<false>, grid, dim3(256), 0, stream, S, ld, nullptr, 0, 0, rows, cols, skip, v0, bias, tgt,
                       stats, lse, upstream, scale, alpha);
  }
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
