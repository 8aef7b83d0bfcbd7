// Streaming retrieval ranks: for every query row the best positive score and the number of non-positive gallery rows that beat / tie
// it, over the WHOLE gallery, without ever writing the [N][M] similarity block (include/cxrk.h, "retrieval_ranks").
//
// One tile code for everything (retrieval_tile.h, shared with topk.hip): 128 x 128 tiles of the exact-fp32 MFMA, so s(i,j) depends on
// row i of Q and row j of G only.  A lane owns ONE query row per 32-column accumulator and its 16 registers are 16 gallery rows, so
// the per-row state is two registers per lane, not 32.
//   pass 0: the maximum of s over the positives, into `pos` as an order-preserving integer (atomicMax; NaN = INT_MAX wins);
//   pass 1: per row, counts of non-positive columns with s > pos / s == pos, kept in registers over the block's column range and
//           added with integer atomics; a NaN score in a non-positive column sets the sign bit of ties[i];
//   finish: decode pos to fp32; rows with a NaN pos or the sign bit get greater = ties = -1.
#include "cxrk.h"
#include "cxrk_common.h"
#include "retrieval_tile.h"

using namespace cxrk;

namespace {

using namespace cxrk::rtile;

__global__ void retrieval_init_kernel(int* __restrict__ pos_enc, int* __restrict__ greater, int* __restrict__ ties, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) { pos_enc[i] = ENC_NEG_INF; greater[i] = 0; ties[i] = 0; }
}

__global__ void retrieval_finish_kernel(float* __restrict__ pos, int* __restrict__ greater, int* __restrict__ ties, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float p = dec(reinterpret_cast<const int*>(pos)[i]);
  pos[i] = p;
  if (p != p || ties[i] < 0) { greater[i] = -1; ties[i] = -1; }
}

// PASS 0: best positive.  PASS 1: counts.  KEYED: positives by key equality, else column i + diag_off.
// Block (x, y): query strip x; gallery rows [jbeg, jend): tiles_per_block tiles from tile y * tiles_per_block, or, in the pair form of
// pass 0, the one (unaligned) tile that starts at the strip's first positive.
template <int PASS, bool KEYED>
__global__ __launch_bounds__(256) void retrieval_kernel(const float* __restrict__ Q, long ldq, int N, const float* __restrict__ G,
                                                        long ldg, int M, int D, int diag_off,
                                                        const long long* __restrict__ keys_q, const long long* __restrict__ keys_g,
                                                        int* __restrict__ pos_enc, int* __restrict__ greater, int* __restrict__ ties,
                                                        int tiles_per_block) {
  __shared__ float sQ[STAGE_FLOATS];
  __shared__ float sG[STAGE_FLOATS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;   // gallery half / query half of the tile this wave owns (64 x 64)
  const int l31 = lane & 31, h = lane >> 5;
  const long i0 = (long)blockIdx.x * RT;
  long jbeg, jend;
  if (PASS == 0 && !KEYED) { jbeg = i0 + diag_off; jend = jbeg + RT < (long)M ? jbeg + RT : (long)M; }
  else { jbeg = (long)blockIdx.y * tiles_per_block * RT; jend = jbeg + (long)tiles_per_block * RT; if (jend > M) jend = M; }
  if (jbeg >= jend) return;   // block-uniform

  // per-lane state of its two query rows
  long qi[2]; bool qv[2]; long long kq[2]; float p[2]; int best[2], gt[2], eq[2]; bool sawnan[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    qi[n] = i0 + 64 * wn + 32 * n + l31; qv[n] = qi[n] < N;
    kq[n] = (KEYED && qv[n]) ? keys_q[qi[n]] : 0;
    p[n] = (PASS == 1 && qv[n]) ? dec(pos_enc[qi[n]]) : 0.f;
    best[n] = ENC_NEG_INF; gt[n] = 0; eq[n] = 0; sawnan[n] = false;
  }

  score_tiles(Q, ldq, N, G, ldg, D, i0, jbeg, jend, sQ, sG, [&](int tile, f32x16 (&acc)[2][2]) {
    // epilogue of this tile: C/D register r of accumulator (m, n) is gallery row 64 wm + 32 m + (r & 3) + 8 (r >> 2) + 4 h, query = lane
    // Columns are counted from this lane's first one, j0, so that the masks are 32-bit compares against per-tile values.
    const long j0 = jbeg + (long)tile * RT + 64 * wm + 4 * h;
    const int jrem = (int)(jend - j0 < 64 ? jend - j0 : 64);   // valid: offset < jrem (may be <= 0)
    int dq[2];                                                   // the pair positive's offset from j0, -1 when it is not in this tile
#pragma unroll
    for (int n = 0; n < 2; ++n) { const long d = qi[n] + diag_off - j0; dq[n] = (d >= 0 && d < 64) ? (int)d : -1; }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int off = 32 * m + (r & 3) + 8 * (r >> 2);
        const bool jv = off < jrem;   // columns of a partial tile are masked, not zero
        const long long kg = (KEYED && jv) ? keys_g[j0 + off] : 0;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const float s = acc[m][n][r];
          const bool positive = KEYED ? kg == kq[n] : off == dq[n];
          if (jv && qv[n]) {
            if (PASS == 0) { if (positive) { const int e = enc(s); best[n] = e > best[n] ? e : best[n]; } }
            else if (!positive) { sawnan[n] |= s != s; gt[n] += s > p[n] ? 1 : 0; eq[n] += s == p[n] ? 1 : 0; }
          }
          acc[m][n][r] = 0.f;
        }
      }
    }
  });

  // the two lane halves (and the two gallery-half waves, through the atomics) share a query row
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if (PASS == 0) {
      const int o = __shfl_xor(best[n], 32, 64);
      const int b = o > best[n] ? o : best[n];
      if (h == 0 && qv[n] && b != ENC_NEG_INF) atomicMax(pos_enc + qi[n], b);
    } else {
      const int g = gt[n] + __shfl_xor(gt[n], 32, 64), t = eq[n] + __shfl_xor(eq[n], 32, 64);
      const int f = (sawnan[n] ? 1 : 0) | __shfl_xor(sawnan[n] ? 1 : 0, 32, 64);
      if (h == 0 && qv[n]) {
        if (g) atomicAdd(greater + qi[n], g);
        if (t) atomicAdd(ties + qi[n], t);
        if (f) atomicOr(ties + qi[n], (int)0x80000000u);   // counts stay below 2^31: the sign bit is free
      }
    }
  }
}

template <int PASS, bool KEYED>
void launch_pass(dim3 grid, const float* Q, long ldq, int N, const float* G, long ldg, int M, int D, int diag_off,
                 const long long* keys_q, const long long* keys_g, float* pos, int* greater, int* ties, int tiles_per_block,
                 hipStream_t stream) {
  hipLaunchKernelGGL((retrieval_kernel<PASS, KEYED>), grid, dim3(256), 0, stream, Q, ldq, N, G, ldg, M, D, diag_off, keys_q, keys_g,
                     reinterpret_cast<int*>(pos), greater, ties, tiles_per_block);
}

}  // namespace

extern "C" int cxrk_retrieval_ranks(const float* Q, long ldq, int N, const float* G, long ldg, int M, int D, int diag_off,
                                    const long long* keys_q, const long long* keys_g, float* pos, int* greater, int* ties,
                                    hipStream_t stream) {
  CXRK_CHECK_ARG(Q && G && pos && greater && ties);
  CXRK_CHECK_ARG(N >= 1 && M >= 1 && D >= 1 && ldq >= D && ldg >= D);
  CXRK_CHECK_ARG((keys_q == nullptr) == (keys_g == nullptr));
  const bool keyed = keys_q != nullptr;
  if (!keyed) CXRK_CHECK_ARG(diag_off >= 0 && (long)diag_off + N <= (long)M);

  const Split sp = gallery_split(N, M);
  const int strips = sp.strips, tiles_per_block = sp.tiles_per_block;
  const dim3 grid(strips, sp.split);

  hipLaunchKernelGGL(retrieval_init_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream, reinterpret_cast<int*>(pos), greater, ties, N);
  if (keyed) {
    launch_pass<0, true>(grid, Q, ldq, N, G, ldg, M, D, 0, keys_q, keys_g, pos, greater, ties, tiles_per_block, stream);
    launch_pass<1, true>(grid, Q, ldq, N, G, ldg, M, D, 0, keys_q, keys_g, pos, greater, ties, tiles_per_block, stream);
  } else {
    launch_pass<0, false>(dim3(strips, 1), Q, ldq, N, G, ldg, M, D, diag_off, keys_q, keys_g, pos, greater, ties, 1, stream);
    launch_pass<1, false>(grid, Q, ldq, N, G, ldg, M, D, diag_off, keys_q, keys_g, pos, greater, ties, tiles_per_block, stream);
  }
  hipLaunchKernelGGL(retrieval_finish_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream, pos, greater, ties, N);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
