// The one tile code of the gallery searches (retrieval.hip: ranks of the positives; topk.hip: the k best gallery rows).
//
// A 256-thread block forms 128 x 128 tiles of s(i,j) = sum_k Q[i][k] G[j][k] with the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: bit
// for bit a k-ascending fmaf chain, so s(i,j) depends on row i of Q and row j of G only, never on the tile, the block or the pass
// that formed it), K in chunks of 32 through one LDS buffer with the next chunk prefetched into registers.  The gallery rows are
// the A operand and the query rows the B operand: a lane then owns ONE query row per 32-column accumulator (the C/D column =
// lane & 31) and its 16 registers are 16 gallery rows.
#pragma once
#include "cxrk_common.h"

namespace cxrk {
namespace rtile {

constexpr int RT = 128;        // tile edge (query rows per strip, gallery rows per tile)
constexpr int RK = 32;         // K chunk
constexpr int RLD = RT + 1;    // LDS row pitch of the [k][row] images
constexpr int STAGE_FLOATS = RK * RLD;   // one operand's staging image
constexpr int ENC_NEG_INF = (int)0x807fffffu;   // enc(-inf)
constexpr int ENC_NAN = 0x7fffffff;

// fp32 -> int32 with the same order (signed compare); every NaN maps to INT_MAX, which decodes to a NaN.
__device__ __forceinline__ int enc(float s) {
  if (s != s) return ENC_NAN;
  const int b = __builtin_bit_cast(int, s);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float dec(int e) { return __builtin_bit_cast(float, e >= 0 ? e : e ^ 0x7fffffff); }

// Grid (strips, split): query strips of RT rows; the gallery's tiles split over blockIdx.y so that a short query set still gives
// every CU (256) two blocks.  Block (x, y) owns tiles [y * tiles_per_block, (y + 1) * tiles_per_block); no y is empty.
struct Split { int strips, split, tiles_per_block; };
static inline Split gallery_split(int N, int M) {
  const int strips = ceil_div(N, RT), tiles = ceil_div(M, RT);
  int split = ceil_div(512, strips);
  if (split > tiles) split = tiles;
  const int tiles_per_block = ceil_div(tiles, split);
  return {strips, ceil_div(tiles, tiles_per_block), tiles_per_block};
}

// Forms the tiles of query strip [i0, i0 + RT) against gallery rows [jbeg, jend), RT at a time (jbeg < jend), and hands each finished
// tile to epilogue(tile, acc).  C/D register r of acc[m][n] is gallery row (tile's first) + 64 wm + 32 m + (r & 3) + 8 (r >> 2) + 4 h
// and query row i0 + 64 wn + 32 n + (lane & 31), with wm = wave & 1, wn = wave >> 1, h = lane >> 5.  The epilogue leaves acc zero.
// Rows >= N, columns >= jend and k >= D are never read (they enter as zeros: mask them).  sQ / sG: STAGE_FLOATS each; they are free
// for the epilogue's own use between a __syncthreads() of its own and its return.
template <class Epilogue>
__device__ __forceinline__ void score_tiles(const float* __restrict__ Q, long ldq, int N, const float* __restrict__ G, long ldg, int D,
                                            long i0, long jbeg, long jend, float* sQ, float* sG, Epilogue&& epilogue) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;   // gallery half / query half of the tile this wave owns (64 x 64)
  const int l31 = lane & 31, h = lane >> 5;
  const int ntiles = (int)((jend - jbeg + RT - 1) / RT);
  const int nch = (D + RK - 1) / RK;

  // staging map: thread -> (k = tid & 31, rows (tid >> 5) + 8 u): a wave reads two 128-byte row pieces per load
  const int kcol = tid & 31, rbase = tid >> 5;
  float rq[16], rg[16];
  const int nq = (int)((long)N - i0 < RT ? (long)N - i0 : RT) - rbase;   // this thread's rows rbase + 8 u are valid while 8 u < nq
  const float* qbase = Q + (i0 + rbase) * ldq + kcol;
  const long qstep = 8 * ldq, gstep = 8 * ldg;
  auto fetch = [&](int tile, int ch) {
    const long j0 = jbeg + (long)tile * RT;
    const int ng = (int)(jend - j0 < RT ? jend - j0 : RT) - rbase;
    const bool kv = ch * RK + kcol < D;
    const float* qp = qbase + ch * RK;
    const float* gp = G + (j0 + rbase) * ldg + ch * RK + kcol;
#pragma unroll
    for (int u = 0; u < 16; ++u) {   // rows >= N, columns >= jend and k >= D are never read
      rq[u] = (kv && 8 * u < nq) ? qp[u * qstep] : 0.f;
      rg[u] = (kv && 8 * u < ng) ? gp[u * gstep] : 0.f;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  const float* Ap = sG + 64 * wm + l31 + h * RLD;   // A[row = gallery][k = 2 kk + h]
  const float* Bp = sQ + 64 * wn + l31 + h * RLD;   // B[k = 2 kk + h][col = query]

  fetch(0, 0);
  for (int tile = 0; tile < ntiles; ++tile) {
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();   // the previous chunk's reads are done
#pragma unroll
      for (int u = 0; u < 16; ++u) { sQ[kcol * RLD + rbase + 8 * u] = rq[u]; sG[kcol * RLD + rbase + 8 * u] = rg[u]; }
      __syncthreads();
      if (ch + 1 < nch) fetch(tile, ch + 1);
      else if (tile + 1 < ntiles) fetch(tile + 1, 0);
#pragma unroll
      for (int kk = 0; kk < RK / 2; ++kk) {   // k ascending: chunk, then kk, then the instruction's own k = 0, 1
        const float a0 = Ap[2 * kk * RLD], a1 = Ap[2 * kk * RLD + 32];
        const float b0 = Bp[2 * kk * RLD], b1 = Bp[2 * kk * RLD + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    epilogue(tile, acc);
  }
}

}  // namespace rtile
}  // namespace cxrk
