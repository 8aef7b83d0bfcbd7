// Fused top-k neighbour search and the kNN label vote (include/cxrk.h, "topk_neighbours" / "knn_vote"): for every query row the k
// best gallery rows by s(i,j) = sum_d Q[i][d] G[j][d], without ever writing the [N][M] similarity block.
//
// Scores come from the tile code of retrieval.hip (retrieval_tile.h), so s(i,j) depends on row i and row j only.  One total order
// decides everything: score descending (every NaN above every number, as enc() orders them), then gallery index ascending.  The
// signed 64-bit key (enc(s) << 32) | (0xFFFFFFFF - j) carries exactly that order; keys of distinct columns differ, so sorted partial
// lists merge without ambiguity and the result depends neither on the split nor on the order in which a block meets its columns.
//   stage 1, grid (strips, split) as cxrk_retrieval_ranks: per query row of the strip the k largest keys over the block's gallery
//            range, kept in LDS as list[slot][row].  A finished tile's scores go to LDS in two halves of 64 gallery rows (the half
//            tile lies over the staging buffers, which are idle then); thread `row` reads its row's 64 columns 16 at a time and
//            tests each against the list's smallest key, which it caches in a register (with its slot and its score: one float
//            compare per column).  On a pass only (about k ln(M / k) times per row in all) it overwrites that slot and finds the
//            new smallest with k independent LDS reads: the list is a bag while the block runs, not a sorted array whose shifts
//            would each wait for an LDS round trip.  At the end the bag is ranked (slot a goes to position #{b: key_b > key_a})
//            into the workspace slab [N][split][k], sorted; empty slots hold KEY_EMPTY, below every key of a column.
//   stage 2, one wave per query row: a `split`-way merge of sorted lists.  Lane l holds the heads of lists l, l + 64, ... (at most 8:
//            split <= 512) in registers; k rounds of a wave maximum, the winner's lane advances.  No atomics, no host sync.
#include "cxrk.h"
#include "cxrk_common.h"
#include "retrieval_tile.h"

#include <limits.h>

using namespace cxrk;

namespace {

using namespace cxrk::rtile;

constexpr int KMAX = 64;
constexpr long long KEY_EMPTY = LLONG_MIN;   // enc() never gives 0x80000000: enc(-inf) = 0x807fffff is its smallest value
constexpr int HALF = RT / 2;                  // gallery rows of a half tile
constexpr int MAX_LISTS_PER_LANE = 8;         // split <= 512 (gallery_split)
constexpr size_t STAGE_BYTES = 2 * STAGE_FLOATS * sizeof(float);
static_assert(STAGE_BYTES >= HALF * RT * sizeof(float) && STAGE_BYTES % 8 == 0, "the half tile lies over the staging buffers");

__device__ __forceinline__ long long make_key(float s, int j) {
  return (long long)(((unsigned long long)(unsigned)enc(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j));
}
__device__ __forceinline__ int key_index(long long key) { return (int)(0xFFFFFFFFu - (unsigned)(unsigned long long)key); }   // -1 if empty
__device__ __forceinline__ float key_score(long long key) {
  return key == KEY_EMPTY ? -__builtin_inff() : dec((int)(key >> 32));
}

static size_t stage1_lds_bytes(int k) { return STAGE_BYTES + (size_t)k * RT * sizeof(long long); }

__global__ __launch_bounds__(256) void topk_stage1_kernel(const float* __restrict__ Q, long ldq, int N, const float* __restrict__ G,
                                                          long ldg, int M, int D, int k, int exclude_off,
                                                          long long* __restrict__ slab, int split, int tiles_per_block) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sQ = reinterpret_cast<float*>(smem);
  float* sG = sQ + STAGE_FLOATS;
  float* sS = sQ;                                                        // half tile [gallery 64][query 128], over sQ / sG
  long long* list = reinterpret_cast<long long*>(smem + STAGE_BYTES);    // [k][RT]: a bag until the block ranks it

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, h = lane >> 5;
  const long i0 = (long)blockIdx.x * RT;
  const long jbeg = (long)blockIdx.y * tiles_per_block * RT;
  long jend = jbeg + (long)tiles_per_block * RT;
  if (jend > M) jend = M;

  for (int e = tid; e < k * RT; e += 256) list[e] = KEY_EMPTY;   // visible after the tile code's first barrier

  // the scanning thread's row: threads 0..127, one query row each
  const bool scans = tid < RT && i0 + tid < N;
  const long excl = exclude_off >= 0 ? i0 + tid + exclude_off : -1;
  long long* mine = list + (tid & (RT - 1));
  long long kth = KEY_EMPTY;   // the smallest key of the row's list, its slot, and its score (-inf while a slot is empty)
  int kpos = 0;
  float kthf = -__builtin_inff();

  if (jbeg < jend) {   // block-uniform; gallery_split leaves no block without columns
    score_tiles(Q, ldq, N, G, ldg, D, i0, jbeg, jend, sQ, sG, [&](int tile, f32x16 (&acc)[2][2]) {
      const long jt = jbeg + (long)tile * RT;
      const int rem = (int)(jend - jt < RT ? jend - jt : RT);                           // valid columns: offset < rem
      const int exoff = (excl >= jt && excl < jt + RT) ? (int)(excl - jt) : -1;         // the excluded column's offset, if in this tile
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        __syncthreads();   // the last chunk's reads (m = 0) / the first half's scan (m = 1) are done
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            sS[(32 * wm + (r & 3) + 8 * (r >> 2) + 4 * h) * RT + 64 * wn + 32 * n + l31] = acc[m][n][r];
            acc[m][n][r] = 0.f;
          }
        __syncthreads();
        if (scans) {
          // half-tile row g is the tile's gallery row 64 (g >> 5) + 32 m + (g & 31); columns >= jend entered as zeros: masked
#pragma unroll 1
          for (int g0 = 0; g0 < HALF; g0 += 16) {
            const int base = 64 * (g0 >> 5) + 32 * m + (g0 & 31);   // the 16 columns base + u: one run of the tile's gallery rows
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = sS[(g0 + u) * RT + tid];
            unsigned cand = 0;   // bit u: not below the smallest listed score (a NaN score, or a NaN kthf, is not below)
#pragma unroll
            for (int u = 0; u < 16; ++u) cand |= v[u] < kthf ? 0u : 1u << u;
            cand &= rem - base >= 16 ? 0xFFFFu : rem > base ? (1u << (rem - base)) - 1u : 0u;
            if (exoff >= base && exoff < base + 16) cand &= ~(1u << (exoff - base));
            while (cand) {   // rare once the list has warmed up
              const int u = __builtin_ctz(cand);
              cand &= cand - 1;
              const float s = sS[(g0 + u) * RT + tid];
              if (s < kthf) continue;   // kthf has risen since the batch was tested
              const long long key = make_key(s, (int)(jt + base + u));
              if (key <= kth) continue;
              mine[kpos * RT] = key;
              long long mn = mine[0];
              int mp = 0;
#pragma unroll 4
              for (int a = 1; a < k; ++a) {
                const long long e = mine[a * RT];
                if (e < mn) { mn = e; mp = a; }
              }
              kth = mn; kpos = mp; kthf = key_score(mn);
            }
          }
        }
      }
    });
  }

  // rank the bag: slot a goes to position #{b: key_b > key_a}; equal keys are empty slots, which keep their slot order behind the rest
  __syncthreads();
  const int row = tid & (RT - 1);
  if (i0 + row < N) {
    long long* out = slab + ((i0 + row) * split + blockIdx.y) * k;
    for (int a = tid >> 7; a < k; a += 2) {
      const long long key = mine[a * RT];
      int rank = 0;
#pragma unroll 4
      for (int b = 0; b < k; ++b) {
        const long long e = mine[b * RT];
        rank += (e > key || (e == key && b < a)) ? 1 : 0;
      }
      out[rank] = key;
    }
  }
}

__global__ __launch_bounds__(256) void topk_stage2_kernel(const long long* __restrict__ slab, int N, int k, int split,
                                                          float* __restrict__ score, int* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;   // wave-uniform
  const long long* base = slab + row * split * k;
  float* srow = score + row * k;
  int* irow = index + row * k;

  if (split == 1) {   // nothing to merge
    if (lane < k) { const long long key = base[lane]; srow[lane] = key_score(key); irow[lane] = key_index(key); }
    return;
  }

  long long head[MAX_LISTS_PER_LANE];
  int pos[MAX_LISTS_PER_LANE];
#pragma unroll
  for (int u = 0; u < MAX_LISTS_PER_LANE; ++u) {
    const int l = lane + 64 * u;
    pos[u] = 0;
    head[u] = l < split ? base[(long)l * k] : KEY_EMPTY;
  }
  for (int n = 0; n < k; ++n) {
    long long best = head[0];
#pragma unroll
    for (int u = 1; u < MAX_LISTS_PER_LANE; ++u) best = head[u] > best ? head[u] : best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long other = __shfl_xor(best, o, 64); best = other > best ? other : best; }
    if (lane == 0) { srow[n] = key_score(best); irow[n] = key_index(best); }
    if (best == KEY_EMPTY) continue;   // wave-uniform: every list is used up, the remaining slots are padding
#pragma unroll
    for (int u = 0; u < MAX_LISTS_PER_LANE; ++u) {   // keys of distinct columns differ: exactly one head matches
      if (head[u] == best) {
        ++pos[u];
        head[u] = pos[u] < k ? base[(long)(lane + 64 * u) * k + pos[u]] : KEY_EMPTY;
      }
    }
  }
}

// One thread per output element; the k weights are recomputed per class (k <= 64 exponentials), in slot order.
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ score, const int* __restrict__ index, long N, int k,
                                                       const float* __restrict__ labels, long ldl, int M, int C,
                                                       float inv_temperature, float* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * C) return;
  const long i = e / C;
  const int c = (int)(e - i * C);
  const float* s = score + i * k;
  const int* idx = index + i * k;
  const float s0 = s[0];
  float num = 0.f, den = 0.f;
  bool bad = false;
  for (int n = 0; n < k; ++n) {
    const int j = idx[n];
    if (j == -1) continue;                            // padding: weight 0
    if (j < 0 || j >= M) { bad = true; continue; }    // not a gallery row: never read, never a plausible vote
    const float sn = s[n];
    bad |= sn != sn;
    const float w = expf((sn - s0) * inv_temperature);
    num = fmaf(w, labels[(long)j * ldl + c], num);
    den += w;
  }
  out[e] = bad ? __builtin_nanf("") : num / den;   // no valid neighbour: 0 / 0
}

}  // namespace

extern "C" size_t cxrk_topk_neighbours_slab_bytes(int N, int M, int k) {
  if (N < 1 || M < 1 || k < 1 || k > KMAX) return 0;
  return (size_t)N * gallery_split(N, M).split * k * sizeof(long long);
}

extern "C" int cxrk_topk_neighbours(const float* Q, long ldq, int N, const float* G, long ldg, int M, int D, int k, int exclude_off,
                                    float* score, int* index, void* slab_mem, size_t slab_bytes, hipStream_t stream) {
  CXRK_CHECK_ARG(Q && G && score && index);
  CXRK_CHECK_ARG(N >= 1 && M >= 1 && D >= 1 && ldq >= D && ldg >= D);
  CXRK_CHECK_ARG(k >= 1 && k <= KMAX);
  CXRK_CHECK_ARG(exclude_off >= -1 && (exclude_off < 0 || (long)exclude_off + N <= (long)M));
  CXRK_CHECK_WS(slab_mem, slab_bytes, cxrk_topk_neighbours_slab_bytes(N, M, k));

  const Split sp = gallery_split(N, M);
  CXRK_CHECK_ARG(sp.split <= 64 * MAX_LISTS_PER_LANE);
  long long* slab = static_cast<long long*>(slab_mem);
  const size_t lds = stage1_lds_bytes(k);
  if (lds > 64 * 1024 &&   // beyond the default limit of dynamic LDS the kernel has to be told (k > 31); a host-side setting, no launch
      hipFuncSetAttribute(reinterpret_cast<const void*>(topk_stage1_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)stage1_lds_bytes(KMAX)) != hipSuccess)
    return CXRK_ERR_LAUNCH;
  hipLaunchKernelGGL(topk_stage1_kernel, dim3(sp.strips, sp.split), dim3(256), lds, stream, Q, ldq, N, G, ldg, M, D, k, exclude_off,
                     slab, sp.split, sp.tiles_per_block);
  hipLaunchKernelGGL(topk_stage2_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, stream, slab, N, k, sp.split, score, index);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_knn_vote(const float* score, const int* index, int N, int k, const float* labels, long ldl, int M, int C,
                             float inv_temperature, float* out, hipStream_t stream) {
  CXRK_CHECK_ARG(score && index && labels && out);
  CXRK_CHECK_ARG(N >= 1 && M >= 1 && C >= 1 && ldl >= C && k >= 1 && k <= KMAX);
  hipLaunchKernelGGL(knn_vote_kernel, dim3(ceil_div((long)N * C, 256)), dim3(256), 0, stream, score, index, (long)N, k, labels, ldl, M,
                     C, inv_temperature, out);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
