// The stem of the image encoder with its max-pool fused (resnet.py:34-38: conv1 7x7 / 2 / 3, bn1, relu, maxpool 3x3 / 2 / 1).
//
// Unfused, the stem output — [N, 112, 112, 64] at 4 bytes per element, 3.29 GB at batch 1024 — is written by the convolution, read by
// the max-pool, and in the backward written again as its gradient and read twice (BatchNorm sums, weight gradient), although the
// step needs only the pooled activation, the winner bytes and the stem's parameter gradients.
//
//  * stem_pool_fwd_kernel: one block computes the stem pixels under a 7 x 8 tile of POOLED pixels, halo included (15 x 17 = 255
//    rows of the 256 x 64 register-staged mainloops of gemm_core.h), leaves them in LDS as the values the planes format would
//    have stored (hi + lo) and pools from there: the stem output never reaches HBM.  Per output element the arithmetic is that of
//    gemm_x3_kernel / gemm_f32_kernel with ConvIm2colKC<.., TAPWISE = false>, the epilogue of gemm_epilogue.h and
//    maxpool_fwd_pl_kernel, in the same order: the pooled planes and the winner bytes are bit-identical to the unfused pair.
//  * stem_pool_sums_*: the column sums of the max-pool backward's output (the stem's BatchNorm beta gradient, and an input of the
//    gamma gradient) taken in pooled space: every window has exactly one winner, so the sum over stem pixels of dstem[., c] is the
//    sum over windows of g[window, c] * [pooled > 0].  Per-block partials and a fixed-order final pass: no atomics.
#include "conv_common.h"

using namespace cxrk;

namespace {

constexpr int SP_PH = 7, SP_PW = 8;                           // pooled pixels per block
constexpr int SP_RH = 2 * SP_PH + 1, SP_RW = 2 * SP_PW + 1;   // stem pixels under them: 15 x 17
constexpr int SP_C = 4, SP_R = 7, SP_S = 7, SP_KO = 64;       // the stem: 7x7 taps of 4 (3 + 1 zero) channels, 64 filters
constexpr int SP_K = SP_R * SP_S * SP_C;                      // 196
constexpr int SP_STRIDE = 2, SP_PAD = 3;
static_assert(SP_RH * SP_RW <= 256, "the stem region of a block must fit the 256 rows of the tile");

// A operand: ConvIm2colKC<256, F32, TAPWISE = false> (a tap per lane, fp32 image) with a tile-local row map: row m of the block is
// stem pixel (hs0 + m / 17, ws0 + m % 17) of ONE image.  Rows outside the stem image (and row 255) are dead: zero operand.
struct StemTileKC : KCGeom<256, F32, NTHREADS> {
  typedef KCGeom<256, F32, NTHREADS> G;
  typedef float4 V;
  using G::NV; using G::NVR; using G::RP; using G::KQ; using G::LD;
  const float* bp;
  unsigned off[NVR];            // byte offset of (row, tap 0) from bp (wraps below zero in the halo; only valid taps are loaded)
  int hi0[NVR], wi0[NVR];
  int kq, r0, H, W;
  __device__ __forceinline__ void init(const float* img, int H_, int W_, int Hs, int Ws, int hs0, int ws0, int tid) {
    kq = tid % KQ; r0 = tid / KQ; H = H_; W = W_; bp = img;
#pragma unroll
    for (int j = 0; j < NVR; ++j) {
      const int m = r0 + j * RP;
      const int lr = m / SP_RW, lc = m - lr * SP_RW;
      const int hs = hs0 + lr, ws = ws0 + lc;
      const bool in = lr < SP_RH && (unsigned)hs < (unsigned)Hs && (unsigned)ws < (unsigned)Ws;
      const int h0 = hs * SP_STRIDE - SP_PAD, w0 = ws * SP_STRIDE - SP_PAD;
      off[j] = in ? (unsigned)(((h0 * W + w0) * SP_C) * 4) : 0u;
      hi0[j] = in ? h0 : -(1 << 28); wi0[j] = in ? w0 : 0;
    }
  }
  __device__ __forceinline__ void load(int k0, V (&v)[NV]) {
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(bp);
    const int k = k0 + kq * 4;
    const int tap = k / SP_C;
    const int r = tap / SP_S, s = tap - r * SP_S;
    const unsigned toff = (unsigned)(((r * W + s) * SP_C) * 4);
#pragma unroll
    for (int j = 0; j < NVR; ++j) {
      const bool ok = (k < SP_K) && ((unsigned)(hi0[j] + r) < (unsigned)H) && ((unsigned)(wi0[j] + s) < (unsigned)W);
      v[j] = bload4(rs, ok ? off[j] + toff : VOFF_OOB);
    }
  }
  __device__ __forceinline__ void store2(unsigned short* hi, unsigned short* lo, const V (&v)[NV]) const { stage2_kc<NV, RP>(hi, lo, r0, kq, v); }
  __device__ __forceinline__ void store(float* Sm, const float4 (&v)[NV]) const { stage_kc<NV, LD, RP>(Sm, r0, kq, v); }
};

struct StemPoolP {
  const float* x; const float* w; const float* shift;
  unsigned short* y; long yplane; unsigned char* idx;
  int N, H, W, Hs, Ws, Hp, Wp, TH, TW;
  float alpha;
};

// SPLIT: the split-bf16 mainloop of gemm_x3_kernel (three bf16 MFMAs per term, lo*hi, hi*lo, hi*hi); else that of gemm_f32_kernel.
// Which one a call takes is launch_gemm's rule for the unfused stem, so that the two agree bit for bit at every size.
template <bool SPLIT>
__global__ __launch_bounds__(NTHREADS, 2) void stem_pool_fwd_kernel(StemPoolP p) {
  typedef StemTileKC LA;
  typedef DenseKC<SP_KO, F32, NTHREADS> LB;
  constexpr int PLANE_A = LA::PLANE, PLANE_B = LB::PLANE;   // halfwords
  constexpr int LDA = LA::LD, LDB = LB::LD;
  constexpr int STG = 256 * SP_KO;                           // floats: the post-ReLU stem values of the block
  static_assert(2 * (PLANE_A + PLANE_B) * 2 <= STG * 4 && BK * (LDA + LDB) <= STG, "operand tiles must fit the staging area");
  // ONE array: operand tiles in the mainloop, the block's stem values after it
  __shared__ __attribute__((aligned(16))) float smem[STG];

  int tile, nt_, z_;
  tile_coords(p.N * p.TH * p.TW, 1, 1, tile, nt_, z_);
  const int tw = tile % p.TW; const int t_ = tile / p.TW; const int th = t_ % p.TH; const int n = t_ / p.TH;
  const int ph0 = th * SP_PH, pw0 = tw * SP_PW;
  const int hs0 = 2 * ph0 - 1, ws0 = 2 * pw0 - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  LA la; LB lb;
  la.init(p.x + (long)n * p.H * p.W * SP_C, p.H, p.W, p.Hs, p.Ws, hs0, ws0, tid);
  lb.init(LB::P{p.w, (long)SP_K, SP_KO, SP_K, 0}, 0, tid);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  float4 ra[LA::NV], rb[LB::NV];
  if constexpr (SPLIT) {
    unsigned short* const Ahi = reinterpret_cast<unsigned short*>(smem);
    unsigned short* const Alo = Ahi + PLANE_A;
    unsigned short* const Bhi = Alo + PLANE_A;
    unsigned short* const Blo = Bhi + PLANE_B;
    la.load(0, ra); lb.load(0, rb);
    la.store2(Ahi, Alo, ra); lb.store2(Bhi, Blo, rb);
    __syncthreads();
    if (BK < SP_K) { la.load(BK, ra); lb.load(BK, rb); }
    for (int k0 = 0; k0 < SP_K; k0 += BK) {
#pragma unroll
      for (int kc = 0; kc < BK / 16; ++kc) {
        bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ah[i] = frag_kc(Ahi, wave * 64 + i * 32, kc, lane); al[i] = frag_kc(Alo, wave * 64 + i * 32, kc, lane);
          bh[i] = frag_kc(Bhi, i * 32, kc, lane); bl[i] = frag_kc(Blo, i * 32, kc, lane);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          }
      }
      __syncthreads();  // everyone is done reading before the single buffer is overwritten
      if (k0 + BK < SP_K) { la.store2(Ahi, Alo, ra); lb.store2(Bhi, Blo, rb); }
      __syncthreads();
      if (k0 + 2 * BK < SP_K) { la.load(k0 + 2 * BK, ra); lb.load(k0 + 2 * BK, rb); }
    }
  } else {
    float* const As0 = smem;
    float* const Bs0 = smem + BK * LDA;
    la.load(0, ra); lb.load(0, rb);
    la.store(As0, ra); lb.store(Bs0, rb);
    __syncthreads();
    if (BK < SP_K) { la.load(BK, ra); lb.load(BK, rb); }
    for (int k0 = 0; k0 < SP_K; k0 += BK) {
      const float* Ap = As0 + wave * 64 + r + h * LDA;
      const float* Bp = Bs0 + r + h * LDB;
      float a0 = Ap[0], a1 = Ap[32], b0 = Bp[0], b1 = Bp[32];
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {
        float a0n = 0.f, a1n = 0.f, b0n = 0.f, b1n = 0.f;
        if (kk + 1 < BK / 2) {
          a0n = Ap[(2 * kk + 2) * LDA]; a1n = Ap[(2 * kk + 2) * LDA + 32];
          b0n = Bp[(2 * kk + 2) * LDB]; b1n = Bp[(2 * kk + 2) * LDB + 32];
        }
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        a0 = a0n; a1 = a1n; b0 = b0n; b1 = b1n;
      }
      __syncthreads();  // single buffer: everyone must be done reading before it is overwritten
      if (k0 + BK < SP_K) { la.store(As0, ra); lb.store(Bs0, rb); }
      __syncthreads();
      if (k0 + 2 * BK < SP_K) { la.load(k0 + 2 * BK, ra); lb.load(k0 + 2 * BK, rb); }
    }
  }
  __syncthreads();  // every wave is done reading operand tiles

  // Epilogue, per element as gemm_epilogue.h computes and stores it: alpha * acc + shift, ReLU (a NaN stays), split into bf16
  // hi / lo; what a reader of the planes gets back is hi + lo, and that value goes to LDS as [row][64].
  // (C/D map of the 32x32 MFMAs: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).)
  const float bj[2] = {p.shift[r], p.shift[32 + r]};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const float v0 = relu_keep_nan(p.alpha * acc[i][j][e] + bj[j]), v1 = relu_keep_nan(p.alpha * acc[i][j][e + 1] + bj[j]);
        unsigned hp, lp;
        split2(v0, v1, hp, lp);
        const float u0 = __builtin_bit_cast(float, hp << 16) + __builtin_bit_cast(float, lp << 16);
        const float u1 = __builtin_bit_cast(float, hp & 0xffff0000u) + __builtin_bit_cast(float, lp & 0xffff0000u);
        const int row = wave * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        smem[row * SP_KO + j * 32 + r] = u0;
        smem[(row + 1) * SP_KO + j * 32 + r] = u1;
      }
  __syncthreads();

  // The pool of maxpool_fwd_pl_kernel on the block's 7 x 8 pooled pixels, 8 channels per thread: taps in (r, s) order, taps outside
  // the stem image skipped (not zero: the first valid tap must win the ties at 0), `v > best || v != v` replaces.
  for (int it = tid; it < SP_PH * SP_PW * (SP_KO / 8); it += NTHREADS) {
    const int c8 = it & 7, pp = it >> 3;
    const int pr = pp / SP_PW, pc = pp - pr * SP_PW;
    const int ph = ph0 + pr, pw = pw0 + pc;
    if (ph >= p.Hp || pw >= p.Wp) continue;
    float best[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unsigned bi[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    bool first = true;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      const int hs = 2 * ph - 1 + rr;
      if ((unsigned)hs >= (unsigned)p.Hs) continue;
#pragma unroll
      for (int ss = 0; ss < 3; ++ss) {
        const int ws = 2 * pw - 1 + ss;
        if ((unsigned)ws >= (unsigned)p.Ws) continue;
        const float* sp = smem + ((2 * pr + rr) * SP_RW + 2 * pc + ss) * SP_KO + c8 * 8;
        const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
        const float v[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const unsigned tap = (unsigned)(rr * 3 + ss);
#pragma unroll
        for (int q = 0; q < 8; ++q) if (first || v[q] > best[q] || v[q] != v[q]) { best[q] = v[q]; bi[q] = tap; }
        first = false;
      }
    }
    const long o = ((((long)n * p.Hp + ph) * p.Wp + pw) * (SP_KO / 8) + c8) * 8;
    planes_store8(p.y, p.yplane, o, best);
    if (p.idx)
      *reinterpret_cast<uint2*>(p.idx + o) = make_uint2(bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24),
                                                        bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24));
  }
}

// ---- the BatchNorm sums of the stem's backward, in pooled space ----------------------------------------------------------------
// one partial row per block; the buffer is the one cxrk_colsum_ws_bytes(rows, 64) sizes (512 rows per part, 512 parts at most)
static int sums_parts(long rows) { return (int)(cxrk_colsum_ws_bytes(rows, SP_KO) / (SP_KO * sizeof(float))); }

// part[block][c] = sum over the block's rows of g[row][c] * [pooled[row][c] > 0]   (g, pooled: planes [rows][64]; the sign of a
// planes value is that of its hi half, as maxpool_bwd_pl_kernel reads it).  A thread owns 8 channels and every 32nd row.
__global__ __launch_bounds__(256) void stem_pool_sums_partial_kernel(const unsigned short* __restrict__ g, long gplane,
                                                                     const unsigned short* __restrict__ pooled, long rows, long rows_per,
                                                                     float* __restrict__ part) {
  __shared__ float sh[32][SP_KO];
  const int c8 = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const long r0 = (long)blockIdx.x * rows_per;
  const long r1 = min(rows, r0 + rows_per);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto add = [&](const uint4& gh, const uint4& gl, const uint4& ph) {
    float v[8]; planes_unpack8(gh, gl, v);
    const unsigned pw[4] = {ph.x, ph.y, ph.z, ph.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float pv = __builtin_bit_cast(float, (q & 1) ? (pw[q >> 1] & 0xffff0000u) : (pw[q >> 1] << 16));
      s[q] += pv > 0.f ? v[q] : 0.f;
    }
  };
  long r = r0 + rl;
  for (; r + 96 < r1; r += 128) {
    uint4 gh[4], gl[4], ph[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long o = (r + 32 * u) * SP_KO + c8 * 8;
      gh[u] = *reinterpret_cast<const uint4*>(g + o); gl[u] = *reinterpret_cast<const uint4*>(g + gplane + o);
      ph[u] = *reinterpret_cast<const uint4*>(pooled + o);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) add(gh[u], gl[u], ph[u]);
  }
  for (; r < r1; r += 32) {
    const long o = r * SP_KO + c8 * 8;
    add(*reinterpret_cast<const uint4*>(g + o), *reinterpret_cast<const uint4*>(g + gplane + o), *reinterpret_cast<const uint4*>(pooled + o));
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) sh[rl][c8 * 8 + q] = s[q];
  __syncthreads();
  if (threadIdx.x < SP_KO) {
    float t = sh[0][threadIdx.x];
    for (int i = 1; i < 32; ++i) t += sh[i][threadIdx.x];
    part[(long)blockIdx.x * SP_KO + threadIdx.x] = t;
  }
}
// out[c] = sum of the partials, in a fixed order: sixteen interleaved chains per column, then added in chain order
__global__ __launch_bounds__(1024) void stem_pool_sums_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out) {
  __shared__ float sh[16][SP_KO];
  const int c = threadIdx.x & (SP_KO - 1), grp = threadIdx.x >> 6;
  float s = 0.f;
  for (int q = grp; q < nparts; q += 16) s += part[(long)q * SP_KO + c];
  sh[grp][c] = s;
  __syncthreads();
  if (grp == 0) {
    float t = sh[0][c];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += sh[i][c];
    out[c] = t;
  }
}

}  // namespace

// Stem convolution (7x7 / stride 2 / pad 3, 4 -> 64 channels, BatchNorm folded into w_scaled / shift) + ReLU + 3x3 / 2 / 1 max-pool.
// x: fp32 [N,H,W,4]; w_scaled: fp32 [64][7][7][4]; y: planes [N,Hp,Wp,64]; idx: uint8 [N,Hp,Wp,64] or null (no-grad forwards).
// Bit-identical to cxrk_conv_bn_act_fwd_pl(in_planes = 0, relu = 1) followed by cxrk_maxpool_fwd_pl.
extern "C" int cxrk_stem_pool_fwd(const float* x, const float* w_scaled, const float* shift, void* y, long yplane, unsigned char* idx,
                                  int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad, hipStream_t stream) {
  last_launch = {};
  CXRK_CHECK_ARG(x && w_scaled && shift && y && N > 0 && H > 0 && W > 0);
  CXRK_CHECK_ARG(aligned16(x) && aligned16(w_scaled) && aligned16(shift) && aligned16(y) && (yplane % 8) == 0 && (((uintptr_t)idx) & 7) == 0);
  if (C != SP_C || Ko != SP_KO || R != SP_R || S != SP_S || stride != SP_STRIDE || pad != SP_PAD) return CXRK_ERR_UNSUPPORTED;
  const ConvGeom g = make_geom(N, H, W, C, Ko, R, S, stride, pad);
  CXRK_CHECK_ARG(g.Ho > 0 && g.Wo > 0);
  const int Hp = (g.Ho - 1) / 2 + 1, Wp = (g.Wo - 1) / 2 + 1;
  const int TH = ceil_div(Hp, SP_PH), TW = ceil_div(Wp, SP_PW);
  // a block addresses its image with 32-bit byte offsets; the grid is one list of tiles
  if ((long)H * W * C * 4 >= (1L << 31) || (long)N * TH * TW >= (1L << 31) || (long)N * g.Ho * g.Wo >= (1L << 31)) return CXRK_ERR_UNSUPPORTED;
  StemPoolP p{x, w_scaled, shift, static_cast<unsigned short*>(y), yplane, idx, N, H, W, g.Ho, g.Wo, Hp, Wp, TH, TW, 1.f};
  // launch_gemm's rule for the unfused stem: the split-bf16 mainloop in that precision mode from 1 GFLOP on, else exact fp32
  const bool split = gemm_precision_mode() == 1 && 2.0 * ((double)N * g.Ho * g.Wo) * SP_KO * (double)SP_K >= 1073741824.0;
  const dim3 grid((unsigned)(N * TH * TW));
  if (split) hipLaunchKernelGGL(stem_pool_fwd_kernel<true>, grid, dim3(NTHREADS), 0, stream, p);
  else hipLaunchKernelGGL(stem_pool_fwd_kernel<false>, grid, dim3(NTHREADS), 0, stream, p);
  CXRK_LAUNCH_CHECK();
  // the label is the instantiation as scripts/pmc_summary_key.py abbreviates its rocprofv3 name
  note_launch({"stem_pool_fwd_kernel", split ? "true" : "false", nullptr, nullptr, 0, 0, split}, (double)N * g.Ho * g.Wo * SP_KO * SP_K);
  return CXRK_OK;
}

// sums[c] = sum over the stem pixels of what cxrk_maxpool_bwd_pl writes for (g, idx, pooled), without writing it:
// sum over the pooled pixels of g * [pooled > 0].  g, pooled: planes [N,Hp,Wp,64]; part: the
// per-block partial sums, cxrk_colsum_ws_bytes(N*Hp*Wp, 64) bytes, 256-byte aligned (a workspace: its contents mean nothing afterwards).
extern "C" int cxrk_stem_pool_bwd_sums(const void* g, long gplane, const void* pooled, float* sums, int N, int Hp, int Wp, int C,
                                       float* part, size_t part_bytes, hipStream_t stream) {
  last_launch = {};
  CXRK_CHECK_ARG(g && pooled && sums && N > 0 && Hp > 0 && Wp > 0 && aligned16(g) && aligned16(pooled) && (gplane % 8) == 0);
  if (C != SP_KO) return CXRK_ERR_UNSUPPORTED;
  const long rows = (long)N * Hp * Wp;
  const int nparts = sums_parts(rows);
  CXRK_CHECK_WS(part, part_bytes, (size_t)nparts * SP_KO * sizeof(float));
  const long rows_per = (rows + nparts - 1) / nparts;
  hipLaunchKernelGGL(stem_pool_sums_partial_kernel, dim3((unsigned)nparts), dim3(256), 0, stream, static_cast<const unsigned short*>(g), gplane,
                     static_cast<const unsigned short*>(pooled), rows, rows_per, part);
  CXRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(stem_pool_sums_final_kernel, dim3(1), dim3(1024), 0, stream, part, nparts, sums);
  CXRK_LAUNCH_CHECK();
  note_launch({"stem_pool_sums_partial_kernel", nullptr, nullptr, nullptr, 0, 0, 0}, (double)rows * SP_KO);
  return CXRK_OK;
}
