// Weight gradient of the 3x3 / stride 1 / pad 1 convolutions with 64 input channels and 64 filters on planes operands (the layers
// conv_halo.h takes forward and for the data gradient): the activation stays RESIDENT in LDS for all nine taps.
//
//   dW_raw[ko][r][s][c] = sum_m dy[m][ko] * x[m + (r-1) W + (s-1)][c]   over the flattened pixel index m in [0, N*H*W),
//   a term counting only where (h + r - 1, w + s - 1) lies inside the image.
//
// Why.  As an implicit GEMM (gemm_pw_kernel<Pw64x256, DmaDenseMC, DmaConvIm2colMC>) the contraction runs over the pixels and the
// im2col operand is staged once per tap: nine times the activation bytes through L2 -> LDS, at 4.4x the MFMA floor
// (profiles/r03_final_layer_table.log).  Here the contraction index is still the pixel, but a block owns the whole K range of one
// split-K slab — the SAME slabs the implicit GEMM writes (launch_conv3x3_wgrad_window) — and keeps the 64 x 576 accumulator in
// registers for the launch: no per-tile epilogue, one store at the end, and wgrad_reduce_bn_kernel sums the slabs as before.
// Same slabs, and per accumulator element the same MFMAs in the same order: the result is BIT-IDENTICAL to the implicit GEMM's
// (a training run does not change by a bit when these layers move to this kernel; tests compare the two paths with
// torch.equal).  The price: the slab count is the split-K policy's (308 at batch 1024), not the CU count; the slabs beyond one
// per CU are computed by three blocks each, one filter row per block (ROW form, below).  Both operands stream along the
// pixel axis by LDS-DMA, each pixel fetched once per block (the W+1 halo pixels at the two ends of a range are the only re-reads):
//   * dy K-tiles [32 pixels][64 ko], hi | lo planes, a ring of WG_NSD = 4 tiles;
//   * x in a ring of WG_RING = 256 pixel slots [pixel][64 c] per plane, pixel p of the block's range in slot p & 255, fetched in
//     groups of 32 pixels aligned with the K-tiles.  K-tile t reads pixels 32 t - (W+1) .. 32 t + 31 + (W+1), i.e. (W <= 58)
//     groups t-2 .. t+2; the ring holds eight groups, so groups t+3 .. t+5 are in flight while tile t computes.
// Tap (r, s) of K-tile t is the SAME ring read at the pixel rows shifted by (r-1) W + (s-1).  A neighbour that does not exist
// (image border: the flattened index then points into the previous / next row or image; or a pixel >= M) is a per-lane
// redirect of that pixel row to an all-zero slot (slot WG_RING of each plane), the `vm` / HALO_HP-1 device of conv_halo.h.
// Which neighbours exist is a 9-bit word per dy pixel that ONE loader wave writes to LDS three tiles ahead (it walks (w, h) along
// the pixels, one pixel per lane); the compute waves only pick their three bits.  Deriving the masks in the compute waves (four
// pixels per lane and tile) took ~150 VALU instructions per wave and K-tile and the launch 0.72 ms; with the words ~70 and 0.67.
//
// Fragments.  Both operands are pixel-major = k-major, so both fragment reads are the transposing kind (ds_read_tr16_b64, two per
// fragment; lane 4q+p of a 16-lane group supplies pixel row q, 8 bytes at column 4p: pw_frag_mc).  A pixel row is 128 bytes =
// half a bank row, and the 32 lanes one LDS cycle serves read four CONSECUTIVE pixel rows, 64 bytes of each.  Rows s and s+1 sit
// in different halves of the bank row; rows s and s+2 are separated by XOR-ing the 64-byte half of slot s with bit 1 of s:
//   byte of (slot s, logical byte column b) = 128 s + (b ^ (((s >> 1) & 1) << 6)).
// Four consecutive slots take all four values of (s & 3), so the four 64-byte pieces cover the 64 banks exactly once for EVERY
// shift (the map depends on the shift only through s & 3, and a shift moves all four rows together; also enumerated over the
// lane map for every W <= 58, all nine shifts and the ring wrap: 64 distinct banks per half-wave in all 75 168 cases).  The ring
// size is a multiple of four, so the wrap keeps this.  Only a K-step that mixes live rows with redirected ones can conflict (the
// zero slot against one live row: 2-way, at image borders).
// pw_mc_swz keys the same XOR on the tile row k; keyed on the ring slot it is applied, as everywhere here, to the per-lane DMA
// SOURCE address (the LDS-DMA writes lane-linear).  The dy tiles use the same map (slot = tile row), which is pw_frag_mc<64>.
//
// Waves.  12 compute waves + 4 loader waves, one block per CU (98 KiB of LDS), 4 waves per SIMD -> 128 registers each.
// The 36 accumulator blocks of 32 x 32 (2 ko halves x 9 taps x 2 c halves) are spread as compute wave (kh, ch, r) -> taps
// (r, 0..2): 48 accumulator registers; a dy fragment feeds three taps.  A K-tile is read tap by tap (dy and taps 0, 1 first,
// tap 2 into the registers tap 0 leaves), the next tile's addresses are selected under the MFMAs; no scheduling fences (110
// registers, no scratch).  Only the loader waves issue LDS-DMA: loader (L, G) stages pieces 2G, 2G+1 (8 pixels each) of plane L
// of one x group and of one dy tile per K-tile: four pieces, so vmcnt — a per-wave, in-order counter — is a constant in the
// loop.  Every wave executes the same barrier sequence: PRE, then one per K-tile:
//   PRE         loaders: groups -2 .. 4, dy tiles 0-2 and the mask words of tiles 0-2 are in LDS;  compute: the zero slots are
//   barrier t   loaders: x group t+2 and dy tile t have landed (issued three tiles ago: vmcnt(8) leaves the two younger sets),
//                        the mask words of tile t+2 are written
//               compute: my reads of K-tile t-1 (and of the mask words of tile t) have retired (lgkmcnt(0))
//               -> behind it the loaders issue x group t+5 into the slots of group t-3, dy tile t+3 into those of tile t-1 and
//                  the mask words of tile t+3 into those of tile t-1 (read during tile t-2); compute reads the words of tile t+1.
// Loads past the end of a range go through the out-of-bounds lane bit: they move no data and write zeros into slots nobody reads.
//
// Determinism: no atomics; the pixel -> slab map is the split-K policy's, and which block computes a slab does not change a bit.
//
// Measured at batch 1024 on the 56 x 56 layers (profiles/layer_table_parent.log, layer_table_window_wgrad.log, one box): see
// DESIGN section 5.  A first form with one block per CU and CU-count slabs (256 ranges of 392 K-tiles) took 0.62 ms, but its sums
// differ from the implicit GEMM's in the last bits, and a bench run drifts from the parent's by more than rounding; with the
// GEMM's 308 slabs the 52 beyond the CU count cost a second, ROW-form round (0.17 ms, ~1 300 cycles per K-tile for a third of the
// MFMAs, after 0.43 ms for the first 256): 0.69 ms in the layer table against 1.23.
// What is left in the full form: ~3 000 cycles per K-tile against 1 725 of MFMA work — every wave drains its LDS reads at the
// K-tile's barrier, so reads and MFMAs run in phases.
#pragma once
#include "conv_halo.h"

namespace cxrk {

constexpr int WG_RING = 256;                               // pixel slots of the x ring: eight groups of 32
constexpr int WG_XPLANE = (WG_RING + 8) * 128;             // one plane of the ring + the all-zero slot, a multiple of 1 KiB
constexpr int WG_ZERO = WG_RING * 128;                     // byte offset of the all-zero slot in its plane
constexpr int WG_NSD = 4;                                  // dy K-tiles in their ring
constexpr int WG_DPLANE = 32 * 128;                        // one plane of a dy K-tile
constexpr int WG_DSTAGE = 2 * WG_DPLANE;                   // hi | lo
constexpr int WG_NCW = 12, WG_NLW = 4;                     // compute / loader waves
constexpr int WG_NT = 64 * (WG_NCW + WG_NLW);
constexpr int WG_LDS = 2 * WG_XPLANE + WG_NSD * WG_DSTAGE + WG_NSD * 32 * 4;   // + the tap-mask words
static_assert(HALO_MAXW + 1 < 64, "a K-tile's halo must stay within two 32-pixel groups on either side");

// ROW = false: a block computes one whole slab (compute wave (kh, ch, r) -> taps (r, 0..2)).  ROW = true: three blocks share a slab,
// one filter row r each (compute wave (kh, ch, s) -> tap (r, s)): the form of the slabs beyond one per CU, which would otherwise be
// a second round of full-length blocks on a fifth of the chip.  Either way an accumulator element sees the same sequence of MFMAs.
template <bool ROW>
__global__ __launch_bounds__(WG_NT) void conv3x3_wgrad_window_kernel(const unsigned short* __restrict__ x, long xplane,
                                                                    const unsigned short* __restrict__ dy, long dyplane,
                                                                    float* __restrict__ slabs, long slab_stride, int ldc, int M, int H, int W,
                                                                    int nKt, int tiles_per_slab, int slab0) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[WG_LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char* sX = smem;
  unsigned char* sD = smem + 2 * WG_XPLANE;
  unsigned* sMask = reinterpret_cast<unsigned*>(smem + 2 * WG_XPLANE + WG_NSD * WG_DSTAGE);   // [WG_NSD tiles][32 pixels]
  const int slab = slab0 + (ROW ? (int)blockIdx.x / 3 : (int)blockIdx.x);
  const int kt0 = slab * tiles_per_slab, kt1 = min(nKt, kt0 + tiles_per_slab);     // the K range of split-K slab `slab`
  const int nT = kt1 - kt0;                 // >= 1: the launcher starts no slab without pixels
  const int P0 = kt0 * 32;                  // first pixel of the range; ring slots and group numbers are relative to it
  const int Pend = min(M, kt1 * 32);
  const int W1 = W + 1;
#define WG_BARRIER() do { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

  if (wave >= WG_NCW) {
    // ================================================================================================ loader waves
    const int L = (wave - WG_NCW) & 1, G = (wave - WG_NCW) >> 1;
    // piece j of this wave covers rows 8 (2G + j) .. +7 of a 32-pixel group; lane -> (row kk[j], physical 16-byte chunk lane & 7),
    // which holds the logical chunk (lane & 7) ^ (4 * bit 1 of the row).  32 g is a multiple of 4: the same for x groups and dy tiles.
    int kk[2]; unsigned voff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      kk[j] = (2 * G + j) * 8 + (lane >> 3);
      const int lc = (lane & 7) ^ (((kk[j] >> 1) & 1) << 2);
      voff[j] = (unsigned)(kk[j] * 128 + lc * 16);
    }
    const int xlo = max(0, P0 - W1), xhi = min(M, Pend + W1);     // the x pixels this block needs
    auto issue_x = [&](int g) {               // x group g (pixels P0 + 32 g ..), g >= -2
      const long p0 = (long)P0 + 32 * g;
      const __amdgpu_buffer_rsrc_t rs = tile_rsrc(x + L * xplane + p0 * HALO_CH);
      unsigned char* dst = sX + L * WG_XPLANE + (g & 7) * 4096 + 2 * G * 1024;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long p = p0 + kk[j];
        dma16(rs, dst + j * 1024, (p >= xlo && p < xhi) ? voff[j] : VOFF_OOB);
      }
    };
    auto issue_d = [&](int t) {               // dy K-tile t of the range
      const long p0 = (long)P0 + 32 * t;
      const __amdgpu_buffer_rsrc_t rs = tile_rsrc(dy + L * dyplane + p0 * 64);
      unsigned char* dst = sD + (t & (WG_NSD - 1)) * WG_DSTAGE + L * WG_DPLANE + 2 * G * 1024;
#pragma unroll
      for (int j = 0; j < 2; ++j) dma16(rs, dst + j * 1024, (p0 + kk[j] < Pend) ? voff[j] : VOFF_OOB);
    };
    // Loader 0 also writes the tap masks: bit 3 r + s of word [tile & 3][pixel] says that neighbour (r, s) of that dy pixel exists
    // (0 for pixels >= M).  One pixel per lane (the upper half-wave duplicates the lower); (w, h) walk along with the tiles.
    const bool masker = wave == WG_NCW;
    int mw = 0, mh = 0, mm = P0 + (lane & 31);
    if (masker) { mw = mm % W; mh = (mm / W) % H; }
    const int stepr = 32 % W, stepq = (32 / W) % H;
    auto write_mask = [&](int t) {
      unsigned hv = 0, wv = 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if ((unsigned)(mh + d - 1) < (unsigned)H) hv |= 7u << (3 * d);
        if ((unsigned)(mw + d - 1) < (unsigned)W) wv |= 0x49u << d;
      }
      sMask[(t & (WG_NSD - 1)) * 32 + (lane & 31)] = mm < M ? (hv & wv) : 0u;
      mm += 32; mw += stepr; mh += stepq;
      if (mw >= W) { mw -= W; ++mh; }
      if (mh >= H) mh -= H;
    };
    for (int g = -2; g <= 4; ++g) issue_x(g);
    for (int t = 0; t < WG_NSD - 1; ++t) issue_d(t);
    if (masker) for (int t = 0; t < WG_NSD - 1; ++t) write_mask(t);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    WG_BARRIER();                                           // PRE: the masks of tiles 0-2 are written
#pragma unroll 1
    for (int t = 0; t < nT; ++t) {
      // x group t+2, dy tile t; younger: the sets of tiles t-2 and t-1, 4 loads each.  My mask words of tile t+2 are written.
      asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
      WG_BARRIER();
      issue_x(t + 5);
      issue_d(t + 3);
      if (masker) write_mask(t + 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // nothing of mine may land in the LDS of the next block
    return;
  }

  // ================================================================================================== compute waves
  if (tid < 64) *reinterpret_cast<unsigned*>(smem + (tid >> 5) * WG_XPLANE + WG_ZERO + (tid & 31) * 4) = 0u;   // the all-zero slots
  constexpr int NTAP = ROW ? 1 : 3;
  const int kh = wave & 1, ch = (wave >> 1) & 1;                     // ko half, c half
  const int r = ROW ? (int)blockIdx.x % 3 : wave >> 2;               // filter row
  const int s0 = ROW ? wave >> 2 : 0;                                // taps (r, s0 .. s0 + NTAP - 1)
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int colx = ch * 64 + 32 * (g & 1) + 8 * pp;                  // logical byte column of this lane's 8 bytes in an x pixel row
  const int dead = WG_ZERO + colx;
  // the four pixel rows this lane addresses in a K-tile: u = 2 kc + j -> row prow[u] = 16 kc + 8 (g >> 1) + q + 4 j.  live[u][s]:
  // ring byte offset of that row shifted by tap (r, s), for the current tile; a tile later it is 32 slots = 4 KiB further (mod ring).
  int prow[4], live[4][NTAP], ad[4][NTAP];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    prow[u] = 16 * (u >> 1) + 8 * (g >> 1) + q + 4 * (u & 1);
#pragma unroll
    for (int s = 0; s < NTAP; ++s) {
      const int rr = prow[u] + (r - 1) * W + s0 + s - 1;
      live[u][s] = ((rr & (WG_RING - 1)) << 7) | (colx ^ ((rr & 2) << 5));
    }
  }
  // ad = the mask bit says the neighbour exists ? live : dead, without a branch (EXEC stays all ones for the transposing reads)
  auto select = [&](const unsigned (&mk)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < NTAP; ++s) {
        const int sel = (int)(mk[u] << (31 - (3 * r + s0 + s))) >> 31;
        ad[u][s] = dead ^ ((live[u][s] ^ dead) & sel);
        live[u][s] = (live[u][s] + 32 * 128) & (WG_RING * 128 - 1);
      }
  };
  f32x16 acc[NTAP];
#pragma unroll
  for (int s = 0; s < NTAP; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;

  typedef s16x4 __attribute__((address_space(3))) * lds_v4;
  auto tr2 = [&](const unsigned char* a0, const unsigned char* a1) {
    const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(a0));
    const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(a1));
    const s16x8 v = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  struct BFrag { bf16x8 h[2], l[2]; };        // one tap, both k-steps, hi / lo
  auto read_b = [&](BFrag& f, int s) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      f.h[kc] = tr2(sX + ad[2 * kc][s], sX + ad[2 * kc + 1][s]);
      f.l[kc] = tr2(sX + WG_XPLANE + ad[2 * kc][s], sX + WG_XPLANE + ad[2 * kc + 1][s]);
    }
  };
  bf16x8 ah[2], al[2];
  auto mfma6 = [&](f32x16& c, const BFrag& f) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[kc], f.h[kc], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kc], f.l[kc], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kc], f.h[kc], c, 0, 0, 0);
    }
  };
  auto read_mask = [&](unsigned (&mk)[4], int t) {
#pragma unroll
    for (int u = 0; u < 4; ++u) mk[u] = sMask[(t & (WG_NSD - 1)) * 32 + prow[u]];
  };

  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  WG_BARRIER();                                             // PRE
  {
    unsigned mk[4];
    read_mask(mk, 0);
    select(mk);
  }
#pragma unroll 1
  for (int t = 0; t < nT; ++t) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    WG_BARRIER();
    const unsigned char* dt = sD + (t & (WG_NSD - 1)) * WG_DSTAGE;
    BFrag B0, B1;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      ah[kc] = pw_frag_mc<64>(dt, kh * 32, kc, lane);
      al[kc] = pw_frag_mc<64>(dt + WG_DPLANE, kh * 32, kc, lane);
    }
    read_b(B0, 0);
    if constexpr (!ROW) read_b(B1, 1);
    unsigned mk[4];
    read_mask(mk, t + 1);          // written two tiles ago (the loader's barrier sequence)
    mfma6(acc[0], B0);
    if constexpr (!ROW) read_b(B0, 2);
    select(mk);                    // the addresses of tile t+1, under the MFMAs
    if constexpr (!ROW) { mfma6(acc[1], B1); mfma6(acc[NTAP - 1], B0); }
  }
  // exit: the accumulators straight to the slab, [ko][tap][c] with row stride ldc.  C/D map of the 32 x 32 MFMA:
  // column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): a register is two 128-byte runs.
  float* out = slabs + (long)slab * slab_stride;
#pragma unroll
  for (int s = 0; s < NTAP; ++s) {
    const int col = (r * 3 + s0 + s) * HALO_CH + ch * 32 + (lane & 31);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = kh * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
      out[(long)row * ldc + col] = acc[s][e];
    }
  }
#undef WG_BARRIER
}

// CXRK_HALO_WGRAD=0 sends these layers back to the implicit GEMM; read on every call, so one process can run both paths
static inline bool halo_wgrad_enabled() { const char* e = getenv("CXRK_HALO_WGRAD"); return e ? atoi(e) != 0 : true; }
// the shapes the kernel takes (the process-wide CXRK_HALO switch aside): those of halo_applies, and pixel indices that stay in int
static inline bool halo_wgrad_shape(int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad) {
  return R == 3 && S == 3 && stride == 1 && pad == 1 && C == HALO_CH && Ko == 64 && W >= 1 && W <= HALO_MAXW && H >= 1 && N >= 1 &&
         (long)N * H * W < (1L << 31) - 4096;
}
// The slabs are those of the split-K implicit GEMM (launch_gemm_pw: `splitk` K ranges of kchunk pixels, a multiple of the K-tile),
// and every accumulator element sees the MFMAs of its range in that kernel's order (per K-tile and k-step lo*hi, hi*lo, hi*hi), so
// slabs, reduction and result are BIT-IDENTICAL to that path.  Returns the number of slabs written (>= 1) or an error.
static int launch_conv3x3_wgrad_window(const unsigned short* x, long xplane, const unsigned short* dy, long dyplane, float* slabs, long slab_stride,
                                       int ldc, int M, int H, int W, int splitk, hipStream_t stream) {
  if (M <= 0 || W > HALO_MAXW || W < 1 || H < 1) return CXRK_ERR_ARG;
  int kchunk = M;
  if (splitk > 1) { kchunk = ceil_div(ceil_div(M, splitk), BK) * BK; splitk = ceil_div(M, kchunk); }
  else splitk = 1;
  const int nKt = ceil_div(M, 32);
  const int tiles = splitk > 1 ? kchunk / 32 : nKt;
  // one whole slab per block for as many slabs as there are CUs; the rest as three blocks per slab
  const int nfull = splitk < halo_cus() ? splitk : halo_cus();
  hipLaunchKernelGGL(conv3x3_wgrad_window_kernel<false>, dim3((unsigned)nfull), dim3(WG_NT), 0, stream, x, xplane, dy, dyplane, slabs, slab_stride,
                     ldc, M, H, W, nKt, tiles, 0);
  CXRK_LAUNCH_CHECK();
  const LaunchLabel label{"conv3x3_wgrad_window_kernel", nullptr, nullptr, nullptr, 0, 0, 1};
  note_launch(label, 64.0 * ldc * 32 * tiles * nfull);
  if (splitk > nfull) {
    hipLaunchKernelGGL(conv3x3_wgrad_window_kernel<true>, dim3((unsigned)(3 * (splitk - nfull))), dim3(WG_NT), 0, stream, x, xplane, dy, dyplane,
                       slabs, slab_stride, ldc, M, H, W, nKt, tiles, nfull);
    CXRK_LAUNCH_CHECK();
    note_launch(label, 64.0 * ldc * 32 * tiles * (splitk - nfull));
  }
  return splitk;
}

}  // namespace cxrk
