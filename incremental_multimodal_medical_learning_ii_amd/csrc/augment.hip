// On-device image augmentation for the joint step (opt-in): random affine (rotation, translation, zoom, horizontal flip) with
// bilinear sampling and zero fill, brightness / contrast jitter, fused into the NCHW -> NHWC transform that feeds the ResNet stem.
// The contract -- what is drawn, from which Philox block, and the map -- is stated in include/cxrk.h ("augment") and restated in
// numpy by tests/augment_ref.py.  Two kernels:
//   augment_params_kernel  one block per image: the image's eight uniforms -> its parameter row
//                          (a00 a01 a02 a10 a11 a12 gain bias), plus the image mean when the contrast jitter needs it;
//   augment_nhwc_kernel    one thread per output pixel: source coordinates by two fmaf each, four range-checked taps per channel,
//                          one 16-byte store per four output channels.
// No workspace, no atomics; every random quantity of image n is a function of (seed, call counter, global image index n) only.
#include "cxrk_common.h"
#include "dropout.h"
#include "../../include/cxrk.h"

using namespace cxrk;

namespace {

constexpr int AUG_PARAMS_THREADS = 256;   // fixed: the order of the mean's reduction is part of the contract

struct AugSpec {
  float rotate_rad;       // rotate_deg * pi / 180
  float translate;        // fraction of the output size
  float log_zlo, log_zd;  // log lo, log hi - log lo
  float flip_p, brightness, contrast;
};

// uniform in (0, 1), exactly representable in fp32: 23 random bits and a trailing one
__device__ __forceinline__ float aug_uniform(unsigned w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__global__ __launch_bounds__(AUG_PARAMS_THREADS) void augment_params_kernel(const float* __restrict__ x, long img_elems, AugSpec sp,
                                                                             unsigned k0, unsigned k1, unsigned c3, long row_offset,
                                                                             float Hs, float Ws, float Ho, float Wo,
                                                                             float* __restrict__ params) {
  __shared__ float sh[16];
  const int i = blockIdx.x;
  float mean = 0.f;
  if (x) {   // wave-uniform: null when contrast == 0 (the source is not read at all then)
    const float* __restrict__ xi = x + (long)i * img_elems;
    float s = 0.f;
#pragma unroll 4
    for (long e = threadIdx.x; e < img_elems; e += AUG_PARAMS_THREADS) s += xi[e];
    mean = block_sum(s, sh) / (float)img_elems;
  }
  if (threadIdx.x != 0) return;
  const unsigned n = (unsigned)(row_offset + i);
  const uint4 r0 = philox4x32_10(make_uint4(0u, n, 0u, c3), k0, k1);
  const uint4 r1 = philox4x32_10(make_uint4(1u, n, 0u, c3), k0, k1);
  const float s0 = 2.f * aug_uniform(r0.x) - 1.f, s1 = 2.f * aug_uniform(r0.y) - 1.f, s2 = 2.f * aug_uniform(r0.z) - 1.f;
  const float u3 = aug_uniform(r0.w), u4 = aug_uniform(r1.x);
  const float s5 = 2.f * aug_uniform(r1.y) - 1.f, s6 = 2.f * aug_uniform(r1.z) - 1.f;
  const float phi = s0 * sp.rotate_rad;
  const float cs = cosf(phi), sn = sinf(phi);
  const float tx = s1 * sp.translate * Wo, ty = s2 * sp.translate * Ho;
  const float iz = 1.f / expf(sp.log_zlo + u3 * sp.log_zd);
  const float f = u4 < sp.flip_p ? -1.f : 1.f;
  const float kx = (Ws / Wo) * iz, ky = (Hs / Ho) * iz;
  const float a00 = kx * cs * f, a01 = -(kx * sn), a10 = ky * sn * f, a11 = ky * cs;
  const float ox = 0.5f - 0.5f * Wo - tx, oy = 0.5f - 0.5f * Ho - ty;   // output pixel (0, 0) relative to the shifted centre
  const float bb = 1.f + s5 * sp.brightness, cc = 1.f + s6 * sp.contrast;
  float4* __restrict__ row = reinterpret_cast<float4*>(params + (long)i * 8);
  row[0] = make_float4(a00, a01, 0.5f * Ws + (a00 * ox + a01 * oy), a10);
  row[1] = make_float4(a11, 0.5f * Hs + (a10 * ox + a11 * oy), bb * cc, bb * mean * (1.f - cc));
}

// value of source pixel (yy, xx) of one channel plane, 0 outside the image
__device__ __forceinline__ float aug_tap(const float* __restrict__ plane, int yy, int xx, int Hs, int Ws) {
  return ((unsigned)yy < (unsigned)Hs && (unsigned)xx < (unsigned)Ws) ? plane[(long)yy * Ws + xx] : 0.f;
}
// acc + w * v, a tap of weight zero left out altogether: its value (a NaN, an Inf) must not reach the output
__device__ __forceinline__ float aug_acc(float acc, float w, float v) { return w != 0.f ? fmaf(w, v, acc) : acc; }

template <int C>   // channels of the source: 3, or 1 replicated to three (ExpandChannels)
__global__ __launch_bounds__(256) void augment_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                           float* __restrict__ y, long total, int Hs, int Ws, int Ho, int Wo,
                                                           int Cpad, int clamp01) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;   // output pixel (n, yo, xo); a wave writes 64 adjacent pixels of a row
  if (t >= total) return;
  const int xo = (int)(t % Wo); const long q = t / Wo;
  const int yo = (int)(q % Ho); const long n = q / Ho;
  const float4 pa = *reinterpret_cast<const float4*>(params + n * 8);
  const float4 pb = *reinterpret_cast<const float4*>(params + n * 8 + 4);
  const float xs = fmaf(pa.x, (float)xo, fmaf(pa.y, (float)yo, pa.z));
  const float ys = fmaf(pa.w, (float)xo, fmaf(pb.x, (float)yo, pb.y));
  // pixel centres at +0.5.  Clamped first: every coordinate below -1 or above the size has four empty taps anyway, and the
  // conversion to int stays in range whatever the parameters are.
  const float fx = fminf(fmaxf(xs - 0.5f, -2.f), (float)Ws + 1.f), fy = fminf(fmaxf(ys - 0.5f, -2.f), (float)Hs + 1.f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float wx1 = fx - x0f, wy1 = fy - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
  const float gain = pb.z, bias = pb.w;
  const long plane = (long)Hs * Ws;
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ p = x + (n * C + c) * plane;
    float a = aug_acc(0.f, w00, aug_tap(p, y0, x0, Hs, Ws));
    a = aug_acc(a, w01, aug_tap(p, y0, x0 + 1, Hs, Ws));
    a = aug_acc(a, w10, aug_tap(p, y0 + 1, x0, Hs, Ws));
    a = aug_acc(a, w11, aug_tap(p, y0 + 1, x0 + 1, Hs, Ws));
    a = fmaf(gain, a, bias);
    if (clamp01) a = a < 0.f ? 0.f : (a > 1.f ? 1.f : a);   // comparisons: a NaN stays a NaN
    v[c] = a;
  }
  float4* __restrict__ o = reinterpret_cast<float4*>(y + t * Cpad);
  o[0] = C == 3 ? make_float4(v[0], v[1], v[2], 0.f) : make_float4(v[0], v[0], v[0], 0.f);
  for (int c4 = 1; c4 < Cpad / 4; ++c4) o[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

extern "C" int cxrk_augment_params(const float* x, int N, int C, int Hs, int Ws, int Ho, int Wo, float rotate_deg, float translate,
                                   float zoom_lo, float zoom_hi, float flip_p, float brightness, float contrast,
                                   unsigned long long seed, unsigned counter, long row_offset, float* params, hipStream_t stream) {
  CXRK_CHECK_ARG(params && aligned16(params) && N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0 && row_offset >= 0);
  CXRK_CHECK_ARG(zoom_lo > 0.f && zoom_hi >= zoom_lo && flip_p >= 0.f && flip_p <= 1.f && brightness < 1.f && contrast < 1.f);
  CXRK_CHECK_ARG(contrast == 0.f || x != nullptr);
  if (C != 1 && C != 3) return CXRK_ERR_UNSUPPORTED;
  const float llo = logf(zoom_lo);
  const AugSpec sp = {rotate_deg * 0.017453292519943295f, translate, llo, logf(zoom_hi) - llo, flip_p, brightness, contrast};
  hipLaunchKernelGGL(augment_params_kernel, dim3(N), dim3(AUG_PARAMS_THREADS), 0, stream, contrast != 0.f ? x : nullptr,
                     (long)C * Hs * Ws, sp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32),
                     ((counter & 0xffffffu) << 8) | 0xF0u, row_offset, (float)Hs, (float)Ws, (float)Ho, (float)Wo, params);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}

extern "C" int cxrk_augment_nhwc(const float* x, const float* params, float* y, int N, int C, int Hs, int Ws, int Ho, int Wo, int Cpad,
                                 int clamp01, hipStream_t stream) {
  CXRK_CHECK_ARG(x && params && y && N > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0);
  CXRK_CHECK_ARG(Cpad >= 4 && (Cpad % 4) == 0 && aligned16(y) && aligned16(params));   // 16-byte stores / parameter loads only
  if (C != 1 && C != 3) return CXRK_ERR_UNSUPPORTED;
  const long total = (long)N * Ho * Wo;
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return CXRK_ERR_UNSUPPORTED;
  if (C == 3)
    hipLaunchKernelGGL(augment_nhwc_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, stream, x, params, y, total, Hs, Ws, Ho, Wo, Cpad, clamp01);
  else
    hipLaunchKernelGGL(augment_nhwc_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stream, x, params, y, total, Hs, Ws, Ho, Wo, Cpad, clamp01);
  CXRK_LAUNCH_CHECK();
  return CXRK_OK;
}
