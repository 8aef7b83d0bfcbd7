/* cxrk — C-ABI of the MI355X (gfx950) kernels behind the joint image+text contrastive training step.
 *
 * The reference (marcomistretta/incremental_multimodal_medical_learning_II) is pure Python on PyTorch: it has no
 * FFI layer of its own, so each entry point cites the Python function whose arithmetic it replaces
 * (paths relative to the reference root).  The host side (incremental_multimodal_medical_learning_ii_amd/) binds this
 * library with ctypes and keeps the reference's class / method surface; INTEGRATION.md shows the binding stub.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; fp32 data; int64 ids/masks; no hidden allocation, no hidden synchronisation;
 *   - work is enqueued on `stream` (the caller's current HIP stream) and the call returns immediately;
 *   - scratch memory is passed in (`ws`, `ws_bytes`); the matching `*_ws_bytes` function sizes it: an entry point touches
 *     nothing outside [ws, ws + that many bytes) and reads nothing there that it has not written in the same call.  `ws` must
 *     be 256-byte aligned (hipMalloc and every caching allocator give that): it is carved into regions at 256-byte offsets
 *     and read as 16-byte vectors / 8-byte sort keys; an entry point that uses a workspace returns -1 for a misaligned one;
 *   - return 0 on success, <0 on error: -1 bad argument/alignment, -2 workspace too small, -3 launch failure,
 *     -4 unsupported shape.  The Python wrappers raise RuntimeError/ValueError for these, mirroring the
 *     reference's exception behaviour;
 *   - row-major tensors; activations of the image encoder are NHWC, filters are [Ko][R][S][C] (= a torch OIHW
 *     tensor in channels_last memory format);
 *   - non-finite values propagate as in the torch operation the entry point cites (float64 CPU reference, autograd for the
 *     backwards): an output element that is NaN there is non-finite here, and one that is finite there is finite here (a NaN does
 *     not leak into other rows / channels / segments / images).  ReLU, max-pool, the L2-norm clamp, the cosine maximum and the
 *     weight_reset threshold keep a NaN (comparisons, never fmaxf / fminf on the value itself); the ReLU decision bit of a NaN
 *     output is 0; masks select (a NaN gradient at a ReLU-off position gives 0).  For +Inf only "non-finite there => non-finite
 *     here" holds: planes storage turns Inf into NaN (lo = Inf - Inf).  Where the reference multiplies by an exact zero (masked
 *     keys, dropped elements) the result may be 0 or NaN.  Backward entry points are specified for a non-finite incoming gradient
 *     with finite saved state.
 */
#ifndef CXRK_H
#define CXRK_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------
 * gemm_bias_act — every nn.Linear of the path: BERT query/key/value/dense/intermediate/output
 * (HF BertLayer under health_multimodal/text/model/modelling_cxrbert.py:87-95), BertProjectionHead
 * (modelling_cxrbert.py:43-49), models.myMLP / myLinearModel (models.py:7-26), the projector's 1x1 conv with bias
 * (health_multimodal/image/model/modules.py:32-33) and the logits block I_hat @ T_hat^T.
 *   C[M,N] = act( alpha * op(A)[M,K] @ op(B)[K,N] + bias[N] + R ) (* gelu'(aux) | * (aux>0))
 *   transA=0: A[m*lda+k]   transA=1: A[k*lda+m]      transB=0: B[k*ldb+n]   transB=1: B[n*ldb+k]
 *   act: 0 none, 1 relu, 2 gelu(erf).  auxmode: 0 none, 1 multiply by (aux>0), 2 multiply by gelu'(aux).
 *   C2 (optional) receives the pre-activation value.  accumulate: C += result (R must be NULL).
 *   splitk>1: deterministic split-K through `ws` (plain epilogue only) — used for weight gradients.
 * fwd:  Y = X W^T + b           -> transA=0, transB=1
 * bwd:  dX = dY W               -> transA=0, transB=0 ;  dW = dY^T X -> transA=1, transB=0 (split-K)
 */
size_t cxrk_gemm_splitk_ws_bytes(int M, int N, int splitk);
/* Split-K factor the library recommends for a weight-gradient shaped GEMM (M x N output, K = rows reduced over): enough
 * slabs to fill the chip with the tile the launch will take in the current precision mode. */
int cxrk_gemm_wgrad_splitk(int M, int N, int K, int planes);
/* 1 when a launch of this GEMM shape takes the 256x256 tile (reporting only).  kind: 0 or 3 dense layer / weight gradient,
 * 1 convolution forward, 2 convolution data gradient. */
int cxrk_gemm_wide_tile(int M, int N, long K, int splitk, int kind);
/* What the last call of a GEMM-family entry point (cxrk_gemm_f32 / _pl, cxrk_conv_bn_act_fwd* / _bwd_data* / _bwd_params*, cxrk_stem_pool_*) on the
 * calling thread launched: the kernel instantiation as scripts/pmc_summary_key.py abbreviates its rocprofv3 name ("" if the call
 * launched nothing; valid until the thread's next query), the number of MFMA kernel launches (reductions not counted), and whether
 * the mainloop is the split-bf16 one.  Of several launches the label is that of the largest M*N*K (the first on ties). */
const char* cxrk_last_launch_label(void);
int cxrk_last_launch_count(void);
int cxrk_last_launch_split_bf16(void);
int cxrk_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                  float* C, long ldc, const float* bias, const float* R, long ldr, const float* aux, long ldaux,
                  int auxmode, float* C2, long ldc2, int act, float alpha, int accumulate, int splitk, float* ws,
                  size_t ws_bytes, hipStream_t stream);

/* The same contraction on planes operands (see "Storage formats" below): A and B are planes; the output is fp32 (C) or planes
 * (Cp), the residual fp32 (R) or planes (Rp).  auxmode 2 = multiply by gelu'(aux) (aux fp32), 3 = multiply by the ReLU decision
 * bits `maskin`; `maskout` (with act 1) receives the decision bits of this launch's ReLU.  transA && transB is not provided. */
int cxrk_gemm_pl(int transA, int transB, int M, int N, int K, const void* A, long lda, long aplane, const void* B, long ldb,
                 long bplane, float* C, void* Cp, long ldc, long cplane, const float* bias, const float* R, const void* Rp,
                 long ldr, long rplane, const float* aux, long ldaux, int auxmode, const unsigned char* maskin, long ldmaskin,
                 unsigned char* maskout, long ldmaskout, float* C2, long ldc2, int act, float alpha, int accumulate, int splitk,
                 float* colsum, int colsum_accumulate, float* ws, size_t ws_bytes, hipStream_t stream);
size_t cxrk_gemm_pl_colsum_ws_bytes(int M, int N);   /* ws for the fused column sums (`colsum` != NULL; needs splitk == 1) */
/* fp32 tensor -> planes (weights once per step, inputs of the path) and back (host-side consumers, tests); n % 8 == 0. */
int cxrk_split_planes(const float* x, long n, void* out, long plane, hipStream_t stream);
int cxrk_merge_planes(const void* x, long plane, long n, float* out, hipStream_t stream);

/* out[cols] (+)= alpha * sum_rows X[rows, cols] — bias gradients, BN beta gradients, position/type embedding grads. */
size_t cxrk_colsum_ws_bytes(long rows, int cols);
int cxrk_colsum(const float* X, long ldx, long rows, int cols, float* out, float alpha, int accumulate, float* ws,
                size_t ws_bytes, hipStream_t stream);
int cxrk_colsum_pl(const void* X, long ldx, long plane, long rows, int cols, float* out, float alpha, int accumulate, float* ws,
                   size_t ws_bytes, hipStream_t stream);
/* out[cols] = alpha * sum_rows (X[r][c] - mean[c])^2, X fp32 (plane == 0) or planes (plane > 0); ws as for cxrk_colsum.  The second
 * pass of the batch variance `torch.nn.BatchNorm2d` stores in train mode (momentum 1): `ImageModel.calibrate_batchnorm_`, which
 * gives synthetic weights statistics that match their activations (the reference only loads trained weights, model.py:117-118). */
int cxrk_colvar(const void* X, long ldx, long plane, long rows, int cols, const float* mean, float* out, float alpha, float* ws,
                size_t ws_bytes, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * conv_bn_act — torchvision Bottleneck conv + eval-mode BatchNorm + ReLU (+ residual) as used by
 * health_multimodal/image/model/resnet.py:34-47 and the projector's conv+BN+ReLU (modules.py:43-46).
 * cxrk_bn_fold: w_scaled = w * gamma*rsqrt(var+eps) (per output channel, channel-padded to Cpad),
 *               scale = gamma*rstd, shift = beta - mean*scale, rstd = rsqrt(var+eps).
 * fwd:        y = relu?( conv(x, w_scaled) + shift + residual? )
 * bwd_data:   dx = (relu_src>0)? * ( conv^T(dy, w_scaled) + residual? )        (dy already masked by its own ReLU)
 * bwd_params: dW = scale * wgrad(x, dy);  dbeta = sumdy = sum dy;
 *             dgamma = sum dy * xhat = rstd * (<w, wgrad(x, dy)> - mean * sumdy): taken from the raw weight gradient the
 *             call forms anyway (no activation is re-read, gamma is never divided by).
 *
 * Storage formats.  The fp32 entry points take fp32 tensors.  The `_pl` entry points take "planes" tensors: x stored as two
 * bf16 planes hi = bf16(x), lo = bf16(x - hi) of the same shape, the lo plane `*plane` ELEMENTS behind the hi plane (4 bytes
 * per element like fp32; pointers are `void*`).  They are what the encoders use in split-bf16 mode: the MFMA mainloops then
 * load operands without any conversion work.  ReLU decisions travel as bit masks: byte [pixel][channel / 8], bit channel % 8.
 *
 * Geometry contract (tests/test_conv_geometry_gpu.py).  x [N][H][W][C], w [Ko][R][S][C], y / dy [N][Ho][Wo][Ko] with
 * Ho = floor((H + 2 pad - R) / stride) + 1, Wo likewise; one stride and one pad for both axes; H != W and R != S are computed like
 * squares, and pad is free of R (0 .. any, not only R / 2).  A call either computes exactly that or returns an error with no
 * output byte written.
 *   all three, both storage forms — CXRK_ERR_ARG: N, H, W, R or S <= 0; pad < 0; stride other than 1 or 2; Ho <= 0 or Wo <= 0 (the
 *     filter does not fit the padded image once); 2^31 or more GEMM rows (N Ho Wo; data gradient: N H W); operands not 16-byte aligned.
 *     CXRK_ERR_UNSUPPORTED: the images under one 256-row tile span 2 GiB or more.
 *   fwd       fp32: C % 4 == 0, else CXRK_ERR_ARG; any R, S (C % 32 == 0 with R S <= 32 and R <= 8 gathers tap-wise, anything else per
 *             lane: the stem).  _pl: Ko % 8 == 0, and Ko % 64 == 0 with maskout (the bits are written 64 channels at a time), else
 *             CXRK_ERR_ARG; with in_planes = 1, C % 32 == 0, R S <= 32 and R <= 8, else CXRK_ERR_UNSUPPORTED; with in_planes = 0 the
 *             fp32 rules.
 *   bwd_data  C and Ko % 4 == 0 (_pl: % 8), else CXRK_ERR_ARG.  Ko % 32 != 0, R S > 32 or R > 8: CXRK_ERR_UNSUPPORTED.  Stride 2 runs
 *             per output-parity class and takes R, S <= 3 only (CXRK_ERR_ARG above); pad < R - 1 is fine (taps then reach row / column
 *             -1 of dy and are masked like those past the end).  A class no tap reaches (a 1-wide filter extent at stride 2 along an axis
 *             of >= 2 pixels) is exactly zero and exists in the plain form only: residual, relu_src / maskin -> CXRK_ERR_ARG; sums
 *             -> CXRK_ERR_ARG whenever R == 1 at stride 2.  _pl_s2res: stride 1 only (CXRK_ERR_ARG).
 *   bwd_params Cpad and Ko % 4 == 0 (_pl: C and Ko % 8), 1 <= C <= Cpad, else CXRK_ERR_ARG; any R, S; dw has the REAL channel count C
 *             and nothing is written for the padded channels.  One image of 2^31 / 12 bytes or more: CXRK_ERR_UNSUPPORTED.
 *             cxrk_conv_wgrad_ws_bytes returns 0 for a geometry the call refuses.
 */
int cxrk_bn_fold(const float* w, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                 float eps, int Ko, int taps, int C, int Cpad, float* w_scaled, float* scale, float* shift,
                 float* rstd, hipStream_t stream);
int cxrk_bn_fold_pl(const float* w, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                    float eps, int Ko, int taps, int C, int Cpad, void* w_scaled, long wplane, float* scale, float* shift,
                    float* rstd, hipStream_t stream);
int cxrk_conv_bn_act_fwd(const float* x, const float* w_scaled, const float* shift, const float* residual, float* y,
                         int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad, int relu,
                         hipStream_t stream);
/* y (and the optional residual) are planes; in_planes = 1: x and w_scaled are planes too, 0: they are fp32 (the stem).
 * maskout (optional, needs relu) receives the ReLU decision bits of y. */
int cxrk_conv_bn_act_fwd_pl(const void* x, long xplane, const void* w_scaled, long wplane, int in_planes, const float* shift,
                            const void* residual, long rplane, void* y, long yplane, unsigned char* maskout, int N, int H,
                            int W, int C, int Ko, int R, int S, int stride, int pad, int relu, hipStream_t stream);
/* sums (optional, [C]) = column sums of dx: the BatchNorm beta gradient of the unit that produced relu_src / maskin (dx is
 * that unit's masked output gradient), reduced in the data-gradient epilogue; needs ws of
 * cxrk_conv_bwd_data_colsum_ws_bytes().  Not for 1x1 stride-2 filters.  With sums, dx / residual / relu_src must be 16-byte
 * aligned (CXRK_ERR_ARG otherwise: the column sums exist in the 16-byte epilogue only). */
size_t cxrk_conv_bwd_data_colsum_ws_bytes(int N, int H, int W, int C, int stride);
int cxrk_conv_bn_act_bwd_data(const float* dy, const float* w_scaled, const float* residual, const float* relu_src,
                              float* dx, int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad,
                              float* sums, float* ws, size_t ws_bytes, hipStream_t stream);
int cxrk_conv_bn_act_bwd_data_pl(const void* dy, long dyplane, const void* w_scaled, long wplane, const void* residual,
                                 long rplane, const unsigned char* maskin, void* dx, long dxplane, int N, int H, int W, int C,
                                 int Ko, int R, int S, int stride, int pad, float* sums, float* ws, size_t ws_bytes,
                                 hipStream_t stream);
/* The same with a COMPACT residual: planes [N, (H + 1) / 2, (W + 1) / 2, C] = the identity-branch gradient at the pixels with even
 * (h, w) only (the data gradient of a 1x1 / stride-2 projection shortcut, torchvision Bottleneck.downsample, resnet.py:36-47);
 * stride must be 1; CXRK_ERR_UNSUPPORTED when the compact tensor exceeds 2 GiB per plane (use the dense form then). */
int cxrk_conv_bn_act_bwd_data_pl_s2res(const void* dy, long dyplane, const void* w_scaled, long wplane, const void* residual_s2,
                                 long rplane, const unsigned char* maskin, void* dx, long dxplane, int N, int H, int W, int C,
                                 int Ko, int R, int S, int stride, int pad, float* sums, float* ws, size_t ws_bytes,
                                 hipStream_t stream);
size_t cxrk_conv_wgrad_ws_bytes(int N, int H, int W, int Cpad, int Ko, int R, int S, int stride, int pad);
int cxrk_conv_bn_act_bwd_params(const float* x, const float* dy, const float* w, const float* scale, const float* rstd,
                                const float* rmean, const float* sumdy, float* dw, float* dgamma, float* dbeta,
                                int accumulate, int N, int H, int W, int C, int Cpad, int Ko, int R, int S, int stride,
                                int pad, float* ws, size_t ws_bytes, hipStream_t stream);
/* Planes operands.  Which kernel takes which shapes: 3x3 / stride 1 / pad 1 with C = Ko = 64 and rows of <= 58 pixels go to the
 * window-resident kernel (csrc/conv_halo_wgrad.h: x resident in an LDS ring for all nine taps, one block per split-K slab — the
 * implicit GEMM's slabs, bit-identical result) unless CXRK_HALO=0 (read once) or CXRK_HALO_WGRAD=0 (read on every call); everything else is a split-K
 * implicit GEMM on the LDS-DMA tiles (256 x 256 where the policy picks it, 64 x 256 for Ko <= 64, 128 x 128 otherwise).
 * Both paths write the same slabs: cxrk_conv_wgrad_ws_bytes is one bound for both. */
int cxrk_conv_bn_act_bwd_params_pl(const void* x, long xplane, const void* dy, long dyplane, const float* w, const float* scale,
                                   const float* rstd, const float* rmean, const float* sumdy, float* dw, float* dgamma,
                                   float* dbeta, int accumulate, int N, int H, int W, int C, int Ko, int R, int S, int stride,
                                   int pad, float* ws, size_t ws_bytes, hipStream_t stream);

/* Boundary layout transforms: torch NCHW input (model.py:141) <-> NHWC working layout. */
int cxrk_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, int Cpad, hipStream_t stream);
int cxrk_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, hipStream_t stream);

/* ---- augment (train mode, opt-in through ImageModel.augment_call / JointContrastiveTrainer(augment=...)) ----
 * The same boundary transform with a random affine map (rotation, translation, zoom, horizontal flip; bilinear taps, zero fill)
 * and a brightness / contrast jitter: the train-time transforms BioViL's image encoder was trained with, which the reference keeps
 * commented out above `get_bio_vil_pipeline` (DataRetrieval.py).  It takes the place of cxrk_nchw_to_nhwc in front of the stem.
 * Every random quantity of image n is a pure function of (seed, call counter, n = row_offset + index within the call).  Rule:
 *   Philox4x32-10 (csrc/dropout.h), key = (seed & 0xffffffff, seed >> 32), two blocks b = 0, 1 per image with
 *   counter = (b, n, 0, (counter & 0xffffff) << 8 | 0xF0)   (the low byte 0xF0 = layer 60, site 0 is no dropout word: site 0 exists at layer 0 only),
 *   u_k = ((w_k >> 9) + 0.5) * 2^-23 for the eight output words w_0..w_7: 24 significant bits, so exactly an fp32 value in (0, 1);
 *   phi = (2 u0 - 1) rotate_deg pi / 180;  tx = (2 u1 - 1) translate Wo;  ty = (2 u2 - 1) translate Ho;
 *   z = exp(log zoom_lo + u3 (log zoom_hi - log zoom_lo));  flip iff u4 < flip_p;
 *   b = 1 + (2 u5 - 1) brightness;  c = 1 + (2 u6 - 1) contrast;  u7 is reserved.
 * Inverse map, pixel centres at + 0.5, F = diag(flip ? -1 : 1, 1), R(phi) = [cos -sin; sin cos]:
 *   (xs, ys) = (Ws / 2, Hs / 2) + diag(Ws / Wo, Hs / Ho) (1 / z) R(phi) F (xo + 1/2 - Wo / 2 - tx, yo + 1/2 - Ho / 2 - ty)
 * sampled bilinearly at (xs - 1/2, ys - 1/2), taps outside the source contributing zero (torch grid_sample, mode "bilinear",
 * padding_mode "zeros", align_corners False), then v' = gain v + bias on the sampled value (fill included) with gain = b c,
 * bias = b m (1 - c), m = the mean of source image n over all its elements, and with clamp01 v' clamped to [0, 1].
 * augment_params: params[N][8] (an output, 16-byte aligned) = a00 a01 a02 a10 a11 a12 gain bias per image, with
 *               xs = a00 xo + a01 yo + a02, ys = a10 xo + a11 yo + a12.  One block per image; m is summed by 256 threads over
 *               elements e = thread, thread + 256, ... and then in a fixed order, so it does not depend on how a batch is cut.  The
 *               source is not read when contrast == 0 (x may be NULL then).
 * augment_nhwc:  x[N][C][Hs][Ws] (C = 3, or 1 replicated to three as ExpandChannels does) -> y[N][Ho][Wo][Cpad], padded channels 0;
 *               Cpad % 4 == 0 and y, params 16-byte aligned (-1 otherwise); C other than 1 or 3: -4.  A tap of weight zero is left
 *               out: an output is non-finite iff one of its taps of non-zero weight is (a NaN survives clamp01; -0 may become +0).
 *               With the identity spec and Ho x Wo = Hs x Ws the output equals cxrk_nchw_to_nhwc's.
 */
int cxrk_augment_params(const float* x, int N, int C, int Hs, int Ws, int Ho, int Wo, float rotate_deg, float translate,
                        float zoom_lo, float zoom_hi, float flip_p, float brightness, float contrast, unsigned long long seed,
                        unsigned counter, long row_offset, float* params, hipStream_t stream);
int cxrk_augment_nhwc(const float* x, const float* params, float* y, int N, int C, int Hs, int Ws, int Ho, int Wo, int Cpad,
                      int clamp01, hipStream_t stream);

/* maxpool — nn.MaxPool2d(3, stride 2, pad 1) of the ResNet stem (resnet.py:37). idx = winning tap per output. */
int cxrk_maxpool_fwd(const float* x, float* y, unsigned char* idx, int N, int H, int W, int C, hipStream_t stream);
int cxrk_maxpool_bwd(const float* dy, const unsigned char* idx, const float* x, float* dx, int N, int H, int W, int C,
                     int relu_mask, hipStream_t stream);
/* planes variants: x / y / dy / pooled are planes.  The backward masks with the stem ReLU through the sign of `pooled` (the
 * pooled value IS the winning input) and writes dx in fp32 (it feeds the stem's exact-fp32 weight gradient). */
int cxrk_maxpool_fwd_pl(const void* x, long xplane, void* y, long yplane, unsigned char* idx, int N, int H, int W, int C,
                        hipStream_t stream);
int cxrk_maxpool_bwd_pl(const void* dy, long dyplane, const unsigned char* idx, const void* pooled, float* dx, int N, int H,
                        int W, int C, hipStream_t stream);

/* The stem with its max-pool fused — self.conv1, self.bn1, self.relu, self.maxpool (resnet.py:34-38) in one kernel: the stem output
 * [N,Hs,Ws,64] never reaches memory.  x: fp32 [N,H,W,4]; w_scaled: fp32 [64][7][7][4] and shift as for cxrk_conv_bn_act_fwd_pl with
 * in_planes = 0; y: planes [N,Hp,Wp,64]; idx: uint8 [N,Hp,Wp,64], or null when no backward follows.  Bit-identical to
 * cxrk_conv_bn_act_fwd_pl(relu = 1) followed by cxrk_maxpool_fwd_pl.  Any other geometry than 7x7 / stride 2 / pad 3, 4 -> 64
 * channels: CXRK_ERR_UNSUPPORTED (the caller takes the two calls). */
int cxrk_stem_pool_fwd(const float* x, const float* w_scaled, const float* shift, void* y, long yplane, unsigned char* idx, int N,
                       int H, int W, int C, int Ko, int R, int S, int stride, int pad, hipStream_t stream);
/* sums[c] = sum over the stem pixels of the dx cxrk_maxpool_bwd_pl writes for (g, idx, pooled) — the stem's BatchNorm sums — without
 * that tensor: every window has one winner, so it is the sum over the pooled pixels of g * [pooled > 0].  g, pooled: planes
 * [N,Hp,Wp,64].  Deterministic: per-block partials in `part` (scratch memory of cxrk_colsum_ws_bytes(N*Hp*Wp, 64)
 * bytes, sized and aligned like every workspace), then a fixed-order final pass. */
int cxrk_stem_pool_bwd_sums(const void* g, long gplane, const void* pooled, float* sums, int N, int Hp, int Wp, int C, float* part,
                            size_t part_bytes, hipStream_t stream);

/* spatial_mean — torch.mean(projected_patch_embeddings, dim=(2,3)) (model.py:145). x[N][P][C] -> y[N][C]. */
int cxrk_spatial_mean_fwd(const float* x, float* y, int N, int P, int C, hipStream_t stream);
int cxrk_spatial_mean_bwd(const float* dy, float* dx, int N, int P, int C, hipStream_t stream);
/* dx (planes [N][P][C]) = dy[n][c] / P + add[n][p][c] (add optional, fp32) */
int cxrk_spatial_mean_bwd_pl(const float* dy, const float* add, void* dx, long dxplane, int N, int P, int C, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm2d around the convolutions (csrc/bn_train.hip): the mode the reference's `ImageModel` constructor leaves the
 * model in (`self.train()`, health_multimodal/image/model/model.py:119) — batch statistics in the forward, running statistics updated
 * with momentum, the batch-statistics terms in the backward (torch.nn.BatchNorm2d, training=True).  Tensors `void* p, long plane`:
 * fp32 when plane == 0, split-bf16 planes otherwise; [rows = pixels][C], C % 8 == 0.
 *   forward:   z = conv(x, w) (cxrk_conv_bn_act_fwd* with an identity fold); cxrk_colstats -> batch mean and biased variance;
 *              cxrk_bn_train_fwd_coeffs -> scale = gamma rstd, shift = beta - mean scale, rstd (+ running statistics update when
 *              rmean / rvar are given: r = (1 - momentum) r + momentum stat, variance unbiased);  cxrk_bn_apply: y = relu?(z scale +
 *              shift + residual?), ReLU decision bits (byte [row][c / 8]) when mask != null.
 *   backward:  dot = cxrk_coldot(dy, z, bshift = mean) = sum_rows dy (z - mean);  cxrk_bn_train_bwd_coeffs -> dbeta (+)= sum dy,
 *              dgamma (+)= rstd dot, and A, B, Cc with dz = A dy + B + Cc z = gamma rstd (dy - mean(dy) - xhat mean(dy xhat));  cxrk_bn_train_dz;
 *              dz then takes the place of dy in cxrk_conv_bn_act_bwd_data* / _bwd_params* (identity fold).
 */
/* mean[c], var[c] = var_scale * sum_rows (x - mean)^2 in ONE pass over x (per-block shifted sums merged with Chan's formula);
 * ws: 2 * cxrk_coldot_ws_bytes(rows, C) */
int cxrk_colstats(const void* x, long plane, long rows, int C, float* mean, float* var, float var_scale, float* ws, size_t ws_bytes,
                  hipStream_t stream);
int cxrk_bn_train_fwd_coeffs(const float* mean, const float* var, const float* gamma, const float* beta, float eps, long n, float momentum,
                             float* scale, float* shift, float* rstd, float* rmean, float* rvar, int C, hipStream_t stream);
int cxrk_bn_apply(const void* z, long zplane, const float* scale, const float* shift, const void* res, long rplane, void* y, long yplane,
                  unsigned char* mask, long rows, int C, int relu, hipStream_t stream);
size_t cxrk_coldot_ws_bytes(long rows, int C);
/* out[c] = sum_rows a[r][c] * (b[r][c] - bshift[c]); bshift may be null (= 0) */
int cxrk_coldot(const void* a, long aplane, const void* b, long bplane, const float* bshift, long rows, int C, float* out, float* ws,
                size_t ws_bytes, hipStream_t stream);
int cxrk_bn_train_bwd_coeffs(const float* gamma, const float* mean, const float* rstd, const float* sumdy, const float* dot, long n, float* A,
                             float* B, float* Cc, float* dgamma, float* dbeta, int accumulate, int C, hipStream_t stream);
int cxrk_bn_train_dz(const void* dy, long dyplane, const void* z, long zplane, const float* A, const float* B, const float* Cc, void* dz,
                     long dzplane, long rows, int C, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * CXR-BERT pieces (HF BertForMaskedLM under modelling_cxrbert.py:87-99; config configuration_cxrbert.py:11-22).
 * embed_ln:    y = LayerNorm(word[ids] + pos[t % L] + type[0])                    (BertEmbeddings)
 * residual_ln: y = LayerNorm(x + res)                                             (BertSelfOutput / BertOutput)
 *              xhat, rstd saved for bwd; bwd: dx = LN'(dy) + dx_add, dgamma/dbeta reduced deterministically.
 * attn:        ctx = softmax(Q K^T / sqrt(d) + keymask) V per (sequence, head); qkv is the fused [T][3*nH*d]
 *              projection output; probs [B][nH][L][L] saved for bwd.  d <= 64 (multiple of 4); L <= 64: one workgroup per
 *              (sequence, head), everything in LDS; 64 < L <= 512 (the reference's max_position_embeddings,
 *              text/inference_engine.py:30,44-46): tiled over 32 queries / 64 keys, bwd needs the dS workspace.
 * embed_bwd:   dword[ids[t]] += dx[t], summed in token order per row (sort by (id, position) + segmented sums: deterministic, no atomics)
 * Outputs declared `void* y, long yplane`: yplane = 0 -> fp32 tensor; yplane > 0 -> planes (bf16 hi at y, lo at y + yplane
 * elements), the format the following GEMM consumes in split-bf16 mode.
 */
int cxrk_embed_ln_fwd(const long* ids, const float* word, const float* pos, const float* type, const float* gamma,
                      const float* beta, float eps, long T, int L, int H, void* y, long yplane, float* xhat, float* rstd,
                      hipStream_t stream);
int cxrk_residual_ln_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps, long rows,
                         int H, void* y, long yplane, float* xhat, float* rstd, hipStream_t stream);
size_t cxrk_residual_ln_bwd_ws_bytes(long rows, int H);
/* dxsum (optional, [H]): column sums of the gradient this call writes (dx, dx_add included) = the bias gradient of the dense layer
 * whose output fed this LayerNorm (BertSelfOutput / BertOutput dense), reduced in the same pass. */
int cxrk_residual_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, long rows, int H,
                         const float* dx_add, void* dx, long dxplane, float* dgamma, float* dbeta, int accumulate, float* dxsum,
                         int dxsum_accumulate, float* ws, size_t ws_bytes, hipStream_t stream);
/* dst[r*ld + c] += src[r][c] for a planes tensor src [rows][cols] (the CLS-row gradient added into a [N, L, H] fp32 gradient) */
int cxrk_planes_add_rows(const void* src, long plane, long rows, int cols, float* dst, long ld, hipStream_t stream);
int cxrk_attn_fwd(const float* qkv, const long* mask, int B, int L, int nH, int dH, void* ctx, long ctxplane, float* probs,
                  hipStream_t stream);
size_t cxrk_attn_bwd_ws_bytes(int B, int L, int nH, int dH);
int cxrk_attn_bwd(const float* qkv, const float* probs, const float* dctx, int B, int L, int nH, int dH, void* dqkv,
                  long dqkvplane, float* ws, size_t ws_bytes, hipStream_t stream);
/* ---- dropout (train mode, HF BertModel's four sites; opt-in through CXRBertModel.enable_dropout_) ----
 * Every entry below takes the dropout descriptor (seed, counter, layer, site, row_offset, p), 0 <= p < 1, layer < 64,
 * site: 0 = embeddings, 1 = attention probabilities, 2 = attention output, 3 = FFN output.  Keep rule (csrc/dropout.h):
 *   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32),
 *   counter = (c >> 2, n, t | h << 16, (counter & 0xffffff) << 8 | layer << 2 | site), draw = output word c & 3,
 *   keep iff draw >= floor(float(p) * 2^32 + 0.5); kept values are scaled by 1 / (1 - p).
 * n = row_offset + the sequence index within the call, t = token (the query for site 1), c = column (the key for site 1),
 * h = head (0 for the hidden sites).  The masks are regenerated in the backward, never stored.
 * dropout_mask:       keep[N][nH][L][C] (uint8) of one site; hidden sites: nH = 1, C = H (the [N*L, H] activation).
 * embed_ln_fwd_drop:  y = keep * s * LayerNorm(...); xhat / rstd are those of the LayerNorm.
 * residual_ln_fwd_drop: y = LayerNorm(keep * s * x + res); res fp32 (resplane = 0) or planes (resplane > 0), row stride res_ld
 *                     (0: H); rows_per_seq = tokens per sequence of the tensor (L, or 1 for the CLS rows of the last layer).
 * residual_ln_bwd_drop: mode 1 (y = LN(drop(x) + res)): dx = LN'(dy) + dx_add (the residual path), dxm = keep * s * dx in the same
 *                     format (the dense output's gradient), dxsum = column sums of dxm; mode 2 (y = drop(LN(x))): dy is masked on
 *                     load, dxm must be NULL.
 * attn_fwd_drop:      ctx = (keep * s o P) V; probs stay undropped.  attn_bwd_drop: dV = (keep * s o P)^T dO,
 *                     dP = keep * s o (dO V^T), dS = P o (dP - rowsum(dP o P)) / sqrt(d).
 */
int cxrk_dropout_mask(unsigned long long seed, unsigned counter, int layer, int site, long row_offset, float p, int N, int L, int nH,
                      int C, unsigned char* keep, hipStream_t stream);
int cxrk_embed_ln_fwd_drop(const long* ids, const float* word, const float* pos, const float* type, const float* gamma,
                           const float* beta, float eps, long T, int L, int H, void* y, long yplane, float* xhat, float* rstd,
                           unsigned long long seed, unsigned counter, int layer, int site, long row_offset, float p,
                           hipStream_t stream);
int cxrk_residual_ln_fwd_drop(const float* x, const void* res, long resplane, long res_ld, const float* gamma, const float* beta,
                              float eps, long rows, int H, int rows_per_seq, void* y, long yplane, float* xhat, float* rstd,
                              unsigned long long seed, unsigned counter, int layer, int site, long row_offset, float p,
                              hipStream_t stream);
int cxrk_residual_ln_bwd_drop(const float* dy, const float* xhat, const float* rstd, const float* gamma, long rows, int H,
                              int rows_per_seq, int mode, const float* dx_add, void* dx, void* dxm, long dxplane, float* dgamma,
                              float* dbeta, int accumulate, float* dxsum, int dxsum_accumulate, float* ws, size_t ws_bytes,
                              unsigned long long seed, unsigned counter, int layer, int site, long row_offset, float p,
                              hipStream_t stream);
int cxrk_attn_fwd_drop(const float* qkv, const long* mask, int B, int L, int nH, int dH, void* ctx, long ctxplane, float* probs,
                       unsigned long long seed, unsigned counter, int layer, int site, long row_offset, float p, hipStream_t stream);
int cxrk_attn_bwd_drop(const float* qkv, const float* probs, const float* dctx, int B, int L, int nH, int dH, void* dqkv,
                       long dqkvplane, float* ws, size_t ws_bytes, unsigned long long seed, unsigned counter, int layer, int site,
                       long row_offset, float p, hipStream_t stream);
size_t cxrk_embed_bwd_ws_bytes(long T, int H);
int cxrk_embed_bwd(const long* ids, const float* dx, long T, int H, float* dword, float* ws, size_t ws_bytes, hipStream_t stream);
/* dx = dy * gelu'(pre): the erf-GELU between dense_to_hidden and LayerNorm of BertProjectionHead (modelling_cxrbert.py:45-46). */
int cxrk_gelu_bwd(const float* dy, const float* pre, long n, float* dx, hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Similarity / loss heads.
 * l2norm:      F.normalize(x, dim=1) (modelling_cxrbert.py:138-139; vlp/inference_engine.py:51): xhat = x / max(|x|, eps).
 *              xhat rows are ldxhat floats apart (the data-parallel step writes image and text halves of one [B][2D] send buffer).
 * infonce:     north-star head (not in the reference): on a logits block S[rows][cols] = X_hat_local @ Y_hat_all^T / tau,
 *              row_lse gives lse + diagonal (+ accumulates sum(lse-diag)*scale into loss_out);
 *              grad_inplace turns S into exp(S-lse_row[i]) + exp(S-lse_col[j]) - 2*[j==diag_off+i].
 * multipos:    the same head with label-aware targets: every row and column carries a 64-bit key (any int64 value), and the
 *              positives of row i are the columns j with keys_col[j] == keys_row[i] (n_i of them).  row_stats gives, per row, lse,
 *              the mean of S[i][j] over the positives (0 when there is none) and n_i as a float (exact: cols < 2^24), in one pass
 *              over S (+ accumulates sum(lse-posmean)*scale into loss_out, in a fixed order: no atomics);
 *              grad_inplace turns S into exp(S-lse_row[i]) + exp(S-lse_col[j]) - 2*[keys_row[i]==keys_col[j]] / n_row[i].
 *              S rows are ld >= cols floats apart; 16-byte accesses where ld % 4 == 0 and the bases are 16-byte aligned, scalar
 *              otherwise.  No scratch memory: lse / posmean / npos are outputs of the caller.
 * *_scaled:    the two heads with a LEARNABLE temperature: the block holds the unscaled cosines C (logits GEMM with alpha = 1) and
 *              log_scale points at theta = log(1/tau) on the device; the logits are x = exp(theta) * c.  row_lse_scaled /
 *              row_stats_scaled write what their fixed-temperature forms write, computed on x in one pass over each row.
 *              grad_scaled_inplace turns C into exp(theta) * g (g = the gradient term of the fixed-temperature form on x), so the
 *              backward GEMMs need nothing of theta on the host, and writes the partial sums of g * x that make d theta:
 *              partials[i * nchunk + k] = sum of g*x over columns [1024 k, 1024 (k+1)) of row i, nchunk = ceil(cols / 1024); the
 *              caller provides rows * nchunk floats and every one of them is written (an output, not scratch memory).
 * logit_scale_grad: dtheta[0] = (accumulate ? dtheta[0] : 0) + upstream[0] * scale * (sum partials1[0..n1) + sum partials2[0..n2));
 *              one block, fixed order; upstream is a device scalar; partials2 may be NULL with n2 = 0.
 * sigmoid_pairs: the pairwise sigmoid loss (SigLIP): the reference's BCE-with-logits criterion (ZERO_JOINT_BOUNDS.py:36,
 *              Trainer.py:575-582) carried to every pair of the block, nothing normalised over the batch.  The block holds the
 *              unscaled cosines C; log_scale points at theta = log(1/tau) and bias at b, one fp32 each, read on the device.  With
 *              t = exp(theta) and x = fma(t, c, b):  l = softplus(-x) for a positive pair, softplus(x) otherwise;
 *              g = dl/dx = -sigmoid(-x) or sigmoid(x); the positive branch is never formed as sigmoid(x) - 1.
 *              fwd_bwd_inplace turns C into t * g in ONE pass.  Positives: keys_row and keys_col both NULL: the one positive of row i
 *              is column diag_off + i (0 <= diag_off, diag_off + rows <= cols); both given: the columns j with keys_col[j] ==
 *              keys_row[i] (a row may have none; diag_off is ignored); exactly one NULL: -1.  partials == NULL: no sums are formed.
 *              Otherwise partials holds 3 * rows * nchunk floats, nchunk = ceil(cols / 1024), as three planes of rows * nchunk:
 *              plane 0 sum l, plane 1 sum g * (t c) (= g * (x - b)), plane 2 sum g; entry [i * nchunk + k] of a plane sums over
 *              columns [1024 k, 1024 (k+1)) of row i in a fixed order (no atomics).  Every one of them is written (an output of the
 *              caller, not scratch memory).  Exact fp32 in both precision modes; 16-byte accesses where ld % 4 == 0 and C is
 *              16-byte aligned, scalar otherwise.  A NaN cosine makes its own element and its row's three sums non-finite and
 *              touches nothing else; at +-Inf, g * (t c) may be 0 * Inf (the "0 or NaN" clause above).
 * sigmoid_pairs_loss: loss_out[0] = (accumulate ? loss_out[0] : 0) + scale * sum partials[0..n); one block, fixed order (plane 0 with
 *              scale 1/Bg gives the loss; logit_scale_grad on plane 1 gives d theta and on plane 2 d b, with partials2 = NULL).
 * distill:     similarity distillation from a frozen teacher: S is the student's logits block and St the teacher's,
 *              both [rows][cols] (rows ld / ldt >= cols floats apart), St read-only and distinct from S.  With p = softmax of a row
 *              of S and pt = that of St, row_stats writes per row lse[i], lse_t[i] and
 *                  kl[i] = sum_j pt_ij (St_ij - S_ij) + (lse[i] - lse_t[i])      (= KL(pt_i || p_i)),
 *              in one pass over the two rows, and, with loss_out, loss_out[0] = (accumulate ? loss_out[0] : 0) + loss_scale * sum_i
 *              kl[i] from one block in a fixed order (no atomics).  grad_inplace turns S into
 *                  (exp(S-lse_row[i]) - exp(St-lse_t_row[i])) + (exp(S-lse_col[j]) - exp(St-lse_t_col[j])).
 *              Exact fp32 in both precision modes.  One 256-thread block per row; 16-byte accesses where ld % 4 == 0, ldt % 4 == 0 and
 *              both bases are 16-byte aligned, scalar otherwise; columns cols..ld of a row are never read or written.  No scratch
 *              memory: every output is the caller's.  Two runs are bit-identical.  IDENTICAL INPUTS GIVE EXACT ZEROS: if St equals S
 *              bit for bit (and lse_t_row / lse_t_col equal lse_row / lse_col), every kl[i] and every element of the gradient block is
 *              exactly 0.0 -- each summand of kl carries the factor (St_ij - S_ij), the two log-sum-exps come from the same code, and
 *              the gradient groups student - teacher per direction.  Non-finite values: a NaN in row i of S makes lse[i], kl[i] and
 *              the loss NaN, a NaN in row i of St makes lse_t[i], kl[i] and the loss NaN; no other row's outputs are touched and
 *              nothing is clamped or replaced.
 * clamp_inplace: x[i] = min(max(x[i], lo), hi) for lo <= hi; a NaN stays a NaN.
 * pairwise_cosine: torchmetrics pairwise_cosine_similarity as called by Trainer.myCosineSimilarity (Trainer.py:1682-1704).
 * pairwise_cosine_max: the MAX_EMB branch of the same function (Trainer.py:1691-1693): y holds G groups of Pg prompt
 *              vectors (group g = rows g*Pg .. g*Pg+Pg-1); besides cos [B][G*Pg] it returns, per image and group, the maximum
 *              over the group's prompts (first winner on ties, as torch.max), the mean (logged at Trainer.py:1697-1703) and
 *              the winner's index, which max_bwd uses to route dmax [B][G] to one prompt per group.
 * patch_similarity: sim[r] = <patches[r,:], text> — `projected_patch_embeddings.view(-1, D) @ text.t()`
 *              (health_multimodal/vlp/inference_engine.py:104); smoothing and resizing stay on the host.
 * bce_posneg:  logits = cos_pos - cos_neg (Trainer.py:575) + nn.BCEWithLogitsLoss() mean (ZERO_JOINT_BOUNDS.py:36);
 *              cos is [B][2C] with column 2c = positive prompt of class c, 2c+1 = negative; writes dloss/dcos.
 * eval_score:  Trainer.val/test scoring (Trainer.py:825-836).
 * group_mean:  prompt-embedding mean over the prompts of a class (Trainer.py:1665-1666).
 */
int cxrk_l2norm_fwd(const float* x, long rows, int D, float eps, float* xhat, long ldxhat, float* norm, hipStream_t stream);
int cxrk_l2norm_bwd(const float* dxhat, const float* xhat, long ldxhat, const float* norm, long rows, int D, float* dx,
                    hipStream_t stream);
int cxrk_infonce_row_lse(const float* S, long ld, int rows, int cols, int diag_off, float* lse, float* diag,
                         float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream);
int cxrk_infonce_grad_inplace(float* S, long ld, int rows, int cols, int diag_off, const float* lse_row,
                              const float* lse_col, hipStream_t stream);
int cxrk_multipos_row_stats(const float* S, long ld, int rows, int cols, const long long* keys_row,
                            const long long* keys_col, float* lse, float* posmean, float* npos, float* loss_out,
                            float loss_scale, int loss_accumulate, hipStream_t stream);
int cxrk_multipos_grad_inplace(float* S, long ld, int rows, int cols, const long long* keys_row,
                               const long long* keys_col, const float* n_row, const float* lse_row, const float* lse_col,
                               hipStream_t stream);
int cxrk_infonce_row_lse_scaled(const float* C, long ld, int rows, int cols, int diag_off, const float* log_scale, float* lse,
                                float* diag, float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream);
int cxrk_infonce_grad_scaled_inplace(float* C, long ld, int rows, int cols, int diag_off, const float* lse_row,
                                     const float* lse_col, const float* log_scale, float* partials, hipStream_t stream);
int cxrk_multipos_row_stats_scaled(const float* C, long ld, int rows, int cols, const long long* keys_row,
                                   const long long* keys_col, const float* log_scale, float* lse, float* posmean, float* npos,
                                   float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream);
int cxrk_multipos_grad_scaled_inplace(float* C, long ld, int rows, int cols, const long long* keys_row,
                                      const long long* keys_col, const float* n_row, const float* lse_row, const float* lse_col,
                                      const float* log_scale, float* partials, hipStream_t stream);
int cxrk_logit_scale_grad(const float* partials1, long n1, const float* partials2, long n2, const float* upstream, float scale,
                          float* dtheta, int accumulate, hipStream_t stream);
int cxrk_sigmoid_pairs_fwd_bwd_inplace(float* C, long ld, int rows, int cols, int diag_off, const long long* keys_row,
                                       const long long* keys_col, const float* log_scale, const float* bias, float* partials,
                                       hipStream_t stream);
int cxrk_sigmoid_pairs_loss(const float* partials, long n, float scale, float* loss_out, int accumulate, hipStream_t stream);
int cxrk_distill_row_stats(const float* S, long ld, const float* St, long ldt, int rows, int cols, float* lse, float* lse_t,
                           float* kl, float* loss_out, float loss_scale, int loss_accumulate, hipStream_t stream);
int cxrk_distill_grad_inplace(float* S, long ld, const float* St, long ldt, int rows, int cols, const float* lse_row,
                              const float* lse_col, const float* lse_t_row, const float* lse_t_col, hipStream_t stream);
int cxrk_clamp_inplace(float* x, long n, float lo, float hi, hipStream_t stream);
int cxrk_pairwise_cosine_fwd(const float* x, const float* y, long B, int P, int D, float* cosv, float* xnorm,
                             float* ynorm, hipStream_t stream);
size_t cxrk_pairwise_cosine_bwd_ws_bytes(long B, int P, int D);
int cxrk_pairwise_cosine_bwd(const float* x, const float* y, const float* cosv, const float* dcos, const float* xnorm,
                             const float* ynorm, long B, int P, int D, float* dx, float* dy, int accumulate_dy,
                             float* ws, size_t ws_bytes, hipStream_t stream);
int cxrk_pairwise_cosine_max_fwd(const float* x, const float* y, long B, int G, int Pg, int D, float* cosv, float* xnorm,
                                 float* ynorm, float* maxv, float* meanv, int* argmax, hipStream_t stream);
int cxrk_pairwise_cosine_max_bwd(const float* x, const float* y, const float* cosv, const float* dmax, const int* argmax,
                                 const float* xnorm, const float* ynorm, long B, int G, int Pg, int D, float* dx, float* dy,
                                 int accumulate_dy, float* ws, size_t ws_bytes, hipStream_t stream);
int cxrk_patch_similarity(const float* patches, const float* text, long R, int D, float* sim, hipStream_t stream);
size_t cxrk_bce_posneg_ws_bytes(void);
int cxrk_bce_posneg_fwd_bwd(const float* cosv, const float* labels, long B, int C, int ldlab, int diff, float* logits,
                            float* dcos, float* loss, float* ws, size_t ws_bytes, hipStream_t stream);
int cxrk_eval_score(const float* cosv, long B, int C, int pred_diff, float* score, float* pred, hipStream_t stream);
int cxrk_group_mean_fwd(const float* in, int G, int n, int D, float* out, hipStream_t stream);
int cxrk_group_mean_bwd(const float* dout, int G, int n, int D, float* din, hipStream_t stream);
/* retrieval_ranks — image<->text retrieval evaluation over a whole gallery (Recall@K, median / mean rank; not in the reference, the
 * standard check of a contrastive model) WITHOUT the [N][M] similarity block: 128 x 128 tiles of s(i,j) = sum_k Q[i][k] G[j][k] are
 * formed and consumed in registers (csrc/retrieval.hip).  Q rows are ldq >= D floats apart, G rows ldg >= D; the padding is never read.
 *   positives of row i: keys_q == keys_g == NULL: the one column i + diag_off (the data-parallel shard convention of
 *     cxrk_infonce_row_lse; 0 <= diag_off, diag_off + N <= M); otherwise every column j with keys_g[j] == keys_q[i] (all 64 bits).
 *   pos[i]     = the largest s(i,j) over the positives (-inf when the row has none);
 *   greater[i] = the number of non-positive columns with s(i,j) >  pos[i];
 *   ties[i]    = the number of non-positive columns with s(i,j) == pos[i].
 * All three outputs ([N]) are fully defined by the call: nothing is zeroed by the caller, there is no workspace.
 * Exact fp32 in BOTH precision modes (a metric must not move with CXRK_PRECISION): v_mfma_f32_32x32x2_f32, k ascending, no split
 * over k, so s(i,j) is a function of row i of Q and row j of G alone — two identical gallery rows tie bit for bit, and the result
 * does not depend on the grid (integer atomics only).
 * Non-finite: +-Inf compare as numbers.  A row whose best positive is NaN (pos keeps the NaN), or that meets a NaN score in a
 * non-positive column, gets greater[i] = ties[i] = -1: a NaN never turns into a plausible rank.
 * -1 for N, M, D < 1, ld < D, exactly one key pointer NULL, or (pair form) diag_off outside [0, M - N]. */
int cxrk_retrieval_ranks(const float* Q, long ldq, int N, const float* G, long ldg, int M, int D, int diag_off,
                         const long long* keys_q, const long long* keys_g, float* pos, int* greater, int* ties, hipStream_t stream);
/* topk_neighbours — for every query row i the k best gallery rows j by s(i,j) = sum_d Q[i][d] G[j][d] (csrc/topk.hip), again WITHOUT
 * the [N][M] block and with the scores of retrieval_ranks bit for bit (same tile code, both precision modes).  One total order:
 * score descending, every NaN above every number, then gallery index ascending — the order of the signed 64-bit key
 * (enc(s) << 32) | (0xFFFFFFFF - j).  score[N][k] fp32 / index[N][k] int32, each row sorted by it, no index twice; with fewer
 * than k candidates the remaining slots are index -1, score -inf.  exclude_off >= 0: column i + exclude_off is no candidate of
 * row i (leave-one-out of a bank against itself; the rank offset under data parallelism; exclude_off + N <= M); -1: none.
 * Two launches, no atomics, no host sync: per-block sorted lists into `slab` as [N][split][k] keys, then a merge per row; the result
 * does not depend on the split.  slab: the lists' memory, 256-byte aligned; exactly cxrk_topk_neighbours_slab_bytes(N, M, k) bytes
 * are written (the query gives 0 for bad arguments; CXRK_ERR_WS when slab_bytes is below it).
 * -1 for k outside [1, 64], N, M, D < 1, ld < D, exclude_off < -1 or exclude_off + N > M; nothing is launched then. */
size_t cxrk_topk_neighbours_slab_bytes(int N, int M, int k);
int cxrk_topk_neighbours(const float* Q, long ldq, int N, const float* G, long ldg, int M, int D, int k, int exclude_off,
                         float* score, int* index, void* slab, size_t slab_bytes, hipStream_t stream);
/* knn_vote — the weighted kNN vote (Wu et al. 2018) for multi-hot labels[M][C] (row pitch ldl >= C) on the lists above:
 *   out[i][c] = sum_n w_n labels[index[i][n]][c] / sum_n w_n,  w_n = expf((score[i][n] - score[i][0]) * inv_temperature),
 * n ascending in fp32 (one thread per output, no atomics).  Slots with index -1 have weight 0.  A row that holds a NaN score, an
 * index outside [-1, M) (never read) or no neighbour at all gives NaN in all C outputs.  1 <= k <= 64. */
int cxrk_knn_vote(const float* score, const int* index, int N, int k, const float* labels, long ldl, int M, int C,
                  float inv_temperature, float* out, hipStream_t stream);
/* out = alpha * (alpha_dev ? *alpha_dev : 1) * x * (mask_src > 0): nn.ReLU backward (models.py:10) and chain-rule scaling
 * by an upstream scalar gradient that lives on the device. */
int cxrk_scale_mask(const float* x, const float* mask_src, const float* alpha_dev, float alpha, long n, float* out,
                    hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * mlm — the masked-language-modelling auxiliary loss of the joint step (csrc/mlm.hip): HF BertForMaskedLM's loss
 * (the head the reference computes and discards, modelling_cxrbert.py:87-95) on tokens masked on the device by the rule of HF
 * DataCollatorForLanguageModeling.  No entry point takes scratch memory, none uses an atomic, none synchronises: the number of rows
 * that count travels in device memory (`stats`), and two runs on the same inputs give the same bits.
 * mask_tokens:  ids / mask [N][L] int64 (mask may be NULL = all attended).  Token (n, t) is a CANDIDATE iff its mask is non-zero and
 *              its id is none of special[0..nspecial) (a HOST array of at most 8 ids, copied into the launch).  Draw:
 *                Philox4x32-10 (csrc/dropout.h), key = (seed & 0xffffffff, seed >> 32), ONE block per token with
 *                counter = (0, row_offset + n, t, (counter & 0xffffff) << 8 | 0xF4)   (low byte 0xF4 = layer 61, site 0: no dropout
 *                word and not the augmentation's 0xF0), output words w0..w3;
 *                selected iff candidate and w0 < floor(p * 2^32 + 0.5);
 *                a selected token becomes mask_id if w1 < 3435973837 (= ceil(0.8 * 2^32)), the id (w2 * V) >> 32 if
 *                w1 < 3865470567 (= ceil(0.9 * 2^32)), and keeps its id otherwise; w3 is reserved.
 *              The draw is a function of (seed, counter, global sequence index, token, the token's id and mask) and of nothing else: a
 *              batch cut anywhere and masked with the matching row_offset gives the ids of the whole-batch call.
 *              Outputs: ids_out [N][L]; the compact list in ASCENDING token order, sel[k] = index n * L + t (within the call) of the
 *              k-th selected token and tgt[k] = its original id, for k < kept = min(selected, cap); sel[k] = tgt[k] = -1 for
 *              kept <= k < cap; stats = {kept, selected} (selected > kept reports an overflow: the tokens past the cap stay corrupted
 *              in ids_out and carry no loss); count_f[0] = float(kept).  block_counts: ceil(N L / 256) ints, an output of the caller
 *              (the selected tokens per block of 256, from which every block derives its offset in a fixed order), not scratch memory.
 *              -1 for p outside [0, 1], V outside [1, 2^31), mask_id outside [0, V), nspecial > 8, N L >= 2^31, cap outside [1, N L].
 * gather_rows: out[r] = last[sel[r]] for r < kept, zero rows for kept <= r < cap; last [T][H] fp32; out fp32 [cap][H] (plane = 0,
 *              H % 4 == 0) or planes (plane > 0, H % 8 == 0).  scatter_rows: dlast[sel[r]] = dx[r] for r < kept by plain stores (the
 *              caller zeroes dlast [T][H]; sel lists no token twice).  An index outside [0, T) is skipped.
 * xent_stats:  S [rows][ld] holds the logits WITHOUT the decoder bias of vocabulary columns [v0, v0 + cols); x = S + bias[column]
 *              (bias = the whole [V] vector).  For every row r < kept the call folds columns [v0 + skip, v0 + cols) into
 *              state [4][rows][64] (running maximum, sum of exp(x - maximum), best value, best column as int bits; `first` != 0: the
 *              state is started, not read) and writes x of column tgt[r] to target_logit[r] when the chunk holds it.  Lane l of the
 *              row's wave takes, in ascending order, the groups of four columns with (column / 4) mod 64 == l: chunk boundaries at
 *              multiples of 4 change nothing of what a lane adds up, so the statistics do not depend on the chunk size (exact fp32
 *              logits).  skip != 0, or v0 / cols / ld not multiples of 4: column by column, lane = column mod 64.
 * xent_finish: per row r < kept the 64 lanes merged in a fixed order: lse[r], rowloss[r] = lse[r] - target_logit[r], hit[r] = [first
 *              maximum of the row == tgt[r]] (a NaN is the maximum, as torch.argmax); zeros for r >= kept.  Then from one block in a
 *              fixed order loss_out[0] = scale[0] * sum_{r < kept} rowloss[r] and correct_out[0] = sum hit.  kept = 0 gives exactly 0.
 *              A NaN logit of a row r < kept reaches the loss; rows >= kept are never read.
 * xent_grad:   the recomputed chunk S -> g = (exp(x - lse[r]) - [column == tgt[r]]) * upstream[0] * scale[0] * alpha for r < kept and
 *              column >= v0 + skip, exactly 0 elsewhere (whatever S holds there); in place (G == NULL) or as planes G (row stride ldg,
 *              lo plane gplane elements behind).  cols % 8 == 0, ld % 4 == 0 (ldg, gplane % 8 == 0), 16-byte aligned bases, else -1.
 * stats / tgt / sel are int32; scale and upstream one fp32 each, read on the device. */
int cxrk_mlm_mask_tokens(const long* ids, const long* mask, int N, int L, long row_offset, unsigned long long seed, unsigned counter,
                         double p, long V, long mask_id, const long* special, int nspecial, int cap, long* ids_out, int* sel,
                         int* tgt, int* stats, float* count_f, int* block_counts, hipStream_t stream);
int cxrk_mlm_gather_rows(const float* last, long T, int H, const int* sel, const int* stats, int cap, void* out, long plane,
                         hipStream_t stream);
int cxrk_mlm_scatter_rows(const float* dx, const int* sel, const int* stats, int cap, long T, int H, float* dlast, hipStream_t stream);
int cxrk_mlm_xent_stats(const float* S, long ld, int rows, int cols, int skip, int v0, const float* bias, const int* tgt,
                        const int* stats, float* state, float* target_logit, int first, hipStream_t stream);
int cxrk_mlm_xent_finish(const float* state, const float* target_logit, const int* tgt, const int* stats, int rows, const float* scale,
                         float* lse, float* rowloss, int* hit, float* loss_out, int* correct_out, hipStream_t stream);
int cxrk_mlm_xent_grad(float* S, long ld, void* G, long ldg, long gplane, int rows, int cols, int skip, int v0, const float* bias,
                       const int* tgt, const int* stats, const float* lse, const float* upstream, const float* scale, float alpha,
                       hipStream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimiser / continual learning.
 * adam_fused:   torch.optim.Adam defaults (Trainer.py:172-175), one launch over a flat parameter buffer.
 * sgd:          optim.SGD (Trainer.py:176-178).
 * weight_reset: Trainer.myIncremental per tensor (Trainer.py:1562-1572); counters[0] += #restored.
 * grad_sqnorm:  partials[b] = sum of g[i]^2 over block b's share of g, b < nparts(n) = min(1024, max(1, ceil(floor(n / 4) / 1024)));
 *               cxrk_grad_sqnorm_partials_bytes(n) = 4 * nparts(n).  The partial sums are an output that adamw_clipped reads, sized
 *               by the caller: ws_bytes below that size (or partials == NULL) gives CXRK_ERR_WS and nothing is written; no
 *               256-byte alignment is asked of it.  float4 loads (g 16-byte aligned), four accumulators per thread, the n % 4 tail in
 *               block 0, no atomics.  Partition and summation order depend on n alone, never on the device: the same buffer gives
 *               the same bits in every run and on every data-parallel rank.  g is read only.
 * adamw_clipped: torch.optim.AdamW (decoupled decay) behind torch.nn.utils.clip_grad_norm_, one launch over the flat buffers.
 *               Every block re-derives total = sum partials[0..nparts(n)) in one fixed order;  norm = |grad_scale| * sqrt(total);
 *               coef = min(max_norm / (norm + 1e-6), 1), a NaN norm giving a NaN coef; max_norm = +inf gives coef = 1 exactly
 *               (monitoring).  partials == NULL with max_norm <= 0: no clipping, coef = 1, nothing is read; partials == NULL with
 *               max_norm > 0: CXRK_ERR_ARG; partials given with max_norm <= 0: the norm is reported, coef = 1.  ws_bytes is the size
 *               of partials (CXRK_ERR_WS below cxrk_grad_sqnorm_partials_bytes(n)).  Per element, in AdamW's order:
 *               gg = g * (grad_scale * coef);  p *= 1 - lr * weight_decay where the mask says so;  then adam_fused's moment and
 *               parameter lines without its L2 term: with coef = 1 and no decay applied the result is adam_fused(weight_decay = 0)
 *               bit for bit.  decay_mask: ceil(n / 4) bytes, one per aligned group of four elements, non-zero = the group decays;
 *               NULL = every element decays.  g, the mask and the partials are read only (the gradient stays unclipped).
 *               stats (optional, 2 floats): stats[0] = norm before clipping, stats[1] = coef (0 and 1 without partials), written
 *               by one thread with ordinary stores.  p, g, m, v 16-byte aligned, n > 0, step >= 1 as for adam_fused.
 *
 * Elastic weight consolidation over the same flat buffers (penalty strength / 2 * sum_i F[i] * (p[i] - anchor[i])^2).  All three
 * follow grad_sqnorm's conventions: float4 accesses (every buffer 16-byte aligned, else CXRK_ERR_ARG), a scalar n % 4 tail,
 * grid-stride loops, no atomics, n > 0, and nothing is written when a call is refused.
 * fisher_accumulate: acc[i] = fma(w, g[i] * g[i], acc[i]), i.e. acc += w * g^2 (two roundings).  g is read only.
 * ewc_consolidate: one pass: F[i] = fma(gamma, F[i], scale * acc[i]) and anchor[i] = p[i].  acc == NULL: only the anchor is written
 *               (identity Fisher) and F must be NULL too; F == NULL with acc given is CXRK_ERR_ARG.  acc and p are read only.
 * ewc_penalty:  d = p[i] - anchor[i];  t = F[i] * d;  g[i] = fma(strength, t, g[i]);  partials[b] = sum of t * d over block b's share.
 *               The partition is grad_sqnorm's, a function of n alone: nparts(n) blocks, the n % 4 tail in block 0, each block's sum
 *               in a fixed order, so the same buffers give the same bits in every run and on every data-parallel rank.
 *               cxrk_ewc_penalty_partials_bytes(n) = cxrk_grad_sqnorm_partials_bytes(n); partials == NULL or ws_bytes below it gives
 *               CXRK_ERR_WS with nothing written; no 256-byte alignment is asked of it.  F == NULL: F = 1 everywhere (L2-SP), bit for
 *               bit the result of an all-ones F.  The penalty's value is strength / 2 * sum of the partials (the caller's sum).
 *               p, anchor and F are read only; g is updated in place.
 *               Non-finite: as the torch expression g + strength * F * (p - anchor).  A NaN or Inf in element i of g, p, anchor or F
 *               reaches g[i] (0 * Inf = NaN included) and the partial sum of the block that holds i; it reaches no other element
 *               of g and no other partial.
 *
 * A-GEM gradient projection (Chaudhry et al. 2019) over the same flat buffers: g is the step's gradient, gref the gradient of a batch
 * drawn from an episodic memory.  Both calls follow grad_sqnorm's conventions as the three above do (float4 accesses, 16-byte alignment
 * or CXRK_ERR_ARG, a scalar n % 4 tail in block 0, no atomics, n > 0, nothing written when a call is refused).
 * agem_dots:    one pass over both buffers (8 B read per parameter): partials[b] = block b's share of sum g[i] * gref[i] and
 *               partials[nparts + b] = its share of sum gref[i] * gref[i], nparts = cxrk_grad_sqnorm_partials_bytes(n) / 4.  The
 *               partition is grad_sqnorm's, a function of n alone; each term enters its accumulator by one fma, each block's sums in
 *               a fixed order: the same buffers give the same bits in every run and on every data-parallel rank.
 *               cxrk_agem_dots_partials_bytes(n) = 2 * cxrk_grad_sqnorm_partials_bytes(n); partials == NULL or ws_bytes below it gives
 *               CXRK_ERR_WS with nothing written; no 256-byte alignment is asked of it.  g and gref are read only.
 * agem_project: every block re-derives dot and rr from the partials of agem_dots(g, gref, n) in adamw_clipped's fixed order (thread
 *               t takes partials t, t + 256, ..., then the block sum).  Iff !(dot >= 0): coef = dot / rr and
 *               g[i] = fma(-coef, gref[i], g[i]).  With dot >= 0 (dot == 0 with an all-zero gref included) every block returns
 *               before it touches g or gref: g stays bit for bit.  stats (4 floats, written by one thread with ordinary stores):
 *               stats[0] = dot, stats[1] = rr, stats[2] = coef (0 when not projected), stats[3] += 1 when projected (a running count
 *               the caller zeroes once).  gref and the partials are read only.
 *               Non-finite: a NaN anywhere in g or gref makes its block's partial NaN, hence dot NaN, the projection taken with
 *               coef = NaN and every element of g NaN; a bad reference gradient never silently disables the projection.
 *
 * Exponential moving average of the parameters over the same flat buffers.  Both calls follow grad_sqnorm's
 * conventions (float4 accesses, 16-byte alignment or CXRK_ERR_ARG, a scalar n % 4 tail, grid-stride loops, n > 0, nothing launched
 * and nothing written when a call is refused); neither takes scratch memory, uses an atomic or LDS, or synchronises.
 * ema_update:   c = 1 - decay, formed once in fp32;  d = p[i] - avg[i];  avg[i] = fma(c, d, avg[i]): two roundings, nothing else
 *               contracted.  8 B read + 4 B written per parameter; p is read only.  decay outside [0, 1] or NaN: CXRK_ERR_ARG.
 *               The lerp form is the contract: p[i] == avg[i] leaves avg[i] as it is bit for bit (d = 0), so the average of a
 *               parameter that never moved IS the parameter; decay == 1 (c = 0) leaves every avg[i] with a finite d as it is bit for
 *               bit; decay == 0 gives avg[i] = p[i] up to the rounding of d.  Whenever the result equals avg[i] as a number, avg[i]
 *               keeps its own bits: a negative zero stays a negative zero (the addition alone would make it +0).
 *               Non-finite: as the torch expression avg + c * (p - avg).  A NaN or Inf in p[i] or avg[i] reaches avg[i] and no other
 *               element; Inf - Inf and 0 * Inf give NaN, so at decay == 1 an infinite p[i] or avg[i] makes avg[i] NaN.
 * flat_swap:    a[i] <-> b[i], moves only: every bit pattern (NaN payloads included) arrives as it left, and two swaps are the
 *               identity.  8 B read + 8 B written per parameter, no temporary of the buffers' size.  a == b or overlapping ranges:
 *               CXRK_ERR_ARG.
 */
int cxrk_adam_fused(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, float grad_scale, hipStream_t stream);
int cxrk_sgd(float* p, const float* g, long n, float lr, float weight_decay, float grad_scale, hipStream_t stream);
size_t cxrk_grad_sqnorm_partials_bytes(long n);
int cxrk_grad_sqnorm(const float* g, long n, float* partials, size_t ws_bytes, hipStream_t stream);
int cxrk_adamw_clipped(float* p, const float* g, float* m, float* v, const unsigned char* decay_mask, long n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float max_norm,
                       const float* partials, size_t ws_bytes, float* stats, hipStream_t stream);
int cxrk_fisher_accumulate(float* acc, const float* g, long n, float w, hipStream_t stream);
int cxrk_ewc_consolidate(float* F, const float* acc, float* anchor, const float* p, long n, float gamma, float scale,
                         hipStream_t stream);
size_t cxrk_ewc_penalty_partials_bytes(long n);
int cxrk_ewc_penalty(float* g, const float* p, const float* anchor, const float* F, long n, float strength, float* partials,
                     size_t ws_bytes, hipStream_t stream);
size_t cxrk_agem_dots_partials_bytes(long n);
int cxrk_agem_dots(const float* g, const float* gref, long n, float* partials, size_t ws_bytes, hipStream_t stream);
int cxrk_agem_project(float* g, const float* gref, long n, const float* partials, float* stats, hipStream_t stream);
int cxrk_ema_update(float* avg, const float* p, long n, float decay, hipStream_t stream);
int cxrk_flat_swap(float* a, float* b, long n, hipStream_t stream);
size_t cxrk_weight_reset_ws_bytes(void);
int cxrk_weight_reset(float* pnew, const float* pold, long n, float threshold, unsigned long long* counters, float* ws,
                      size_t ws_bytes, hipStream_t stream);

/* Contraction precision of every GEMM / implicit-GEMM entry point above (process-wide):
 *   0 (default) exact fp32: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain;
 *   1 split-bf16: operands split into bf16 hi+lo while staged, a*b = hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16
 *     with fp32 accumulation (~2^-16 relative per product; inputs, outputs and all other kernels stay fp32). */
int cxrk_set_precision(int mode);
int cxrk_get_precision(void);
/* Policy of the 256x256 LDS-DMA kernel (planes operands): 0 never, 1 where it pays (default; CXRK_WIDE), 2 every planes launch
 * (test coverage of small / ragged shapes).  Returns the previous mode. */
int cxrk_set_wide_mode(int mode);

/* Library identification: returns a static string "cxrk <version> gfx950". */
const char* cxrk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CXRK_H */
