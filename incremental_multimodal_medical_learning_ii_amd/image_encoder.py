"""BioViL image encoder (ResNet-50 trunk + projector + spatial mean) forward and hand-written backward on the cxrk
kernels, exposed as one `torch.autograd.Function`.

Reference arithmetic: `health_multimodal/image/model/resnet.py:34-47` (stem, max-pool, layer1..4),
torchvision 0.10 `Bottleneck` (1x1 -> 3x3(stride) -> 1x1, BN after each, residual add, ReLU; 1x1-stride downsample
+ BN on the first block of a stage), `model.py:141-145` (trunk -> projector -> mean over (H, W)) and
`modules.py:43-47` (projector).  Eval-mode BatchNorm (running statistics) is the only mode the reference runs the encoder in
(`chexpert-get-embedding.py:41-42`) and the one everything below is organised around — gamma/beta (and every conv weight) still
receive gradients:

    y = conv(x, w)*s + t,  s = gamma*rsqrt(var+eps),  t = beta - mean*s
    dx = conv^T(dy, w*s);  dw = s * wgrad(x, dy);  dbeta = sum(dy);  dgamma = rstd * (<w, wgrad(x, dy)> - mean*sum(dy))

(dgamma = sum dy*xhat written through the raw weight gradient: nothing of the forward has to be re-read for it and gamma is
never divided by; measured against the direct sum on this network: < 1e-6 of the tensor maximum, scripts/exp_dgamma.py.)

Train-mode BatchNorm (`ImageModel.train()`, the state the reference's constructor leaves the model in, `model.py:119`) runs the same
GEMM kernels with an identity fold: batch statistics, normalisation + ReLU, running-statistics update and the batch-statistics terms
of the backward are separate kernels around them (`_conv_bn_train`, `through_bn` in `_backward`, csrc/bn_train.hip).

Working layout: activations NHWC, filters [Ko][R][S][C] (the parameters are kept in torch `channels_last` memory
format, so state-dict shapes stay OIHW).  The stem's 3 input channels are zero-padded to 4 (16-byte loads).

Two storage modes, chosen by the library's contraction precision (`_lib.get_precision()`):
  fp32        activations, folded filters and gradients are fp32 tensors; ReLU masks are taken from the sign of the saved
              activation (exact-fp32 MFMA mainloop).
  split_bf16  every activation / gradient / folded filter that feeds a contraction is a `kernels.Planes` tensor (bf16 hi + lo
              planes, 4 bytes per element) written by the producing kernel's epilogue, so the MFMA mainloops load operands with
              no conversion work; ReLU decisions are saved as bit masks (1 bit per element) by the forward epilogues and read
              by the data-gradient epilogues.  The stem reads the fp32 image (fp32 gather, split on the fly), in the forward
              and in its weight gradient.
Parameter gradients are written (accumulated) straight into `param.grad` when that exists with the parameter's own memory
layout — the flat gradient buffer of `optim._FlatOptimizer` — so autograd has nothing to add afterwards.

What a grad-enabled forward keeps for its backward is one `_Saved` record (`ctx.state`) with one `_BlockSaved` per bottleneck; the
storage mode is decided once per pass and read from `_Fold.pl` (`_Fold.on_planes`: the stem's operands stay fp32 in either mode).
"""
from __future__ import annotations

import os
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from . import kernels as K
from .augment import AugmentCall
from .gradsink import GradSink
from .kernels import Planes

LAYERS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5


class ConvSpec:
    __slots__ = ("conv", "bn", "cin", "cpad", "cout", "k", "stride", "pad", "widx", "off")

    def __init__(self, conv, bn, cin, cout, k, stride, pad):
        self.conv, self.bn, self.cin, self.cout, self.k, self.stride, self.pad = conv, bn, cin, cout, k, stride, pad
        self.cpad = (cin + 3) // 4 * 4


def resnet50_specs(prefix: str = "encoder.encoder.", joint: int = 128) -> Tuple[List[ConvSpec], List[dict]]:
    """Conv+BN units in execution order and the block wiring."""
    specs: List[ConvSpec] = [ConvSpec(prefix + "conv1", prefix + "bn1", 3, 64, 7, 2, 3)]
    blocks: List[dict] = []
    inpl = 64
    for li, (nblk, planes) in enumerate(zip(LAYERS, PLANES), start=1):
        for b in range(nblk):
            pre = f"{prefix}layer{li}.{b}."
            stride = 2 if (b == 0 and li > 1) else 1
            blk = {"c1": len(specs)}
            specs.append(ConvSpec(pre + "conv1", pre + "bn1", inpl, planes, 1, 1, 0))
            blk["c2"] = len(specs)
            specs.append(ConvSpec(pre + "conv2", pre + "bn2", planes, planes, 3, stride, 1))
            blk["c3"] = len(specs)
            specs.append(ConvSpec(pre + "conv3", pre + "bn3", planes, planes * 4, 1, 1, 0))
            blk["ds"] = None
            if b == 0:
                blk["ds"] = len(specs)
                specs.append(ConvSpec(pre + "downsample.0", pre + "downsample.1", inpl, planes * 4, 1, stride, 0))
            blocks.append(blk)
            inpl = planes * 4
    specs.append(ConvSpec("projector.model.0", "projector.model.1", 2048, joint, 1, 1, 0))
    return specs, blocks


def param_names(specs: Sequence[ConvSpec]) -> List[str]:
    names: List[str] = []
    for s in specs:
        names += [s.conv + ".weight", s.bn + ".weight", s.bn + ".bias"]
    return names + ["projector.model.3.weight", "projector.model.3.bias"]


def buffer_names(specs: Sequence[ConvSpec]) -> List[str]:
    names: List[str] = []
    for s in specs:
        names += [s.bn + ".running_mean", s.bn + ".running_var"]
    return names


def _planes_mode() -> bool:
    return _lib.get_precision() == "split_bf16"


class EncodeMeta(NamedTuple):
    """The non-tensor arguments of one `ImageEncodeFn` call (built by `ImageModel._run`)."""
    specs: Sequence[ConvSpec]
    blocks: Sequence[dict]
    n_params: int
    want_patch: bool
    on_grads_ready: Optional[Callable] = None     # per-call hook of the backward (ImageModel.grad_ready_hook at forward time)
    bn_momentum: Optional[float] = None           # None: eval-mode BatchNorm; float: train mode (ImageModel.train())
    augment: Optional[AugmentCall] = None         # on-device augmentation of this call (ImageModel.augment_call at forward time)
    save_free: bool = False                       # keep nothing for a backward (ImageModel.save_free: pass 1 of a micro-batched step)


def _filter_rsc(w: torch.Tensor) -> torch.Tensor:
    """OIHW parameter -> its [Ko][R][S][C] memory (no copy when the parameter is channels_last)."""
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


class _Fold:
    """Per-forward folded filters and BN vectors (one flat buffer each).  In planes mode the folded filters of every unit but
    the stem live in ONE [2, total] bf16 buffer (unit i = a column slice of both planes)."""

    def __init__(self, specs: Sequence[ConvSpec], device, pl: bool):
        self.pl = pl
        sizes = [s.cout * s.k * s.k * s.cpad for s in specs]
        tot_c = sum(s.cout for s in specs)
        self.vec = torch.empty(3, tot_c, dtype=torch.float32, device=device)
        self.woff, self.coff = [], []
        a = b = 0
        for s, n in zip(specs, sizes):
            self.woff.append(a)
            self.coff.append(b)
            a += (n + 7) // 8 * 8
            b += s.cout
        self.sizes = sizes
        self._ident = {}
        if pl:
            self.wp = torch.empty(2, a, dtype=torch.bfloat16, device=device)
            self.w = torch.empty(sizes[0], dtype=torch.float32, device=device)    # the stem's filters stay fp32
        else:
            self.w = torch.empty(a, dtype=torch.float32, device=device)

    def on_planes(self, i) -> bool:
        """whether unit i reads Planes operands (input and folded filter): every unit of planes mode but the stem, which reads the
        fp32 image in either mode"""
        return self.pl and i > 0

    def ws(self, i, s):
        """folded filter of unit i: fp32 [Ko*R*S*cpad] (fp32 mode, and the stem always) or Planes [Ko, R*S*cpad]"""
        n = self.sizes[i]
        if self.on_planes(i):
            return Planes(self.wp[:, self.woff[i]: self.woff[i] + n].view(2, s.cout, n // s.cout))
        return self.w[:n] if self.pl else self.w[self.woff[i]: self.woff[i] + n]

    def scale(self, i, s):
        return self.vec[0, self.coff[i]: self.coff[i] + s.cout]

    def shift(self, i, s):
        return self.vec[1, self.coff[i]: self.coff[i] + s.cout]

    def rstd(self, i, s):
        return self.vec[2, self.coff[i]: self.coff[i] + s.cout]

    def identity(self, cout):
        """(gamma, beta, mean, var) of an identity BatchNorm, rsqrt(var + eps) = 1: folded with it (train mode), the GEMM kernels
        produce the raw convolution output (scale 1, shift 0)"""
        if cout not in self._ident:
            one, zero = torch.ones(cout, device=self.vec.device), torch.zeros(cout, device=self.vec.device)
            self._ident[cout] = (one, zero, zero, one - BN_EPS)
        return self._ident[cout]

    def fold(self, i, s, w, gamma, beta, mean, var):
        """fold the BatchNorm (gamma, beta, mean, var) into filter `w` of unit i -> ws / scale / shift / rstd of the unit"""
        fn = K.bn_fold_pl if self.on_planes(i) else K.bn_fold
        fn(_filter_rsc(w), gamma, beta, mean, var, BN_EPS, s.cout, s.k * s.k, s.cin, s.cpad,
           self.ws(i, s), self.scale(i, s), self.shift(i, s), self.rstd(i, s))


def _bn_of(p, bufs, i):
    """(gamma, beta, running mean, running var) of unit i"""
    return p[3 * i + 1], p[3 * i + 2], bufs[2 * i], bufs[2 * i + 1]


class _BlockSaved:
    """One bottleneck's saved activations: input x, o1, o2 (after relu1 / relu2) with their spatial sizes (h, w) / (h2, w2), and its
    ReLU decisions: planes mode keeps the three bit masks m1, m2, m3 (the output lives on as the next block's x), fp32 mode keeps
    `out` for its sign."""
    __slots__ = ("x", "o1", "o2", "out", "h", "w", "h2", "w2", "m1", "m2", "m3")

    def __init__(self, *fields):
        self.x, self.o1, self.o2, self.out, self.h, self.w, self.h2, self.w2, self.m1, self.m2, self.m3 = fields

    def relu_of(self, k: int):
        """what masks a gradient flowing into o1 / o2 / out (k = 1, 2, 3): the bit mask (planes) or the tensor itself (fp32)"""
        m = (self.m1, self.m2, self.m3)[k - 1]
        return m if m is not None else (self.o1, self.o2, self.out)[k - 1]


class _Saved:
    """What a grad-enabled forward keeps for its backward (`ctx.state`): the fold, the padded image x0, the stem output (fp32 mode; planes
    mode only inside `capture_relu_decisions`) of size (Hs, Ws), the max-pool winners and output, one `_BlockSaved` per bottleneck,
    the trunk output `last` [N, h, w, 2048], the projector's hidden activation pj1 with its mask mp and split second weight w3p
    (planes mode).  train: train-mode BatchNorm (the filters were folded with an identity BatchNorm, see `_conv_bn_train`), with
    bn = {unit: (raw convolution output z, batch mean, batch rstd)}."""
    __slots__ = ("fold", "pl", "train", "bn", "N", "H", "W", "Hs", "Ws", "h", "w",
                 "x0", "stem", "idx", "pooled", "blocks", "last", "pj1", "mp", "w3p")

    def __init__(self, fold: _Fold, train: bool, N, H, W):
        self.fold, self.pl, self.train, self.bn, self.N, self.H, self.W = fold, fold.pl, train, ({} if train else None), N, H, W
        self.blocks: List[Optional[_BlockSaved]] = []


def _out_hw(s, H, W):
    return (H + 2 * s.pad - s.k) // s.stride + 1, (W + 2 * s.pad - s.k) // s.stride + 1


def _conv(i, s, fold, x, residual, relu, N, H, W, want_mask=True):
    """unit i forward -> (y, mask).  planes mode: y Planes, mask = ReLU decision bits (uint8 [N*Ho*Wo, Ko/8]) when relu;
    fp32 mode: y fp32, mask None (the backward reads the sign of y)."""
    Ho, Wo = _out_hw(s, H, W)
    dev = fold.vec.device
    if not fold.pl:
        y = torch.empty(N, Ho, Wo, s.cout, dtype=torch.float32, device=dev)
        K.conv_fwd(x, fold.ws(i, s), fold.shift(i, s), residual, y, N, H, W, s.cpad, s.cout, s.k, s.k, s.stride, s.pad, relu)
        return y, None
    y = Planes.empty(N, Ho, Wo, s.cout, device=dev)
    mask = torch.empty(N * Ho * Wo, s.cout // 8, dtype=torch.uint8, device=dev) if (relu and want_mask) else None
    K.conv_fwd_pl(x, fold.ws(i, s), fold.shift(i, s), residual, y, mask, N, H, W, s.cpad, s.cout, s.k, s.k, s.stride, s.pad, relu)
    return y, mask


def _conv_bn_train(i, s, fold, p, bufs, x, residual, relu, N, H, W, want_mask, momentum, keep: Optional[dict]):
    """Unit i in TRAIN mode (`torch.nn.BatchNorm2d`, training=True): z = conv(x, w) by the GEMM kernel (identity fold), batch
    statistics over all N*Ho*Wo pixels (one pass: per-block shifted sums merged with Chan's formula), y = relu(gamma (z - mean) rstd
    + beta + residual), running statistics updated with `momentum` (unbiased variance).  keep (`_Saved.bn`, when the pass is
    saved) receives (z, mean, rstd).  -> (y, mask)"""
    z, _ = _conv(i, s, fold, x, None, False, N, H, W, want_mask=False)
    rows = z.numel() // s.cout
    mean, var = K.colstats(z)                                        # one pass; biased variance, as the forward uses it
    gamma, beta, rmean, rvar = _bn_of(p, bufs, i)
    scale, shift, rstd = K.bn_train_fwd_coeffs(mean, var, gamma, beta, BN_EPS, rows, momentum, rmean, rvar)
    y, mask = K.bn_apply(z, scale, shift, residual, relu, want_mask and fold.pl)
    if keep is not None:
        keep[i] = (z, mean, rstd)
    return y, mask


def _stem_pool_on() -> bool:
    """CXRK_STEM_POOL=0 restores the unfused stem (convolution, max-pool, column sums of the max-pool gradient as separate kernels)"""
    return os.environ.get("CXRK_STEM_POOL", "1") != "0"


def _trunk(specs, blocks, unit, x0, H, W, pl, st: Optional[_Saved] = None, keep_stem=False, stages: Optional[list] = None,
           stem_pool: Optional[Callable] = None):
    """The walk the forward and the BatchNorm calibration share: stem, max-pool, the bottlenecks, the projector's conv + BN + ReLU,
    every unit through `unit(i, x, residual, relu, H, W, want_mask=True) -> (y, mask)`.  Fills `st` when the pass is saved.
    stem_pool (planes mode, eval-mode BatchNorm, stem output not kept): `stem_pool(x0, H, W, want_idx) -> (pooled, idx) or None`, the
    stem and its max-pool in one kernel (kernels.stem_pool_fwd_pl); None = this geometry is not fused, take the two kernels.
    -> (projector hidden activation pj1, h, w)"""
    s0 = specs[0]
    fused = stem_pool(x0, H, W, st is not None) if stem_pool is not None else None
    if fused is not None:
        (cur, idx), stem = fused, None
        Hs, Ws = _out_hw(s0, H, W)
    else:
        stem, _ = unit(0, x0, None, True, H, W, want_mask=False)   # its ReLU mask = sign of the pooled value
        cur, idx = K.maxpool_fwd_pl(stem) if pl else K.maxpool_fwd(stem)
        Hs, Ws = stem.shape[1], stem.shape[2]
    if st is not None:
        st.x0, st.idx, st.pooled, st.Hs, st.Ws = x0, idx, cur, Hs, Ws
        st.stem = stem if (keep_stem or not pl) else None     # planes mode: the max-pool backward needs only `pooled`
    del stem, x0, idx
    h, w = cur.shape[1], cur.shape[2]
    if stages is not None:
        stages.append(cur)
    for bi, blk in enumerate(blocks):
        o1, m1 = unit(blk["c1"], cur, None, True, h, w)
        o2, m2 = unit(blk["c2"], o1, None, True, h, w)
        h2, w2 = o2.shape[1], o2.shape[2]
        idt = unit(blk["ds"], cur, None, False, h, w)[0] if blk["ds"] is not None else cur
        out, m3 = unit(blk["c3"], o2, idt, True, h2, w2)
        if st is not None:
            st.blocks.append(_BlockSaved(cur, o1, o2, out if not pl else None, h, w, h2, w2, m1, m2, m3))
        cur, h, w = out, h2, w2
        if stages is not None and (bi + 1 == len(blocks) or blocks[bi + 1]["ds"] is not None):
            stages.append(cur)
    pj1, mp = unit(len(specs) - 1, cur, None, True, h, w)
    if st is not None:
        st.last, st.pj1, st.mp, st.h, st.w = cur, pj1, mp, h, w
    return pj1, h, w


def _proj_linear(pj1m, w3, b3, pl):
    """The projector's second linear on pixel rows [N*h*w, C] -> (fp32 [N*h*w, J], the split weight the planes backward reads or None)"""
    w3m = w3.reshape(w3.shape[0], -1)
    if pl:
        w3p = K.split_planes(w3m)
        return K.linear_fwd_pl(pj1m, w3p, b3), w3p
    return K.linear_fwd(pj1m, w3m, b3), None


def _stem_input(x: torch.Tensor, augment: Optional[AugmentCall]) -> torch.Tensor:
    """NCHW images -> the stem's NHWC input (3 channels zero-padded to 4): the plain layout transform, or the augmenting one"""
    if augment is None:
        return K.nchw_to_nhwc(x, 4)
    sp = augment.spec
    params = K.augment_params(x, sp, augment.seed, augment.counter, augment.row_offset)
    return K.augment_nhwc(x, 4, params, sp.size_for(x.shape[2], x.shape[3]), sp.clamp01)


def _forward(specs, blocks, p: Sequence[torch.Tensor], bufs: Sequence[torch.Tensor], x: torch.Tensor, save: bool,
             want_patch: bool, stages: Optional[list] = None, keep_stem: bool = False, bn_momentum: Optional[float] = None,
             augment: Optional[AugmentCall] = None):
    """bn_momentum: None = eval-mode BatchNorm (running statistics folded into the filters, the reference's only use of the encoder);
    a float = train-mode BatchNorm with that momentum (batch statistics; `ImageModel.train()`).  augment: the boundary transform
    NCHW -> NHWC samples the images through that call's random maps (csrc/augment.hip; 1-channel images are expanded to three) and
    the trunk runs at the size it samples to; the augmented tensor is the stem input the backward reads, so nothing else changes.
    -> (emb, patch, `_Saved` or None)"""
    N, C, H, W = x.shape
    if C != 3 and not (augment is not None and C == 1):
        raise ValueError(f"ImageModel expects 3-channel input (ExpandChannels, transforms.py:12-38), got {C}")
    if augment is not None:
        H, W = augment.spec.size_for(H, W)       # the trunk runs at the size the augmentation samples to
    pl = _planes_mode()
    fold = _Fold(specs, x.device, pl)
    train = bn_momentum is not None
    st = _Saved(fold, train, N, H, W) if save else None
    for i, s in enumerate(specs):
        fold.fold(i, s, p[3 * i], *(fold.identity(s.cout) if train else _bn_of(p, bufs, i)))

    def unit(i, x, residual, relu, H, W, want_mask=True):   # conv + BatchNorm (+ residual, ReLU) of unit i in the mode of this pass
        if train:
            return _conv_bn_train(i, specs[i], fold, p, bufs, x, residual, relu, N, H, W, want_mask, bn_momentum, st.bn if save else None)
        return _conv(i, specs[i], fold, x, residual, relu, N, H, W, want_mask)

    stem_pool = None
    s0 = specs[0]
    if (pl and not train and not keep_stem and stages is None and _stem_pool_on()
            and (s0.k, s0.stride, s0.pad, s0.cout, s0.cpad) == (7, 2, 3, 64, 4)):
        def stem_pool(x0, H, W, want_idx):
            return K.stem_pool_fwd_pl(x0, fold.ws(0, s0), fold.shift(0, s0), N, H, W, s0.cpad, s0.cout, s0.k, s0.k, s0.stride, s0.pad, want_idx)

    pj1, h, w = _trunk(specs, blocks, unit, _stem_input(x, augment), H, W, pl, st, keep_stem, stages, stem_pool)
    pj2, w3p = _proj_linear(pj1.view(N * h * w, pj1.shape[-1]), p[3 * len(specs)], p[3 * len(specs) + 1], pl)
    if save:
        st.w3p = w3p
    emb = K.spatial_mean_fwd(pj2.view(N, h * w, -1))
    patch = pj2.view(N, h, w, -1) if want_patch else None
    return emb, patch, st


def _unit_params_bwd(i, s, st: _Saved, p, bufs, x, dy, sumdy, N, H, W, sink: GradSink):
    """Parameter gradients of conv+BN unit i.  x: its input; dy: masked gradient w.r.t. its BN output; sumdy = sum of dy over
    pixels ([cout], reduced by the kernel that produced dy)."""
    fold = st.fold
    w = _filter_rsc(p[3 * i])
    if st.train:     # train-mode BatchNorm: dy is dz (gradient w.r.t. the raw convolution output), gamma / beta gradients are already
        #              written by `through_bn`; the kernel's own gamma / beta outputs go to scratch
        gw, acc = sink.dst(3 * i)
        dg = torch.empty(s.cout, dtype=torch.float32, device=w.device)
        db = torch.empty(s.cout, dtype=torch.float32, device=w.device)
    else:
        (gw, dg, db), acc = sink.dst_group(3 * i, 3 * i + 1, 3 * i + 2)
    if not acc and not gw.permute(0, 2, 3, 1).is_contiguous():     # fresh tensor: give it the filter's [Ko][R][S][C] memory
        gw = torch.empty_like(w).permute(0, 3, 1, 2)
        sink.ret[3 * i] = gw
    dw = gw.permute(0, 2, 3, 1)
    args = (w, fold.scale(i, s), fold.rstd(i, s), bufs[2 * i], sumdy, dw, dg, db, acc, N, H, W)
    if fold.on_planes(i):
        K.conv_bwd_params_pl(x, dy, *args, s.cpad, s.cout, s.k, s.k, s.stride, s.pad)
    else:           # fp32 mode; the stem (the fp32 image, split on the fly in split_bf16 mode)
        K.conv_bwd_params(x, dy, *args, s.cin, s.cpad, s.cout, s.k, s.k, s.stride, s.pad)


def _dgrad(i, s, fold, dy, residual, relu, N, H, W, want_sums, residual_s2=False):
    """Data gradient of unit i, masked by `relu` (planes mode: the bit mask of the tensor the gradient flows into; fp32 mode:
    that tensor itself).  want_sums: also the column sums of the result (-> (dx, sums[C])).  residual_s2 (planes mode): the
    residual is the compact gradient of a stride-2 projection shortcut (kernels.conv1x1_s2_bwd_data_compact_pl)."""
    dev = fold.vec.device
    sums = torch.empty(s.cpad, dtype=torch.float32, device=dev) if want_sums else None
    if fold.pl:
        dx = Planes.empty(N, H, W, s.cpad, device=dev)
        K.conv_bwd_data_pl(dy, fold.ws(i, s), residual, relu, dx, N, H, W, s.cpad, s.cout, s.k, s.k, s.stride, s.pad, sums,
                           residual_s2=residual_s2)
    else:
        dx = torch.empty(N, H, W, s.cpad, dtype=torch.float32, device=dev)
        K.conv_bwd_data(dy, fold.ws(i, s), residual, relu, dx, N, H, W, s.cpad, s.cout, s.k, s.k, s.stride, s.pad, sums)
    return (dx, sums) if want_sums else dx


def stage_of_param(name: str) -> str:
    """Stage tag of an image-encoder parameter, in the order the backward completes them: "head" (projector + layer4),
    "layer3", "layer2", "stem" (layer1 + the stem)."""
    if name.startswith("projector.") or ".layer4." in name:
        return "head"
    if ".layer3." in name:
        return "layer3"
    if ".layer2." in name:
        return "layer2"
    return "stem"


def _head_bwd(st: _Saved, p, demb, dpatch, sink: GradSink):
    """Backward of the projector head, pj2 = pj1 @ w3^T + b3, emb = mean of pj2 over the P patches: the cotangent of pj2 from those
    of the embedding and / or the patch output, the gradients of w3 and b3, the data gradient masked by the projector's ReLU and
    its column sums.  -> (g [N, h, w, C], sums [C]); the two storage modes side by side."""
    pl, N, P = st.pl, st.N, st.h * st.w
    jw = len(p) - 2
    w3m = p[jw].reshape(p[jw].shape[0], -1)
    J = w3m.shape[0]
    gw3, acc3 = sink.dst(jw)
    gb3, accb3 = sink.dst(jw + 1)
    gw3m = gw3.permute(0, 2, 3, 1).reshape(J, -1) if gw3.dim() == 4 else gw3.reshape(J, -1)   # [J, C, 1, 1] is [J, C] in memory
    assert gw3m.data_ptr() == gw3.data_ptr()
    if demb is None:
        dpj2 = dpatch.reshape(N * P, J).contiguous()
        dpj2 = K.split_planes(dpj2) if pl else dpj2
    elif pl:
        dpj2 = K.spatial_mean_bwd_pl(demb.contiguous(), P, add=dpatch.reshape(N, P, J) if dpatch is not None else None).view(N * P, J)
    else:
        dpj2 = K.spatial_mean_bwd(demb.contiguous(), P).view(N * P, J)
        if dpatch is not None:
            dpj2 = dpj2 + dpatch.reshape(N * P, J)
    pj1m = st.pj1.view(N * P, st.pj1.shape[-1])
    (K.linear_bwd_weight_pl if pl else K.linear_bwd_weight)(dpj2, pj1m, gw3m, accumulate=acc3)
    K.colsum(dpj2, gb3, accumulate=accb3)
    if pl:
        g = K.linear_bwd_data_pl(dpj2, st.w3p, maskin=st.mp, out_planes=True)
    else:
        g = K.linear_bwd_data(dpj2, w3m, aux=pj1m, auxmode=K.AUX_RELU_MASK)
    sums = K.colsum(g, torch.empty(g.shape[1], dtype=torch.float32, device=w3m.device))
    return g.view(N, st.h, st.w, g.shape[1]), sums


_STAGE_DONE_AT = {LAYERS[0] + LAYERS[1] + LAYERS[2]: "head", LAYERS[0] + LAYERS[1]: "layer3", LAYERS[0]: "layer2"}   # first block of layer4 / 3 / 2


def _backward(specs, blocks, p, bufs, st: _Saved, demb: Optional[torch.Tensor], dpatch: Optional[torch.Tensor], sink: GradSink,
              on_grads_ready=None):
    """`on_grads_ready(tag)` (optional) is called on the current stream when every parameter gradient of a stage has been written
    in place: "head" after the projector and layer4, "layer3", "layer2", and "stem" (layer1 + stem) at the end — only while no
    gradient of the stage had to be returned to autograd as a fresh tensor."""
    fold, N, dev = st.fold, st.N, st.fold.vec.device

    def params_bwd(i, x_, dy_, sum_, H_, W_):
        # (Running these launches on a side stream, beside the data-gradient chain they depend on but which does not depend on them,
        #  was measured in round 3: 158.74 against 158.66 / 158.94 ms per step, bit-identical results — the GPU is not idle at kernel
        #  tails, the step is the sum of its kernels' times.  Not kept.)
        _unit_params_bwd(i, specs[i], st, p, bufs, x_, dy_, sum_, N, H_, W_, sink)

    def dgrad(i, dy_, residual, relu, H_, W_, want_sums, residual_s2=False):
        return _dgrad(i, specs[i], fold, dy_, residual, relu, N, H_, W_, want_sums, residual_s2)

    def through_bn(i, dy_, sum_):
        """TRAIN-mode BatchNorm of unit i: the gradient w.r.t. its output (already masked by the unit's ReLU) and its column sums ->
        the gradient w.r.t. the raw convolution output, dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)); writes dgamma = sum dy
        xhat and dbeta = sum dy.  Eval mode: the identity (the running statistics are constants folded into the filters)."""
        if st.bn is None:
            return dy_, sum_
        z, mean, rstd = st.bn.pop(i)
        C = specs[i].cout
        (dg, db), acc = sink.dst_group(3 * i + 1, 3 * i + 2)
        dot = K.coldot(dy_, z, mean)                                # sum dy (z - mean): centred before it is summed
        A, B, Cc = K.bn_train_bwd_coeffs(p[3 * i + 1], mean, rstd, sum_, dot, z.numel() // C, dg, db, acc)
        return K.bn_train_dz(dy_, z, A, B, Cc), torch.zeros(C, dtype=torch.float32, device=dev)   # sum of dz over the pixels is 0

    ip = len(specs) - 1
    g, sum_p = through_bn(ip, *_head_bwd(st, p, demb, dpatch, sink))
    params_bwd(ip, st.last, g, sum_p, st.h, st.w)
    g, gs = dgrad(ip, g, None, st.blocks[-1].relu_of(3), st.h, st.w, True)
    for bi in reversed(range(len(blocks))):
        blk, b = blocks[bi], st.blocks[bi]
        c1, c2, c3, ds = blk["c1"], blk["c2"], blk["c3"], blk["ds"]
        # out = relu(bn3(conv3(o2)) + identity): g (already masked by out > 0) is dy of bn3 and of the downsample BN; its
        # channel sums gs were reduced by the kernel that produced g
        g3, gs3 = through_bn(c3, g, gs)       # (eval mode: g itself; the downsample BatchNorm below sees the same g)
        params_bwd(c3, b.o2, g3, gs3, b.h2, b.w2)
        d2, q2 = dgrad(c3, g3, None, b.relu_of(2), b.h2, b.w2, True)
        del g3
        d2, q2 = through_bn(c2, d2, q2)
        params_bwd(c2, b.o1, d2, q2, b.h, b.w)
        d1, q1 = dgrad(c2, d2, None, b.relu_of(1), b.h, b.w, True)
        del d2
        d1, q1 = through_bn(c1, d1, q1)
        params_bwd(c1, b.x, d1, q1, b.h, b.w)
        if ds is not None:
            sd = specs[ds]
            gd, gsd = through_bn(ds, g, gs)
            params_bwd(ds, b.x, gd, gsd, b.h, b.w)
            # a stride-2 projection: its data gradient is non-zero at the even pixels only -> compact [N, h/2, w/2, C], added
            # by the epilogue of conv1's data gradient at those pixels (instead of zero-filling, writing and re-reading a
            # full-resolution tensor that is 3/4 zeros: 12.8 -> 2.8 GB per step at batch 1024)
            res = None
            if st.pl and sd.k == 1 and sd.stride == 2 and sd.pad == 0 and os.environ.get("CXRK_S2RES", "1") != "0":
                res = K.conv1x1_s2_bwd_data_compact_pl(gd, fold.ws(ds, sd), N, b.h, b.w, sd.cpad, sd.cout)   # None: too large
            res_s2 = res is not None
            if res is None:
                res = dgrad(ds, gd, None, None, b.h, b.w, False)
            del gd
        else:
            res, res_s2 = g, False
        if bi > 0:
            g, gs = dgrad(c1, d1, res, st.blocks[bi - 1].relu_of(3), b.h, b.w, True, residual_s2=res_s2)
        else:   # the block input is the max-pool output: its ReLU (the stem's) is applied by the max-pool backward
            g, gs = dgrad(c1, d1, res, None, b.h, b.w, False, residual_s2=res_s2), None
        del d1, res
        st.blocks[bi] = None
        if on_grads_ready is not None and bi in _STAGE_DONE_AT and all(r is None for r in sink.ret[3 * c1:]):
            on_grads_ready(_STAGE_DONE_AT[bi])     # every gradient from this block's first unit onwards is complete
    if st.pl:
        dstem = K.maxpool_bwd_pl(g, st.idx, st.pooled, st.Hs, st.Ws)
    else:
        dstem = K.maxpool_bwd(g, st.idx, st.stem, True)
    if _debug is not None:
        _debug["ds"], _debug["x0"] = dstem, st.x0
    if st.pl and st.bn is None and _stem_pool_on() and dstem.shape[-1] == 64:
        sum_s = K.stem_pool_bwd_sums(g, st.pooled)     # the same sums in pooled space: no pass over the [N, Hs, Ws, 64] gradient
    else:
        sum_s = K.colsum(dstem.view(-1, dstem.shape[-1]), torch.empty(dstem.shape[-1], dtype=torch.float32, device=dev))
    dstem, sum_s = through_bn(0, dstem, sum_s)
    params_bwd(0, st.x0, dstem, sum_s, st.H, st.W)
    if on_grads_ready is not None and all(r is None for r in sink.ret):
        on_grads_ready("stem")
    return sink.ret


class Decisions(list):
    """ReLU decisions of a forward pass (a list, in execution order) + the max-pool winners (`pool_taps`, NCHW uint8)."""
    pool_taps: Optional[torch.Tensor] = None


def relu_decisions(st: _Saved) -> List[torch.Tensor]:
    """The 0/1 decision of every ReLU of a forward pass, in execution order (stem, relu1/relu2/relu_out per
    bottleneck, projector), as NCHW bool tensors on the CPU.  Used by the parity tests: gradients of a ReLU network
    are only comparable between two fp32 implementations under identical decisions (see oracle/ref_image.ReluPolicy).
    Planes mode keeps the decisions as bit masks; the stem's come from its output, which `capture_relu_decisions` makes the
    forward keep for this purpose."""
    def nchw(t):
        return (t > 0).permute(0, 3, 1, 2).contiguous().cpu()

    def unpacked(m, hh, ww):
        C = m.shape[1] * 8
        return K.unpack_mask(m, C).view(st.N, hh, ww, C).permute(0, 3, 1, 2).contiguous()

    if not st.pl:
        out = Decisions(nchw(a) for a in [st.stem] + [a for b in st.blocks for a in (b.o1, b.o2, b.out)] + [st.pj1])
    elif st.stem is None:
        raise RuntimeError("relu_decisions: the stem output was not kept (run the forward inside capture_relu_decisions())")
    else:
        out = Decisions([nchw(st.stem.float())])
        for b in st.blocks:
            out += [unpacked(b.m1, b.h, b.w), unpacked(b.m2, b.h2, b.w2), unpacked(b.m3, b.h2, b.w2)]
        out.append(unpacked(st.mp, st.h, st.w))
    out.pool_taps = st.idx.permute(0, 3, 1, 2).contiguous().cpu()
    return out


def _pack_bits(a: torch.Tensor) -> torch.Tensor:
    """bool [rows, C] (device) -> the ReLU bit-mask layout of the epilogues: uint8 [rows, C/8], bit c % 8 of byte c / 8."""
    rows, C = a.shape
    w = 1 << torch.arange(8, device=a.device, dtype=torch.int32)
    return (a.view(rows, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def device_decisions(st: _Saved) -> dict:
    """Every 0/1 decision of a saved forward pass, kept ON THE DEVICE in the layout the planes backward reads: per bottleneck the
    three ReLU bit masks, the projector's, the max-pool winners and the stem's ReLU decision at the winning input.  Works on the
    state of either storage mode; `impose_decisions_` writes such a set into a planes-mode state.  Test / bench instrumentation
    (full-size cross-precision gradient check): two correct forwards differ in the last bits, so a few 1e-5 of the decisions
    differ, and a gradient is only comparable under equal decisions."""
    def bits(act):
        return _pack_bits((act > 0).view(-1, act.shape[-1]))

    if st.pl:
        blocks = [(b.m1, b.m2, b.m3) for b in st.blocks]
        proj = st.mp
        stem_pos = st.pooled.t[0].float() > 0
    else:
        blocks = [(bits(b.o1), bits(b.o2), bits(b.out)) for b in st.blocks]
        proj = bits(st.pj1)
        stem_pos = st.pooled > 0
    return {"blocks": [tuple(m.clone() for m in t) for t in blocks], "proj": proj.clone(), "pool_taps": st.idx.clone(), "stem_pos": stem_pos}


def count_decision_differences(a: dict, b: dict) -> dict:
    """How many decisions differ between two `device_decisions` sets (population counts of the XOR-ed masks)."""
    def bits(x, y):
        d = (x ^ y).to(torch.int32)
        n = 0
        for k in range(8):
            n += int(((d >> k) & 1).sum())
        return n
    relu = sum(bits(x, y) for ta, tb in zip(a["blocks"], b["blocks"]) for x, y in zip(ta, tb)) + bits(a["proj"], b["proj"])
    total = sum(x.numel() * 8 for ta in a["blocks"] for x in ta) + a["proj"].numel() * 8
    return {"relu": relu + int((a["stem_pos"] != b["stem_pos"]).sum()), "relu_total": total + a["stem_pos"].numel(),
            "pool_taps": int((a["pool_taps"] != b["pool_taps"]).sum()), "pool_total": a["pool_taps"].numel()}


def impose_decisions_(node, dec: dict) -> None:
    """Overwrite the decisions a planes-mode forward saved for its backward (`node` = the `grad_fn` of its output) with `dec`:
    the backward then differentiates the function the OTHER forward selected.  The stem's ReLU decision is read by the max-pool
    backward from the sign of the pooled activation's hi plane; it gets a stand-in tensor that carries the imposed signs, the
    pooled activation itself (the weight-gradient operand of layer1.0) stays untouched."""
    st = node.state
    if not st.pl:
        raise RuntimeError("impose_decisions_: only the planes (split_bf16) backward reads stored decisions")
    for b, t in zip(st.blocks, dec["blocks"]):
        for m, src in zip((b.m1, b.m2, b.m3), t):
            m.copy_(src)
    st.mp.copy_(dec["proj"])
    st.idx.copy_(dec["pool_taps"])
    sign = Planes(torch.zeros_like(st.pooled.t))
    sign.t[0].copy_(dec["stem_pos"].to(torch.bfloat16))
    st.pooled = sign                       # `st.blocks[0].x` still is the true pooled activation


@torch.no_grad()
def calibrate_batchnorm_(specs, blocks, params, bufs, x: torch.Tensor) -> None:
    """Set the running statistics of every BatchNorm of the encoder to the statistics of its input over the batch `x` (what one
    train-mode pass with momentum 1 would leave behind; `torch.nn.BatchNorm2d` semantics: unbiased variance), unit by unit in
    execution order on the encoder's own kernels: the raw convolution output of a unit is obtained by folding an identity
    BatchNorm, then the unit is re-run with its new statistics to feed the next one.  Used to give SYNTHETIC weights the property
    every trained checkpoint has — statistics that match the activations — without which a random ResNet-50 in eval mode maps all
    images to nearly the same embedding (bench.py; the reference only ever loads trained BioViL weights, model.py:117-118)."""
    import math
    N, C, H, W = x.shape
    pl = _planes_mode()
    fold = _Fold(specs, x.device, pl)
    p = [t.detach() for t in params]
    b = [t.detach() for t in bufs]
    k = math.sqrt(1.0 + BN_EPS)          # the identity fold below (variance 1) scales by rsqrt(1 + eps)

    def unit(i, xin, residual, relu, h, w, want_mask=True):
        s = specs[i]
        one, zero = fold.identity(s.cout)[:2]
        fold.fold(i, s, p[3 * i], one, zero, zero, one)
        raw, _ = _conv(i, s, fold, xin, None, False, N, h, w, want_mask=False)
        r = raw.view(-1, s.cout)                       # [pixels, channels], fp32 or planes
        rows = r.shape[0]
        # two-pass batch statistics on the path's own reductions; the identity fold scaled the output by 1 / k
        K.colsum(r, b[2 * i], alpha=1.0 / rows)                                       # mean of raw
        K.colvar(r, b[2 * i], b[2 * i + 1], alpha=k * k / max(1, rows - 1))           # unbiased variance of k * raw
        K.scale_mask(b[2 * i], alpha=k, out=b[2 * i])                                 # mean of k * raw
        del raw, r
        fold.fold(i, s, p[3 * i], *_bn_of(p, b, i))
        return _conv(i, s, fold, xin, residual, relu, N, h, w, want_mask=want_mask)

    _trunk(specs, blocks, unit, K.nchw_to_nhwc(x, 4), H, W, pl)


_capture: Optional[list] = None
_debug: Optional[dict] = None      # diagnostics (scripts/exp_grad_err.py): set to a dict to receive the stem's gradient tensors


class capture_relu_decisions:
    """Test hook: `with capture_relu_decisions() as cap:` makes every grad-enabled image-encoder forward inside the block
    append its ReLU decisions (`relu_decisions`, CPU bool tensors) to `cap`.  Nothing is kept outside the block, and the
    saved-activation state itself is never referenced from module level (it lives on the autograd node only)."""

    def __enter__(self):
        global _capture
        self._old, _capture = _capture, []
        return _capture

    def __exit__(self, *exc):
        global _capture
        _capture = self._old
        return False


class ImageEncodeFn(torch.autograd.Function):
    """(x[N,3,H,W], meta: EncodeMeta, *params, *buffers) -> (global embedding [N,J], projected patch embeddings NHWC or None)."""

    @staticmethod
    def forward(ctx, x, meta, *tensors):
        ctx.set_materialize_grads(False)
        params, bufs = tensors[:meta.n_params], tensors[meta.n_params:]
        save = any(t.requires_grad for t in params) and not meta.save_free
        p = [t.detach() for t in params]
        b = [t.detach() for t in bufs]
        emb, patch, state = _forward(meta.specs, meta.blocks, p, b, x.detach(), save, meta.want_patch, keep_stem=_capture is not None,
                                     bn_momentum=meta.bn_momentum, augment=meta.augment)
        if save:
            ctx.state, ctx.p, ctx.b, ctx.meta, ctx.params = state, p, b, meta, params
            if _capture is not None:
                _capture.append(relu_decisions(state))
        if patch is None:
            patch = emb.new_empty(0)
        return emb, patch

    @staticmethod
    def backward(ctx, demb, dpatch):
        meta = ctx.meta
        if dpatch is not None and dpatch.numel() == 0:
            dpatch = None
        sink = GradSink(ctx.params)
        grads = _backward(meta.specs, meta.blocks, ctx.p, ctx.b, ctx.state, demb, dpatch, sink, meta.on_grads_ready)
        ctx.state = None
        return (None, None) + tuple(grads) + (None,) * len(ctx.b)


@torch.no_grad()
def forward_stages(specs, blocks, params, bufs, x: torch.Tensor) -> List[torch.Tensor]:
    """Diagnostic (parity tests): the trunk's stage outputs [max-pooled stem, layer1, layer2, layer3, layer4] as fp32 NCHW
    tensors, from the same kernels `ImageEncodeFn` runs."""
    stages: list = []
    _forward(specs, blocks, [t.detach() for t in params], [t.detach() for t in bufs], x, False, False, stages=stages)
    return [K.nhwc_to_nchw((t.float() if isinstance(t, Planes) else t).contiguous()) for t in stages]


@torch.no_grad()
def project_patches(specs, params, bufs, patch_nchw: torch.Tensor) -> torch.Tensor:
    """The projector alone (`modules.MLP`, reference modules.py:29-47): trunk patch embeddings [N,2048,h,w] -> projected patch
    embeddings [N,J,h,w], on the same kernels the encoder uses (fixture check against the reference's own MLP)."""
    N, C, h, w = patch_nchw.shape
    pl = _planes_mode()
    ip = len(specs) - 1
    p = [t.detach() for t in params]
    fold = _Fold(specs, patch_nchw.device, pl)
    fold.fold(ip, specs[ip], p[3 * ip], *_bn_of(p, [t.detach() for t in bufs], ip))
    x = K.nchw_to_nhwc(patch_nchw.contiguous(), C)
    if pl:
        x = K.split_planes(x)
    pj1, _ = _conv(ip, specs[ip], fold, x, None, True, N, h, w, want_mask=False)
    pj2, _ = _proj_linear(pj1.view(N * h * w, pj1.shape[-1]), p[3 * ip + 3], p[3 * ip + 4], pl)
    return K.nhwc_to_nchw(pj2.view(N, h, w, -1))
