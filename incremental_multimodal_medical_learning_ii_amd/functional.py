"""Autograd-enabled operators of the hot path (each a `torch.autograd.Function` over the cxrk kernels).

    l2_normalize                 F.normalize(x, dim=1)            modelling_cxrbert.py:138-139, vlp/inference_engine.py:51
    linear / mlp_adapter         nn.Linear, models.myMLP          models.py:7-26
    pairwise_cosine_similarity   torchmetrics call                Trainer.py:1682-1704
    group_mean                   prompt-embedding mean            Trainer.py:1665-1666
    posneg_bce_loss              pos-neg logits + BCEWithLogits   Trainer.py:575-583, ZERO_JOINT_BOUNDS.py:36
    infonce_loss                 north-star contrastive head (not in the reference), data-parallel aware
    distill_loss                 similarity distillation from a frozen teacher's embeddings (not in the reference), data-parallel aware
    augment_images               on-device random affine + jitter (train-time transforms; no gradient)
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import kernels as K
from .gradsink import GradSink


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        xhat, norm = K.l2norm_fwd(x.detach(), eps)
        ctx.save_for_backward(xhat, norm)
        return xhat

    @staticmethod
    def backward(ctx, g):
        xhat, norm = ctx.saved_tensors
        return K.l2norm_bwd(g, xhat, norm), None


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """F.normalize(x, p=2, dim=1) for a 2-D (or 1-D) tensor."""
    if x.dim() == 1:
        return _L2Norm.apply(x.unsqueeze(0), eps).squeeze(0)
    return _L2Norm.apply(x, eps)


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b); act in {none, relu}.  Saves x and (for relu) y."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        xd, wd = x.detach(), w.detach()
        if xd.dim() != 2:
            raise ValueError(f"linear: expected a 2-D input, got {tuple(xd.shape)}")
        xd = xd.contiguous()
        y = K.linear_fwd(xd, wd, None if b is None else b.detach(), act=act)
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.save_for_backward(xd, wd, y if act == K.ACT_RELU else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.act == K.ACT_RELU:
            # mask the incoming gradient by the ReLU of this layer: dz = dy * (y > 0)
            dz = K.scale_mask(dy, mask_src=y)
        else:
            dz = dy
        dx = K.linear_bwd_data(dz, w) if ctx.needs_input_grad[0] else None
        dw = K.linear_bwd_weight(dz, x, torch.empty_like(w)) if ctx.needs_input_grad[1] else None
        db = K.colsum(dz, torch.empty(w.shape[0], dtype=torch.float32, device=w.device)) if ctx.has_bias else None
        return dx, dw, db, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = K.ACT_NONE):
    return _Linear.apply(x, weight, bias, act)


class _MLPAdapter(torch.autograd.Function):
    """models.myMLP: Linear(128,256) -> ReLU -> Linear(256,128), one Function so the ReLU mask rides the dgrad GEMM."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        xd = x.detach().contiguous()
        h = K.linear_fwd(xd, w1.detach(), b1.detach(), act=K.ACT_RELU)
        y = K.linear_fwd(h, w2.detach(), b2.detach())
        ctx.save_for_backward(xd, h, w1.detach(), w2.detach())
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, w1, w2 = ctx.saved_tensors
        dy = dy.contiguous()
        dev = dy.device
        dw2 = K.linear_bwd_weight(dy, h, torch.empty_like(w2))
        db2 = K.colsum(dy, torch.empty(w2.shape[0], dtype=torch.float32, device=dev))
        dh = K.linear_bwd_data(dy, w2, aux=h, auxmode=K.AUX_RELU_MASK)
        dw1 = K.linear_bwd_weight(dh, x, torch.empty_like(w1))
        db1 = K.colsum(dh, torch.empty(w1.shape[0], dtype=torch.float32, device=dev))
        dx = K.linear_bwd_data(dh, w1) if ctx.needs_input_grad[0] else None
        return dx, dw1, db1, dw2, db2


def mlp_adapter(x, w1, b1, w2, b2):
    return _MLPAdapter.apply(x, w1, b1, w2, b2)


class _PairwiseCosine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        cosv, xn, yn = K.pairwise_cosine_fwd(xd, yd)
        ctx.save_for_backward(xd, yd, cosv, xn, yn)
        return cosv

    @staticmethod
    def backward(ctx, dcos):
        x, y, cosv, xn, yn = ctx.saved_tensors
        dx, dy = K.pairwise_cosine_bwd(x, y, cosv, dcos.contiguous(), xn, yn, need_dx=ctx.needs_input_grad[0])
        return dx, (dy if ctx.needs_input_grad[1] else None)


def pairwise_cosine_similarity(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """torchmetrics.functional.pairwise_cosine_similarity(x, y): [B,D] x [P,D] -> [B,P] (no epsilon)."""
    return _PairwiseCosine.apply(x, y)


class _PairwiseCosineMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, groups):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        cosv, xn, yn, mx, mean, arg = K.pairwise_cosine_max_fwd(xd, yd, groups)
        ctx.save_for_backward(xd, yd, cosv, xn, yn, arg)
        ctx.mark_non_differentiable(mean, arg)
        return mx, mean, arg

    @staticmethod
    def backward(ctx, dmax, _dmean, _darg):
        x, y, cosv, xn, yn, arg = ctx.saved_tensors
        dx, dy = K.pairwise_cosine_max_bwd(x, y, cosv, dmax, arg, xn, yn, need_dx=ctx.needs_input_grad[0])
        return dx, (dy if ctx.needs_input_grad[1] else None), None


def pairwise_cosine_max(x: torch.Tensor, y: torch.Tensor, groups: int = 1):
    """MAX_EMB scoring (`Trainer.py:1691-1693`) for `groups` prompt sets at once: x [B,D], y [groups*Pg, D] ->
    (max over each set's prompts [B,groups], their mean [B,groups] (logged only, not differentiable), winner index)."""
    return _PairwiseCosineMax.apply(x, y, groups)


class _GroupMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, groups, n):
        ctx.gn = (groups, n)
        return K.group_mean_fwd(x.detach(), groups, n)

    @staticmethod
    def backward(ctx, g):
        groups, n = ctx.gn
        return K.group_mean_bwd(g, groups, n), None, None


def group_mean(x: torch.Tensor, groups: int, n: int) -> torch.Tensor:
    """x [groups*n, D] -> [groups, D]: mean over the n prompts of each group."""
    return _GroupMean.apply(x, groups, n)


class _PosNegBCE(torch.autograd.Function):
    """cos [B,2C] -> scalar BCE-with-logits of (cos_pos - cos_neg), mean (scale 1) or sum (scale B*C) over the B*C logits; the
    gradient is computed in the same pass."""

    @staticmethod
    def forward(ctx, cosv, labels, diff, scale):
        logits, dcos, loss = K.bce_posneg_fwd_bwd(cosv.detach().contiguous(), labels, diff=diff, need_grad=True)
        ctx.save_for_backward(dcos)
        ctx.scale = float(scale)
        ctx.mark_non_differentiable(logits)
        if scale != 1.0:
            loss = K.scale_mask(loss.reshape(1), alpha=float(scale)).reshape(())
        return loss, logits

    @staticmethod
    def backward(ctx, gloss, _glogits):
        (dcos,) = ctx.saved_tensors
        return K.scale_mask(dcos, alpha_dev=gloss.reshape(()).contiguous(), alpha=ctx.scale), None, None, None


def posneg_bce_loss(cosv: torch.Tensor, labels: torch.Tensor, diff: bool = True, reduction: str = "mean") -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, logits).  cos column 2c = positive prompt of class c, 2c+1 = negative.  `reduction`: "mean" (`nn.BCEWithLogitsLoss()`,
    the reference's criterion, ZERO_JOINT_BOUNDS.py:36) or "sum"."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"posneg_bce_loss: reduction must be 'mean' or 'sum', got {reduction!r}")
    n_logits = cosv.shape[0] * (cosv.shape[1] // 2)
    return _PosNegBCE.apply(cosv, labels, diff, 1.0 if reduction == "mean" else float(n_logits))


# --------------------------------------------------------------------------------------------------------------
# The global-batch loss heads: InfoNCE (north star), pairwise sigmoid, similarity distillation.
# One protocol (`_shard` .. `_backward_tail`), then the three heads with what is their own.
# --------------------------------------------------------------------------------------------------------------

def _all_gather_rows(t: torch.Tensor, group) -> torch.Tensor:
    """[rows, ...] contiguous on every rank -> [world * rows, ...], rank-major.  One collective, no staging copy on RCCL."""
    import torch.distributed as dist
    ws = dist.get_world_size(group)
    assert t.is_contiguous()
    out = torch.empty((ws * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    if t.is_cuda and dist.get_backend(group) == "gloo":
        # gloo has no GPU all-gather: stage through the host (rehearsals of the N>1 path on one GPU; RCCL takes the line below)
        host = torch.empty(out.shape, dtype=t.dtype)
        dist.all_gather_into_tensor(host, t.detach().cpu(), group=group)
        out.copy_(host)
        return out
    dist.all_gather_into_tensor(out, t, group=group)
    return out


def _shard(group) -> Tuple[bool, int, int]:
    """(data parallel?, this rank, number of ranks).  A step is data parallel with an explicit `group`, or with an initialised
    default group of more than one rank; otherwise it is the single process (False, 0, 1) and reaches no collective."""
    import torch.distributed as dist
    if group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return True, dist.get_rank(group), dist.get_world_size(group)
    return False, 0, 1


# Every check of a head's inputs runs BEFORE its first collective: a rank that raised inside loss.backward(), or after its peers
# had entered a gather, would leave them waiting in the collective.

def _check_pairs(what: str, img: torch.Tensor, txt: torch.Tensor, world: int) -> Tuple[int, int]:
    """(B, D) of this rank's [B, D] image and text embeddings; `what` is the public function the message names"""
    if img.dim() != 2 or tuple(txt.shape) != tuple(img.shape):
        raise ValueError(f"{what}: image embeddings are {tuple(img.shape)} but text embeddings {tuple(txt.shape)}")
    B, D = img.shape
    if (B * world) % 4 != 0 or D % 4 != 0:
        # the backward GEMMs contract over the global batch with 16-byte row accesses
        raise ValueError(f"{what}: global batch {B * world} (= {B} rows x {world} ranks) and embedding size {D} must be "
                         f"multiples of 4 (drop or pad the ragged last batch)")
    return B, D


def _check_keys(what: str, keys, B: int, device) -> Optional[torch.Tensor]:
    if keys is None:
        return None
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64:
        raise ValueError(f"{what}: keys must be an int64 tensor, got {getattr(keys, 'dtype', type(keys).__name__)}")
    if tuple(keys.shape) != (B,):
        raise ValueError(f"{what}: keys must have shape ({B},), one per local row, got {tuple(keys.shape)}")
    if keys.device != device:
        raise ValueError(f"{what}: keys are on {keys.device} but the embeddings on {device}")
    return keys.detach().contiguous()


def _device_scalar(what: str, t, name: str, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be an fp32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.numel() != 1 or t.dim() > 1:
        raise ValueError(f"{what}: {name} must be 0-d or have shape (1,), got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device} but the embeddings on {device}")
    return t.detach()


def _gather_normalised(embs, keys, group, shard):
    """The data-parallel form of every head (one process per GPU): rank r owns B rows of each [B, D] tensor of `embs` (image and
    text embeddings; the distillation head adds the teacher's two).  They are L2-normalised into the column slices of ONE [B, n D]
    send buffer, written in place by the normalisation kernels, and ONE all-gather makes it the [Bg, n D] buffer of the global
    batch, which the GEMMs read through its column slices (row stride n D): no cat / contiguous copies.  With the per-row statistics
    a head exchanges on top (none, or a few floats per row), every rank then holds what it needs to form the exact gradient of the
    global-mean loss w.r.t. its own rows: no reduce-scatter of embedding gradients and no second matmul exchange.
    `keys` (int64 [B] or None) are gathered next to the embeddings, one more all-gather: row keys of a block are the local slice,
    column keys the gathered vector.  In a single process the local tensors stand in for the gathered ones.

    -> ([(xhat, norm, xhat_all) per tensor of `embs`], keys_all, the offset rank * B of this rank's rows in the global batch, Bg);
    the order is: every normalisation, the embedding gather, the keys gather."""
    on, rank, world = shard
    B, D = embs[0].shape
    cols = [slice(q * D, (q + 1) * D) for q in range(len(embs))]
    send = torch.empty(B, len(embs) * D, dtype=torch.float32, device=embs[0].device) if on else None
    local = [K.l2norm_fwd(e, out=send[:, c] if on else None) for e, c in zip(embs, cols)]
    if on:
        every = _all_gather_rows(send, group)                                        # [Bg, n D]
        keys_all = _all_gather_rows(keys, group) if keys is not None else None      # [Bg] int64
        gathered = [every[:, c] for c in cols]
    else:
        keys_all, gathered = keys, [xhat for xhat, _ in local]
    return [(xhat, norm, xhat_all) for (xhat, norm), xhat_all in zip(local, gathered)], keys_all, rank * B, B * world


def _logit_blocks(im, tx, alpha: float):
    """The two [B, Bg] logits blocks of a rank, from the (xhat, norm, xhat_all) triples of the image and the text side:
    S1 = alpha * local images x all texts, S2 = alpha * local texts x all images.  Row i of S1 is row `off + i` of the global
    S = I_hat T_hat^T, row i of S2 the same row of S^T: column j of S1 is text j over all images, so its statistics are row j's of
    the global S2, and the other way round."""
    (ih, _, ih_all), (th, _, th_all) = im, tx
    B, D = ih.shape
    Bg = ih_all.shape[0]
    S1 = torch.empty(B, Bg, dtype=torch.float32, device=ih.device)
    S2 = torch.empty(B, Bg, dtype=torch.float32, device=ih.device)
    K.gemm(ih, th_all, S1, B, Bg, D, False, True, alpha=alpha)
    K.gemm(th, ih_all, S2, B, Bg, D, False, True, alpha=alpha)
    return S1, S2


def _scalar_grad(p, part1, part2, upstream, scale: float):
    """d p = upstream * scale * (sum part1 + sum part2) for a one-element parameter, straight into a leaf's `.grad` (the flat
    gradient buffer's slot) when it has one of its own layout: autograd then adds nothing and gets None.  Any other `p` gets a
    fresh tensor, returned to autograd."""
    sink = GradSink([p])
    dst, accumulate = sink.dst(0, force_fresh=not p.is_leaf)
    K.logit_scale_grad(part1, part2, upstream, scale, dst, accumulate)
    return sink.result()[0]


def _backward_tail(S1, S2, im, tx, alpha: float, gloss, scalars=()):
    """From the gradient blocks a head left in S1 / S2 to the gradients of this rank's unnormalised embeddings:
    d I_hat = alpha * S1 @ T_hat_all and d T_hat = alpha * S2 @ I_hat_all (the GEMMs contract over the global batch), back through
    the normalisation, times the upstream scalar, which is read on the device.  `scalars`: the head's one-element parameters, each
    as (p, part1, part2, scale) for `_scalar_grad` or None for no gradient; they are formed between the two.
    -> (d img, d txt, [d p per entry of `scalars`])"""
    (ih, inorm, ih_all), (th, tnorm, th_all) = im, tx
    B, D = ih.shape
    Bg = S1.shape[1]
    dih = torch.empty(B, D, dtype=torch.float32, device=ih.device)
    dth = torch.empty(B, D, dtype=torch.float32, device=ih.device)
    K.gemm(S1, th_all, dih, B, D, Bg, False, False, alpha=alpha)
    K.gemm(S2, ih_all, dth, B, D, Bg, False, False, alpha=alpha)
    di, dt = (K.l2norm_bwd(d, xhat, norm) for d, xhat, norm in ((dih, ih, inorm), (dth, th, tnorm)))
    g = gloss.reshape(()).contiguous()
    dscalars = [None if s is None else _scalar_grad(s[0], s[1], s[2], g, s[3]) for s in scalars]
    return K.scale_mask(di, alpha_dev=g, out=di), K.scale_mask(dt, alpha_dev=g, out=dt), dscalars


def _infonce_stats(S, off, keys, keys_all, theta, loss, loss_scale: float):
    """(row log-sum-exp, positives per row or None) of one logits block; its share of the loss is added into `loss`.  The four
    kernels: plain or keyed targets, S as it stands or, with a learnable temperature, exp(theta) * S."""
    kw = dict(loss_out=loss, loss_scale=loss_scale, loss_accumulate=True)
    if keys is None:
        lse, _ = K.infonce_row_lse(S, off, **kw) if theta is None else K.infonce_row_lse_scaled(S, off, theta, **kw)
        return lse, None
    lse, _, npos = (K.multipos_row_stats(S, keys, keys_all, **kw) if theta is None else
                    K.multipos_row_stats_scaled(S, keys, keys_all, theta, **kw))
    return lse, npos


def _infonce_grad(S, off, keyed, theta, lse_row, lse_col):
    """S <- G = softmax_row + softmax_col - 2 * targets in place (`keyed`: None, or (keys, keys_all, positives per row)).  With a
    learnable temperature the block is left as exp(theta) * G and the partial sums of G o S are returned; otherwise None."""
    if theta is None:
        if keyed is None:
            K.infonce_grad_inplace(S, off, lse_row, lse_col)
        else:
            K.multipos_grad_inplace(S, *keyed, lse_row, lse_col)
        return None
    if keyed is None:
        return K.infonce_grad_scaled_inplace(S, off, lse_row, lse_col, theta)[1]
    return K.multipos_grad_scaled_inplace(S, *keyed, lse_row, lse_col, theta)[1]


class _InfoNCE(torch.autograd.Function):
    """loss = ( CE(S, diag) + CE(S^T, diag) ) / 2 with S = I_hat T_hat^T / tau over the GLOBAL batch.

    Data-parallel form: `_gather_normalised`, plus one all-gather each of the two [B] row log-sum-exps (the column statistics of
    the other block) and the scalar all-reduce of the reported loss.

    With `keys` (int64 [B], one per local pair; image i and text i share it) the targets are multi-positive: the positives of
    row i are the columns j of the global batch with k_j = k_i (n_i of them, i itself included), and
        loss = 1/(2 Bg) sum_i [ lse_row_i - 1/n_i sum_{j in P(i)} S_ij ]  +  the same over the columns,
        dL/dS_ij = ( softmax_row_ij + softmax_col_ij - 2 [k_i = k_j] / n_i ) / (2 Bg).
    n_i comes from the stats kernel (it counts against the global columns).  Because a key belongs to a PAIR, entry (i, j) matches
    exactly when (j, i) does, so the column count of a matching entry equals its row count (n_j = n_i): the column term needs no
    exchange of counts.  With all keys distinct this is the plain loss.

    With `log_scale` (theta = log(1/tau), a one-element fp32 device tensor, differentiable) the temperature is LEARNED
    (DESIGN.md §5.3): `temperature` is ignored, the logits GEMMs run with alpha = 1 and the *_scaled kernels form
    S = exp(theta) * C on the device, so nothing on the host depends on theta and nothing is read back.
        dL/dtheta = sum_ij dL/dS_ij * S_ij = 1/(2 Bg) sum_ij G_ij S_ij,
    for the plain and the keyed loss alike.  The gradient kernels leave exp(theta) * G in the block (the backward GEMMs keep the
    host alpha 0.5/Bg) and the partial sums of G o S; one single-block kernel folds them, times the upstream scalar, into
    theta's gradient.  Data-parallel: a rank's S1 block carries the complete G of its image rows, its S2 block the transpose's,
    so each rank adds (sum_S1 + sum_S2) G o S / (4 Bg) and the sum all-reduce of the flat gradient buffer completes it: no new
    collective.
    """

    @staticmethod
    def forward(ctx, img, txt, temperature, group, keys=None, log_scale=None):
        import torch.distributed as dist
        img, txt = img.detach().contiguous(), txt.detach().contiguous()
        shard = _shard(group)
        B, D = _check_pairs("infonce_loss", img, txt, shard[2])
        keys = _check_keys("infonce_loss", keys, B, img.device)
        theta = None if log_scale is None else _device_scalar("infonce_loss", log_scale, "log_scale", img.device)
        (im, tx), keys_all, off, Bg = _gather_normalised((img, txt), keys, group, shard)
        inv_tau = 1.0 if theta is not None else 1.0 / float(temperature)    # learnable: the kernels scale by exp(theta)
        S1, S2 = _logit_blocks(im, tx, inv_tau)
        loss = torch.zeros((), dtype=torch.float32, device=img.device)
        lse1, npos = _infonce_stats(S1, off, keys, keys_all, theta, loss, 0.5 / Bg)
        lse2, _ = _infonce_stats(S2, off, keys, keys_all, theta, loss, 0.5 / Bg)
        if shard[0]:
            dist.all_reduce(loss, group=group)
            lse1_all, lse2_all = _all_gather_rows(lse1, group), _all_gather_rows(lse2, group)   # [Bg] each (4 KiB per rank)
        else:
            lse1_all, lse2_all = lse1, lse2
        # theta is saved as the parameter itself, not a copy: the backward reads it again and writes into its `.grad`, and autograd's
        # version check refuses a theta that was updated in place between forward and backward
        ctx.save_for_backward(S1, S2, lse1, lse2, lse1_all, lse2_all, *im, *tx, log_scale)
        ctx.meta = (off, inv_tau, Bg)
        ctx.keys = None if keys is None else (keys, keys_all, npos)   # integer / count tensors: not autograd inputs or outputs
        return loss

    @staticmethod
    def backward(ctx, gloss):
        S1, S2, lse1, lse2, lse1_all, lse2_all, ih, inorm, ih_all, th, tnorm, th_all, log_scale = ctx.saved_tensors
        off, inv_tau, Bg = ctx.meta
        theta = None if log_scale is None else log_scale.detach()
        # dL/dS_ij = (softmax_row + softmax_col - 2*delta) / (2 Bg); fold 1/tau into alpha
        part1 = _infonce_grad(S1, off, ctx.keys, theta, lse1, lse2_all)
        part2 = _infonce_grad(S2, off, ctx.keys, theta, lse2, lse1_all)
        want_theta = theta is not None and ctx.needs_input_grad[5]
        di, dt, (dtheta,) = _backward_tail(S1, S2, (ih, inorm, ih_all), (th, tnorm, th_all), inv_tau * 0.5 / Bg, gloss,
                                           [(log_scale, part1, part2, 0.25 / Bg) if want_theta else None])
        return di, dt, None, None, None, dtheta


def infonce_loss(img_emb: torch.Tensor, txt_emb: torch.Tensor, temperature: float = 0.07, group=None,
                 keys: Optional[torch.Tensor] = None, log_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Symmetric InfoNCE over the global batch (all ranks of `group`, or the default group when initialised).

    `keys` (optional): int64 [B] on the embeddings' device, one key per local (image, text) pair; pairs of the global batch with
    equal keys are positives of each other (multi-positive targets, see `_InfoNCE`; `contrastive.keys_from_labels` /
    `keys_from_tokens` build them).  `keys=None` is the plain loss: one positive per row, the diagonal.

    `log_scale` (optional): theta = log(1/tau) as a 0-d or [1] fp32 tensor on the embeddings' device, differentiable (a parameter):
    the learnable temperature.  When given, `temperature` is ignored and the loss is computed with tau = exp(-theta) read on the
    device; `log_scale=None` is the fixed-temperature path, unchanged.  A leaf `log_scale` with a `.grad` of its own layout (a
    parameter of the flat optimiser) has its gradient added there directly; any other gets it through autograd.  It must not be
    updated in place between forward and backward (autograd's version check raises)."""
    return _InfoNCE.apply(img_emb, txt_emb, temperature, group, keys, log_scale)


class _SigmoidPairs(torch.autograd.Function):
    """Pairwise sigmoid loss (SigLIP) over the GLOBAL batch: with C = I_hat T_hat^T, t = exp(theta), x = t C + b,
        L = 1/Bg sum_ij softplus(-x_ij) [pair (i,j) positive] + softplus(x_ij) [negative],      g = dl/dx,
        dL/dC = t g / Bg,    dL/dtheta = 1/Bg sum g (x - b),    dL/db = 1/Bg sum g.
    Positives: j is i's pair, or, with `keys`, every pair of equal keys.  Nothing is normalised over the batch, so there is no
    log-sum-exp to exchange: the data-parallel step issues `_gather_normalised`'s collectives and the scalar all-reduce of the
    reported loss.  One fused kernel per block does forward and backward: S1 = local images x all texts carries the
    complete rows of g, so it also yields the loss and the d theta / d b partial sums; S2 = local texts x all images is the
    transpose coverage that the text gradient needs and yields no sums.  A key belongs to a pair, so S2 uses the same row and
    column keys.  Summed over the ranks the S1 blocks cover every (i, j) once: the sum all-reduce of the flat gradient buffer
    completes d theta and d b."""

    @staticmethod
    def forward(ctx, img, txt, log_scale, logit_bias, group, keys=None):
        import torch.distributed as dist
        img, txt = img.detach().contiguous(), txt.detach().contiguous()
        shard = _shard(group)
        B, D = _check_pairs("sigmoid_pairs_loss", img, txt, shard[2])
        keys = _check_keys("sigmoid_pairs_loss", keys, B, img.device)
        theta = _device_scalar("sigmoid_pairs_loss", log_scale, "log_scale", img.device)
        bias = _device_scalar("sigmoid_pairs_loss", logit_bias, "logit_bias", img.device)
        (im, tx), keys_all, off, Bg = _gather_normalised((img, txt), keys, group, shard)
        S1, S2 = _logit_blocks(im, tx, 1.0)
        # forward and backward of the head in one pass per block: S <- t * g
        _, parts = K.sigmoid_pairs_fwd_bwd_inplace(S1, off, keys, keys_all, theta, bias)
        K.sigmoid_pairs_fwd_bwd_inplace(S2, off, keys, keys_all, theta, bias, partials=False)
        loss = K.sigmoid_pairs_loss(parts[0], 1.0 / Bg)
        if shard[0]:
            dist.all_reduce(loss, group=group)
        # the two scalars are saved as the inputs themselves (their `.grad` is written in backward; autograd's version check
        # refuses one that was updated in place in between)
        ctx.save_for_backward(S1, S2, parts, *im, *tx, log_scale, logit_bias)
        ctx.Bg = Bg
        return loss

    @staticmethod
    def backward(ctx, gloss):
        S1, S2, parts, ih, inorm, ih_all, th, tnorm, th_all, log_scale, logit_bias = ctx.saved_tensors
        Bg = ctx.Bg
        scalars = [(p, plane, None, 1.0 / Bg) if ctx.needs_input_grad[2 + k] else None
                   for k, (p, plane) in enumerate(((log_scale, parts[1]), (logit_bias, parts[2])))]
        di, dt, (dtheta, dbias) = _backward_tail(S1, S2, (ih, inorm, ih_all), (th, tnorm, th_all), 1.0 / Bg, gloss, scalars)
        return di, dt, dtheta, dbias, None, None


def sigmoid_pairs_loss(img_emb: torch.Tensor, txt_emb: torch.Tensor, log_scale: torch.Tensor, logit_bias: torch.Tensor, group=None,
                       keys: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pairwise sigmoid loss over the global batch (all ranks of `group`, or the default group when initialised): every (image,
    report) pair is an independent binary problem on x = exp(log_scale) * cos + logit_bias, summed and divided by the global batch
    size (= `F.binary_cross_entropy_with_logits(x, positive, reduction="sum") / Bg`).

    `log_scale` (theta = log(1/tau)) and `logit_bias` are 0-d or [1] fp32 tensors on the embeddings' device, read on the device;
    each may be a parameter (its gradient is produced, written straight into a leaf's own `.grad` where it has one) or a plain
    constant.  `keys`: as in `infonce_loss`: pairs with equal keys are positives of each other; None: only a pair's own two
    halves are.  A row may have no positive at all.  The scalars must not be updated in place between forward and backward."""
    return _SigmoidPairs.apply(img_emb, txt_emb, log_scale, logit_bias, group, keys)


class _Distill(torch.autograd.Function):
    """Similarity distillation from a frozen teacher over the GLOBAL batch: with S = I_hat T_hat^T / tau_d of the
    student and St of the teacher's embeddings, p_i / q_j the softmax of row i / column j of S and pt / qt those of St,
        L_d = 1/(2 Bg) [ sum_i KL(pt_i || p_i) + sum_j KL(qt_j || q_j) ],      dL_d/dS_ij = (p_ij - pt_ij + q_ij - qt_ij) / (2 Bg).
    Returns (weight * L_d, L_d); only the first is differentiable, and only with respect to the student's embeddings.

    Data-parallel form: `_gather_normalised` with the teacher riding along (a [B, 4D] send buffer), ONE all-gather of the [B, 4]
    log-sum-exps (student rows, student columns, teacher rows, teacher columns) and the scalar all-reduce of the loss."""

    @staticmethod
    def forward(ctx, img, txt, img_t, txt_t, temperature, weight, group):
        import torch.distributed as dist
        img, txt = img.detach().contiguous(), txt.detach().contiguous()
        img_t, txt_t = img_t.detach().contiguous(), txt_t.detach().contiguous()
        shard = _shard(group)
        B, D = _check_pairs("distill_loss", img, txt, shard[2])
        if tuple(img_t.shape) != (B, D) or tuple(txt_t.shape) != (B, D):
            raise ValueError(f"distill_loss: the student's embeddings are {(B, D)} but the teacher's {tuple(img_t.shape)} and "
                             f"{tuple(txt_t.shape)}")
        (im, tx, im_t, tx_t), _, _, Bg = _gather_normalised((img, txt, img_t, txt_t), None, group, shard)
        inv_tau = 1.0 / float(temperature)
        S1, S2 = _logit_blocks(im, tx, inv_tau)
        T1, T2 = _logit_blocks(im_t, tx_t, inv_tau)                   # the teacher's two blocks
        loss = torch.zeros((), dtype=torch.float32, device=img.device)
        lse1, lt1, _ = K.distill_row_stats(S1, T1, loss_out=loss, loss_scale=0.5 / Bg, loss_accumulate=True)
        lse2, lt2, _ = K.distill_row_stats(S2, T2, loss_out=loss, loss_scale=0.5 / Bg, loss_accumulate=True)
        if shard[0]:
            dist.all_reduce(loss, group=group)
            lse_all = _all_gather_rows(torch.stack((lse1, lse2, lt1, lt2), dim=1), group).t().contiguous()    # [4, Bg]
            lse1_all, lse2_all, lt1_all, lt2_all = lse_all[0], lse_all[1], lse_all[2], lse_all[3]
        else:
            lse1_all, lse2_all, lt1_all, lt2_all = lse1, lse2, lt1, lt2
        ctx.save_for_backward(S1, S2, T1, T2, lse1, lse2, lt1, lt2, lse1_all, lse2_all, lt1_all, lt2_all, *im, *tx)
        ctx.alpha = float(weight) * inv_tau * 0.5 / Bg
        weighted = K.scale_mask(loss.reshape(1), alpha=float(weight)).reshape(())
        ctx.mark_non_differentiable(loss)
        return weighted, loss

    @staticmethod
    def backward(ctx, gloss, _gunweighted):
        (S1, S2, T1, T2, lse1, lse2, lt1, lt2, lse1_all, lse2_all, lt1_all, lt2_all, ih, inorm, ih_all, th, tnorm,
         th_all) = ctx.saved_tensors
        # column j of S1 is text j over all images: its log-sum-exp is row j's of the global S2, and the other way round
        K.distill_grad_inplace(S1, T1, lse1, lse2_all, lt1, lt2_all)
        K.distill_grad_inplace(S2, T2, lse2, lse1_all, lt2, lt1_all)
        di, dt, _ = _backward_tail(S1, S2, (ih, inorm, ih_all), (th, tnorm, th_all), ctx.alpha, gloss)
        return di, dt, None, None, None, None, None


def _distill_pair(img_emb, txt_emb, img_teacher, txt_teacher, temperature, weight=1.0, group=None):
    """(weight * L_d, L_d) of `distill_loss`; the second scalar carries no graph (the joint trainer reports it)"""
    for t, name in ((img_teacher, "img_teacher"), (txt_teacher, "txt_teacher")):
        if not isinstance(t, torch.Tensor) or t.requires_grad:
            raise ValueError(f"distill_loss: {name} requires grad; the teacher is a constant (detach it, or run it under no_grad)")
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"distill_loss: weight must be finite and >= 0, got {weight!r}")
    if not (float(temperature) > 0.0 and math.isfinite(float(temperature))):
        raise ValueError(f"distill_loss: the temperature must be positive and finite, got {temperature!r}")
    return _Distill.apply(img_emb, txt_emb, img_teacher, txt_teacher, temperature, weight, group)


def distill_loss(img_emb: torch.Tensor, txt_emb: torch.Tensor, img_teacher: torch.Tensor, txt_teacher: torch.Tensor,
                 temperature: float, weight: float = 1.0, group=None) -> torch.Tensor:
    """weight * L_d, the similarity-distribution distillation loss against a frozen teacher (see `_Distill`), over
    the global batch (all ranks of `group`, or the default group when initialised), as a device scalar.

    `img_emb` / `txt_emb` [B, D] are the student's unnormalised embeddings of this rank's rows and receive the gradient;
    `img_teacher` / `txt_teacher` [B, D] are the teacher's embeddings of the same rows, constants: one that requires grad is refused.
    `temperature` is the fixed distillation temperature tau_d of both logits blocks.  When the teacher's embeddings equal the
    student's bit for bit, the loss and the gradient are exactly zero."""
    return _distill_pair(img_emb, txt_emb, img_teacher, txt_teacher, temperature, weight, group)[0]


# --------------------------------------------------------------------------------------------------------------
# The masked-language-modelling head: HF BertOnlyMLMHead + cross-entropy on the selected tokens, with the
# vocabulary swept in chunks so that the [tokens, V] logits never exist.
# --------------------------------------------------------------------------------------------------------------
MLM_CHUNK_BYTES = 128 << 20


def mlm_vocab_chunks(vocab_size: int, rows: int, chunk_bytes: int = MLM_CHUNK_BYTES, planes: bool = False):
    """The (first column, columns, leading columns not counted) triples of one vocabulary sweep over `rows` logits rows with a
    workspace of at most `chunk_bytes` (split-bf16 mode keeps the fp32 logits AND their gradient planes: half the columns).  Chunks
    hold a multiple of 128 columns (at least 128, whatever the budget) and tile [0, V - V % 8); every GEMM of the sweep then has
    sizes and offsets that are multiples of 8.  The V % 8 columns left are taken by one more chunk of 8 columns, [V - 8, V), whose
    first 8 - V % 8 columns overlap the chunk before: they are not counted and get a zero gradient."""
    V = int(vocab_size)
    if V < 8:
        raise ValueError(f"mlm_loss: the vocabulary must hold at least 8 ids, got {V}")
    if int(chunk_bytes) < 1 or int(rows) < 1:
        raise ValueError(f"mlm_loss: chunk_bytes and the number of rows must be positive, got {chunk_bytes!r} and {rows!r}")
    vc = max(128, int(chunk_bytes) // (int(rows) * (8 if planes else 4)) // 128 * 128)
    V8 = V // 8 * 8
    chunks = [(v0, min(vc, V8 - v0), 0) for v0 in range(0, V8, vc)]
    if V8 != V:
        chunks.append((V - 8, 8, 8 - (V - V8)))
    return chunks


class _MLMLoss(torch.autograd.Function):
    """(weight * L, L, correct) with L = scale * sum over the kept selected tokens of -log softmax(logits)[original id], logits those of
    HF BertOnlyMLMHead (dense + erf-GELU + LayerNorm, decoder tied to the word embeddings + bias) on the selected rows of the last
    hidden state.  Only the first output is differentiable: with respect to the last hidden state and the six head parameters.

    Forward: gather -> transform -> for every vocabulary chunk (logits GEMM into the workspace, `mlm_xent_stats`) -> `mlm_xent_finish`.
    Backward: for every chunk the same logits GEMM again (the same bits), `mlm_xent_grad`, then the data gradient accumulated into
    d[cap, H], the chunk's rows of the decoder weight gradient and its slice of the decoder bias gradient; LayerNorm, GELU and dense
    backward; scatter into a zeroed gradient of the last hidden state.  Parameter gradients go through `GradSink`: a parameter of the
    flat optimiser gets them accumulated in place (the tied word embeddings receive the encoder's share later, in the same way)."""

    @staticmethod
    def forward(ctx, last, sel, tgt, stats, scale, weight, eps, chunk_bytes, wd, bd, gamma, beta, wdec, bdec):
        from . import _lib
        ctx.set_materialize_grads(False)
        pl = _lib.get_precision() == "split_bf16"
        H = last.shape[-1]
        flat = last.detach().reshape(-1, H).contiguous()
        cap = sel.shape[0]
        V = wdec.shape[0]
        if tuple(wd.shape) != (H, H) or wdec.shape[1] != H or bdec.numel() != V or tgt.shape[0] != cap:
            raise ValueError(f"mlm_loss: hidden size {H}, transform {tuple(wd.shape)}, decoder {tuple(wdec.shape)}, bias {tuple(bdec.shape)}, "
                             f"{cap} slots and {tgt.shape[0]} targets do not fit together")
        p = [t.detach() for t in (wd, bd, gamma, beta, wdec, bdec)]
        wd_w, wdec_w = (K.split_planes(p[0]), K.split_planes(p[4])) if pl else (p[0], p[4])
        lin = K.linear_fwd_pl if pl else K.linear_fwd
        x = K.mlm_gather_rows(flat, sel, stats, out_planes=pl)
        h1_pre = torch.empty(cap, H, dtype=torch.float32, device=flat.device)
        h1 = lin(x, wd_w, p[1], act=K.ACT_GELU, preact_out=h1_pre)
        h2, xhat, rstd = K.residual_ln_fwd(h1, None, p[2], p[3], eps, out_planes=pl)
        chunks = mlm_vocab_chunks(V, cap, chunk_bytes, pl)
        ws = torch.empty(cap, max(c for _, c, _ in chunks), dtype=torch.float32, device=flat.device)
        state, tl = K.mlm_xent_state(cap, flat.device)
        for k, (v0, cols, skip) in enumerate(chunks):
            S = lin(h2, _rows(wdec_w, v0, cols), None, out=ws[:, :cols])
            K.mlm_xent_stats(S, v0, skip, p[5], tgt, stats, state, tl, first=k == 0)
        lse, loss, correct = K.mlm_xent_finish(state, tl, tgt, stats, scale)
        ctx.save_for_backward(sel, tgt, stats, scale, h1_pre, xhat, rstd, lse, *p)
        ctx.ops = (x, h2, wd_w, wdec_w)            # GEMM operands in the storage format of the mode (Planes are no autograd tensors)
        ctx.meta = (pl, float(weight), chunks, tuple(last.shape))
        ctx.params = (wd, bd, gamma, beta, wdec, bdec)
        weighted = K.scale_mask(loss.reshape(1), alpha=float(weight)).reshape(())
        ctx.mark_non_differentiable(loss, correct)
        return weighted, loss, correct

    @staticmethod
    def backward(ctx, gloss, _gl, _gc):
        sel, tgt, stats, scale, h1_pre, xhat, rstd, lse, wd, bd, gamma, beta, wdec, bdec = ctx.saved_tensors
        x, h2, wd_w, wdec_w = ctx.ops
        pl, weight, chunks, shape = ctx.meta
        ctx.ops = None
        cap, H = h1_pre.shape
        dev = h1_pre.device
        lin, dgrad, wgrad = ((K.linear_fwd_pl, K.linear_bwd_data_pl, K.linear_bwd_weight_pl) if pl else
                             (K.linear_fwd, K.linear_bwd_data, K.linear_bwd_weight))
        sink = GradSink(ctx.params, ctx.needs_input_grad[8:])
        up = gloss.reshape(()).contiguous()
        width = max(c for _, c, _ in chunks)
        ws = torch.empty(cap, width, dtype=torch.float32, device=dev)
        gpl = K.Planes.empty(cap, width, device=dev) if pl else None
        d = torch.empty(cap, H, dtype=torch.float32, device=dev)
        dwdec, _ = sink.dst(4, zero=True)           # both accumulate: the chunks write row ranges, the last one overlapping
        dbdec, _ = sink.dst(5, zero=True)
        for k, (v0, cols, skip) in enumerate(chunks):
            S = lin(h2, _rows(wdec_w, v0, cols), None, out=ws[:, :cols])                 # the forward's call: the same bits
            G = K.mlm_xent_grad(S, v0, skip, bdec, tgt, stats, lse, up, scale, alpha=weight,
                                out=K.Planes(gpl.t[:, :, :cols]) if pl else None)
            dgrad(G, _rows(wdec_w, v0, cols), out=d, accumulate=k > 0)
            wgrad(G, h2, dwdec[v0:v0 + cols], accumulate=True)
            K.colsum(G, dbdec[v0:v0 + cols], accumulate=True)
        (dg, db), acc = sink.dst_group(2, 3)
        dh1 = K.residual_ln_bwd(d, xhat, rstd, gamma, dg, db, accumulate=acc)
        dpre = K.gelu_bwd(dh1, h1_pre)
        dpo = K.split_planes(dpre) if pl else dpre
        g, acc = sink.dst(0)
        wgrad(dpo, x, g, accumulate=acc)
        g, acc = sink.dst(1)
        K.colsum(dpre, g, accumulate=acc)
        dlast = None
        if ctx.needs_input_grad[0]:
            T = 1
            for s in shape[:-1]:
                T *= s
            dlast = K.mlm_scatter_rows(dgrad(dpo, wd_w), sel, stats, T).view(shape)
        return (dlast, None, None, None, None, None, None, None) + sink.result()


def _rows(w, v0: int, n: int):
    """rows v0 .. v0 + n of a weight matrix in either storage format"""
    return w.rows(slice(v0, v0 + n)) if isinstance(w, K.Planes) else w[v0:v0 + n]


def _mlm_triple(last_hidden, sel, tgt, stats, model_params, scale, chunk_bytes=MLM_CHUNK_BYTES, weight=1.0, eps=1e-12):
    """(weight * L, L, correct) of `mlm_loss`; the last two carry no graph (the joint trainer reports them)"""
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"mlm_loss: weight must be finite and >= 0, got {weight!r}")
    params = tuple(model_params)
    if len(params) != 6:
        raise ValueError("mlm_loss: model_params are (transform.dense.weight, transform.dense.bias, transform.LayerNorm.weight, "
                         f"transform.LayerNorm.bias, decoder.weight, decoder bias); got {len(params)} tensors")
    if last_hidden.dim() not in (2, 3):
        raise ValueError(f"mlm_loss: the last hidden state must be [T, H] or [N, L, H], got {tuple(last_hidden.shape)}")
    scale = _device_scalar("mlm_loss", scale, "scale", last_hidden.device)
    return _MLMLoss.apply(last_hidden, sel, tgt, stats, scale, weight, float(eps), int(chunk_bytes), *params)


def mlm_loss(last_hidden: torch.Tensor, sel: torch.Tensor, tgt: torch.Tensor, stats: torch.Tensor, model_params, scale: torch.Tensor,
             chunk_bytes: int = MLM_CHUNK_BYTES, weight: float = 1.0, eps: float = 1e-12) -> torch.Tensor:
    """weight * scale * sum over the kept selected tokens of -log softmax(MLM logits)[original id] (see `_MLMLoss`) as
    a device scalar: HF `BertForMaskedLM.forward(labels=)`'s loss when `scale` holds 1 / (number of selected tokens).

    `last_hidden` [N, L, H] (or [T, H]) is the encoder's last hidden state ON THE MASKED IDS and receives a gradient; `sel` / `tgt` /
    `stats` are the compact list of `kernels.mlm_mask_tokens` (int32 token indices and original ids in `cap` slots, stats[0] = the
    slots that count, read on the device); `model_params` = the head's six parameters, `cls.predictions.transform.dense.weight /
    .bias`, `.transform.LayerNorm.weight / .bias`, `.decoder.weight` (tied to the word embeddings) and the decoder bias; `scale` a
    0-d or [1] fp32 device tensor (the data-parallel step puts 1 / max(selected tokens of the global batch, 1) there).  The
    vocabulary runs in chunks whose logits workspace follows `chunk_bytes`, never the vocabulary size.  With no slot counting, the
    loss and every gradient are exactly zero.  No atomics: two runs give the same bits."""
    return _mlm_triple(last_hidden, sel, tgt, stats, model_params, scale, chunk_bytes, weight, eps)[0]


@torch.no_grad()
def similarity_logits(img_emb: torch.Tensor, txt_emb: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """normalize(img) @ normalize(txt).T / tau — the zero-shot score matrix (trash/lower_bound_mcs.py:79-117)."""
    ih, _ = K.l2norm_fwd(img_emb.contiguous())
    th, _ = K.l2norm_fwd(txt_emb.contiguous())
    out = torch.empty(ih.shape[0], th.shape[0], dtype=torch.float32, device=ih.device)
    return K.gemm(ih, th, out, ih.shape[0], th.shape[0], ih.shape[1], False, True, alpha=1.0 / temperature)


@torch.no_grad()
def retrieval_ranks(queries: torch.Tensor, gallery: torch.Tensor, keys: Optional[torch.Tensor] = None, group=None,
                    normalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Ranks of this rank's `queries` [B,D] against the WHOLE gallery (include/cxrk.h, "retrieval_ranks"): returns
    (pos fp32 [B], greater int32 [B], ties int32 [B]) — the best positive score of each query and the number of non-positive
    gallery rows that beat / equal it (-1 / -1 for a row that met a NaN).  The [B, M] score block is never formed.

    `gallery` [B,D] holds this rank's rows, paired with the queries row by row.  Without `keys` the one positive of query i is
    gallery row i; with `keys` (int64 [B], one per local pair) every gallery row of the global set with the query's key is.
    With a process `group`, the gallery rows (and the keys) of all ranks are gathered, rank-major, and the positives of this
    rank's queries sit at `rank * B` (the shard convention of `infonce_loss`): one [B,D] and at most one [B] all-gather.
    `normalize`: L2-normalise both sides first (cosine scores).  No autograd."""
    q, g = queries.detach().contiguous(), gallery.detach().contiguous()
    if q.dim() != 2 or tuple(g.shape) != tuple(q.shape):
        raise ValueError(f"retrieval_ranks: queries are {tuple(q.shape)} but this rank's gallery rows {tuple(g.shape)} "
                         f"(they are paired row by row)")
    B = q.shape[0]
    if keys is not None:
        if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or tuple(keys.shape) != (B,) or keys.device != q.device:
            raise ValueError(f"retrieval_ranks: keys must be an int64 [{B}] tensor on {q.device}, got "
                             f"{getattr(keys, 'dtype', type(keys).__name__)} {tuple(getattr(keys, 'shape', ()))}")
        keys = keys.detach().contiguous()
    if normalize:
        q, g = K.l2norm_fwd(q)[0], K.l2norm_fwd(g)[0]
    off, g_all, keys_all = 0, g, keys
    if group is not None:
        import torch.distributed as dist
        off = dist.get_rank(group) * B
        g_all = _all_gather_rows(g, group)
        keys_all = _all_gather_rows(keys, group) if keys is not None else None
    if keys is None:
        return K.retrieval_ranks(q, g_all, diag_off=off)
    return K.retrieval_ranks(q, g_all, keys_q=keys, keys_g=keys_all)


@torch.no_grad()
def topk_neighbours(queries: torch.Tensor, gallery: torch.Tensor, k: int, normalize: bool = True, exclude_self: bool = False,
                    group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The `k` nearest gallery rows of this rank's `queries` [B,D] (include/cxrk.h, "topk_neighbours"): returns
    (score fp32 [B,k], index int32 [B,k]), each row sorted by score descending (a NaN first), then index ascending, padded with
    index -1 / score -inf when the gallery has fewer than k candidates.  The [B, M] score block is never formed.

    `gallery` [Bg,D] holds this rank's rows.  With a process `group` the gallery rows of all ranks are gathered, rank-major, and the
    indices refer to the gathered gallery: one [Bg,D] all-gather and nothing else.  `exclude_self` drops gallery row
    `rank * B + i` from query i's candidates (leave-one-out of a set queried against itself); it needs `queries` and `gallery`
    paired row by row as in `retrieval_ranks`.  `normalize`: L2-normalise both sides first (cosine scores).  No autograd."""
    q, g = queries.detach().contiguous(), gallery.detach().contiguous()
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError(f"topk_neighbours: queries are {tuple(q.shape)} but the gallery rows {tuple(g.shape)}")
    if exclude_self and tuple(g.shape) != tuple(q.shape):
        raise ValueError(f"topk_neighbours: exclude_self needs queries and gallery paired row by row, got {tuple(q.shape)} and "
                         f"{tuple(g.shape)}")
    if normalize:
        q, g = K.l2norm_fwd(q)[0], K.l2norm_fwd(g)[0]
    off = 0
    if group is not None:
        import torch.distributed as dist
        off = dist.get_rank(group) * q.shape[0]
        g = _all_gather_rows(g, group)
    return K.topk_neighbours(q, g, k, exclude_off=off if exclude_self else -1)


@torch.no_grad()
def augment_images(images: torch.Tensor, spec, seed: int, counter: int, row_offset: int = 0, cpad: int = 4) -> torch.Tensor:
    """Random affine + brightness / contrast augmentation on the device (include/cxrk.h, "augment"):
    images [N, 3 | 1, H, W] -> fp32 NHWC [N, Ho, Wo, cpad] (three channels, the padding zero), the tensor the ResNet stem reads.
    Image i of the call is drawn for (seed, counter, row_offset + i) and for nothing else, so a batch cut anywhere gives the same
    pixels.  No input gradient: `images` must not require grad."""
    params = K.augment_params(images, spec, seed, counter, row_offset)
    return K.augment_nhwc(images, cpad, params, spec.size_for(images.shape[2], images.shape[3]), spec.clamp01)
