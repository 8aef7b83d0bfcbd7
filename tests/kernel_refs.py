"""Reference constructions shared by the kernel test modules (plain torch on the CPU, in the dtype the caller asks for)."""
import math

import torch


def rnd(*shape, seed=0, scale=1.0):
    """the seeded inputs of tests/test_kernels_gpu.py (same generator rule, so the same values)"""
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_case(rows, H):
    """(dy, xhat, rstd, gamma, dx_add) of a LayerNorm backward: xhat normalised per row as the forward leaves it"""
    xhat = rnd(rows, H, seed=1)
    xhat = (xhat - xhat.mean(1, keepdim=True)) / xhat.std(1, unbiased=False, keepdim=True)
    return rnd(rows, H), xhat, 0.5 + rnd(rows, seed=2).abs(), 1 + 0.1 * rnd(H, seed=3), rnd(rows, H, seed=4)


def ln_bwd_ref(dy, xhat, rstd, gamma):
    """(dx, dgamma, dbeta) of y = xhat gamma + beta, xhat = (x - mean) rstd, in the dtype of the operands"""
    gdy = dy * gamma
    dx = rstd[:, None] * (gdy - gdy.mean(1, keepdim=True) - xhat * (gdy * xhat).mean(1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def ln_fwd_ref(s, gamma, beta, eps):
    """(y, xhat, rstd) of LayerNorm over the last dimension of `s` (biased variance), in the dtype of the operands"""
    mean = s.mean(1, keepdim=True)
    var = ((s - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (s - mean) * rstd
    return xhat * gamma + beta, xhat, rstd[:, 0]


# ------------------------------------------------------------------------------------------------ attention
def attention_mask(B, L, ragged):
    """key mask [B, L]: ragged = sequence i loses its last 3 i + 2 keys (at least one stays); "empty" = sequence 1 has none"""
    mask = torch.ones(B, L, dtype=torch.int64)
    if ragged:
        for i in range(B):
            mask[i, max(1, L - 3 * i - 2):] = 0
    if ragged == "empty":
        mask[1] = 0     # a padding-only row of a sharded batch: HF (additive finfo.min) gives a uniform, finite attention row
    return mask


def attention_reference(B, L, nH, dH, ragged, dtype=torch.float32):
    """Multi-head attention on the fused [B L, 3 nH dH] projection, HuggingFace semantics (additive finfo(float32).min key mask),
    through autograd in `dtype` from the float32 inputs as given.  (The padding-only row of "empty" is uniform only where the score
    is absorbed by the mask constant, i.e. in float32: that mask is for the float32 reference.)
    Returns (qkv fp32, mask, cotangent fp32, ctx reference, d qkv reference)."""
    qkv = rnd(B * L, 3 * nH * dH, scale=0.7)
    mask = attention_mask(B, L, ragged)
    x = qkv.clone().to(dtype).requires_grad_(True)
    q, k, v = x.view(B, L, 3, nH, dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(dH) + (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(torch.float32).min
    ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, nH * dH)
    gc = rnd(B * L, nH * dH, seed=2)
    ctx.backward(gc.to(dtype))
    return qkv, mask, gc, ctx.detach(), x.grad
