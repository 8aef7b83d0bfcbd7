"""TEST-ONLY float64 restatement of the clipped, masked AdamW step and the learning-rate schedule: the global
gradient norm, `torch.nn.utils.clip_grad_norm_`'s coefficient, `torch.optim.AdamW`'s update with a per-element decay mask, and the
closed form of `optim.LRSchedule`.  tests/test_adamw_host.py pins it to torch; the GPU tests compare the kernels with it."""
import math

import numpy as np
import torch


def by_block(terms: np.ndarray, nparts: int) -> np.ndarray:
    """float64 sums of per-element terms over the partition of the flat reductions (grad_sqnorm, ewc_penalty, agem_dots): group i of
    four elements belongs to block (i mod (nparts * 256)) div 256; the n mod 4 tail to block 0"""
    n4 = terms.size // 4
    out = np.zeros(nparts, dtype=np.float64)
    np.add.at(out, (np.arange(n4) % (nparts * 256)) // 256, terms[:4 * n4].reshape(n4, 4).sum(1))
    out[0] += terms[4 * n4:].sum()
    return out


def grad_norm(g: torch.Tensor, grad_scale: float = 1.0) -> float:
    """|grad_scale| * ||g||_2 in float64"""
    return abs(float(grad_scale)) * math.sqrt(float((g.double() ** 2).sum()))


def clip_coef(norm: float, max_norm) -> float:
    """clip_grad_norm_: min(max_norm / (norm + 1e-6), 1), a NaN staying a NaN; None or <= 0 -> 1 (no clipping)"""
    if max_norm is None or not max_norm > 0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c != c or c < 1.0) else 1.0


def expand_mask(mask_bytes: torch.Tensor, n: int) -> torch.Tensor:
    """uint8 [ceil(n / 4)], one byte per aligned group of four elements -> bool [n]"""
    return mask_bytes.bool().repeat_interleave(4)[:n]


def adamw_step(p, g, m, v, decay, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=None):
    """One step in float64 -> (p, m, v, norm, coef).  `decay`: bool [n] (None: every element decays).  The order is AdamW's:
    clip, decay the parameter, update the moments, move the parameter."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    norm = grad_norm(g, grad_scale)
    coef = clip_coef(norm, max_norm)
    gg = g * (float(grad_scale) * coef)
    if weight_decay != 0:
        dec = torch.ones_like(p, dtype=torch.bool) if decay is None else decay
        p = torch.where(dec, p * (1.0 - lr * weight_decay), p)
    m = m + (gg - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * gg * gg
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v, norm, coef


def lr_at(step, base_lr, warmup_steps=0, total_steps=None, decay="constant", min_lr_ratio=0.0) -> float:
    """the schedule's closed form; steps count from 1"""
    if step <= warmup_steps:
        return base_lr * step / warmup_steps
    if decay == "constant":
        return base_lr
    t = min(1.0, max(0.0, (step - warmup_steps) / max(1, total_steps - warmup_steps)))
    f = {"linear": 1.0 - t, "cosine": 0.5 * (1.0 + math.cos(math.pi * t))}[decay]
    return base_lr * (min_lr_ratio + (1.0 - min_lr_ratio) * f)


# ---- the error bound of the norm kernel -------------------------------------------------------------------------------------
U = 2.0 ** -24          # unit roundoff of fp32


def sqnorm_depth(n: int, nparts: int) -> int:
    """The longest chain of fp32 additions a term g[i]^2 passes through on its way into a partial sum: nparts blocks of 256 threads,
    a thread takes every (nparts * 256)-th group of four elements, round-robin over 4 accumulators (4 fused multiply-adds per group:
    one rounding each), thread 0 of block 0 also the n % 4 tail; then 2 levels to fold the accumulators, 6 levels of the 64-lane
    butterfly and a sequential sum over the block's 4 waves."""
    groups_per_thread = -(-(n // 4) // (nparts * 256)) if n >= 4 else 0
    per_acc = 4 * -(-groups_per_thread // 4)
    return per_acc + n % 4 + 2 + 6 + 4


def sqnorm_rtol(n: int, nparts: int, extra_levels: int = 0) -> float:
    """Relative error bound of a sum of non-negative fp32 terms through k additions: (1 + u)^k - 1 <= k u / (1 - k u) (Higham, gamma_k)"""
    k = sqnorm_depth(n, nparts) + extra_levels
    return k * U / (1.0 - k * U)


def norm_rtol(n: int, nparts: int) -> float:
    """The norm adamw_clipped reports: the partials are summed again (<= 4 per thread, 6 butterfly levels, 4 waves), the square root
    halves the relative error of the sum and rounds once, the product with |grad_scale| rounds once."""
    return 0.5 * sqnorm_rtol(n, nparts, extra_levels=-(-nparts // 256) + 6 + 4) + 2 * U
