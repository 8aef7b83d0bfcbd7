"""TEST-ONLY: tests/cpu_kernels_sigmoid.py plus torch emulations of `kernels.grad_sqnorm` and `kernels.adamw_clipped`, so that
`optim.AdamW` runs on gloo / CPU.  fp32, the kernel's partition (block b holds the groups of four i with (i mod (nparts * 256)) div
256 == b, the n mod 4 tail goes to block 0) and the kernel's formulas (include/cxrk.h, "grad_sqnorm" / "adamw_clipped"); the order of
the additions inside a block is torch's.  Never imported by the package."""
import math

import torch

from cpu_kernels_sigmoid import *  # noqa: F401,F403


def grad_sqnorm_nparts(n: int) -> int:
    return min(1024, max(1, -(-(n // 4) // 1024)))


def by_block(terms, nparts):
    """fp32 sums of per-element terms over the partition of the flat reductions (the module's docstring)"""
    n4 = terms.numel() // 4
    part = torch.zeros(nparts, dtype=torch.float32)
    if n4:
        block = (torch.arange(n4) % (nparts * 256)) // 256
        part.index_add_(0, block, terms[:4 * n4].view(n4, 4).sum(1))
    part[0] += terms[4 * n4:].sum()
    return part


def partials_out(part, out):
    """the partial sums where the kernel leaves them: at the front of `out` when given"""
    if out is None:
        return part
    out[:part.numel()].copy_(part)
    return out[:part.numel()]


def grad_sqnorm(g, out=None):
    nparts = grad_sqnorm_nparts(g.numel())
    if out is not None and out.numel() < nparts:
        raise RuntimeError("cxrk_grad_sqnorm: workspace too small (cxrk code -2)")
    return partials_out(by_block(g.detach().float() ** 2, nparts), out)


def adamw_clipped(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=0.0, decay_mask=None, partials=None,
                  stats=None):
    if step < 1 or p.numel() == 0 or (partials is None and max_norm > 0):
        raise ValueError("cxrk_adamw_clipped: bad argument / shape / alignment (cxrk code -1)")
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    n = p.numel()
    norm, coef = f(0.0), f(1.0)
    if partials is not None:
        norm = f(abs(grad_scale)) * partials.sum().sqrt()
        if max_norm > 0:
            c = f(max_norm) / (norm + f(1e-6))
            coef = c if bool(c != c) or bool(c < 1) else f(1.0)
    if stats is not None:
        stats[0], stats[1] = norm, coef
    with torch.no_grad():
        gg = g * (f(grad_scale) * coef)
        if weight_decay != 0:
            dec = torch.ones(n, dtype=torch.bool) if decay_mask is None else decay_mask.bool().repeat_interleave(4)[:n]
            p.copy_(torch.where(dec, p * f(1.0 - float(f(lr)) * float(f(weight_decay))), p))
        m.add_((gg - m) * (1.0 - f(beta1)))
        v.mul_(f(beta2)).add_((1.0 - f(beta2)) * gg * gg)
        bc1, bc2s = f(1.0 - beta1 ** step), f(math.sqrt(1.0 - beta2 ** step))
        p.sub_((f(lr) / bc1) * (m / (v.sqrt() / bc2s + f(eps))))
