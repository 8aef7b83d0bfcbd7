"""TEST-ONLY: tests/cpu_kernels_adamw.py plus torch emulations of `kernels.fisher_accumulate`, `kernels.ewc_consolidate`,
`kernels.ewc_penalty` and `kernels.sgd`, so that `optim.EWC` runs on gloo / CPU.  fp32, the kernels' formulas and the penalty's
partition (`cpu_kernels_adamw.by_block`; include/cxrk.h, "ewc_penalty"); the order of the additions inside a block is torch's.  Never
imported by the package."""
import torch

from cpu_kernels_adamw import *  # noqa: F401,F403
from cpu_kernels_adamw import by_block, grad_sqnorm_nparts, partials_out

_BAD = "bad argument / shape / alignment (cxrk code -1)"


def _f(x):
    return torch.tensor(x, dtype=torch.float32)


def fisher_accumulate(acc, g, w=1.0):
    if acc.numel() == 0 or g.numel() != acc.numel():
        raise ValueError("cxrk_fisher_accumulate: " + _BAD)
    with torch.no_grad():
        acc.add_(_f(w) * (g * g))


def ewc_consolidate(F, acc, anchor, p, gamma=1.0, scale=1.0):
    if anchor.numel() == 0 or p.numel() != anchor.numel() or (F is None) != (acc is None):
        raise ValueError("cxrk_ewc_consolidate: " + _BAD)
    with torch.no_grad():
        anchor.copy_(p)
        if F is not None:
            F.mul_(_f(gamma)).add_(_f(scale) * acc)


def ewc_penalty_nparts(n: int) -> int:
    return grad_sqnorm_nparts(n)


def ewc_penalty(g, p, anchor, F, strength, out=None):
    n = g.numel()
    if n == 0 or p.numel() != n or anchor.numel() != n or (F is not None and F.numel() != n):
        raise ValueError("cxrk_ewc_penalty: " + _BAD)
    nparts = ewc_penalty_nparts(n)
    if out is not None and out.numel() < nparts:
        raise RuntimeError("cxrk_ewc_penalty: workspace too small (cxrk code -2)")
    with torch.no_grad():
        d = p - anchor
        t = d if F is None else F * d
        g.add_(_f(strength) * t)
        return partials_out(by_block(t * d, nparts), out)


def sgd(p, g, lr, weight_decay=0.0, grad_scale=1.0):
    with torch.no_grad():
        gg = g * _f(grad_scale)
        if weight_decay != 0:
            gg = gg + _f(weight_decay) * p
        p.sub_(_f(lr) * gg)
