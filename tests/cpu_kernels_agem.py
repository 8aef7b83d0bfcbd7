"""TEST-ONLY: tests/cpu_kernels_ewc.py plus torch emulations of `kernels.agem_dots` and `kernels.agem_project`, so that `optim.AGEM`
runs on gloo / CPU.  fp32, the kernels' formulas and partition (`cpu_kernels_adamw.by_block`; include/cxrk.h, "agem_dots"); the order
of the additions inside a block is torch's.  Never imported by the package."""
import torch

from cpu_kernels_ewc import *  # noqa: F401,F403
from cpu_kernels_ewc import by_block, grad_sqnorm_nparts, partials_out

_BAD = "bad argument / shape / alignment (cxrk code -1)"


def agem_dots_nparts(n: int) -> int:
    return grad_sqnorm_nparts(n)


def agem_dots(g, gref, out=None):
    n = g.numel()
    if n == 0 or gref.numel() != n:
        raise ValueError("cxrk_agem_dots: " + _BAD)
    nparts = agem_dots_nparts(n)
    if out is not None and out.numel() < 2 * nparts:
        raise RuntimeError("cxrk_agem_dots: workspace too small (cxrk code -2)")
    with torch.no_grad():
        return partials_out(torch.cat([by_block(g * gref, nparts), by_block(gref * gref, nparts)]), out)


def agem_project(g, gref, partials, stats):
    n = g.numel()
    nparts = agem_dots_nparts(n)
    if n == 0 or gref.numel() != n or partials.numel() != 2 * nparts or stats.numel() != 4:
        raise ValueError("cxrk_agem_project: " + _BAD)
    with torch.no_grad():
        dot, rr = partials[:nparts].sum(), partials[nparts:].sum()
        project = not bool(dot >= 0)
        coef = dot / rr if project else torch.zeros(())
        stats[0], stats[1], stats[2] = dot, rr, coef
        if project:
            stats[3] += 1.0
            g.sub_(coef * gref)
