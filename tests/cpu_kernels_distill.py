"""TEST-ONLY: tests/cpu_kernels_sigmoid.py plus torch emulations of the distillation wrappers (`kernels.distill_row_stats`,
`kernels.distill_grad_inplace`), so that the data-parallel protocol of `functional._Distill` runs on gloo / CPU.  The formulas are the
kernel's (include/cxrk.h, "distill").  Never imported by the package."""
import torch

from cpu_kernels_sigmoid import *  # noqa: F401,F403


def distill_row_stats(S, St, loss_out=None, loss_scale=0.0, loss_accumulate=False):
    lse, lse_t = torch.logsumexp(S, dim=1), torch.logsumexp(St, dim=1)
    kl = (torch.exp(St - lse_t[:, None]) * (St - S)).sum(1) + (lse - lse_t)
    if loss_out is not None:
        v = kl.sum() * loss_scale
        with torch.no_grad():
            loss_out.copy_(loss_out + v if loss_accumulate else v)
    return lse, lse_t, kl


def distill_grad_inplace(S, St, lse_row, lse_col, lse_t_row, lse_t_col):
    g = ((torch.exp(S - lse_row[:, None]) - torch.exp(St - lse_t_row[:, None]))
         + (torch.exp(S - lse_col[None, :]) - torch.exp(St - lse_t_col[None, :])))
    S.copy_(g)
    return S
