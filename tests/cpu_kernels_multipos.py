"""TEST-ONLY: tests/cpu_kernels.py plus torch emulations of the two multi-positive InfoNCE wrappers (`kernels.multipos_row_stats`,
`kernels.multipos_grad_inplace`), so that the keyed data-parallel protocol of `functional._InfoNCE` runs on gloo / CPU.
Never imported by the package."""
import torch

from cpu_kernels import *  # noqa: F401,F403


def multipos_row_stats(S, keys_row, keys_col, loss_out=None, loss_scale=0.0, loss_accumulate=False):
    eq = keys_row[:, None] == keys_col[None, :]
    npos = eq.sum(1).to(torch.float32)
    lse = torch.logsumexp(S, dim=1)
    posmean = (S * eq).sum(1) / npos.clamp_min(1.0)
    if loss_out is not None:
        v = (lse - posmean).sum() * loss_scale
        loss_out.copy_(loss_out + v if loss_accumulate else v)
    return lse, posmean, npos


def multipos_grad_inplace(S, keys_row, keys_col, n_row, lse_row, lse_col):
    eq = (keys_row[:, None] == keys_col[None, :]).to(S.dtype)
    S.copy_(torch.exp(S - lse_row[:, None]) + torch.exp(S - lse_col[None, :]) - 2.0 * eq / n_row[:, None])
    return S
