"""TEST-ONLY: tests/cpu_kernels_multipos.py plus torch emulations of the learnable-temperature wrappers (`kernels.*_scaled*`,
`kernels.logit_scale_grad`, `kernels.clamp_inplace`), so that the data-parallel protocol of `functional._InfoNCE(log_scale=)` runs on
gloo / CPU.  Never imported by the package."""
import torch

import cpu_kernels_multipos as _mp
from cpu_kernels_multipos import *  # noqa: F401,F403


def _partials(G, S):
    nchunk = (S.shape[1] + 1023) // 1024
    gs = G * S
    return torch.stack([gs[:, k * 1024:(k + 1) * 1024].sum(1) for k in range(nchunk)], 1).reshape(-1).contiguous()


def infonce_row_lse_scaled(C, diag_off, log_scale, loss_out=None, loss_scale=0.0, loss_accumulate=False):
    return _mp.infonce_row_lse(torch.exp(log_scale.reshape(())) * C, diag_off, loss_out, loss_scale, loss_accumulate)


def infonce_grad_scaled_inplace(C, diag_off, lse_row, lse_col, log_scale):
    s = torch.exp(log_scale.reshape(()))
    S = s * C
    G = _mp.infonce_grad_inplace(S.clone(), diag_off, lse_row, lse_col)
    C.copy_(s * G)
    return C, _partials(G, S)


def multipos_row_stats_scaled(C, keys_row, keys_col, log_scale, loss_out=None, loss_scale=0.0, loss_accumulate=False):
    return _mp.multipos_row_stats(torch.exp(log_scale.reshape(())) * C, keys_row, keys_col, loss_out, loss_scale, loss_accumulate)


def multipos_grad_scaled_inplace(C, keys_row, keys_col, n_row, lse_row, lse_col, log_scale):
    s = torch.exp(log_scale.reshape(()))
    S = s * C
    G = _mp.multipos_grad_inplace(S.clone(), keys_row, keys_col, n_row, lse_row, lse_col)
    C.copy_(s * G)
    return C, _partials(G, S)


def logit_scale_grad(part1, part2, upstream, scale, out, accumulate):
    v = upstream.reshape(()) * scale * (part1.sum() + (part2.sum() if part2 is not None else 0.0))
    with torch.no_grad():
        out.copy_((out + v if accumulate else v).reshape(out.shape))
    return out


def clamp_inplace(x, lo, hi):
    with torch.no_grad():
        x.copy_(torch.where(x < lo, torch.full_like(x, lo), torch.where(x > hi, torch.full_like(x, hi), x)))
    return x


def sgd(p, g, lr, weight_decay=0.0, grad_scale=1.0):
    with torch.no_grad():
        p.sub_(lr * (g * grad_scale + weight_decay * p))
