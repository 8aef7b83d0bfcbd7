"""TEST-ONLY: tests/cpu_kernels_logit_scale.py plus torch emulations of the pairwise-sigmoid wrappers
(`kernels.sigmoid_pairs_fwd_bwd_inplace`, `kernels.sigmoid_pairs_loss`), so that the data-parallel protocol of
`functional._SigmoidPairs` runs on gloo / CPU.  The formulas are the kernel's (include/cxrk.h, "sigmoid_pairs").  Never imported by
the package."""
import torch

from cpu_kernels_logit_scale import *  # noqa: F401,F403


def _chunks(v):
    nchunk = (v.shape[1] + 1023) // 1024
    return torch.stack([v[:, k * 1024:(k + 1) * 1024].sum(1) for k in range(nchunk)], 1).reshape(-1)


def sigmoid_pairs_fwd_bwd_inplace(C, diag_off, keys_row, keys_col, log_scale, bias, partials=True):
    if (keys_row is None) != (keys_col is None):
        raise ValueError("sigmoid_pairs: keys_row and keys_col go together (both or neither)")
    rows, cols = C.shape
    t, b = torch.exp(log_scale.detach().reshape(())), bias.detach().reshape(())
    if keys_row is None:
        pos = torch.arange(cols)[None, :] == (torch.arange(rows) + diag_off)[:, None]
    else:
        pos = keys_row[:, None] == keys_col[None, :]
    x = t * C + b
    e = torch.exp(-x.abs())
    r = 1.0 / (1.0 + e)
    er = e * r
    g = torch.where(pos, -torch.where(x >= 0, er, r), torch.where(x >= 0, r, er))
    y = torch.where(pos, -x, x)
    l = torch.where(y > 0, y, torch.zeros_like(y)) + torch.log1p(e)
    part = torch.stack([_chunks(l), _chunks(g * (t * C)), _chunks(g)]).contiguous() if partials else None
    C.copy_(t * g)
    return C, part


def sigmoid_pairs_loss(partials, scale, out=None, accumulate=False):
    v = partials.sum() * scale
    if out is None:
        return v.reshape(()).clone()
    with torch.no_grad():
        out.copy_((out + v if accumulate else v).reshape(out.shape))
    return out
