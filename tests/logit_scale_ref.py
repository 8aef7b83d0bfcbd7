"""TEST-ONLY float64 reference of InfoNCE with a learnable temperature: torch autograd over exp(theta) * I_hat T_hat^T,
plain and keyed -- nothing of the package is imported.  Also the float64 restatement of what the *_scaled kernels write for one block."""
import torch
import torch.nn.functional as F

import multipos_ref


def scaled_loss(img, txt, theta, keys=None):
    """(loss, S) in float64; theta a float64 0-d tensor (differentiable); keys=None: one positive per row, the diagonal"""
    Bg = img.shape[0]
    if keys is None:
        keys = torch.arange(Bg, dtype=torch.int64)
    ih = F.normalize(img.double(), dim=1)
    th = F.normalize(txt.double(), dim=1)
    S = torch.exp(theta) * (ih @ th.T)
    eq = (keys[:, None] == keys[None, :]).double()
    target = eq / eq.sum(1, keepdim=True)
    rows = -(target * F.log_softmax(S, dim=1)).sum(1)
    cols = -(target * F.log_softmax(S, dim=0)).sum(0)
    return 0.5 * (rows.mean() + cols.mean()), S


def scaled_grads(img, txt, theta, keys=None):
    """loss (float), d img, d txt (float64), d theta (float), sum |G o S| / (2 Bg) (float: the scale of d theta's summands)"""
    i64 = img.detach().double().requires_grad_(True)
    t64 = txt.detach().double().requires_grad_(True)
    th64 = torch.tensor(float(theta), dtype=torch.float64, requires_grad=True)
    loss, S = scaled_loss(i64, t64, th64, keys)
    loss.backward()
    Sd = S.detach()
    k = torch.arange(Sd.shape[0]) if keys is None else keys
    dS = multipos_ref.closed_form_dS(Sd, k)
    closed = float((dS * Sd).sum())
    assert abs(closed - float(th64.grad)) <= 1e-12 * max(1.0, float((dS * Sd).abs().sum())), (closed, float(th64.grad))   # the issue's identity
    return float(loss.detach()), i64.grad, t64.grad, float(th64.grad), float((dS * Sd).abs().sum())


def block_keys(rows, cols, off, keys_row=None, keys_col=None):
    """(keys_row, keys_col) of a block: the plain loss is the keyed one with the column index as the key"""
    if keys_row is None:
        keys_col = torch.arange(cols, dtype=torch.int64)
        keys_row = keys_col[off:off + rows]
    return keys_row, keys_col


def block_stats(C, theta, off, keys_row=None, keys_col=None):
    """float64 (lse, posmean, npos) of x = exp(theta) * C: what the two scaled stats entry points compute"""
    kr, kc = block_keys(C.shape[0], C.shape[1], off, keys_row, keys_col)
    return multipos_ref.block_stats(torch.exp(torch.tensor(float(theta), dtype=torch.float64)) * C.double(), kr, kc)


def block_grad(C, theta, off, n_row, lse_row, lse_col, keys_row=None, keys_col=None):
    """float64 (s * G, G o S) of one block: what the scaled gradient entry points leave in C, and the summands of its partial sums"""
    kr, kc = block_keys(C.shape[0], C.shape[1], off, keys_row, keys_col)
    s = torch.exp(torch.tensor(float(theta), dtype=torch.float64))
    S = s * C.double()
    G = multipos_ref.block_grad(S, kr, kc, n_row, lse_row, lse_col)
    return s * G, G * S
