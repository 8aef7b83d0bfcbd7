"""TEST-ONLY float64 reference of the label-aware multi-positive InfoNCE loss, an independent torch restatement:
`log_softmax`, a key-equality matrix and autograd -- nothing of the package is imported.  Also the closed-form gradient w.r.t. the
logits and the numpy uint64 restatement of `contrastive.row_keys`."""
import numpy as np
import torch
import torch.nn.functional as F


def multipos_loss(img, txt, keys, temperature):
    """(loss, S) in float64.  img / txt [Bg, D] (any float dtype; differentiable), keys int64 [Bg] (pair i = image i + text i).
        L = 1/(2 Bg) sum_i [ -1/n_i sum_{j in P(i)} log_softmax_row(S)_ij ] + 1/(2 Bg) sum_j [ -1/n_j sum_{i in P(j)} log_softmax_col(S)_ij ]"""
    ih = F.normalize(img.double(), dim=1)
    th = F.normalize(txt.double(), dim=1)
    S = ih @ th.T / temperature
    eq = (keys[:, None] == keys[None, :]).double()
    target = eq / eq.sum(1, keepdim=True)                       # row i: 1/n_i on P(i); symmetric because n_j = n_i inside a group
    rows = -(target * F.log_softmax(S, dim=1)).sum(1)
    cols = -(target * F.log_softmax(S, dim=0)).sum(0)
    return 0.5 * (rows.mean() + cols.mean()), S


def multipos_grads(img, txt, keys, temperature):
    """loss (float), d img, d txt (float64) by autograd on fresh float64 leaves"""
    i64 = img.detach().double().requires_grad_(True)
    t64 = txt.detach().double().requires_grad_(True)
    loss, _ = multipos_loss(i64, t64, keys, temperature)
    loss.backward()
    return float(loss), i64.grad, t64.grad


def closed_form_dS(S, keys):
    """dL/dS_ij = ( softmax_row(S)_ij + softmax_col(S)_ij - 2 [k_i = k_j] / n_i ) / (2 Bg)"""
    S = S.double()
    eq = (keys[:, None] == keys[None, :]).double()
    n = eq.sum(1, keepdim=True)
    return (torch.softmax(S, 1) + torch.softmax(S, 0) - 2 * eq / n) / (2 * S.shape[0])


def block_stats(S, keys_row, keys_col):
    """float64 (lse, posmean, npos) of a logits block, what cxrk_multipos_row_stats computes"""
    S = S.double()
    eq = keys_row[:, None] == keys_col[None, :]
    n = eq.sum(1)
    pm = (S * eq).sum(1) / n.clamp_min(1)
    return torch.logsumexp(S, 1), pm, n


def block_grad(S, keys_row, keys_col, n_row, lse_row, lse_col):
    """float64 result of cxrk_multipos_grad_inplace"""
    S = S.double()
    eq = (keys_row[:, None] == keys_col[None, :]).double()
    return torch.exp(S - lse_row.double()[:, None]) + torch.exp(S - lse_col.double()[None, :]) - 2 * eq / n_row.double()[:, None]


# ---- contrastive.row_keys in numpy uint64 arithmetic, from its docstring ------------------------------------------------------
def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def row_keys_numpy(rows, mask=None):
    rows = np.asarray(rows).astype(np.int64)
    out = np.zeros(rows.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for b in range(rows.shape[0]):
            acc, p = np.uint64(0), 0
            for t in range(rows.shape[1]):
                if mask is not None and int(np.asarray(mask)[b, t]) == 0:
                    continue
                p += 1
                x = np.array(rows[b, t]).astype(np.int64).view(np.uint64)
                acc = acc + _mix(_mix(x) + np.uint64(p) * np.uint64(0x9E3779B97F4A7C15))
            out[b] = _mix(np.uint64(acc))
    return out.view(np.int64)
