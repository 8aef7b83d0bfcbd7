"""TEST-ONLY float64 reference of the similarity-distillation head (include/cxrk.h, "distill"), its bounds, and the
fp32 restatement of the kernel's formulas that the host test compares with it.  Never imported by the package.

Notation: S / St are the student's / teacher's logits blocks [rows, cols]; p, pt the row softmaxes; the column terms of the gradient
take the column log-sum-exps as inputs (in a data-parallel shard they come from the other block, not from this block's columns).

Bounds.  The head's tolerance is TOL = 2e-5 (tests/test_sigmoid_gpu.py), taken relative to the magnitudes that enter the cancellations:
  kl[i]   = sum_j pt_ij (St_ij - S_ij) + (lse_i - lse_t_i)     is judged against   max_i ( |lse_i| + |lse_t_i| + sum_j pt_ij |St_ij - S_ij| ),
  G_ij    = (p - pt) + (q - qt)                                 is judged against   max_ij ( p + q + pt + qt ).
Relative to its own maximum the gradient of a 1 %-perturbed teacher is off by up to 1.2e-4 (each exponential carries its 1e-7 and the
differences are 1e-3 of them), which is why that maximum is not the yardstick."""
import torch

TOL = 2e-5


def cosines(rows, cols, seed=0):
    """tests/test_logit_scale_gpu.py's `cosines`, restated here so that the host test imports no GPU test module"""
    g = torch.Generator().manual_seed(seed + 7919 * rows + cols)
    return torch.rand(rows, cols, generator=g) * 2 - 1


def block_pair(rows, cols, scale, teacher):
    """(S, St) fp32: uniform cosines times `scale`; the teacher is independent, a 1 % perturbation of the student, or the student"""
    C = cosines(rows, cols)
    if teacher == "independent":
        Ct = cosines(rows, cols, seed=101)
    elif teacher == "perturbed":
        Ct = C * (1.0 + 0.01 * cosines(rows, cols, seed=202))
    elif teacher == "identical":
        Ct = C.clone()
    else:
        raise ValueError(teacher)
    return (C * scale).float(), (Ct * scale).float()


def column_lses(S, St, seed=11):
    """the column log-sum-exps of two taller blocks that contain S / St: every exp(x - lse_col) <= 1, as in the real backward; the
    same offsets for both, so identical blocks get identical vectors"""
    g = torch.Generator().manual_seed(seed + S.shape[1])
    extra = torch.rand(S.shape[1], generator=g).double()
    return (torch.logsumexp(S.double(), 0) + extra).float(), (torch.logsumexp(St.double(), 0) + extra).float()


def block_stats(S, St):
    """float64: (lse, lse_t, kl, scale): scale[i] = |lse_i| + |lse_t_i| + sum_j pt_ij |St_ij - S_ij|"""
    S, St = S.double(), St.double()
    lse, lse_t = torch.logsumexp(S, 1), torch.logsumexp(St, 1)
    pt = torch.exp(St - lse_t[:, None])
    kl = (pt * (St - S)).sum(1) + (lse - lse_t)
    scale = lse.abs() + lse_t.abs() + (pt * (St - S).abs()).sum(1)
    return lse, lse_t, kl, scale


def block_grad(S, St, lse_row, lse_col, lse_t_row, lse_t_col):
    """float64 on the fp32 inputs as given: (G, scale), scale = max_ij (p + q + pt + qt)"""
    S, St = S.double(), St.double()
    p, q = torch.exp(S - lse_row.double()[:, None]), torch.exp(S - lse_col.double()[None, :])
    pt, qt = torch.exp(St - lse_t_row.double()[:, None]), torch.exp(St - lse_t_col.double()[None, :])
    return (p - pt) + (q - qt), float((p + q + pt + qt).max())


def _lse32(X):
    m = X.max(1).values
    s = torch.exp(X - m[:, None]).sum(1)
    return m, s, m + torch.log(s)


def block_stats_fp32(S, St):
    """the kernel's formulas in fp32 torch arithmetic (up to the order of the sums): lse = m + log sum exp(x - m) for both rows,
    kl = sum_j exp(St_ij - mt) (St_ij - S_ij) / sum_t + (lse - lse_t)"""
    S, St = S.float(), St.float()
    _, _, lse = _lse32(S)
    mt, st, lse_t = _lse32(St)
    w = (torch.exp(St - mt[:, None]) * (St - S)).sum(1)
    return lse, lse_t, w / st + (lse - lse_t)


def block_grad_fp32(S, St, lse_row, lse_col, lse_t_row, lse_t_col):
    S, St = S.float(), St.float()
    return ((torch.exp(S - lse_row[:, None]) - torch.exp(St - lse_t_row[:, None]))
            + (torch.exp(S - lse_col[None, :]) - torch.exp(St - lse_t_col[None, :])))


def distill_loss64(img, txt, img_t, txt_t, tau):
    """L_d on float64 embeddings of the global batch, by torch autograd-able ops"""
    F = torch.nn.functional
    S = F.normalize(img, dim=1) @ F.normalize(txt, dim=1).T / tau
    St = F.normalize(img_t, dim=1) @ F.normalize(txt_t, dim=1).T / tau
    rows = (torch.softmax(St, 1) * (torch.log_softmax(St, 1) - torch.log_softmax(S, 1))).sum()
    cols = (torch.softmax(St, 0) * (torch.log_softmax(St, 0) - torch.log_softmax(S, 0))).sum()
    return (rows + cols) / (2 * S.shape[0])


def distill_grads(img, txt, img_t, txt_t, tau, weight=1.0):
    """{"loss": L_d (unweighted), "dimg", "dtxt": d(weight * L_d) / d embeddings}: float64 autograd over the global batch"""
    img = img.detach().double().clone().requires_grad_(True)
    txt = txt.detach().double().clone().requires_grad_(True)
    loss = distill_loss64(img, txt, img_t.detach().double(), txt_t.detach().double(), tau)
    dimg, dtxt = torch.autograd.grad(weight * loss, (img, txt))
    return {"loss": float(loss.detach()), "dimg": dimg, "dtxt": dtxt}
