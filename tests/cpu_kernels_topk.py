"""TEST-ONLY: tests/cpu_kernels.py plus a torch emulation of `kernels.topk_neighbours` and `kernels.knn_vote`, so that the
data-parallel protocol of `functional.topk_neighbours` / `contrastive.KNNBank` runs on gloo / CPU.  Scores are formed in float64
(exact for the integer embeddings the gloo test uses) and rounded to fp32 as the kernel's are; the order is the kernel's: score
descending with every NaN first, then index ascending.  Never imported by the package."""
import torch

from cpu_kernels import *  # noqa: F401,F403

TOPK_MAX = 64


def topk_neighbours(Q, G, k, exclude_off=-1):
    N, M = Q.shape[0], G.shape[0]
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk_neighbours: k must be in [1, {TOPK_MAX}], got {k}")
    if exclude_off < -1 or (exclude_off >= 0 and exclude_off + N > M):
        raise ValueError("topk_neighbours: exclude_off does not fit the gallery")
    S = (Q.double() @ G.double().T).float()
    cand = torch.ones(N, M, dtype=torch.bool)
    if exclude_off >= 0:
        cand[torch.arange(N), exclude_off + torch.arange(N)] = False
    # a sortable stand-in for the order: NaN above +inf, excluded columns below -inf; the sort is stable, so equal scores keep the
    # ascending column order
    rank = torch.where(torch.isnan(S), torch.tensor(float("inf")), S).double()
    rank = torch.where(torch.isnan(S), rank, torch.where(torch.isinf(S), torch.sign(S) * 1e300, rank))
    rank = torch.where(cand, rank, torch.tensor(float("-inf"), dtype=torch.float64))
    order = torch.sort(rank, dim=1, descending=True, stable=True).indices[:, :k]
    score = torch.gather(S, 1, order)
    keep = torch.gather(cand, 1, order)
    index = torch.where(keep, order, torch.tensor(-1)).to(torch.int32)
    score = torch.where(keep, score, torch.tensor(float("-inf")))
    if order.shape[1] < k:
        pad = k - order.shape[1]
        score = torch.cat([score, torch.full((N, pad), float("-inf"))], 1)
        index = torch.cat([index, torch.full((N, pad), -1, dtype=torch.int32)], 1)
    return score.contiguous(), index.contiguous()


def knn_vote(score, index, labels, temperature):
    valid = index >= 0
    w = torch.where(valid, torch.exp((score - score[:, :1]) / float(temperature)), torch.zeros(()))
    lab = labels[index.clamp_min(0).long()]                     # [N, k, C]
    out = (w[:, :, None] * lab).sum(1) / w.sum(1, keepdim=True)
    bad = (torch.isnan(score) & valid).any(1) | ~valid.any(1)
    out[bad] = float("nan")
    return out.float()
