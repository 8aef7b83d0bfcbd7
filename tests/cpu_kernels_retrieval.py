"""TEST-ONLY: tests/cpu_kernels.py plus a torch emulation of `kernels.retrieval_ranks`, so that the data-parallel protocol of
`functional.retrieval_ranks` / `contrastive.retrieval_metrics` runs on gloo / CPU.  Scores are formed in float64 (exact for the
integer embeddings the gloo test uses) and rounded to fp32 as the kernel's are.  Never imported by the package."""
import torch

from cpu_kernels import *  # noqa: F401,F403


def retrieval_ranks(Q, G, diag_off=0, keys_q=None, keys_g=None):
    N, M = Q.shape[0], G.shape[0]
    if (keys_q is None) != (keys_g is None):
        raise ValueError("retrieval_ranks: keys_q and keys_g go together")
    S = (Q.double() @ G.double().T).float()
    if keys_q is None:
        if diag_off < 0 or diag_off + N > M:
            raise ValueError("retrieval_ranks: diag_off outside [0, M - N]")
        P = torch.zeros(N, M, dtype=torch.bool)
        P[torch.arange(N), diag_off + torch.arange(N)] = True
    else:
        P = keys_q[:, None] == keys_g[None, :]
    neg_inf = torch.full_like(S, float("-inf"))
    pos = torch.where(P, S, neg_inf).max(dim=1).values                      # torch.max keeps a NaN
    greater = ((S > pos[:, None]) & ~P).sum(1).to(torch.int32)
    ties = ((S == pos[:, None]) & ~P).sum(1).to(torch.int32)
    flag = torch.isnan(pos) | (torch.isnan(S) & ~P).any(1)
    greater[flag] = -1
    ties[flag] = -1
    return pos, greater, ties
