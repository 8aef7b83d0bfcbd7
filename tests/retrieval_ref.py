"""TEST-ONLY reference of the retrieval ranks and metrics (include/cxrk.h "retrieval_ranks"), numpy on the CPU.

  ranks_exact    integer-valued inputs multiplied in int64: scores, positives (pair offset or key equality), best positive,
                 strict-greater and tie counts -- no rounding anywhere
  ranks_float64  the same on the fp32 inputs converted exactly to float64, plus the score matrix (for the rounding bounds)
  bounds         per row, what an fp32 kernel may return for real-valued unit-norm inputs: lower / upper bound of `greater`, upper
                 bound of `ties`, from the derived dot-product error gamma = D u / (1 - D u), u = 2^-24
  metrics        Recall@K, median and mean rank from (greater, ties), written independently of the package's `rank_metrics`
Never imported by the package."""
import numpy as np
import torch


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def positives_mask(N, M, diag_off=0, keys_q=None, keys_g=None):
    """bool [N, M]: column j is a positive of row i"""
    if keys_q is None:
        assert keys_g is None and diag_off >= 0 and diag_off + N <= M
        m = np.zeros((N, M), dtype=bool)
        m[np.arange(N), diag_off + np.arange(N)] = True
        return m
    kq, kg = _np(keys_q).astype(np.int64), _np(keys_g).astype(np.int64)
    assert kq.shape == (N,) and kg.shape == (M,)
    return kq[:, None] == kg[None, :]


def _counts(S, P):
    """S [N, M] scores (int64 or float64, NaN allowed), P positives -> (pos float64, greater int64, ties int64) by the contract:
    a row whose best positive is NaN, or that has a NaN among its non-positive scores, gets greater = ties = -1"""
    N, M = S.shape
    Sf = S.astype(np.float64)
    nan = np.isnan(Sf)
    pos = np.full(N, -np.inf)
    for i in range(N):
        if P[i].any():
            row = Sf[i, P[i]]
            pos[i] = np.nan if np.isnan(row).any() else row.max()
    with np.errstate(invalid="ignore"):
        greater = ((Sf > pos[:, None]) & ~P).sum(1).astype(np.int64)
        ties = ((Sf == pos[:, None]) & ~P).sum(1).astype(np.int64)
    flag = np.isnan(pos) | (nan & ~P).any(1)
    greater[flag] = -1
    ties[flag] = -1
    return pos, greater, ties


def ranks_exact(Q, G, diag_off=0, keys_q=None, keys_g=None):
    """integer-valued Q [N, D], G [M, D] (any dtype holding integers) -> (pos, greater, ties), every score an exact int64"""
    q, g = _np(Q), _np(G)
    assert np.array_equal(q, np.round(q)) and np.array_equal(g, np.round(g)), "ranks_exact needs integer-valued inputs"
    S = q.astype(np.int64) @ g.astype(np.int64).T
    assert np.abs(S).max(initial=0) < 2 ** 24          # every score, and every partial sum of |terms|, is exact in fp32 too
    return _counts(S, positives_mask(q.shape[0], g.shape[0], diag_off, keys_q, keys_g))


def scores_float64(Q, G):
    return _np(Q).astype(np.float64) @ _np(G).astype(np.float64).T


def ranks_float64(Q, G, diag_off=0, keys_q=None, keys_g=None):
    """fp32 inputs converted exactly to float64 -> (pos, greater, ties, S64, P)"""
    S = scores_float64(Q, G)
    P = positives_mask(S.shape[0], S.shape[1], diag_off, keys_q, keys_g)
    return _counts(S, P) + (S, P)


def gamma(D):
    u = 2.0 ** -24
    return D * u / (1 - D * u)


def bounds(Q, G, diag_off=0, keys_q=None, keys_g=None):
    """For unit-norm rows an fp32 dot product is within gamma(D) of the exact one (|q|.|g| <= 1), so the computed s(i,j) - pos(i)
    has the sign of the exact difference whenever |s64 - pos64| > 2 gamma.  Returns per row (lo, hi, amb):
        lo  = #(non-positive j: s64 > pos64 + 2 gamma)   <= greater <= hi = lo + amb,      0 <= ties <= amb,
        amb = #(non-positive j: |s64 - pos64| <= 2 gamma)    (the ambiguous columns).
    The best positive itself may be any positive within 2 gamma of the exact best: pos64 is the exact maximum, and a computed
    maximum is within gamma of it."""
    pos, _, _, S, P = ranks_float64(Q, G, diag_off, keys_q, keys_g)
    g2 = 2 * gamma(_np(Q).shape[1])
    d = S - pos[:, None]
    lo = ((d > g2) & ~P).sum(1)
    amb = ((np.abs(d) <= g2) & ~P).sum(1)
    return lo, lo + amb, amb


def metrics(greater, ties, ks=(1, 5, 10)):
    """pessimistic rank 1 + greater + ties for R@k and the median; 1 + greater + ties / 2 for the mean; any -1 -> all nan"""
    g, t = _np(greater).astype(np.int64), _np(ties).astype(np.int64)
    n = len(g)
    if (g < 0).any() or (t < 0).any():
        out = {f"R@{k}": float("nan") for k in ks}
        out.update(median_rank=float("nan"), mean_rank=float("nan"), n=n)
        return out
    worst = sorted(int(a) + int(b) + 1 for a, b in zip(g, t))
    out = {f"R@{k}": sum(1 for w in worst if w <= k) / n for k in ks}
    out["median_rank"] = float(worst[n // 2]) if n % 2 else 0.5 * (worst[n // 2 - 1] + worst[n // 2])
    out["mean_rank"] = sum(1 + int(a) + 0.5 * int(b) for a, b in zip(g, t)) / n
    out["n"] = n
    return out


def metrics_both(img, txt, keys=None, ks=(1, 5, 10), ranks=ranks_exact):
    """{"i2t", "t2i"} over the whole set in one process (`ranks`: ranks_exact for integer embeddings)"""
    out = {}
    for name, q, g in (("i2t", img, txt), ("t2i", txt, img)):
        r = ranks(q, g, 0, keys, keys)
        out[name] = metrics(r[1], r[2], ks)
    return out
