"""TEST-ONLY reference of the top-k neighbour search and the kNN vote (include/cxrk.h "topk_neighbours" / "knn_vote", DESIGN.md
§5.15), numpy on the CPU.

  topk_exact    integer-valued inputs multiplied in int64, a stable sort by (-score, index), the excluded column removed, the
                tail padded with index -1 / score -inf -- no rounding anywhere
  topk_float64  the same order on the float64 scores of fp32 inputs (NaN first), plus the score matrix, for the rounding bounds
  gamma         the fp32 dot-product error bound of unit-norm rows (tests/retrieval_ref.py)
  vote_ref      the weighted vote in float64
Never imported by the package."""
import numpy as np

from retrieval_ref import _np, gamma, scores_float64  # noqa: F401


def _select(S, k, exclude_off):
    """S [N, M] (int64 or float64; NaN allowed) -> (score float64 [N, k], index int64 [N, k]): score descending with every NaN
    first, then index ascending; column i + exclude_off is no candidate of row i; padding -inf / -1"""
    N, M = S.shape
    score = np.full((N, k), -np.inf)
    index = np.full((N, k), -1, dtype=np.int64)
    for i in range(N):
        row = S[i].astype(np.float64)
        cols = np.arange(M)
        if exclude_off >= 0:
            assert i + exclude_off < M
            cols = np.delete(cols, i + exclude_off)
        v = row[cols]
        nan = np.isnan(v)
        # primary key: NaN first, then the score descending; np.lexsort is stable and the columns are ascending already
        order = np.lexsort((cols, np.where(nan, 0.0, -v), ~nan))[:k]
        score[i, :len(order)] = v[order]
        index[i, :len(order)] = cols[order]
    return score, index


def topk_exact(Q, G, k, exclude_off=-1):
    """integer-valued Q [N, D], G [M, D] -> (score float64, index int64), every score an exact int64 below 2^24"""
    q, g = _np(Q), _np(G)
    assert np.array_equal(q, np.round(q)) and np.array_equal(g, np.round(g)), "topk_exact needs integer-valued inputs"
    S = q.astype(np.int64) @ g.astype(np.int64).T
    assert np.abs(S).max(initial=0) < 2 ** 24
    return _select(S, k, exclude_off)


def topk_float64(Q, G, k, exclude_off=-1):
    """fp32 inputs converted exactly to float64 -> (score, index, S64)"""
    with np.errstate(invalid="ignore"):
        S = scores_float64(Q, G)
    return _select(S, k, exclude_off) + (S,)


def vote_ref(score, index, labels, temperature):
    """out[i][c] = sum_n w_n labels[index_n][c] / sum_n w_n, w_n = exp((s_n - s_0) / T), float64; index -1 weighs nothing; a row with
    a NaN score among its neighbours, or without a neighbour, is NaN"""
    s, idx, lab = _np(score).astype(np.float64), _np(index).astype(np.int64), _np(labels).astype(np.float64)
    N, k = s.shape
    out = np.full((N, lab.shape[1]), np.nan)
    for i in range(N):
        valid = idx[i] >= 0
        if not valid.any() or np.isnan(s[i][valid]).any():
            continue
        w = np.where(valid, np.exp((s[i] - s[i, 0]) / temperature), 0.0)
        out[i] = (w[valid, None] * lab[idx[i][valid]]).sum(0) / w[valid].sum()
    return out
