"""Fused top-k neighbour search and the kNN vote on the GPU (include/cxrk.h "topk_neighbours" / "knn_vote"): the
kernels against the exact integer reference (bit equality of score and index) on shapes that cross every tile, strip and split
boundary; duplicated and all-equal gallery rows; real-valued inputs against the derived fp32 rounding bound; agreement with
`retrieval_ranks`; precision-mode independence; the non-finite contract; the memory contract; argument errors; the vote against its
float64 reference.  The reference is tests/topk_ref.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import memguard as MG  # noqa: E402
import topk_ref as T  # noqa: E402

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
KMAX = 64

#          N    M     D
SHAPES = [(1, 1, 1),            # smallest possible problem
          (1, 5, 3),            # M < k for most k
          (127, 129, 36),       # one strip, two gallery tiles, K tail
          (129, 128, 32),       # two strips, one full tile, no K tail
          (3, 1100, 36),        # one strip over nine gallery blocks: the merge
          (257, 300, 128),      # three strips
          (700, 300, 33)]       # six strips
KS = [1, 5, 20, 64]


def ints(N, M, D, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + N + 7 * M + 13 * D)
    return torch.randint(-3, 4, (N, D), generator=g).float(), torch.randint(-3, 4, (M, D), generator=g).float()


def pitched(x, pad=3):
    """rows ld = D + pad floats apart on the device, the padding NaN"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
    v = buf[:, :x.shape[1]]
    v.copy_(x)
    return v


def excludes(N, M):
    return [-1] + ([0] if M >= N else []) + ([M - N] if M > N else [])


@functools.lru_cache(maxsize=None)
def exact64(N, M, D, exclude_off):
    """the reference at k = 64, computed once per (shape, exclusion): a smaller k is its prefix (the order is total)"""
    Q, G = ints(N, M, D)
    return T.topk_exact(Q, G, KMAX, exclude_off)


def assert_bit_equal(got, want, what=""):
    score, index = (t.cpu().numpy() for t in got)
    rscore, rindex = want
    assert score.dtype == np.float32 and index.dtype == np.int32
    assert np.array_equal(index.astype(np.int64), rindex), (what, "index", np.argwhere(index != rindex)[:8])
    assert np.array_equal(score, rscore.astype(np.float32), equal_nan=True), (what, "score", np.argwhere(score != rscore)[:8])
    assert np.array_equal(np.signbit(score), np.signbit(rscore)), (what, "sign of a zero")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N,M,D", SHAPES)
def test_exact_integer_cases(N, M, D, k):
    """entries in {-3..3}: every dot product is an integer below 2^24, exact in fp32 in any order, and ties are plentiful -> score
    and index EQUAL the int64 reference's stable sort by (-score, index).  Pitched inputs (ld = D + 3, NaN padding); every valid
    exclude_off of {-1, 0, M - N}."""
    Q, G = ints(N, M, D)
    Qd, Gd = pitched(Q), pitched(G)
    sp = K._lib.load().cxrk_topk_neighbours_slab_bytes(N, M, k) // (8 * N * k)
    assert sp == {(3, 1100, 36): 9, (700, 300, 33): 3}.get((N, M, D), sp)      # the merge path and the strip count are what was meant
    for off in excludes(N, M):
        rs, ri = exact64(N, M, D, off)
        want = (rs[:, :k], ri[:, :k])
        if M > 64 and N > 64 and k >= 20:
            assert (np.diff(want[0], axis=1) == 0).any(), "the construction is meant to give ties"
        got = K.topk_neighbours(Qd, Gd, k, off)
        assert_bit_equal(got, want, f"{(N, M, D)} k={k} exclude_off={off}")
        cand = M - (off >= 0)
        if cand < k:                                                            # M < k, and M < k + 1 with the exclusion
            assert (want[1][:, cand:] == -1).all() and np.isneginf(want[0][:, cand:]).all() and (want[1][:, :cand] >= 0).all()
        if off >= 0:
            assert not (got[1].cpu().numpy() == (np.arange(N) + off)[:, None]).any()
    assert bool(torch.isnan(Qd._base[:, D:]).all()) and bool(torch.isnan(Gd._base[:, D:]).all()), "pitch padding written"


def test_duplicated_gallery_rows_appear_in_index_order():
    N, M, D, k = 130, 300, 36, 20
    Q, G = ints(N, M, D, seed=1)
    dup = [5, 40, 128, 131, 290]                # five copies of one row, in three column tiles
    G[dup] = G[40].clone()
    Q[:] = G[40] * (1 + torch.arange(N) % 3)[:, None].float()      # every query is a multiple of that row: its copies tie at the top
    want = T.topk_exact(Q, G, k)
    assert all(want[1][i, :5].tolist() == dup for i in range(N)), "the copies are meant to be the five best of every row"
    got = K.topk_neighbours(Q.to(DEV), G.to(DEV), k)
    assert_bit_equal(got, want)
    idx = got[1].cpu().numpy()
    assert all(idx[i, :5].tolist() == dup and len(set(idx[i].tolist())) == k for i in range(N))
    # excluding one copy (row i's own column for the queries 128..129 -> columns 128, 129... with exclude_off 0) shifts the rest up
    idx0 = K.topk_neighbours(Q.to(DEV), G.to(DEV), k, 0)[1].cpu().numpy()
    assert idx0[5, :4].tolist() == [40, 128, 131, 290] and idx0[128, :4].tolist() == [5, 40, 131, 290] and idx0[0, :5].tolist() == dup


@pytest.mark.parametrize("off", [-1, 0, 170])
@pytest.mark.parametrize("k", [1, 20, 64])
def test_all_equal_gallery_lists_the_first_columns_past_the_excluded_one(k, off):
    N, M, D = 130, 300, 8
    Q = torch.randint(-3, 4, (N, D), generator=torch.Generator().manual_seed(5)).float()
    G = torch.ones(1, D).expand(M, D).contiguous()
    score, index = (t.cpu().numpy() for t in K.topk_neighbours(Q.to(DEV), G.to(DEV), k, off))
    for i in range(N):
        cols = [j for j in range(k + 1) if off < 0 or j != i + off][:k]
        assert index[i].tolist() == cols, (i, index[i][:8])
    assert np.array_equal(score, np.repeat(Q.sum(1).numpy()[:, None], k, 1))


def unit_rows(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True)).float()


@pytest.mark.parametrize("N,M,D", [(257, 257, 36), (130, 300, 128)])
def test_real_valued_cases_within_the_derived_rounding_bound(N, M, D):
    """unit-norm Gaussian rows, k = 10.  u = 2^-24, gamma = D u / (1 - D u): an fp32 dot product of unit vectors is within gamma of
    the exact one, so the computed order of two columns can differ from the exact one only when their float64 scores are within
    2 gamma.  Hence: every returned score within gamma of the float64 score of its index; every column more than 2 gamma above the
    float64 k-th best is listed; every listed column is within 2 gamma of the k-th best; rows sorted by the returned
    (score, index); no index twice."""
    k = 10
    Q, G = unit_rows(N, D, 11), unit_rows(M, D, 111)
    s64, _, S = T.topk_float64(Q, G, k)
    g = T.gamma(D)
    score, index = (t.cpu().numpy() for t in K.topk_neighbours(pitched(Q), pitched(G), k))
    assert (index >= 0).all() and (index < M).all()
    own = np.take_along_axis(S, index.astype(np.int64), 1)
    print(f"max |score - s64[index]| = {np.abs(score - own).max():.3e} (gamma {g:.3e})")
    assert (np.abs(score.astype(np.float64) - own) <= g).all()
    kth = s64[:, k - 1]
    for i in range(N):
        listed = set(index[i].tolist())
        assert len(listed) == k, i
        must = set(np.flatnonzero(S[i] > kth[i] + 2 * g).tolist())
        assert must <= listed, (i, must - listed)
        assert (own[i] >= kth[i] - 2 * g).all(), i
        pairs = list(zip((-score[i]).tolist(), index[i].tolist()))
        assert pairs == sorted(pairs), i


def test_agrees_with_retrieval_ranks_on_the_same_inputs():
    """pair mode: `greater + ties < k` puts the positive in the list whatever the tie order, `greater >= k` keeps it out"""
    N, M, D, off = 130, 300, 36, 100
    Q, G = ints(N, M, D, seed=3)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    _, greater, ties = (t.cpu().numpy() for t in K.retrieval_ranks(Qd, Gd, off))
    seen_in = seen_out = 0
    for k in (1, 5, 20, 64):
        index = K.topk_neighbours(Qd, Gd, k)[1].cpu().numpy()
        listed = (index == (np.arange(N) + off)[:, None]).any(1)
        sure_in, sure_out = greater + ties < k, greater >= k
        assert listed[sure_in].all() and not listed[sure_out].any(), k
        seen_in, seen_out = seen_in + int(sure_in.sum()), seen_out + int(sure_out.sum())
    assert seen_in and seen_out


def test_result_does_not_depend_on_the_precision_mode():
    Q, G = unit_rows(130, 128, 11), unit_rows(300, 128, 111)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    old = _lib.get_precision()
    outs = []
    try:
        for mode in ("fp32", "split_bf16"):
            _lib.set_precision(mode)
            outs.append(K.topk_neighbours(Qd, Gd, 10) + K.topk_neighbours(Qd, Gd[:130], 20, 0))
    finally:
        _lib.set_precision(old)
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_non_finite_scores_sort_by_the_contract():
    N, M, D, k = 6, 140, 8, 5
    Q, G = ints(N, M, D, seed=2)
    Q, G = Q.abs() + 1, G.abs() + 1            # positive entries: no Inf * 0
    G[133, 2] = float("nan")                   # a NaN gallery row in the second column tile
    Q[2, 3] = float("nan")                     # a NaN query
    G[7] = float("inf")
    G[9] = float("-inf")
    with np.errstate(invalid="ignore"):
        want = T.topk_float64(Q, G, k)[:2]
    got = K.topk_neighbours(pitched(Q), pitched(G), k)
    score, index = (t.cpu().numpy() for t in got)
    assert np.array_equal(index.astype(np.int64), want[1]) and np.array_equal(score, want[0].astype(np.float32), equal_nan=True)
    rows = [0, 1, 3, 4, 5]
    assert (index[rows, 0] == 133).all() and np.isnan(score[rows, 0]).all()            # the NaN is every query's first neighbour
    assert (index[rows, 1] == 7).all() and np.isposinf(score[rows, 1]).all()           # +inf sorts as a number, below the NaN
    assert np.isfinite(score[rows, 2:]).all()
    assert index[2].tolist() == list(range(k)) and np.isnan(score[2]).all()            # a NaN query: 0..k-1, all NaN
    # -inf sorts as a number too: gallery rows 6..10 hold +inf at 1 and -inf at 3 -> the first and the last real neighbour
    s2, i2 = (t.cpu().numpy() for t in K.topk_neighbours(pitched(Q[:1]), pitched(G[6:11]), 8))
    assert i2[0, 0] == 1 and i2[0, 4] == 3 and sorted(i2[0, 1:4].tolist()) == [0, 2, 4]
    assert np.isposinf(s2[0, 0]) and np.isfinite(s2[0, 1:4]).all() and np.isneginf(s2[0, 4])
    assert (i2[0, 5:] == -1).all() and np.isneginf(s2[0, 5:]).all()
    # the vote: a NaN row gives NaN, the other rows are untouched
    labels = torch.randint(0, 2, (M, 3), generator=torch.Generator().manual_seed(1)).float().to(DEV)
    Gf = G.clone()
    Gf[[7, 9]] = 1.0
    sc, ix = K.topk_neighbours(pitched(Q), pitched(Gf), k)                             # rows 0,1,3,4,5: one NaN each; row 2 all NaN
    out = K.knn_vote(sc, ix, labels, 0.5).cpu().numpy()
    assert np.isnan(out).all()
    Gc = Gf.clone()
    Gc[133] = 1.0
    sc, ix = K.topk_neighbours(pitched(Q), pitched(Gc), k)
    out = K.knn_vote(sc, ix, labels, 0.5).cpu().numpy()
    clean = K.knn_vote(sc[[0, 1, 3, 4, 5]].contiguous(), ix[[0, 1, 3, 4, 5]].contiguous(), labels, 0.5).cpu().numpy()
    assert np.isnan(out[2]).all() and np.isfinite(out[rows]).all() and np.array_equal(out[rows], clean)


def test_memory_contract_exact_workspace_guards_and_poison():
    """outputs and a workspace of exactly cxrk_topk_neighbours_slab_bytes between guard regions, poisoned with two fills: guards
    intact, every element written, the result independent of the poison"""
    lib = _lib.load()
    N, M, D, k = 129, 300, 36, 5
    Q, G = ints(N, M, D, seed=4)
    Qd, Gd = pitched(Q), pitched(G)
    need = lib.cxrk_topk_neighbours_slab_bytes(N, M, k)
    assert need == N * 3 * k * 8                       # two strips -> three gallery blocks of one tile each

    def call(o):
        ws = K.workspace(need, Qd.device)
        _lib.check(lib.cxrk_topk_neighbours(Qd.data_ptr(), Qd.stride(0), N, Gd.data_ptr(), Gd.stride(0), M, D, k, 100,
                                            o["score"].data_ptr(), o["index"].data_ptr(), ws.data_ptr(), ws.numel() * 4, K._stream()),
                   "cxrk_topk_neighbours")

    spec = {"score": Out((N, k)), "index": Out((N, k), torch.int32)}
    o = MG.run_contract(call, spec, None, None, module=K, device=DEV, runs=("session", "nan", "alt"))
    assert_bit_equal((o["score"].t, o["index"].t), T.topk_exact(Q, G, k, 100))
    MG.refuses_short_workspace(call, spec, module=K, device=DEV)
    MG.refuses_misaligned_workspace(call, spec, module=K, device=DEV)
    # the vote has no workspace: guarded output, two fills
    labels = torch.randint(0, 2, (M, 5), generator=torch.Generator().manual_seed(2)).float().to(DEV)
    sc, ix = o["score"].t.contiguous(), o["index"].t.contiguous()

    def vote(v):
        _lib.check(lib.cxrk_knn_vote(sc.data_ptr(), ix.data_ptr(), N, k, labels.data_ptr(), 5, M, 5, 2.0, v["out"].data_ptr(),
                                     K._stream()), "cxrk_knn_vote")

    v = MG.run_contract(vote, {"out": Out((N, 5))}, None, None, module=K, device=DEV, runs=("session", "alt"))
    assert np.abs(v["out"].t.cpu().numpy() - T.vote_ref(sc, ix, labels, 0.5)).max() < 1e-5


def test_argument_errors_raise_and_leave_the_outputs_untouched():
    lib = _lib.load()
    Q, G = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV)
    score = torch.full((4, 64), 7.0, device=DEV)
    index = torch.full((4, 64), 7, dtype=torch.int32, device=DEV)
    ws = K.workspace(lib.cxrk_topk_neighbours_slab_bytes(4, 6, 64), Q.device)
    P = lambda t: t.data_ptr()  # noqa: E731
    #       0     1  2  3     4  5  6  7  8
    good = [P(Q), 8, 4, P(G), 8, 6, 8, 2, -1, P(score), P(index), P(ws), ws.numel() * 4]
    bad = [(7, 0), (7, 65), (7, -1),                 # k outside [1, 64]
           (8, 3), (8, -2),                          # exclude_off + N > M; below -1
           (1, 7), (4, 7),                           # ld < D
           (2, 0), (5, 0), (6, 0)]                   # N, M, D < 1
    for idx, v in bad:
        a = list(good)
        a[idx] = v
        assert lib.cxrk_topk_neighbours(*a, K._stream()) == -1, (idx, v)
        with pytest.raises(ValueError, match="cxrk code -1"):
            _lib.check(lib.cxrk_topk_neighbours(*a, K._stream()), "cxrk_topk_neighbours")
    torch.cuda.synchronize()
    assert bool((score == 7.0).all()) and bool((index == 7).all()), "an output was written by a refused call"
    assert lib.cxrk_topk_neighbours_slab_bytes(4, 6, 0) == 0 and lib.cxrk_topk_neighbours_slab_bytes(4, 6, 65) == 0
    _lib.check(lib.cxrk_topk_neighbours(*good, K._stream()), "cxrk_topk_neighbours")
    good[8] = 2                                      # exclude_off + N == M is the largest valid offset
    _lib.check(lib.cxrk_topk_neighbours(*good, K._stream()), "cxrk_topk_neighbours")
    torch.cuda.synchronize()
    for args in ((Q, G, 0), (Q, G, 65), (Q, G, 2, 3), (Q, G[:, :7], 2), (Q.cpu(), G, 2), (Q.t(), G.t(), 2), (Q.double(), G, 2)):
        with pytest.raises(ValueError):
            K.topk_neighbours(*args)
    s, i = K.topk_neighbours(Q, G, 2)
    lab = torch.zeros(6, 3, device=DEV)
    for args in ((s, i.long(), lab, 1.0), (s, i[:3], lab, 1.0), (s, i, lab, 0.0), (s, i, lab.cpu(), 1.0), (s, i, lab.t(), 1.0)):
        with pytest.raises(ValueError):
            K.knn_vote(*args)


E_EXP = 2       # ulp error assumed for the device expf: the installed ROCm documentation does not state one (searched; not found)


@pytest.mark.parametrize("temperature", [0.07, 1.0])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("k", [1, 20, 64])
def test_vote_against_the_float64_reference(k, C, temperature):
    """Tolerance 2 (2 u x_max + (E_EXP + k + 2) u), u = 2^-24, x_max = 2 / T.  Derivation: the exponent's argument
    x = (s_n - s_0) / T has |x| <= x_max for cosine scores, and its two roundings (the difference, the product) move it by at most
    2 u x_max, which is the relative change of exp(x); expf adds E_EXP u; the k-term sums of positive terms (numerator with labels
    in [0, 1], denominator) add at most k u, the multiply-add and the division 2 u.  Numerator and denominator each carry that
    relative error, their ratio twice it, and the ratio -- a weighted mean of values in [0, 1] -- is at most 1, so the bound is
    absolute.  E_EXP = 2: the ROCm documentation on this machine gives no ulp figure for expf."""
    N, M = 70, 90
    g = torch.Generator().manual_seed(17 * k + C)
    score = torch.sort(torch.rand(N, k, generator=g) * 2 - 1, dim=1, descending=True).values
    index = torch.randint(0, M, (N, k), generator=g, dtype=torch.int32)
    n_valid = torch.randint(0, k + 1, (N,), generator=g)
    n_valid[:4] = torch.tensor([k, 0, 1, max(k - 1, 0)])           # full, empty, one neighbour, one padding slot
    pad = torch.arange(k)[None, :] >= n_valid[:, None]
    index[pad] = -1
    score[pad] = float("-inf")
    labels = torch.randint(0, 2, (M, C), generator=g).float()
    want = T.vote_ref(score, index, labels, temperature)
    lab = pitched(labels, pad=2)
    out = K.knn_vote(score.to(DEV), index.to(DEV), lab, temperature).cpu().numpy()
    u = 2.0 ** -24
    tol = 2 * (2 * u * (2 / temperature) + (E_EXP + k + 2) * u)
    empty = (n_valid == 0).numpy()
    assert np.isnan(out[empty]).all() and np.isnan(want[empty]).all() and empty.any()
    err = np.abs(out[~empty] - want[~empty]).max()
    print(f"k={k} C={C} T={temperature}: max abs err {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    assert bool(torch.isnan(lab._base[:, C:]).all())
    again = K.knn_vote(score.to(DEV), index.to(DEV), lab, temperature).cpu().numpy()
    assert np.array_equal(out, again, equal_nan=True)              # no atomics: bit-reproducible


def test_functional_normalizes_and_excludes_self():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(140, 96, generator=g) * 3 + 0.5).to(DEV)
    xh = Fh.l2_normalize(x)
    want = K.topk_neighbours(xh, xh, 7, 0)
    got = Fh.topk_neighbours(x, x, 7, exclude_self=True)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not bool((got[1] == torch.arange(140, device=DEV, dtype=torch.int32)[:, None]).any())
    keep = Fh.topk_neighbours(x, x, 7)
    assert bool((keep[1][:, 0] == torch.arange(140, device=DEV, dtype=torch.int32)).all())     # a row's nearest row is itself
    raw = Fh.topk_neighbours(x, x, 7, normalize=False)
    assert not torch.equal(raw[0], keep[0])
    with pytest.raises(ValueError):
        Fh.topk_neighbours(x, x[:139], 7, exclude_self=True)
    with pytest.raises(ValueError):
        Fh.topk_neighbours(x, x[:, :95], 7)
