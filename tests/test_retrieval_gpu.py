"""Streaming retrieval ranks on the GPU (include/cxrk.h "retrieval_ranks"): the fused kernel against the exact
integer reference (equality, no tolerance) on shapes that cross every tile boundary, with pitched NaN-padded inputs and guarded,
poisoned outputs; real-valued inputs against the derived fp32 rounding bound; precision-mode independence; the non-finite contract;
argument errors; `functional.retrieval_ranks`; and `JointContrastiveTrainer.evaluate_retrieval` on tiny encoders.
The reference is tests/retrieval_ref.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import memguard as MG  # noqa: E402
import retrieval_ref as R  # noqa: E402

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out

#          N     M     D    diag_off
SHAPES = [(1, 1, 1, 0),             # smallest possible problem
          (4, 4, 8, 0),             # smallest square
          (5, 13, 7, 6),            # K tail, everything inside one partial tile
          (130, 300, 128, 100),     # row strip boundary, column tail
          (257, 257, 36, 0),        # three strips
          (8, 5000, 128, 4000),     # many column ranges per strip
          (64, 1030, 128, 900)]     # multi-range plus tail
G3, G2, NEG, HI = 7, 0x1234, -(1 << 62) - 5, 1 << 35


def key_vector(kind, N, M, off):
    """gallery keys [M] (int64, CPU); the query keys are its slice [off, off + N), as in a data-parallel shard (the ideas of
    tests/test_multipos_gpu.py::key_vector, for any shape)"""
    k = 100000 + 3 * torch.arange(M, dtype=torch.int64)       # above G3 and G2: no accidental member of a group
    if kind == "distinct":
        return k
    if kind == "equal":
        return torch.full((M,), -42, dtype=torch.int64)
    assert kind == "mixed"
    if M < 8 or N < 5:
        # too small for all groups at once: a pair, a key that differs from the pair's only in bit 35, a negative singleton
        for j, v in zip(range(min(M, 4)), (G2, G2, G2 + HI, NEG)):
            k[j] = v
        return k
    outside = 0 if off >= 1 else M - 1          # a member outside this shard's rows (when there is an outside)
    other = 1 if off >= 2 else M - 2
    k[off], k[off + 1], k[outside] = G3, G3, G3            # a group of 3
    k[off + 2], k[off + 3] = G2, G2                        # a group of 2
    k[other] = G2 + HI                                     # differs from the pair's key only above bit 32
    k[off + 4] = NEG                                       # a negative singleton
    vals = k.tolist()
    assert vals.count(G3) == 3 and vals.count(G2) == 2 and vals.count(G2 + HI) == 1 and vals.count(NEG) == 1
    assert ((G2 + HI) ^ G2) & 0xFFFFFFFF == 0 and NEG < 0
    return k


def ints(N, M, D, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + N + 7 * M + 13 * D)
    return torch.randint(-3, 4, (N, D), generator=g).float(), torch.randint(-3, 4, (M, D), generator=g).float()


def pitched(x, pad=3):
    """rows ld = D + pad floats apart on the device, the padding NaN"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
    v = buf[:, :x.shape[1]]
    v.copy_(x)
    return v


def run_guarded(Qd, Gd, off, kq, kg):
    """the C entry with its three outputs between guard regions, poisoned, twice (two fills): guards intact, every element
    written, both runs bit-identical.  Returns (pos, greater, ties) as numpy."""
    lib = _lib.load()
    N, D = Qd.shape
    M = Gd.shape[0]
    kqd = None if kq is None else kq.to(DEV)
    kgd = None if kg is None else kg.to(DEV)

    def call(o):
        _lib.check(lib.cxrk_retrieval_ranks(Qd.data_ptr(), max(Qd.stride(0), D), N, Gd.data_ptr(), max(Gd.stride(0), D), M, D, off,
                                            None if kqd is None else kqd.data_ptr(), None if kgd is None else kgd.data_ptr(),
                                            o["pos"].data_ptr(), o["greater"].data_ptr(), o["ties"].data_ptr(), K._stream()),
                   "cxrk_retrieval_ranks")

    spec = {"pos": Out((N,)), "greater": Out((N,), torch.int32), "ties": Out((N,), torch.int32)}
    o = MG.run_contract(call, spec, None, None, module=K, device=DEV, runs=("session", "alt"))
    return o["pos"].t.cpu().numpy(), o["greater"].t.cpu().numpy(), o["ties"].t.cpu().numpy()


def assert_equal_ranks(got, want, what=""):
    pos, greater, ties = got
    rpos, rgreater, rties = want[:3]
    assert np.array_equal(greater.astype(np.int64), rgreater), (what, "greater", np.flatnonzero(greater != rgreater)[:8])
    assert np.array_equal(ties.astype(np.int64), rties), (what, "ties", np.flatnonzero(ties != rties)[:8])
    assert np.array_equal(pos.astype(np.float64), rpos, equal_nan=True), (what, "pos", np.flatnonzero(pos != rpos)[:8])


@pytest.mark.parametrize("mode", ["pair", "mixed", "equal", "distinct"])
@pytest.mark.parametrize("N,M,D,off", SHAPES)
def test_exact_integer_cases(N, M, D, off, mode):
    """entries in {-3..3}: every dot product is an integer below 2^24, exact in fp32 in any order -> pos / greater / ties EQUAL the
    int64 reference.  Pitched inputs (ld = D + 3, NaN padding), guarded poisoned outputs."""
    Q, G = ints(N, M, D)
    kg = None if mode == "pair" else key_vector(mode, N, M, off)
    kq = None if kg is None else kg[off:off + N].contiguous()
    want = R.ranks_exact(Q, G, off, kq, kg)
    if M > 64 and mode in ("pair", "distinct"):
        assert (want[2] > 0).any() and (want[0] < 0).any(), "the construction is meant to give ties and negative positives"
    Qd, Gd = pitched(Q), pitched(G)
    assert Qd.stride(0) == D + 3
    got = run_guarded(Qd, Gd, off, kq, kg)
    assert_equal_ranks(got, want, f"{(N, M, D, off)} {mode}")
    assert bool(torch.isnan(Qd._base[:, D:]).all()) and bool(torch.isnan(Gd._base[:, D:]).all()), "pitch padding written"
    # the wrapper (its own outputs, contiguous or strided inputs alike) gives the same bits
    w = K.retrieval_ranks(Qd, Gd, off) if kg is None else K.retrieval_ranks(Qd, Gd, keys_q=kq.to(DEV), keys_g=kg.to(DEV))
    assert_equal_ranks(tuple(t.cpu().numpy() for t in w), want, "wrapper")
    assert w[0].dtype == torch.float32 and w[1].dtype == torch.int32 and w[2].dtype == torch.int32


@pytest.mark.parametrize("keyed", [False, True])
def test_duplicated_gallery_rows_tie_exactly_and_an_absent_key_has_no_positive(keyed):
    N, M, D, off = 130, 300, 128, 100
    Q, G = ints(N, M, D, seed=1)
    G[5] = G[off + 3]            # copies of positives, far away and in another column tile ...
    G[299] = G[off + 129]
    G[off + 4] = G[off + 3]      # ... and next to it
    kg = 50 + torch.arange(M, dtype=torch.int64) if keyed else None          # the copies carry keys of their own
    kq = kg[off:off + N].clone() if keyed else None
    if keyed:
        kq[7] = -999             # row 7's key is nowhere in the gallery
    want = R.ranks_exact(Q, G, off, kq, kg)
    assert want[2][3] >= 2 and want[2][129] >= 1
    got = run_guarded(pitched(Q), pitched(G), off, kq, kg)
    assert_equal_ranks(got, want)
    if keyed:
        assert got[0][7] == -np.inf and got[1][7] == M and got[2][7] == 0


def unit_rows(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True)).float()


@pytest.mark.parametrize("N,M,D,off", [(257, 257, 36, 0), (130, 300, 128, 100)])
def test_real_valued_cases_within_the_derived_rounding_bound(N, M, D, off):
    """unit-norm Gaussian rows.  u = 2^-24, gamma = D u / (1 - D u): an fp32 dot product of unit vectors is within gamma of the exact
    one, so only columns with |s64 - pos64| <= 2 gamma can fall on either side.  Every row is checked; at most 5 % of the rows may
    have such a column at all (asserted on the reference alone, before the GPU is touched; 0.4 % and 1.5 % with these seeds)."""
    Q, G = unit_rows(N, D, 11), unit_rows(M, D, 111)
    lo, hi, amb = R.bounds(Q, G, off)
    frac = float((amb > 0).mean())
    print(f"rows with an ambiguous column: {frac:.4f}")
    assert frac <= 0.05
    pos64 = R.ranks_float64(Q, G, off)[0]
    pos, greater, ties = run_guarded(pitched(Q), pitched(G), off, None, None)
    print(f"max |pos - pos64| = {np.abs(pos - pos64).max():.3e} (gamma {R.gamma(D):.3e}); rows off the lower bound: {int((greater != lo).sum())}")
    assert (np.abs(pos.astype(np.float64) - pos64) <= R.gamma(D)).all()
    assert (lo <= greater).all() and (greater <= hi).all(), np.flatnonzero((greater < lo) | (greater > hi))[:8]
    assert (0 <= ties).all() and (ties <= amb).all(), np.flatnonzero(ties > amb)[:8]


def test_result_does_not_depend_on_the_precision_mode():
    Q, G = unit_rows(130, 128, 11), unit_rows(300, 128, 111)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    kg = key_vector("mixed", 130, 300, 100).to(DEV)
    old = _lib.get_precision()
    outs = []
    try:
        for mode in ("fp32", "split_bf16"):
            _lib.set_precision(mode)
            outs.append(K.retrieval_ranks(Qd, Gd, 100) + K.retrieval_ranks(Qd, Gd, keys_q=kg[100:230].contiguous(), keys_g=kg))
    finally:
        _lib.set_precision(old)
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _nonfinite_case(case):
    N, M, D, off = 6, 140, 8, 130            # the queries' positives sit in the second column tile
    Q, G = ints(N, M, D, seed=2)
    kq = kg = None
    if case == "query":
        Q[2, 3] = float("nan")
    elif case == "positive":                 # a NaN gallery row that is the positive of row 1 (pair form)
        G[off + 1, 0] = float("nan")
    elif case == "positive-of-all":          # all keys equal: the NaN row is a positive of every row, no row has a non-positive
        kg = torch.full((M,), 3, dtype=torch.int64)
        kq = kg[:N].clone()
        G[5, 1] = float("nan")
    elif case == "positive-of-none":         # keyed, the NaN row's key matches no query
        kg = 10 + torch.arange(M, dtype=torch.int64)
        kq = kg[off:off + N].clone()
        G[3, 7] = float("nan")
    elif case == "one-of-two-positives":
        kg = 10 + torch.arange(M, dtype=torch.int64)
        kg[4] = kg[off + 2]
        kq = kg[off:off + N].clone()
        G[4, 2] = float("nan")
    elif case == "inf":                      # +Inf compares as a number: greater everywhere (positive entries: no Inf * 0)
        Q, G = Q.abs() + 1, G.abs() + 1
        G[0] = float("inf")
    return Q, G, off, kq, kg


@pytest.mark.parametrize("case", ["query", "positive", "positive-of-all", "positive-of-none", "one-of-two-positives", "inf"])
def test_non_finite_scores_never_give_a_plausible_rank(case):
    Q, G, off, kq, kg = _nonfinite_case(case)
    N, M = Q.shape[0], G.shape[0]
    with np.errstate(invalid="ignore"):
        want = R.ranks_float64(Q, G, off, kq, kg)[:3]
    got = run_guarded(pitched(Q), pitched(G), off, kq, kg)
    assert_equal_ranks(got, want, case)
    pos, greater, ties = got
    if case == "query":                      # the NaN row is flagged and keeps its NaN; rows that met no NaN score stay exact
        assert np.isnan(pos[2]) and greater[2] == -1 and ties[2] == -1
        assert (greater[[0, 1, 3, 4, 5]] >= 0).all() and np.isfinite(pos[[0, 1, 3, 4, 5]]).all()
    elif case == "positive":                 # its own row keeps the NaN; every other row met it in a non-positive column
        assert np.isnan(pos[1]) and np.isfinite(np.delete(pos, 1)).all() and (greater == -1).all() and (ties == -1).all()
    elif case == "positive-of-all":
        assert np.isnan(pos).all() and (greater == -1).all()
    elif case == "positive-of-none":
        assert np.isfinite(pos).all() and (greater == -1).all() and (ties == -1).all()
    elif case == "one-of-two-positives":
        assert np.isnan(pos[2]) and np.isfinite(np.delete(pos, 2)).all() and (greater == -1).all()
    else:
        assert np.isfinite(pos).all() and (greater >= 1).all() and (ties >= 0).all()


def test_argument_errors_raise_through_check():
    lib = _lib.load()
    Q, G = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV)
    k4, k6 = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.int64, device=DEV)
    pos = torch.zeros(4, device=DEV)
    gr, ti = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    #       0     1  2  3     4  5  6  7  8     9
    good = [P(Q), 8, 4, P(G), 8, 6, 8, 2, None, None, P(pos), P(gr), P(ti)]
    _lib.check(lib.cxrk_retrieval_ranks(*good, K._stream()), "cxrk_retrieval_ranks")
    keyed = list(good)
    keyed[8], keyed[9] = P(k4), P(k6)
    _lib.check(lib.cxrk_retrieval_ranks(*keyed, K._stream()), "cxrk_retrieval_ranks")
    bad = [(2, 0), (2, -1), (5, 0), (5, -3), (6, 0), (6, -8), (1, 7), (4, 7),        # N, M, D < 1; ld < D
           (7, -1), (7, 3)]                                                          # pair form: diag_off outside [0, M - N]
    for idx, v in bad:
        a = list(good)
        a[idx] = v
        assert lib.cxrk_retrieval_ranks(*a, K._stream()) == -1, (idx, v)
        with pytest.raises(ValueError, match="cxrk code -1"):
            _lib.check(lib.cxrk_retrieval_ranks(*a, K._stream()), "cxrk_retrieval_ranks")
    for kq, kg in ((P(k4), None), (None, P(k6))):                                    # exactly one key pointer
        a = list(good)
        a[8], a[9] = kq, kg
        with pytest.raises(ValueError, match="cxrk code -1"):
            _lib.check(lib.cxrk_retrieval_ranks(*a, K._stream()), "cxrk_retrieval_ranks")
    a = list(keyed)
    a[7] = 99                                                                        # keyed form: diag_off is not used
    _lib.check(lib.cxrk_retrieval_ranks(*a, K._stream()), "cxrk_retrieval_ranks")
    torch.cuda.synchronize()
    with pytest.raises(ValueError):                                                  # the wrapper
        K.retrieval_ranks(Q, G, 3)
    with pytest.raises(ValueError):
        K.retrieval_ranks(Q, G, keys_q=k4)
    with pytest.raises(ValueError):
        K.retrieval_ranks(Q, G, keys_q=k4, keys_g=k4)
    with pytest.raises(ValueError):
        K.retrieval_ranks(Q, G, keys_q=k4.int(), keys_g=k6)
    with pytest.raises(ValueError):
        K.retrieval_ranks(Q, G[:, :7])
    with pytest.raises(ValueError):
        K.retrieval_ranks(Q.cpu(), G)


def test_functional_normalize_equals_the_kernel_on_normalised_inputs():
    g = torch.Generator().manual_seed(3)
    q = (torch.randn(40, 96, generator=g) * 3 + 0.5).to(DEV)
    t = (torch.randn(40, 96, generator=g) * 0.2).to(DEV)
    want = K.retrieval_ranks(Fh.l2_normalize(q), Fh.l2_normalize(t))
    got = Fh.retrieval_ranks(q, t, normalize=True)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    raw = Fh.retrieval_ranks(q, t, normalize=False)
    assert not torch.equal(raw[0], got[0])
    keys = (torch.arange(40) // 2).to(DEV)
    want = K.retrieval_ranks(Fh.l2_normalize(q), Fh.l2_normalize(t), keys_q=keys, keys_g=keys)
    for a, b in zip(Fh.retrieval_ranks(q, t, keys=keys), want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        Fh.retrieval_ranks(q, t[:39])
    with pytest.raises(ValueError):
        Fh.retrieval_ranks(q, t, keys=keys.cpu())


# ---------------------------------------------------------------------------------------------------------------- evaluate_retrieval
B, L, IMG = 8, 16, 64
LABELS = [[1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]]


def _build(positives):
    """the tiny encoders of tests/test_multipos_dist_gpu.py::_build, with text dropout and augmentation switched on so that their
    counters exist and can be seen not to move"""
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256,
                        num_hidden_layers=2, max_position_embeddings=32)
    tm = CXRBertModel(cfg).eval()
    im = get_biovil_resnet(None).eval()
    syn.fill_module_(tm)
    syn.fill_module_(im)
    images = syn.synthetic_images(B, IMG, seed=3)
    ids, mask = syn.synthetic_tokens(B, L, vocab=300, seed=4, ragged=True)
    tm.enable_dropout_(seed=5)
    tm.train()
    tr = C.JointContrastiveTrainer(im.to(DEV), tm.to(DEV), lr=1e-4, temperature=0.07, positives=positives, augment=True, augment_seed=9)
    return tr, images, ids, mask, torch.tensor(LABELS, dtype=torch.float32)


def _metric_bounds(q, g, keys, ks):
    """what the metrics of one direction may be, from the per-row count bounds of the reference on the normalised fp32 embeddings:
    pessimistic rank in [1 + lo, 1 + hi]; equal bounds (no ambiguous column) make this an equality"""
    lo, hi, amb = R.bounds(q, g, 0, keys, keys)
    best = R.metrics(lo, np.zeros_like(lo), ks)
    worst = R.metrics(hi, np.zeros_like(hi), ks)
    return best, worst, int((amb > 0).sum())


@pytest.mark.parametrize("positives", [None, "labels"])
def test_evaluate_retrieval_on_tiny_encoders(positives):
    tr, images, ids, mask, labels = _build(positives)
    flat0 = tr.optimizer.flat_p.detach().clone()
    state0 = (tr.optimizer.steps, tr.text_model.dropout_state, tr.augment_state)
    flags0 = [m.training for model in (tr.image_model, tr.text_model) for m in model.modules()]
    assert tr.text_model.training and not tr.image_model.training
    ks = (1, 2, 5)
    batches = [(images[:5], ids[:5], mask[:5], labels[:5]), (images[5:], ids[5:], mask[5:], labels[5:])]     # uneven batches
    metrics, img, txt = tr.evaluate_retrieval(batches, ks=ks, return_embeddings=True)
    again = tr.evaluate_retrieval(batches, ks=ks)
    torch.cuda.synchronize()
    assert again == metrics                                       # no dropout, no augmentation: a pure function of the weights
    assert tuple(img.shape) == (B, 128) and tuple(txt.shape) == (B, 128) and img.is_cuda and txt.is_cuda
    # nothing of the training state moved
    assert torch.equal(tr.optimizer.flat_p, flat0)
    assert (tr.optimizer.steps, tr.text_model.dropout_state, tr.augment_state) == state0
    assert [m.training for model in (tr.image_model, tr.text_model) for m in model.modules()] == flags0
    # the metrics against the reference on the returned embeddings
    keys = C.keys_from_labels(labels) if positives else None
    ih, th = Fh.l2_normalize(img).cpu(), Fh.l2_normalize(txt).cpu()
    for name, q, g in (("i2t", ih, th), ("t2i", th, ih)):
        best, worst, n_amb = _metric_bounds(q, g, keys, ks)
        m = metrics[name]
        print(name, m, "rows with an ambiguous column:", n_amb)
        assert m["n"] == B and set(m) == {"R@1", "R@2", "R@5", "median_rank", "mean_rank", "n"}
        for k in ks:
            assert worst[f"R@{k}"] <= m[f"R@{k}"] <= best[f"R@{k}"]
        assert best["median_rank"] <= m["median_rank"] <= worst["median_rank"]
        assert best["mean_rank"] <= m["mean_rank"] <= worst["mean_rank"]
        assert all(math.isfinite(v) for v in m.values())
    if positives:
        plain = C.retrieval_metrics(img, txt, None, ks)
        assert plain != metrics                                   # the label groups are in use
