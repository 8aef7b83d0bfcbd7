"""Host side of the kNN label probe, no GPU: the references against each other, `KNNBank` bookkeeping on the torch
emulation of the kernels (tests/cpu_kernels_topk.py), the `"knn"` option of `Trainer` and the driver flags, the width-mismatch
refusal, and `_eval_batches` calling nothing new without a bank."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_topk as E  # noqa: E402
import topk_ref as T  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import drivers  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(Fh, "K", E)
    return E


def _ints(N, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (N, D), generator=g).float(), torch.randint(-3, 4, (M, D), generator=g).float()


@pytest.mark.parametrize("N,M,D,k,off", [(9, 12, 7, 5, -1), (9, 12, 7, 20, 0), (9, 12, 7, 12, 3), (4, 4, 3, 1, 0), (1, 1, 1, 3, 0)])
def test_reference_and_emulation_agree_on_integer_inputs(N, M, D, k, off):
    Q, G = _ints(N, M, D, 1)
    G[M // 2] = G[0]                                  # a duplicated row: ties
    ws, wi = T.topk_exact(Q, G, k, off)
    fs, fi, _ = T.topk_float64(Q, G, k, off)
    assert np.array_equal(ws, fs) and np.array_equal(wi, fi)
    s, i = E.topk_neighbours(Q, G, k, off)
    assert s.dtype == torch.float32 and i.dtype == torch.int32
    assert np.array_equal(i.numpy(), wi) and np.array_equal(s.numpy().astype(np.float64), ws)
    cand = M - (off >= 0)
    assert (wi[:, min(cand, k):] == -1).all() and np.isneginf(ws[:, min(cand, k):]).all() and (wi[:, :min(cand, k)] >= 0).all()
    for r in range(N):
        real = wi[r][wi[r] >= 0].tolist()
        assert len(set(real)) == len(real) and (off < 0 or r + off not in real)
        assert list(zip((-ws[r]).tolist(), wi[r].tolist()))[:len(real)] == sorted(zip((-ws[r][:len(real)]).tolist(), real))


def test_reference_orders_nan_first_and_infinities_as_numbers():
    Q = torch.tensor([[1.0, 1.0], [float("nan"), 1.0]])
    G = torch.tensor([[1.0, 0.0], [float("-inf"), 1.0], [float("nan"), 1.0], [float("inf"), 1.0], [2.0, 0.0]])
    s, i, _ = T.topk_float64(Q, G, 6)
    assert i[0].tolist() == [2, 3, 4, 0, 1, -1] and np.isnan(s[0, 0]) and np.isposinf(s[0, 1]) and np.isneginf(s[0, 4])
    assert i[1].tolist() == [0, 1, 2, 3, 4, -1] and np.isnan(s[1, :5]).all() and np.isneginf(s[1, 5])
    es, ei = E.topk_neighbours(Q, G, 6)
    assert np.array_equal(ei.numpy(), i) and np.array_equal(es.numpy().astype(np.float64), s, equal_nan=True)
    lab = torch.tensor([[1.0], [0.0], [1.0], [0.0], [1.0]])
    assert np.isnan(T.vote_ref(s, i, lab, 1.0)).all() and bool(torch.isnan(E.knn_vote(es, ei, lab, 1.0)).all())


def test_vote_reference_by_hand():
    score = torch.tensor([[1.0, 0.0, float("-inf")], [float("-inf")] * 3])
    index = torch.tensor([[1, 0, -1], [-1, -1, -1]], dtype=torch.int32)
    labels = torch.tensor([[0.0, 1.0], [1.0, 1.0]])
    out = T.vote_ref(score, index, labels, 0.5)
    w = np.exp(-2.0)
    assert np.allclose(out[0], [1 / (1 + w), 1.0], rtol=1e-15) and np.isnan(out[1]).all()
    got = E.knn_vote(score, index, labels, 0.5).numpy()
    assert np.allclose(got[0], out[0], atol=1e-6) and np.isnan(got[1]).all()


def test_bank_bookkeeping(emulated):
    Q, G = _ints(6, 10, 5, 2)
    G = G + 0.25                                       # not normalised: the bank normalises
    labels = torch.randint(0, 2, (10, 3), generator=torch.Generator().manual_seed(3))          # int64 labels: stored as fp32
    bank = C.KNNBank()
    assert len(bank) == 0 and bank.width is None
    bank.add(G[:4], labels[:4])
    bank.add(G[4:], labels[4:])
    assert len(bank) == 10 and bank.width == 3 and bank.emb is None
    with pytest.raises(ValueError, match="finish"):
        bank.predict(Q, 3, 0.1)
    with pytest.raises(ValueError, match="width"):
        bank.add(G[:2, :4], labels[:2])
    with pytest.raises(ValueError, match="width"):
        bank.add(G[:2], labels[:2, :2])
    with pytest.raises(ValueError, match="expected"):
        bank.add(G[:2], labels[:3])
    assert bank.finish() is bank and len(bank) == 10 and bank.width == 3
    gh = G / G.norm(dim=1, keepdim=True)
    assert torch.allclose(bank.emb, gh, atol=1e-6) and bank.labels.dtype == torch.float32 and torch.equal(bank.labels, labels.float())
    with pytest.raises(ValueError, match="finished"):
        bank.add(G[:2], labels[:2])
    with pytest.raises(ValueError, match="finished"):
        bank.finish()
    qh = E.l2norm_fwd(Q + 0.5)[0]
    s, i = E.topk_neighbours(qh, bank.emb, 4)
    want = T.vote_ref(s, i, bank.labels, 0.1)
    got = bank.predict(Q + 0.5, 4, 0.1)
    assert tuple(got.shape) == (6, 3) and np.abs(got.numpy() - want).max() < 1e-5
    assert np.abs(bank.predict(3 * (Q + 0.5), 4, 0.1).numpy() - want).max() < 1e-5              # queries are normalised too
    for k, t in ((0, 0.1), (65, 0.1), (True, 0.1), (3, 0.0), (3, float("inf")), (3, "x")):
        with pytest.raises(ValueError):
            bank.predict(Q, k, t)
    with pytest.raises(ValueError, match="expected embeddings"):
        bank.predict(Q[:, :4], 3, 0.1)
    with pytest.raises(ValueError, match="empty"):
        C.KNNBank().finish()


def test_trainer_option_parsing():
    p = TR.knn_options
    assert p(None) is None and p({}) is None and p({"knn": None}) is None and p({"knn": False}) is None
    assert p({"knn": True}) == {"k": 20, "temperature": 0.07, "bank_batches": 8}
    assert p({"knn": {"k": 5}}) == {"k": 5, "temperature": 0.07, "bank_batches": 8}
    assert p({"knn": {"temperature": 1, "bank_batches": 2}}) == {"k": 20, "temperature": 1.0, "bank_batches": 2}
    for bad in (3, "on", {"k": 0}, {"k": 65}, {"k": 2.0}, {"k": True}, {"temperature": 0}, {"temperature": -1.0}, {"bank_batches": 0},
                {"bank_batches": 1.5}, {"neighbours": 3}):
        with pytest.raises(ValueError):
            p({"knn": bad})
    im = object()
    step, own = TR.joint_options({"image_model": im, "knn": {"k": 5}})
    assert "knn" not in step and own == {"image_model": im, "retrieval": None, "ewc_batches": None}   # `Trainer` reads it itself
    assert "knn" in TR.JOINT_PROBE_KEYS and "knn" not in TR.JOINT_STEP_KEYS
    with pytest.raises(ValueError, match="joint mode"):
        TR.joint_options({"knn": True})
    with pytest.raises(ValueError, match="'k'|k must"):
        TR.joint_options({"image_model": im, "knn": {"k": 99}})
    with pytest.raises(ValueError, match="'knn'"):                         # the list of valid keys names it
        TR.joint_options({"image_model": im, "kn": True})


def test_driver_flags():
    ap = drivers.make_parser()
    je = lambda argv: drivers.joint_encoders_from_args(ap.parse_args(argv), object())  # noqa: E731
    assert "knn" not in je(["zero-joint", "--joint"])                      # the key exists only when the flag is given
    assert je(["zero-joint", "--joint", "--knn"])["knn"] is True
    assert je(["class-inc", "--joint", "--knn", "5"])["knn"] == {"k": 5}
    assert je(["data-inc", "--joint", "--knn", "--knn-temperature", "0.1", "--knn-bank-batches", "3"])["knn"] == {
        "temperature": 0.1, "bank_batches": 3}
    assert TR.knn_options(je(["data-inc", "--joint", "--knn", "7", "--knn-bank-batches", "3"])) == {"k": 7, "temperature": 0.07, "bank_batches": 3}
    for argv in (["zero-joint", "--knn"], ["class-inc", "--knn", "5"], ["data-inc", "--knn-temperature", "0.1"],
                 ["zero-joint", "--joint", "--knn-bank-batches", "2"]):
        with pytest.raises(SystemExit):
            drivers.main(argv)                                             # needs --joint / needs --knn
    calls = []

    class _T:
        def knn_bank(self, loaders):
            calls.append(loaders)

    drivers.knn_bank(_T(), ap.parse_args(["zero-joint", "--joint"]), "loader")
    assert calls == []
    drivers.knn_bank(_T(), ap.parse_args(["zero-joint", "--joint", "--knn"]), "loader")
    assert calls == ["loader"]


class _Joint:
    positives = None
    ema_eval = False

    def pair_keys(self, *a, **k):
        return None

    def _dist_group(self):
        return None


def _eval_trainer(monkeypatch, C_):
    """a Trainer in joint mode whose image model is the identity and whose class-prompt head is stubbed: `_eval_batches` itself runs"""
    monkeypatch.setattr(TR, "TRAIN_LOGIT_DIFF", False)
    t = object.__new__(TR.Trainer)
    t.device, t.writer, t.world, t.rank = torch.device("cpu"), None, 1, 0
    t._joint, t.image_model, t.image_adapter, t.text_adapter = _Joint(), (lambda x: x), None, None
    t._retrieval_ks, t._retrieval_result, t._knn, t._knn_bank, t._knn_result = None, None, None, None, None
    t.class_names = ["c%d" % c for c in range(C_)]
    t.bert_encoder = type("E", (), {"model": object()})()
    t._logits_and_loss = lambda e, labels, names, crit, use_grad: (None, None, torch.zeros(e.shape[0], 2 * C_))
    return t


def _loader(labels):
    g = torch.Generator().manual_seed(7)
    protos = torch.randn(2, 6, generator=g)
    which = torch.tensor([0, 1, 1, 0, 1, 0])
    imgs = protos[which] * torch.tensor([1.0, 2.0, 0.5, 3.0, 1.0, 1.5])[:, None]
    ids = torch.zeros(6, 4, dtype=torch.int64)
    return [(imgs[:4], ids[:4], ids[:4], labels[which][:4]), (imgs[4:], ids[4:], ids[4:], labels[which][4:])]


def test_eval_batches_calls_nothing_new_without_a_bank(monkeypatch, emulated):
    pytest.importorskip("sklearn")
    calls = []
    for name in ("topk_neighbours", "knn_vote"):
        monkeypatch.setattr(E, name, lambda *a, _f=getattr(E, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    rows = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    t = _eval_trainer(monkeypatch, 3)
    y_true, _, _ = t._eval_batches(_loader(rows), None, 1, None)
    assert calls == [] and t._knn_result is None and y_true.shape == (6, 3)
    m = t.val(_loader(rows), None, 1, 1)
    assert calls == [] and not any(k.startswith("kNN/") for k in m)
    with pytest.raises(ValueError, match="'knn'"):
        t.knn_bank(_loader(rows))
    # with the option and a bank, the vote runs once per batch on the embeddings the loop already has
    t._knn = TR.knn_options({"knn": {"k": 2, "temperature": 0.1, "bank_batches": 1}})
    assert t.knn_bank(_loader(rows)) == 4 and calls == []                  # one batch of four; building the bank runs no search
    m = t.val(_loader(rows), None, 1, 1)
    assert calls == ["topk_neighbours", "knn_vote"] * 2
    assert m["kNN/Accuracy"] == 1.0 and m["kNN/F1-macro"] == 1.0 and m["kNN/AUROC-macro"] == 1.0 and m["kNN/AUROC-weighted"] == 1.0
    assert t._knn_result is None                                           # consumed


def test_width_mismatch_names_both_widths(monkeypatch, emulated):
    t = _eval_trainer(monkeypatch, 2)
    t._knn = TR.knn_options({"knn": {"k": 2}})
    t.knn_bank(_loader(torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])))
    with pytest.raises(ValueError, match=r"the bank's labels are 3 wide but the evaluation labels 2"):
        t._eval_batches(_loader(torch.tensor([[1.0, 0.0], [0.0, 1.0]])), None, 1, None)
