"""Host side of the retrieval evaluation, no GPU: the metric formulas and the tie rule from hand-written
(greater, ties) vectors, the NaN flag, `ks` validation, the `Trainer` option, `Trainer.val`'s returned keys with and without it,
and the two forms of the test reference against each other."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import retrieval_ref as R  # noqa: E402

from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import drivers  # noqa: E402


def test_metric_formulas_from_hand_written_counts():
    #          rank: 1   2      3 (1 + 1 + 1)  11       6 (1 + 0 + 5)  1
    greater = [0, 1, 1, 10, 0, 0]
    ties = [0, 0, 1, 0, 5, 0]
    m = C.rank_metrics(torch.tensor(greater, dtype=torch.int32), torch.tensor(ties, dtype=torch.int32), ks=(1, 5, 10))
    assert m["n"] == 6
    assert m["R@1"] == 2 / 6                       # pessimistic ranks 1, 2, 3, 11, 6, 1
    assert m["R@5"] == 4 / 6
    assert m["R@10"] == 5 / 6
    assert m["median_rank"] == 2.5                 # sorted 1 1 2 3 6 11
    assert m["mean_rank"] == (1 + 2 + 2.5 + 11 + 3.5 + 1) / 6     # ties count half in the mean
    assert m == R.metrics(greater, ties)
    odd = C.rank_metrics(np.array([4, 0, 2]), np.array([0, 0, 0]), ks=(3,))
    assert odd == {"R@3": 2 / 3, "median_rank": 3.0, "mean_rank": 3.0, "n": 3}


def test_collapsed_model_scores_zero_not_one_hundred_percent():
    """all embeddings equal: every non-positive column ties with the positive.  Pessimistic: rank M, R@k = 0, median M."""
    M = 50
    m = C.rank_metrics(torch.zeros(M, dtype=torch.int32), torch.full((M,), M - 1, dtype=torch.int32))
    assert m["R@1"] == 0.0 and m["R@5"] == 0.0 and m["R@10"] == 0.0
    assert m["median_rank"] == float(M)
    assert m["mean_rank"] == 1 + (M - 1) / 2
    assert m == R.metrics([0] * M, [M - 1] * M)


def test_nan_flag_makes_every_metric_of_the_direction_nan():
    m = C.rank_metrics(torch.tensor([0, -1, 3]), torch.tensor([0, -1, 0]), ks=(1, 2))
    assert m["n"] == 3
    for k in ("R@1", "R@2", "median_rank", "mean_rank"):
        assert math.isnan(m[k]), k
    r = R.metrics([0, -1, 3], [0, -1, 0], ks=(1, 2))
    assert all(math.isnan(r[k]) for k in ("R@1", "R@2", "median_rank", "mean_rank"))


@pytest.mark.parametrize("ks", [(), (0,), (-1, 5), (1.0,), (True,), (1, 1), "ab", 5, None])
def test_ks_are_validated(ks):
    with pytest.raises(ValueError):
        C.check_ks(ks)
    with pytest.raises(ValueError):
        C.rank_metrics(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), ks=ks)


def test_ks_accepts_lists_and_keeps_the_order():
    assert C.check_ks([10, 1]) == (10, 1)
    assert C.RETRIEVAL_KS == (1, 5, 10)
    with pytest.raises(ValueError):
        C.rank_metrics(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        C.rank_metrics(torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


def test_trainer_option_parsing():
    p = TR.Trainer._parse_retrieval
    assert p(None) is None and p(False) is None
    assert p(True) == (1, 5, 10)
    assert p((1, 3)) == (1, 3) and p([2]) == (2,) and p(7) == (7,)
    for bad in ((), (0,), (1, 1), ("1",), (2.5,)):
        with pytest.raises(ValueError):
            p(bad)


def test_driver_flag():
    ap = drivers.make_parser()
    assert drivers.retrieval_from_args(ap.parse_args(["zero-joint", "--joint"])) is None
    assert drivers.retrieval_from_args(ap.parse_args(["zero-joint", "--joint", "--retrieval"])) is True
    assert drivers.retrieval_from_args(ap.parse_args(["zero-joint", "--joint", "--retrieval", "1", "20"])) == (1, 20)
    with pytest.raises(SystemExit):
        drivers.main(["zero-joint", "--retrieval"])          # needs --joint


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step=None):
        self.rows.append((tag, float(value), step))


def _bare_trainer(result):
    """a Trainer with `_eval_loop` stubbed (no encoders, no GPU): what `val` / `test` do with its outcome is what is under test"""
    t = object.__new__(TR.Trainer)
    t.writer = _Writer()
    t._retrieval_result = None
    y_true = np.array([[1, 0], [0, 1], [1, 1], [0, 0]], dtype=np.float32)
    y_score = np.array([[0.9, 0.2], [0.1, 0.8], [0.7, 0.6], [0.2, 0.1]], dtype=np.float32)

    def loop(loader, criterion, epoch, log_tag):
        t._retrieval_result = result
        return y_true, (y_score > 0.5).astype(np.float32), y_score

    t._eval_loop = loop
    return t


TODAY = {"Accuracy", "F1-macro score", "F1-weighted score", "AUROC-macro", "AUROC-weighted"}


def test_val_and_test_without_the_option_return_exactly_todays_keys():
    pytest.importorskip("sklearn")
    t = _bare_trainer(None)
    m = t.val(None, None, 1, 1)
    assert set(m) == TODAY
    assert {r[0] for r in t.writer.rows} == {"val/" + k for k in TODAY}
    t.writer.rows.clear()
    assert set(t.test(None, None, 1, 1)) == TODAY
    assert {r[0] for r in t.writer.rows} == {"test/" + k for k in TODAY}


def test_val_with_the_option_adds_the_retrieval_scalars():
    pytest.importorskip("sklearn")
    res = {"i2t": C.rank_metrics(np.array([0, 1]), np.array([0, 0]), ks=(1, 5)), "t2i": C.rank_metrics(np.array([0, 0]), np.array([1, 0]), ks=(1, 5))}
    t = _bare_trainer(res)
    m = t.val(None, None, 3, 5)
    new = {f"Retrieval/{d} {k}" for d in ("i2t", "t2i") for k in ("R@1", "R@5", "median_rank", "mean_rank", "n")}
    assert set(m) == TODAY | new
    assert m["Retrieval/i2t R@1"] == 0.5 and m["Retrieval/t2i R@1"] == 0.5 and m["Retrieval/t2i median_rank"] == 1.5
    assert {r[0] for r in t.writer.rows} == {"val/" + k for k in TODAY | new}
    assert all(r[2] == 3 for r in t.writer.rows)
    assert t._retrieval_result is None             # consumed: a later evaluation without retrieval cannot report stale numbers


@pytest.mark.parametrize("N,M,D,off", [(5, 13, 7, 6), (9, 9, 36, 0)])
@pytest.mark.parametrize("keyed", [False, True])
def test_reference_exact_and_float64_forms_agree_on_integer_inputs(N, M, D, off, keyed):
    g = torch.Generator().manual_seed(5)
    Q = torch.randint(-3, 4, (N, D), generator=g).float()
    G = torch.randint(-3, 4, (M, D), generator=g).float()
    G[1] = G[0]                                                            # a duplicated gallery row: exact ties
    kg = torch.arange(M, dtype=torch.int64) // 2 if keyed else None         # pairs of columns share a key
    kq = kg[off:off + N].clone() if keyed else None
    if keyed:
        kq[0] = -77                                                        # a row without any positive
    a = R.ranks_exact(Q, G, off, kq, kg)
    b = R.ranks_float64(Q, G, off, kq, kg)
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x, y)
    if keyed:
        assert a[0][0] == -np.inf and a[1][0] == M and a[2][0] == 0
    lo, hi, amb = R.bounds(Q, G, off, kq, kg)
    assert np.array_equal(amb, a[2]) and np.array_equal(lo, a[1]) and np.array_equal(hi, a[1] + a[2])   # integer scores: ambiguous = tied


def test_reference_flags_nan_rows_only():
    Q = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    G = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [float("nan"), 0.0]])
    pos, gr, ti, _, _ = R.ranks_float64(Q, G, 0)
    assert list(gr) == [-1, -1, -1] and list(ti) == [-1, -1, -1] and list(pos) == [1.0, 1.0, 2.0]   # NaN row is a non-positive of all
    kq, kg = torch.tensor([1, 2, 9]), torch.tensor([1, 2, 3, 9])
    pos, gr, ti, _, _ = R.ranks_float64(Q, G, 0, kq, kg)
    assert np.isnan(pos[2]) and gr[2] == -1 and gr[0] == -1                  # row 2's positive is the NaN row
