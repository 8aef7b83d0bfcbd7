"""The kNN label probe in the trainers with the REAL kernels, on tiny encoders as tests/test_retrieval_trainer_gpu.py
builds them.  The bank's labels are a known function of the images -- two distinct image patterns with distinct label rows -- so
queries drawn from the same patterns must be labelled exactly: `JointContrastiveTrainer.evaluate_knn` and `Trainer.val` / `test`
with `"knn"` report kNN/Accuracy == 1.0, the added keys reach the dict and the writer, no training state moves, `"ema_eval"` makes
bank and queries read the parameter average, and a trainer without the option returns what it did before."""
import pytest
import torch

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.DataRetrieval import CHEXPERT_COMPETITION_CLASSES, create_prompts  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal import text as T  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet  # noqa: E402

DEV = "cuda"
CFG = dict(vocab_size=2048, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=32)
TODAY = {"Accuracy", "F1-macro score", "F1-weighted score", "AUROC-macro", "AUROC-weighted"}
KNN_KEYS = {"kNN/Accuracy", "kNN/F1-macro", "kNN/AUROC-macro", "kNN/AUROC-weighted"}
ROWS = torch.tensor([[1, 0, 0, 1, 1], [0, 1, 1, 0, 0]], dtype=torch.float32)       # the label rows of the two patterns
KNN = {"k": 3, "temperature": 0.07, "bank_batches": 2}                               # k below the 4 copies of a pattern in the bank


def _models():
    im = get_biovil_resnet(None).eval()
    tm = T.CXRBertModel(T.CXRBertConfig(**CFG)).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    return im.to(DEV), tm.to(DEV)


def _batches(which):
    """batches of 4 (images, input_ids, attention_mask, labels): image i is pattern which[i], its labels ROWS[which[i]]"""
    pats = syn.synthetic_images(2, 64, seed=3)
    out = []
    for n in range(0, len(which), 4):
        w = torch.tensor(which[n:n + 4])
        ids, mask = syn.synthetic_tokens(len(w), 16, vocab=CFG["vocab_size"], seed=4 + n, ragged=True)
        out.append((pats[w].contiguous(), ids, mask, ROWS[w].contiguous()))
    return out


BANK = _batches([0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0])        # the third batch lies beyond bank_batches = 2
EVAL = _batches([1, 1, 0, 1, 0, 0, 1, 0])


def _trainer(tmp_path, tag, **joint):
    im, tm = _models()
    engine = T.TextInferenceEngine(T.SyntheticTokenizer(CFG["vocab_size"]), tm)
    names = list(CHEXPERT_COMPETITION_CLASSES)
    return TR.Trainer(False, create_prompts(names), names, "standard", 1e-4, torch.device(DEV), TR.ScalarWriter(str(tmp_path / tag)),
                      bert_encoder=engine, joint_encoders={"image_model": im, "temperature": 0.07, **joint})


def _state(j):
    return (j.optimizer.steps, j.text_model.dropout_state if getattr(j.text_model, "dropout_enabled", False) else None, j.augment_state,
            j.mlm_state, None if j.ema is None else j.ema.updates)


def test_evaluate_knn_labels_the_patterns_and_moves_no_state():
    im, tm = _models()
    tm.enable_dropout_(seed=5)
    tm.train()
    tr = C.JointContrastiveTrainer(im, tm, lr=1e-4, temperature=0.07, augment=True, augment_seed=9, mlm_weight=0.5, mlm_seed=3,
                                   ema_decay=0.9)
    images, ids, mask, _ = BANK[0]
    tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    flat0, avg0, state0 = tr.optimizer.flat_p.detach().clone(), tr.ema.avg.detach().clone(), _state(tr)
    flags0 = [m.training for model in (tr.image_model, tr.text_model) for m in model.modules()]
    assert state0[0] == 1 and state0[1] is not None and state0[2] is not None and state0[3] is not None and state0[4] == 1
    out = tr.evaluate_knn(BANK, EVAL, k=3, temperature=0.07, max_bank_batches=2)
    torch.cuda.synchronize()
    scores, labels = out["scores"], out["labels"]
    assert scores.is_cuda and labels.is_cuda and tuple(scores.shape) == (8, 5) and tuple(labels.shape) == (8, 5)
    assert torch.equal(labels.cpu(), torch.cat([b[3] for b in EVAL]))
    assert torch.equal((scores > 0.5).float(), labels), scores                  # kNN/Accuracy == 1.0
    assert torch.equal(scores, labels)                                          # three neighbours, all copies of the query's pattern
    assert torch.equal(tr.optimizer.flat_p, flat0) and torch.equal(tr.ema.avg, avg0) and _state(tr) == state0
    assert [m.training for model in (tr.image_model, tr.text_model) for m in model.modules()] == flags0
    again = tr.evaluate_knn(BANK, EVAL, k=3, temperature=0.07, max_bank_batches=2)
    assert torch.equal(again["scores"], scores)                                 # a pure function of the weights
    with pytest.raises(ValueError, match="5 wide but the evaluation labels 3"):
        tr.evaluate_knn(BANK, [(b[0], b[3][:, :3].contiguous()) for b in EVAL], k=3)
    with pytest.raises(ValueError, match="k must be"):
        tr.evaluate_knn(BANK, EVAL, k=65)


def test_val_and_test_add_the_knn_metrics(tmp_path):
    tr = _trainer(tmp_path, "on", knn=KNN, augment=True, augment_seed=9)
    crit = torch.nn.BCEWithLogitsLoss()
    before = tr.val(EVAL, crit, 1, 1)
    assert set(before) <= TODAY and tr._knn_bank is None                        # before knn_bank: as without the option
    flat0, state0 = tr._joint.optimizer.flat_p.detach().clone(), _state(tr._joint)
    assert tr.knn_bank(BANK) == 8                                               # two batches of four
    m = tr.val(EVAL, crit, 2, 2)
    assert KNN_KEYS <= set(m) and set(m) - KNN_KEYS <= TODAY
    assert m["kNN/Accuracy"] == 1.0 and m["kNN/F1-macro"] == 1.0 and m["kNN/AUROC-macro"] == 1.0 and m["kNN/AUROC-weighted"] == 1.0
    assert all(m[k] == before[k] for k in before)                               # the class-prompt metrics are what they were
    logged = {t: (v, s) for t, v, s in tr.writer.scalars() if t.startswith("val/kNN/")}
    assert logged == {"val/" + k: (float(m[k]), 2) for k in KNN_KEYS}
    mt = tr.test(EVAL, None, 2, 2)
    assert all(mt[k] == m[k] for k in KNN_KEYS)
    assert {t for t, _, _ in tr.writer.scalars() if t.startswith("test/kNN/")} == {"test/" + k for k in KNN_KEYS}
    assert torch.equal(tr._joint.optimizer.flat_p, flat0) and _state(tr._joint) == state0
    assert tr.knn_bank([BANK, EVAL]) == 16                                      # a sequence of loaders; it replaces the bank
    with pytest.raises(ValueError, match="5 wide but the evaluation labels 3"):
        tr.val([b[:3] + (b[3][:, :3].contiguous(),) for b in EVAL], crit, 3, 3)


def test_ema_eval_makes_bank_and_queries_read_the_average(tmp_path):
    tr = _trainer(tmp_path, "ema", knn=KNN, ema_decay=0.5, ema_warmup=False, ema_eval=True)
    j = tr._joint
    images, ids, mask, _ = BANK[0]
    for _ in range(2):
        j.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    imgs = torch.cat([b[0] for b in BANK[:2]]).to(DEV)
    with torch.no_grad():
        raw = K.l2norm_fwd(tr.image_model(imgs))[0]
        with j.averaged():
            avg = K.l2norm_fwd(tr.image_model(imgs))[0]
    assert not torch.equal(raw, avg)
    tr.knn_bank(BANK)
    assert torch.equal(tr._knn_bank.emb, avg) and not j.ema.swapped
    seen = []
    predict = tr._knn_bank.predict
    tr._knn_bank.predict = lambda emb, k, t: (seen.append(emb.clone()), predict(emb, k, t))[1]
    m = tr.val(BANK[:2], torch.nn.BCEWithLogitsLoss(), 1, 1)
    with torch.no_grad(), j.averaged():
        want = [tr.image_model(b[0].to(DEV)) for b in BANK[:2]]
    assert len(seen) == 2 and all(torch.equal(a, b) for a, b in zip(seen, want))
    assert m["kNN/Accuracy"] == 1.0 and not j.ema.swapped


def test_without_the_option_nothing_is_added(tmp_path, monkeypatch):
    calls = []
    for name in ("topk_neighbours", "knn_vote"):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **k: calls.append(_n))
    tr = _trainer(tmp_path, "off")
    assert tr._knn is None and tr._knn_bank is None
    m = tr.val(EVAL, torch.nn.BCEWithLogitsLoss(), 1, 1)
    assert set(m) <= TODAY and "Accuracy" in m and calls == []
    assert not any("kNN" in t for t, _, _ in tr.writer.scalars())
    with pytest.raises(ValueError, match="'knn'"):
        tr.knn_bank(BANK)
