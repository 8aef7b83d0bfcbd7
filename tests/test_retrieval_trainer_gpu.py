"""`Trainer(joint_encoders={..., "retrieval": ...})`: `val` / `test` in joint mode also rank every report of the split against every
image.  Tiny encoders and synthetic joint loaders, as tests/test_joint_trainer_gpu.py: the added `Retrieval/*`
entries equal `JointContrastiveTrainer.evaluate_retrieval` on the same batches, they reach the writer under `val/` / `test/`, and a
trainer without the option returns and logs exactly what it did before."""
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.DataRetrieval import CHEXPERT_COMPETITION_CLASSES, create_prompts  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal import text as T  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet  # noqa: E402

DEV = "cuda"
CFG = dict(vocab_size=2048, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=32)
TODAY = {"Accuracy", "F1-macro score", "F1-weighted score", "AUROC-macro", "AUROC-weighted"}


def _trainer(tmp_path, tag, **joint):
    im = get_biovil_resnet(None).eval()
    tm = T.CXRBertModel(T.CXRBertConfig(**CFG)).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    engine = T.TextInferenceEngine(T.SyntheticTokenizer(CFG["vocab_size"]), tm.to(DEV))
    names = list(CHEXPERT_COMPETITION_CLASSES)
    return TR.Trainer(False, create_prompts(names), names, "standard", 1e-5, torch.device(DEV), TR.ScalarWriter(str(tmp_path / tag)),
                      bert_encoder=engine, joint_encoders={"image_model": im.to(DEV), "temperature": 0.07, **joint})


@pytest.mark.parametrize("positives", [None, "labels"])
def test_val_and_test_add_the_retrieval_metrics(tmp_path, positives):
    _, val, _ = TR.Trainer.synthetic_joint_loaders(8, 12, 8, 4, image_size=64, seq_len=16, vocab=CFG["vocab_size"], eval_batch_size=8)
    vb = list(val)                                            # 12 pairs in batches of 8 + 4
    assert sum(b[0].shape[0] for b in vb) == 12 and len(vb) == 2
    ks = (1, 3)
    tr = _trainer(tmp_path, "on", retrieval=ks, positives=positives)
    flat0 = tr.optimizer.flat_p.detach().clone()
    crit = torch.nn.BCEWithLogitsLoss()
    m = tr.val(vb, crit, 2, 2)
    want = tr._joint.evaluate_retrieval(vb, ks=ks)
    new = {f"Retrieval/{d} {k}" for d in ("i2t", "t2i") for k in ("R@1", "R@3", "median_rank", "mean_rank", "n")}
    assert new <= set(m) and set(m) - new <= TODAY
    for d in ("i2t", "t2i"):
        for k, v in want[d].items():
            assert m[f"Retrieval/{d} {k}"] == v, (d, k)
        assert m[f"Retrieval/{d} n"] == 12 and 1.0 <= m[f"Retrieval/{d} median_rank"] <= 12.0
        assert all(math.isfinite(m[f"Retrieval/{d} {k}"]) for k in want[d])
    logged = {t: v for t, v, s in tr.writer.scalars() if t.startswith("val/Retrieval/")}
    assert logged == {"val/" + k: float(m[k]) for k in new}
    assert all(s == 2 for t, _, s in tr.writer.scalars() if t.startswith("val/Retrieval/"))
    mt = tr.test(vb, None, 2, 2)
    assert all(mt[k] == m[k] for k in new)
    assert {t for t, _, _ in tr.writer.scalars() if t.startswith("test/Retrieval/")} == {"test/" + k for k in new}
    assert torch.equal(tr.optimizer.flat_p, flat0)


def test_without_the_option_nothing_is_added(tmp_path):
    _, val, _ = TR.Trainer.synthetic_joint_loaders(8, 8, 8, 4, image_size=64, seq_len=16, vocab=CFG["vocab_size"], eval_batch_size=8)
    vb = list(val)
    tr = _trainer(tmp_path, "off")
    assert tr._retrieval_ks is None
    m = tr.val(vb, torch.nn.BCEWithLogitsLoss(), 1, 1)
    assert set(m) <= TODAY and "Accuracy" in m
    assert not any("Retrieval" in t for t, _, _ in tr.writer.scalars())
