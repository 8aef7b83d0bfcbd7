"""The micro-batched joint step (`JointContrastiveTrainer(micro_batch=n)`) with the REAL HIP kernels, at the sizes of
tests/test_dist_gpu.py (ResNet-50 at 64 px, the 2-layer 128-wide CXR-BERT, 16 ragged tokens, `syn.fill_module_` weights).

A chunked step must be the unchunked step on the same batch up to fp32 summation order: the difference is of the kind a row-sharded
data-parallel step has against the single process (partial sums over row ranges, added in another order), so the bounds are those
of tests/test_dist_gpu.py: loss within 1e-5 relative, > 99 % of a strided sample of the Adam update within 2e-6 + 1e-2 |update|."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.augment import DEFAULT_SPEC_ARGS, AugmentCall, AugmentSpec  # noqa: E402

B, L, TAU, IMG = 8, 16, 0.07, 64
CFG = dict(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=32)
# rows 2 and 3 share a label vector: with micro_batch=3 (chunks 0-2, 3-5, 6-7) the positives group straddles a chunk boundary
LABELS = torch.tensor([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1],
                       [1, 0, 1, 0, 0]], dtype=torch.float32)


def _models(dropout_seed=None):
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    tm = CXRBertModel(CXRBertConfig(**CFG)).eval()
    im = get_biovil_resnet(None).eval()
    syn.fill_module_(tm)
    syn.fill_module_(im)
    if dropout_seed is not None:
        tm.enable_dropout_(seed=dropout_seed)
        tm.train()
    return im.to("cuda"), tm.to("cuda")


def _joint(dropout_seed=None, **kw):
    im, tm = _models(dropout_seed)
    return C.JointContrastiveTrainer(im, tm, lr=1e-4, temperature=TAU, **kw)


def _batch(n=B, size=IMG):
    images = syn.synthetic_images(n, size, seed=3)
    ids, mask = syn.synthetic_tokens(n, L, vocab=300, seed=4, ragged=True)
    return images.to("cuda"), ids.to("cuda"), mask.to("cuda")


def _probe(tr):
    """tests/test_dist_gpu.py's fingerprint of the replica: a strided sample of the flat parameter buffer"""
    p = tr.optimizer.flat_p
    return p[:: max(1, p.numel() // 4096)].detach().cpu().numpy()


def _same_step(chunked, plain, before, what):
    """the criteria tests/test_dist_gpu.py applies to a row-sharded step against the single process; `chunked` / `plain` =
    (loss, probe after the step), `before` = the probe of an untouched trainer"""
    (loss_c, after_c), (loss_p, after_p) = chunked, plain
    rel = abs(loss_c - loss_p) / abs(loss_p)
    upd_ref, upd = after_p - before, after_c - before
    agree = float(np.mean(np.abs(upd_ref - upd) <= 2e-6 + 1e-2 * np.abs(upd_ref)))
    print(f"{what}: loss {loss_c!r} (chunked) / {loss_p!r} (unchunked), relative difference {rel:.3e}; update agreement {agree:.5f}")
    assert rel < 1e-5, (loss_c, loss_p)
    assert agree > 0.99, agree


def test_chunked_step_is_the_unchunked_step():
    images, ids, mask = _batch()
    before = _probe(_joint())
    res = []
    for mb in (3, None):
        tr = _joint(micro_batch=mb)
        loss = tr.step(images, ids, mask)
        torch.cuda.synchronize()
        res.append((float(loss.item()), _probe(tr)))
    assert np.abs(res[1][1] - before).max() > 0.5e-4            # Adam's first step moved the weights by ~lr
    _same_step(res[0], res[1], before, "micro_batch=3 at B=8")


def test_off_means_off():
    images, ids, mask = _batch()
    res = []
    for kw in ({}, {"micro_batch": None}, {"micro_batch": 8}, {"micro_batch": 100}):
        tr = _joint(**kw)
        loss = tr.step(images, ids, mask)
        res.append((loss.clone(), tr.optimizer.flat_p.detach().clone()))
    for loss, flat in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(flat, res[0][1])


def test_save_free_forward_is_the_saving_forward():
    """the forward of pass 1 against the forward of pass 3 on a 3-row chunk, augmentation and text dropout on, counters pinned"""
    im, tm = _models(dropout_seed=11)
    images, ids, mask = _batch(3)
    call = AugmentCall(AugmentSpec(**DEFAULT_SPEC_ARGS), 77, 5, 3)
    im.augment_call = call
    plain = im(images)
    im.augment_call = None
    unaugmented = im(images)                                     # the comparison below must see the augmentation's effect
    im.augment_call, im.save_free = call, True
    free = im(images)
    im.augment_call, im.save_free = None, False
    assert plain.requires_grad and plain.grad_fn is not None and not free.requires_grad
    assert not torch.equal(plain, unaugmented)
    assert torch.equal(plain, free)

    tm.dropout_row_offset = 3
    tm.dropout_state = (11, 7)
    plain = tm.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    assert tm.dropout_state == (11, 8)
    tm.eval()
    undropped = tm.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    tm.train()
    tm.dropout_state = (11, 7)
    version = tm._dropout_version
    tm.save_free = True
    free = tm.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    tm.save_free = False
    assert tm.dropout_state == (11, 7) and tm._dropout_version == version          # the save-free call advances nothing
    assert plain.requires_grad and plain.grad_fn is not None and not free.requires_grad
    assert not torch.equal(plain, undropped)
    assert torch.equal(plain, free)


@pytest.mark.parametrize("loss, spec", [("sigmoid", AugmentSpec()), ("infonce", AugmentSpec()), ("infonce", AugmentSpec(**DEFAULT_SPEC_ARGS))],
                         ids=["sigmoid", "infonce", "infonce-affine"])
def test_options_compose(loss, spec):
    images, ids, mask = _batch()
    kw = dict(loss=loss, learn_temperature=True, positives="labels", augment=spec, augment_seed=123)
    assert C.keys_from_labels(LABELS)[2] == C.keys_from_labels(LABELS)[3]
    tr0 = _joint(dropout_seed=9, **kw)
    before = _probe(tr0)
    theta0 = tr0.logit_scale.detach().clone()
    bias0 = tr0.logit_bias.detach().clone() if loss == "sigmoid" else None
    res = []
    for mb in (3, None):
        tr = _joint(dropout_seed=9, micro_batch=mb, **kw)
        assert tr.text_model.dropout_state == (9, 0) and tr.augment_state == (123, 0)
        out = tr.step(images, ids, mask, labels=LABELS)
        torch.cuda.synchronize()
        assert tr.text_model.dropout_state == (9, 1) and tr.augment_state == (123, 1)      # both counters advanced once
        assert not torch.equal(tr.logit_scale.detach(), theta0)
        if loss == "sigmoid":
            assert not torch.equal(tr.logit_bias.detach(), bias0)
        assert tr.image_model.augment_call is None and not tr.image_model.save_free and not tr.text_model.save_free
        res.append((float(out.item()), _probe(tr)))
    assert math.isfinite(res[0][0])
    _same_step(res[0], res[1], before, f"{loss}, learnable theta, label positives, augment, dropout; micro_batch=3 at B=8")


def test_memory_follows_the_chunk():
    size = 128
    tr = _joint(micro_batch=4)
    big, small = _batch(16, size), _batch(8, size)
    extra = sum(t[8:].numel() * t.element_size() for t in big)      # the 8 additional input rows: images, ids, mask
    tr.step(*big)                                                   # untimed warm-up: optimiser state, workspaces, caches

    def peak(batch):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        tr.step(*batch)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    p8, p16 = peak(small), peak(big)
    tr.micro_batch = None
    p16_plain = peak(big)
    print(f"peak bytes at {size} px: micro_batch=4 B=8 {p8}, B=16 {p16} (difference {p16 - p8}, inputs {extra}); unchunked B=16 {p16_plain}")
    assert p16 - p8 <= extra + 4 * 2 ** 20, (p8, p16, extra)
    assert p16 < p16_plain, (p16, p16_plain)


@pytest.mark.parametrize("bad", [0, -1, True, 2.5])
def test_bad_micro_batch_is_refused_at_construction(bad):
    im, tm = _models()
    with pytest.raises(ValueError, match="micro_batch"):
        C.JointContrastiveTrainer(im, tm, micro_batch=bad)


def test_train_mode_batchnorm_is_refused():
    images, ids, mask = _batch(4)
    tr = _joint(micro_batch=2)
    tr.image_model.train()
    flat = tr.optimizer.flat_p.detach().clone()
    with pytest.raises(ValueError, match=r"(?s)micro_batch.*BatchNorm"):
        tr.step(images, ids, mask)
    assert torch.equal(tr.optimizer.flat_p, flat)
    tr.micro_batch = None                                           # the unchunked step trains on batch statistics as before
    ref = _joint()
    ref.image_model.train()
    a, b = tr.step(images, ids, mask), ref.step(images, ids, mask)
    assert torch.equal(a, b) and torch.equal(tr.optimizer.flat_p, ref.optimizer.flat_p)


def test_trainer_surface_against_the_oracle(tmp_path):
    """`Trainer(joint_encoders={..., "micro_batch": 2})` at B = 4 for two steps: each logged loss against the CPU oracle's step on the
    same batches, at the bound tests/test_joint_trainer_gpu.py uses for the Adam trajectory"""
    from incremental_multimodal_medical_learning_ii_amd import Trainer as TR
    from incremental_multimodal_medical_learning_ii_amd.DataRetrieval import CHEXPERT_COMPETITION_CLASSES, create_prompts
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal import text as T
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from oracle import ref_step
    cfg = dict(CFG, vocab_size=2048)
    lr = 1e-5
    im = get_biovil_resnet(None).eval()
    tm = T.CXRBertModel(T.CXRBertConfig(**cfg)).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    ip = {k: v.detach().clone() for k, v in im.state_dict().items()}
    tp = {k: v.detach().clone() for k, v in tm.state_dict().items()}
    engine = T.TextInferenceEngine(T.SyntheticTokenizer(cfg["vocab_size"]), tm.to("cuda"))
    names = list(CHEXPERT_COMPETITION_CLASSES)
    tr = TR.Trainer(False, create_prompts(names), names, "standard", lr, torch.device("cuda"), TR.ScalarWriter(str(tmp_path / "mb")),
                    bert_encoder=engine, joint_encoders={"image_model": im.to("cuda"), "temperature": TAU, "micro_batch": 2})
    assert tr._joint.micro_batch == 2
    leaves = []
    for d in (ip, tp):
        for k, v in d.items():
            if v.dtype == torch.float32 and "running" not in k and not k.startswith("cls.predictions") and ".fc." not in k:
                leaves.append(v.requires_grad_(True))
    opt = torch.optim.Adam(leaves, lr=lr)
    train, _, _ = TR.Trainer.synthetic_joint_loaders(8, 8, 8, 4, image_size=64, seq_len=16, vocab=cfg["vocab_size"], eval_batch_size=8)
    batches = list(train)
    assert len(batches) == 2 and batches[0][0].shape == (4, 3, 64, 64)
    tr.train(batches, torch.nn.BCEWithLogitsLoss(), 1, None, None, part=1, epochs=1, actual_task=1)
    ref = [float(ref_step.joint_step(ip, tp, images, ids, mask, TAU, opt, n_layers=cfg["num_hidden_layers"],
                                     n_heads=cfg["num_attention_heads"])) for images, ids, mask, _ in batches]
    got = [v for _, v, _ in tr.writer.scalars("train/Loss")]
    print("train/Loss", got, "oracle", ref)
    assert len(got) == 2 and np.allclose(got, ref, rtol=1e-3), (got, ref)


def test_driver_runs_micro_batched(tmp_path):
    from incremental_multimodal_medical_learning_ii_amd import Trainer as TR
    from incremental_multimodal_medical_learning_ii_amd import drivers
    args = drivers.make_parser().parse_args(["zero-joint", "--joint", "--micro-batch", "2", "--small-text", "--batch-size", "4", "--n-train", "8",
                                             "--n-eval", "8", "--image-size", "64", "--seq-len", "16", "--epochs", "1", "--log-root", str(tmp_path)])
    try:
        tr, m = drivers.zero_joint_bounds(args)
    finally:
        TR.IMAGE_MODEL = TR.TEXT_MODEL = True
    assert tr._joint.micro_batch == 2 and m is not None
    with open(os.path.join(tr.writer.log_dir, "scalars.jsonl")) as f:
        rows = [json.loads(line) for line in f]
    losses = [r["value"] for r in rows if r["tag"] == "train/Loss"]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), losses
