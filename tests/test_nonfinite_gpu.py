"""Non-finite propagation on the device ("Non-finite values"): a NaN / +Inf that reaches a kernel must reach its output, and
must not leak into rows, channels, segments or images the reference keeps finite.  A non-finite loss is the only alarm a diverged run
raises, so a kernel that turns a NaN into a number (fmaxf(NaN, 0) = 0) hides the divergence from everything behind it.
The cases, their float64 references and the two rules live in tests/nonfinite_ref.py; tests/test_nonfinite_host.py checks their
reference side without a GPU."""
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel  # noqa: E402
import nonfinite_ref as nf  # noqa: E402

DEV = "cuda"
PLANES_GEMM_CONV = [(n, v) for n, v in nf.ids() if n.startswith(("gemm_pl", "colsums", "conv_")) and ("_pl" in n or n == "colsums")]
OTHERS = [p for p in nf.ids() if p not in PLANES_GEMM_CONV]


def _run(name, value):
    c = nf.build(name, value)
    report = []
    try:
        nf.check_device(c, c.device(K), value, _cxr_lib.get_precision() == "split_bf16", report)
    finally:
        print(f"{name}[{value}]: " + ", ".join(report))


@pytest.mark.parametrize("name,value", OTHERS)
def test_kernel_keeps_nonfinite(name, value):
    _run(name, value)


@pytest.mark.parametrize("name,value", PLANES_GEMM_CONV)
def test_planes_gemm_conv_keeps_nonfinite(name, value, wide):
    """the planes GEMM / convolution launches under both tile policies (128x128-class tiles and the 256x256 LDS-DMA kernel)"""
    _run(name, value)


# ------------------------------------------------------------------------------------------------ model level
TEXT_CFG, POISON_ID = nf.TEXT_CFG, nf.POISON_ID


def _image_model():
    im = get_biovil_resnet(None)
    syn.fill_module_(im)
    return im.to(DEV)


def _images():
    clean, bad = nf.model_images(3)
    return clean.to(DEV), bad.to(DEV)


def test_image_model_eval_batchnorm_keeps_the_nan_in_its_image():
    """ResNet-50 at 64 px, eval BatchNorm, batch 3, NaN in one pixel of image 1: embedding row 1 is non-finite, rows 0 and 2 are bit
    for bit those of the clean batch (every ReLU on the way used to turn the NaN into 0: the tower swallowed its own divergence)."""
    im = _image_model().eval()
    clean, bad = _images()
    with torch.no_grad():
        e0, e1 = im(clean), im(bad)
    assert torch.isfinite(e0).all()
    assert not torch.isfinite(e1[1]).any(), e1[1]
    assert torch.equal(e1[0], e0[0]) and torch.equal(e1[2], e0[2])


def test_image_model_train_batchnorm_spreads_the_nan_over_the_batch():
    """train-mode BatchNorm: the batch statistics of the poisoned channel are NaN, so every image's embedding is non-finite"""
    im = _image_model().train()
    _, bad = _images()
    with torch.no_grad():
        e1 = im(bad)
    assert not torch.isfinite(e1).any(), e1


def _text_models():
    tm = CXRBertModel(CXRBertConfig(**TEXT_CFG)).eval()
    syn.fill_module_(tm)
    bad = CXRBertModel(CXRBertConfig(**TEXT_CFG)).eval()
    syn.fill_module_(bad)
    word = [p for k, p in bad.named_parameters() if k.endswith("word_embeddings.weight")]
    assert len(word) == 1
    with torch.no_grad():
        word[0][POISON_ID, nf.POISON_COL] = float("nan")
    return tm.to(DEV), bad.to(DEV)


def _tokens(B):
    ids, mask = nf.model_tokens(B)
    return ids.to(DEV), mask.to(DEV)


def test_text_model_keeps_the_nan_in_its_sequence():
    """2-layer CXR-BERT, NaN in the word-embedding row of a token only sequence 1 uses: only sequence 1's projection is non-finite"""
    tm, bad = _text_models()
    ids, mask = _tokens(3)
    with torch.no_grad():
        e0 = tm.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
        e1 = bad.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    assert torch.isfinite(e0).all()
    assert not torch.isfinite(e1[1]).any(), e1[1]
    assert torch.equal(e1[0], e0[0]) and torch.equal(e1[2], e0[2])


def test_joint_step_reports_a_poisoned_batch():
    """the alarm itself: `JointContrastiveTrainer.step` on a batch with one NaN pixel returns a non-finite loss"""
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    B = 4
    im = _image_model().eval()
    tm, _ = _text_models()
    _, images = nf.model_images(B)
    ids, mask = nf.model_tokens(B)
    tr = JointContrastiveTrainer(im, tm, lr=1e-4, temperature=0.07)
    loss = float(tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV)))
    assert not math.isfinite(loss), loss
