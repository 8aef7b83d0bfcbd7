"""The reference side of every non-finite propagation case (tests/nonfinite_ref.py), without a GPU: the float64 torch reference of
each case has some non-finite and some finite element, and its non-finite elements are the index set the contract states (DESIGN.md,
"Non-finite values").  This pins the fixtures and the torch facts the contract rests on (relu, max_pool2d, F.normalize, torch.max and
min / max keep a NaN; threshold / dropout / key masks select) where no device is present."""
import pytest

import nonfinite_ref as nf


@pytest.mark.parametrize("name,value", nf.ids())
def test_reference_side(name, value):
    nf.check_reference(nf.build(name, value), value)


def test_case_list_covers_every_family():
    fams = ("gemm_f32", "gemm_pl", "colsums", "bn_train", "maxpool", "spatial_mean", "layout", "conv_fwd", "conv_bwd_data", "conv_bwd_params",
            "embed_ln", "residual_ln", "attn_fwd", "attn_bwd", "embed_bwd", "elementwise", "l2norm", "infonce", "multipos", "pairwise_cosine",
            "bce_eval", "adam_sgd", "weight_reset")
    for f in fams:
        assert any(n.startswith(f) for n in nf.CASES), f


def test_model_level_reference_side():
    """The model-level cases of tests/test_nonfinite_gpu.py on the CPU oracle: eval BatchNorm keeps the NaN pixel in its image, train
    BatchNorm spreads it over the batch, a NaN word-embedding row stays in the sequence that uses it."""
    import torch
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    from oracle import ref_image, ref_text
    im = get_biovil_resnet(None)
    syn.fill_module_(im)
    p = {k: v.clone() for k, v in im.state_dict().items()}
    _, x = nf.model_images(3)
    with torch.no_grad():
        e = ref_image.image_model_forward(p, x)
        assert torch.isfinite(e[0]).all() and torch.isfinite(e[2]).all() and not torch.isfinite(e[1]).any()
        with ref_image.bn_training(0.1):
            e = ref_image.image_model_forward({k: v.clone() for k, v in p.items()}, x)
        assert not torch.isfinite(e).any()
    tm = CXRBertModel(CXRBertConfig(**nf.TEXT_CFG)).eval()
    syn.fill_module_(tm)
    tp = {k: v.clone() for k, v in tm.state_dict().items()}
    key = [k for k in tp if k.endswith("word_embeddings.weight")]
    tp[key[0]][nf.POISON_ID, nf.POISON_COL] = float("nan")
    ids, mask = nf.model_tokens(3)
    with torch.no_grad():
        t = ref_text.cxrbert_projected(tp, ids, mask, nf.TEXT_CFG["num_hidden_layers"], nf.TEXT_CFG["num_attention_heads"], normalize=False)
    assert torch.isfinite(t[0]).all() and torch.isfinite(t[2]).all() and not torch.isfinite(t[1]).any()
