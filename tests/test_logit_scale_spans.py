"""`JointContrastiveTrainer(learn_temperature=True).reduce_spans` on the CPU (no kernel runs): theta's slot ends the "text" range, so the
ranges whose all-reduce the backward starts early still tile the whole flat gradient buffer and the reduce after `backward()` has
nothing left -- the learnable step issues no collective that the fixed-temperature step does not (the collectives of
the real two-rank step are counted in tests/test_logit_scale_dist_gpu.py)."""
import pytest

from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel


def _trainer(**kw):
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=32)
    return JointContrastiveTrainer(get_biovil_resnet(None).eval(), CXRBertModel(cfg).eval(), lr=1e-4, **kw)


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_reduce_ranges_tile_the_buffer_with_theta_at_the_end_of_the_text_range(optim):
    fixed, tr = _trainer(optim=optim), _trainer(optim=optim, learn_temperature=True)
    n = tr.optimizer.numel
    assert n == fixed.optimizer.numel + 4
    spans, spans_fixed = tr.reduce_spans(), fixed.reduce_spans()
    assert set(spans) == set(spans_fixed) == {"text", "head", "layer3", "layer2", "stem"}
    off = (tr.logit_scale.grad.data_ptr() - tr.optimizer.flat_g.data_ptr()) // 4
    assert off == n - 4 and spans["text"] == (spans_fixed["text"][0], n)           # the text range, run on over theta's slot
    assert all(spans[t] == spans_fixed[t] for t in ("head", "layer3", "layer2", "stem"))
    ordered = sorted(spans.values())
    assert ordered[0][0] == 0 and ordered[-1][1] == n and all(a[1] == b[0] for a, b in zip(ordered, ordered[1:]))
    # every early range fired: nothing is left to reduce after the backward, with and without theta
    assert cxr_optim._complement(list(spans.values()), n) == []
    assert cxr_optim._complement(list(spans_fixed.values()), fixed.optimizer.numel) == []
