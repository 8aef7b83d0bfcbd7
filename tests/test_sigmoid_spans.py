"""`JointContrastiveTrainer(loss="sigmoid", learn_temperature=True).reduce_spans` on the CPU (no kernel runs): theta's and b's slots,
in that order, end the "text" range, so the ranges whose all-reduce the backward starts early still tile the whole flat gradient
buffer and the reduce after `backward()` has nothing left (the collectives of the real two-rank step are counted in
tests/test_sigmoid_dist_gpu.py).  With fixed scalars the buffer is the InfoNCE trainer's."""
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
def test_reduce_ranges_tile_the_buffer_with_theta_and_b_at_the_end_of_the_text_range(optim):
    fixed, tr = _trainer(optim=optim), _trainer(optim=optim, learn_temperature=True, loss="sigmoid")
    n = tr.optimizer.numel
    assert n == fixed.optimizer.numel + 8                                          # two 4-element slots
    spans, spans_fixed = tr.reduce_spans(), fixed.reduce_spans()
    assert set(spans) == set(spans_fixed) == {"text", "head", "layer3", "layer2", "stem"}
    base = tr.optimizer.flat_g.data_ptr()
    assert (tr.logit_scale.grad.data_ptr() - base) // 4 == n - 8 and (tr.logit_bias.grad.data_ptr() - base) // 4 == n - 4   # theta, then b
    assert tr.optimizer.params[-2] is tr.logit_scale and tr.optimizer.params[-1] is tr.logit_bias
    assert spans["text"] == (spans_fixed["text"][0], n)                            # the text range, run on over both slots
    assert all(spans[t] == spans_fixed[t] for t in ("head", "layer3", "layer2", "stem"))
    ordered = sorted(spans.values())
    assert ordered[0][0] == 0 and ordered[-1][1] == n and all(a[1] == b[0] for a, b in zip(ordered, ordered[1:]))
    assert cxr_optim._complement(list(spans.values()), n) == []                    # nothing is left to reduce after the backward
    assert tr.reduce_spans(None, None) == spans                                    # the spans derived from the optimiser's own list agree


def test_fixed_scalars_add_no_parameter():
    fixed, tr = _trainer(), _trainer(loss="sigmoid", sigmoid_bias=-4.0)
    assert tr.logit_scale is None and tr.logit_bias is None and tr.optimizer.numel == fixed.optimizer.numel
    assert tr.reduce_spans() == fixed.reduce_spans()
    theta, b = tr._sigmoid_consts
    assert not theta.requires_grad and not b.requires_grad and tr.current_bias() == -4.0 and tr.current_temperature() == 0.07
