"""Cross-precision gradient check of the image encoder at BASELINE config 2's size (batch 256, 224 px, full ResNet-50 + projector):
the split-bf16 (bf16x3) backward against the exact-fp32 backward UNDER THE SAME DECISIONS.

A ReLU network's gradient is discontinuous in its forward values: the two contraction precisions differ by ~1e-5 in the forward,
so a few 1e-5 of the 2.8e9 ReLU decisions (and a few max-pool winners) of this batch come out differently, and each flipped
decision moves upstream gradients at the 1e-3 level — a free-running comparison therefore measures the
conditioning of the gradient, not the arithmetic.  Here the fp32 forward's decisions (ReLU bit masks of all 49 activations, the
max-pool winners, the stem's ReLU at the winner) are captured on the device and imposed on the split-bf16 pass before its backward
runs: both backwards then differentiate the same piecewise-linear function and EVERY parameter gradient of the image encoder has to
agree within the north star's 1e-3 (max |diff| / max |ref|, the metric of the oracle tests, and norm-relative).
"""
import pytest
import torch

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import image_encoder as IE  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.diagnostics import imposed_decision_gradient_errors  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet  # noqa: E402

DEV = "cuda"
TOL = 1e-3


def test_cfg2_split_bf16_image_gradients_match_fp32_under_imposed_decisions():
    B = 256
    model = get_biovil_resnet(None).eval()
    syn.fill_module_(model)
    model.to(DEV)
    images = syn.synthetic_images(B, 224, seed=31).to(DEV)
    cot = torch.randn(B, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    imposed, free, flips, emb_err = imposed_decision_gradient_errors(model, images, cot)
    worst_imp = max(((max(v), k) for k, v in imposed.items()), key=lambda t: t[0])
    worst_free = max(((max(v), k) for k, v in free.items()), key=lambda t: t[0])
    probes = ("encoder.encoder.layer1.0.conv1.weight", "encoder.encoder.layer3.2.conv2.weight", "projector.model.0.weight",
              "encoder.encoder.conv1.weight")
    print("cfg2 imposed-decision check: embeddings", emb_err, "decisions overridden", flips,
          "| imposed:", {k: imposed[k] for k in probes}, "worst", worst_imp, "| free-running:", {k: free[k] for k in probes}, "worst", worst_free)
    assert emb_err < TOL
    assert len(imposed) >= 160
    # the two forwards really disagree on some decisions (otherwise this test shows nothing beyond the free-running one) ...
    assert 0 < flips["relu"] < 1e-3 * flips["relu_total"], flips
    # ... and under equal decisions every gradient tensor is within the bar
    assert worst_imp[0] < TOL, (worst_imp, {k: imposed[k] for k in probes})


def test_decisions_round_trip_through_the_saved_state():
    """`device_decisions` / `count_decision_differences` / `impose_decisions_` on the saved state of a small pass (2 images of 64 px,
    2 x 2 patches at the head).  split-bf16: a pass's own decisions differ from themselves nowhere, the totals are the element counts
    of the masks, and imposing them on a second pass changes no gradient bit.  fp32: its decisions have the structure of the planes
    ones, and imposed on a split-bf16 pass they give gradients within 1e-3 of the fp32 backward's (the check of the test above, at the
    small size; so few decisions may well all agree here, so no flip count is required)."""
    model = get_biovil_resnet(None).eval()
    syn.fill_module_(model)
    model.to(DEV)
    x = syn.synthetic_images(2, 64, seed=33).to(DEV)
    cot = torch.randn(2, 128, generator=torch.Generator().manual_seed(6)).to(DEV)
    named = [(n, p) for n, p in model.named_parameters() if not n.startswith("encoder.encoder.fc.")]

    def run(precision, impose=None):
        _lib.set_precision(precision)
        for _, p in named:
            p.grad = None
        e = model(x)
        dec = IE.device_decisions(e.grad_fn.state)
        if impose is not None:
            IE.impose_decisions_(e.grad_fn, impose)
        (e * cot).sum().backward()
        return {n: p.grad.detach().clone() for n, p in named}, dec

    old = _lib.get_precision()
    try:
        g_own, d = run("split_bf16")
        same = IE.count_decision_differences(d, d)
        n_relu = sum(m.numel() * 8 for t in d["blocks"] for m in t) + d["proj"].numel() * 8 + d["stem_pos"].numel()
        assert same == {"relu": 0, "relu_total": n_relu, "pool_taps": 0, "pool_total": d["pool_taps"].numel()}, same
        g_imp, _ = run("split_bf16", impose=d)
        assert all(torch.equal(g_imp[n], g_own[n]) for n, _ in named), [n for n, _ in named if not torch.equal(g_imp[n], g_own[n])]
        g32, d32 = run("fp32")
        assert len(d32["blocks"]) == len(d["blocks"]) == 16
        for ta, tb in zip(d32["blocks"], d["blocks"]):
            assert [(m.shape, m.dtype) for m in ta] == [(m.shape, m.dtype) for m in tb]
        for k in ("proj", "pool_taps", "stem_pos"):
            assert (d32[k].shape, d32[k].dtype) == (d[k].shape, d[k].dtype), k
        flips = IE.count_decision_differences(d32, d)
        gs, _ = run("split_bf16", impose=d32)
    finally:
        _lib.set_precision(old)
        for _, p in named:
            p.grad = None
    errs = {n: max(float((gs[n] - g32[n]).abs().max() / g32[n].abs().max().clamp_min(1e-30)),
                   float((gs[n] - g32[n]).norm() / g32[n].norm().clamp_min(1e-30))) for n, _ in named}
    worst = max((v, k) for k, v in errs.items())
    print("small imposed-decision check: decisions overridden", flips, "worst", worst)
    assert len(errs) >= 160 and worst[0] < TOL, worst
