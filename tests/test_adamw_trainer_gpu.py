"""`JointContrastiveTrainer(optim="adamw", ...)`, the learning-rate schedule and the `Trainer` keys on the GPU, with the
small models of tests/test_sigmoid_gpu.py (ResNet-50 at 64 px, the 2-layer 128-wide CXR-BERT).  The float64 reference of the update
is tests/optim_ref.py, applied to the trainer's own gradient buffer: the step leaves it unclipped."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_ref as R  # noqa: E402
from test_logit_scale_gpu import _batch, _bits, _host_batch, _joint, _trainer  # noqa: E402

pytestmark = [pytest.mark.gpu]
steps = pytest.mark.usefixtures("precision")      # the tests that run the encoders: once per contraction precision

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import optim as O  # noqa: E402

INF = float("inf")
F32 = lambda v: float(np.float32(v))  # noqa: E731


def close(a, b, what, tol=1e-6):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    print(f"{what}: rel-to-max err {err:.3e} (tol {tol})")
    assert torch.isfinite(a).all() and err < tol, f"{what}: rel-to-max err {err:.3e} (tol {tol})"


@steps
def test_monitoring_is_adam_bit_for_bit_and_clipping_follows_the_reference():
    """optim="adamw" with weight_decay=0 and max_grad_norm=inf against optim="adam" from the same initialisation: two steps, the flat
    parameter buffer bit-identical, coefficient exactly 1.  A third trainer clips at half the measured first-step norm: coefficient 0.5
    within the norm kernel's bound; the gradient buffer stays unclipped, so tests/optim_ref.py applied to it gives the parameters."""
    images, ids, mask = _batch()
    adam, mon = _joint(), _joint(optim="adamw", weight_decay=0.0, max_grad_norm=INF)
    assert isinstance(mon.optimizer, O.AdamW) and mon.schedule is None and adam.schedule is None
    norm1 = None
    for step in (1, 2):
        la, lm = adam.step(images, ids, mask), mon.step(images, ids, mask)
        assert torch.equal(_bits(la), _bits(lm))
        assert torch.equal(_bits(adam.optimizer.flat_p), _bits(mon.optimizer.flat_p)), f"step {step}"
        assert float(mon.optimizer.last_clip_coef) == 1.0
        norm = mon.optimizer.current_grad_norm()
        ref = R.grad_norm(mon.optimizer.flat_g.cpu())
        tol = R.norm_rtol(mon.optimizer.numel, K.grad_sqnorm_nparts(mon.optimizer.numel))
        print(f"step {step}: gradient norm {norm:.9e}, float64 of the buffer {ref:.9e}, rel err {abs(norm - ref) / ref:.2e} (bound {tol:.2e})")
        assert abs(norm - ref) <= tol * ref
        norm1 = norm if norm1 is None else norm1
    del adam

    wd, max_norm = 0.05, 0.5 * norm1
    tr = _joint(lr=1e-3, optim="adamw", weight_decay=wd, max_grad_norm=max_norm)     # lr * wd = 5e-5 per step: far above the bound
    opt = tr.optimizer
    decay = R.expand_mask(opt.decay_mask.cpu(), opt.numel)
    p = opt.flat_p.detach().cpu().double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2):
        tr.step(images, ids, mask)
        g = opt.flat_g.detach().cpu()
        if step == 1:
            coef = float(opt.last_clip_coef)
            want = R.clip_coef(norm1, max_norm)
            print(f"clip coefficient {coef:.9f}, reference {want:.9f} (norm {norm1:.6e})")
            assert abs(coef - want) <= (tol + 3 * R.U) * want and abs(coef - 0.5) <= tol + 3 * R.U + 1e-6 / norm1
            assert abs(opt.current_grad_norm() - norm1) <= tol * norm1          # the norm BEFORE clipping
        p, m, v, norm, coef_ref = R.adamw_step(p, g, m, v, decay, F32(opt.lr), F32(0.9), F32(0.999), F32(1e-8), F32(wd), step, max_norm=F32(max_norm))
        assert abs(R.grad_norm(g) - opt.current_grad_norm()) <= tol * norm      # flat_g is the unclipped gradient
        close(opt.flat_p, p, f"clipped step {step}: parameters against the reference on the trainer's own gradient")
    undecayed = R.adamw_step(p, g, m, v, torch.zeros_like(decay), F32(opt.lr), 0.9, 0.999, 1e-8, wd, 3)[0]
    decayed = R.adamw_step(p, g, m, v, decay, F32(opt.lr), 0.9, 0.999, 1e-8, wd, 3)[0]
    assert float((undecayed - decayed).abs().max() / decayed.abs().max()) > 2e-6   # the decay is above the bound of the comparison


@steps
@pytest.mark.parametrize("optim", ["sgd", "adamw"])
def test_schedule_sets_the_learning_rate_the_update_uses(optim):
    """warmup 2, cosine to 0.1 x lr at step 5: after k steps `optimizer.lr` is the schedule at k, and the update of step k used it
    (SGD: p_k = p_(k-1) - lr_k g_k at 1e-6; AdamW without decay: the first step moves every weight by lr_1, up to eps)"""
    base = 2e-3
    kw = dict(warmup_steps=2, total_steps=5, lr_decay="cosine", min_lr_ratio=0.1)
    tr = _joint(lr=base, optim=optim, **kw, **({"weight_decay": 0.0} if optim == "adamw" else {}))
    sched = O.LRSchedule(base, warmup_steps=2, total_steps=5, decay="cosine", min_lr_ratio=0.1)
    images, ids, mask = _batch()
    opt = tr.optimizer
    assert opt.lr == base
    for k in (1, 2, 3):
        before = opt.flat_p.detach().clone()
        tr.step(images, ids, mask)
        want = R.lr_at(k, base, 2, 5, "cosine", 0.1)
        assert opt.lr == sched(k) == pytest.approx(want, rel=1e-15) and opt.steps == k
        if optim == "sgd":
            close(opt.flat_p, before.double() - F32(want) * opt.flat_g.double(), f"SGD step {k} at lr {want:.3e}")
        elif k == 1:
            moved = (opt.flat_p - before).abs()
            moved = moved[opt.flat_g.abs() > 1e-6]                          # |g| >> eps: the first Adam step is lr * sign(g)
            print(f"AdamW step 1: median |update| {float(moved.median()):.6e}, lr_1 {want:.6e}")
            assert moved.numel() > 1000 and abs(float(moved.median()) - want) < 1e-2 * want
    assert sched(1) == base / 2 and sched(2) == base and sched(5) == pytest.approx(0.1 * base)


def test_default_mask_and_the_scalars():
    """exactly the parameters with ndim >= 2 decay; the logit scale and the sigmoid bias do not"""
    tr = _joint(optim="adamw", learn_temperature=True, loss="sigmoid")
    opt = tr.optimizer
    assert opt.weight_decay == 0.01 and opt.max_grad_norm is None
    want = torch.zeros(opt.numel // 4, dtype=torch.uint8)
    base = opt.flat_p.data_ptr()
    n_decay = 0
    for p in opt.params:
        o = (p.data_ptr() - base) // 4
        assert o % 4 == 0
        want[o // 4:o // 4 + (p.numel() + 3) // 4] = int(p.ndim >= 2)
        n_decay += int(p.ndim >= 2)
    assert torch.equal(opt.decay_mask.cpu(), want) and 0 < n_decay < len(opt.params)
    assert opt.decay_mask.is_cuda and opt.decay_mask.dtype == torch.uint8
    for s in (tr.logit_scale, tr.logit_bias):
        assert id(s) in opt.no_decay_ids and int(opt.decay_mask[(s.data_ptr() - base) // 16]) == 0
    assert {id(p) for p in opt.params if p.ndim <= 1} == opt.no_decay_ids


@steps
def test_micro_batched_norm_is_the_unchunked_norm():
    """chunks accumulate into the flat gradient buffer before the step, so the norm is taken once, of the whole gradient: it agrees with
    the unchunked step's up to the fp32 summation order of the gradients, 1e-3 relative (the tighter of the two bounds
    tests/test_microbatch_gpu.py puts on quantities derived from them)"""
    from incremental_multimodal_medical_learning_ii_amd.contrastive import micro_slices
    images, ids, mask = _batch()
    assert len(micro_slices(int(images.shape[0]), 3)) == 3            # the step is chunked: 3 + 3 + 2 rows
    norms = []
    for mb in (3, None):
        tr = _joint(optim="adamw", max_grad_norm=INF, micro_batch=mb)
        tr.step(images, ids, mask)
        norms.append(tr.optimizer.current_grad_norm())
    print(f"gradient norm: micro_batch=3 {norms[0]:.9e}, unchunked {norms[1]:.9e}, rel diff {abs(norms[0] - norms[1]) / norms[1]:.2e}")
    assert norms[1] > 0 and abs(norms[0] - norms[1]) <= 1e-3 * norms[1]


def test_adamw_options_are_refused_with_the_other_optimisers():
    for kw in ({"weight_decay": 0.01}, {"max_grad_norm": 1.0}, {"optim": "sgd", "weight_decay": 0.01}, {"optim": "sgd", "max_grad_norm": INF}):
        with pytest.raises(ValueError, match="adamw"):
            _joint(**kw)


@steps
def test_trainer_keys_reach_the_joint_trainer_and_the_epoch_log(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    tr = _trainer(tmp_path, "w", optim="adamw", weight_decay=0.02, max_grad_norm=1.5, warmup_steps=1, total_steps=4, lr_decay="linear",
                  min_lr_ratio=0.25)
    opt = tr.optimizer
    assert isinstance(opt, O.AdamW) and opt is tr._joint.optimizer and opt.weight_decay == 0.02 and opt.max_grad_norm == 1.5
    s = tr._joint.schedule
    assert (s.base_lr, s.warmup_steps, s.total_steps, s.decay, s.min_lr_ratio) == (1e-4, 1, 4, "linear", 0.25)
    tr.train([_host_batch(), _host_batch()], crit, 1)               # one epoch of two steps
    assert opt.steps == 2 and opt.lr == s(2)
    lr, gn = tr.writer.scalars("train/lr"), tr.writer.scalars("train/grad_norm")
    assert len(lr) == 1 and lr[0][2] == 1 and lr[0][1] == s(2)                                       # once per epoch
    assert len(gn) == 1 and gn[0][2] == 1 and gn[0][1] == opt.current_grad_norm() and gn[0][1] > 0
    # without the keys: the module-level optimiser, no schedule, nothing of it logged
    plain = _trainer(tmp_path, "p")
    assert isinstance(plain.optimizer, O.Adam) and plain._joint.schedule is None
    plain.train([_host_batch()], crit, 1)
    assert plain.writer.scalars("train/lr") == [] and plain.writer.scalars("train/grad_norm") == [] and plain.optimizer.lr == 1e-4
    sched_only = _trainer(tmp_path, "s", warmup_steps=4)
    assert isinstance(sched_only.optimizer, O.Adam) and sched_only._joint.schedule(1) == 1e-4 / 4
    with pytest.raises(ValueError, match="adamw"):
        _trainer(tmp_path, "q", weight_decay=0.1)
