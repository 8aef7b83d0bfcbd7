"""Elastic weight consolidation in the joint trainers with the REAL HIP kernels, on the small models and helpers of
tests/test_logit_scale_gpu.py (ResNet-50 at 64 px, a 2-layer 128-wide CXR-BERT, 8 pairs).

`JointContrastiveTrainer(ewc_lambda=...)`: before the first consolidation a step is the plain step bit for bit; `consolidate` moves
neither the parameters nor the step count nor the schedule; F is the squared gradient of the plain trainer at the same parameters; at
the anchor the penalty is silent; one step later the gradient buffer is the plain one plus lambda F (p - a) within the kernel's
elementwise bound (tests/ewc_ref.py), with lambda chosen from the measured F so that the penalty stands at least 10^3 bounds above
it.  Then clipping's norm, micro-batched consolidation, and `Trainer`: a two-task loop, the epoch log, `ewc.pt`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ewc_ref as E  # noqa: E402
import optim_ref as R  # noqa: E402
from test_logit_scale_gpu import _batch, _bits, _host_batch, _joint, _trainer  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

LR = 1e-2


def _f64(t):
    return t.detach().double().cpu()


def _strength_for(ewc, opt, gmax: float) -> float:
    """lambda that makes the largest penalty gradient lambda F |p - a| as large as the largest task gradient"""
    term = (_f64(ewc.F) * (_f64(opt.flat_p) - _f64(ewc.anchor)).abs()).max()
    assert float(term) > 0
    return E.f32(gmax / float(term))


def test_penalised_steps_against_the_plain_trainer():
    images, ids, mask = _batch()
    kw = dict(lr=LR, optim="sgd", warmup_steps=4)
    A, B = _joint(**kw), _joint(ewc_lambda=1.0, **kw)
    assert A.ewc is None and B.ewc is not None and not B.ewc.active and B.current_penalty() is None and A.current_penalty() is None
    assert torch.equal(_bits(A.optimizer.flat_p), _bits(B.optimizer.flat_p))
    # step 1: nothing consolidated yet, bit-identical
    la, lb = A.step(images, ids, mask), B.step(images, ids, mask)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(A.optimizer.flat_p), _bits(B.optimizer.flat_p))
    assert B.current_penalty() is None and B.ewc._partials is None
    # consolidation: parameters, step count and schedule stay
    p1, lr1 = _bits(B.optimizer.flat_p), B.optimizer.lr
    assert B.consolidate([(images, ids, mask)]) == 1
    assert torch.equal(_bits(B.optimizer.flat_p), p1) and B.optimizer.steps == 1 and B.optimizer.lr == lr1 == LR / 4
    assert B.ewc.active and B.ewc.tasks == 1 and torch.equal(_bits(B.ewc.anchor), p1) and B.ewc._acc is None
    # step 2 of the plain trainer leaves its gradient at p1 in the buffer: F is its square (one accumulation, one merge with F = 0)
    A.step(images, ids, mask)
    g1 = _f64(A.optimizer.flat_g)
    F = _f64(B.ewc.F)
    err, bound = (F - g1 ** 2).abs(), 2 * E.gamma_k(2) * g1 ** 2
    print(f"F: max {float(F.max()):.3e}; worst |F - g^2| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()) and float(F.max()) > 0
    # step 2 of the penalised trainer: at the anchor the penalty's gradient is zero
    B.step(images, ids, mask)
    assert B.optimizer.lr == A.optimizer.lr == LR / 2 and B.optimizer.steps == 2
    assert bool((B.optimizer.flat_p == A.optimizer.flat_p).all()) and B.current_penalty() == 0.0
    # step 3: lambda from the measured F, then the gradient buffer against the plain one plus lambda F (p2 - a)
    lam = _strength_for(B.ewc, B.optimizer, float(g1.abs().max()))
    B.ewc.strength = lam
    p2, a = B.optimizer.flat_p.detach().clone().cpu(), B.ewc.anchor.detach().clone().cpu()
    A.step(images, ids, mask)
    B.step(images, ids, mask)
    g3 = A.optimizer.flat_g.detach().cpu()
    want, bound = E.penalty_grad(g3, p2, a, B.ewc.F.cpu(), lam), E.penalty_grad_bound(g3, p2, a, B.ewc.F.cpu(), lam)
    err = (_f64(B.optimizer.flat_g) - want).abs()
    term = lam * F * (p2.double() - a.double()).abs()
    margin = float((term / bound.clamp_min(1e-300)).max())
    print(f"lambda {lam:.4e}: largest penalty gradient {float(term.max()):.3e}, largest task gradient {float(g3.abs().max()):.3e}; "
          f"penalty / bound {margin:.3e}; worst |err| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert margin >= 1e3                                             # the check cannot pass with the penalty missing
    assert bool((err <= bound).all())
    assert not bool((B.optimizer.flat_p == A.optimizer.flat_p).all())
    # the penalty's value: strength / 2 * the float64 sum of the partials; non-negative terms, the summation tree's bound
    n = B.optimizer.numel
    value, tol = E.penalty_value(p2, a, B.ewc.F.cpu(), lam), E.penalty_partial_rtol(n, K.ewc_penalty_nparts(n))
    got = B.current_penalty()
    print(f"penalty {got:.9e}, float64 {value:.9e} (bound {tol:.2e})")
    assert value > 0 and abs(got - value) <= tol * value


def test_clipping_norm_is_that_of_the_penalised_buffer():
    images, ids, mask = _batch()
    tr = _joint(lr=1e-4, optim="adamw", max_grad_norm=float("inf"), ewc_lambda=0.0)
    tr.step(images, ids, mask)
    tr.consolidate([(images, ids, mask)])
    tr.step(images, ids, mask)
    opt = tr.optimizer
    tr.ewc.strength = _strength_for(tr.ewc, opt, float(opt.flat_g.abs().max()))
    p, a, F = _f64(opt.flat_p), _f64(tr.ewc.anchor), _f64(tr.ewc.F)
    tr.step(images, ids, mask)
    buf = opt.flat_g.detach().cpu()
    norm, tol = R.grad_norm(buf), R.norm_rtol(opt.numel, K.grad_sqnorm_nparts(opt.numel))
    plain = R.grad_norm(buf.double() - tr.ewc.strength * F * (p - a))
    got = opt.current_grad_norm()
    print(f"norm {got:.9e}, penalised buffer {norm:.9e} (bound {tol:.2e}), without the penalty {plain:.9e}")
    assert abs(got - norm) <= tol * norm
    assert abs(norm - plain) > 100 * tol * norm                       # the penalty is in the norm, far above the bound
    assert float(opt.last_clip_coef) == 1.0


def test_micro_batched_consolidation_is_the_unchunked_one():
    """sqrt(F) = |g| of the one batch: chunked against whole by the criterion tests/test_microbatch_gpu.py applies to a chunked against a
    whole step (> 99 % of a strided sample within 2e-6 + 1e-2 |reference|)"""
    images, ids, mask = _batch()
    res = []
    for mb in (4, None):
        tr = _joint(optim="sgd", ewc_lambda=1.0, micro_batch=mb)
        p0 = _bits(tr.optimizer.flat_p)
        tr.consolidate([(images, ids, mask)])
        assert torch.equal(_bits(tr.optimizer.flat_p), p0) and tr.optimizer.steps == 0
        F = tr.ewc.F
        res.append(F[:: max(1, F.numel() // 4096)].detach().double().sqrt().cpu().numpy())
    agree = float(np.mean(np.abs(res[0] - res[1]) <= 2e-6 + 1e-2 * np.abs(res[1])))
    print(f"sqrt(F), micro_batch=4 against the whole batch: agreement {agree:.5f}; largest {res[1].max():.3e}, median {np.median(res[1]):.3e}")
    assert res[1].max() > 1e-4 and agree > 0.99, agree


def test_consolidation_never_augments_and_needs_the_option():
    images, ids, mask = _batch()
    tr = _joint(optim="sgd", ewc_lambda=1.0, augment=True, augment_seed=7)
    plain = _joint(optim="sgd", ewc_lambda=1.0)
    tr.consolidate([(images, ids, mask)])
    plain.consolidate([(images, ids, mask)])
    assert tr.augment_state == (7, 0) and torch.equal(_bits(tr.ewc.F), _bits(plain.ewc.F))
    tr.step(images, ids, mask)
    assert tr.augment_state == (7, 1)
    with pytest.raises(ValueError, match="ewc_lambda"):
        _joint().consolidate([(images, ids, mask)])
    ident = _joint(optim="sgd", ewc_lambda=1.0, ewc_fisher="identity")
    assert ident.consolidate(iter(())) == 0 and ident.ewc.active and ident.ewc.F is None
    with pytest.raises(ValueError, match="accumulate"):
        _joint(optim="sgd", ewc_lambda=1.0).consolidate([])           # empirical, no batch


def test_trainer_two_tasks_log_and_checkpoint(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    tr = _trainer(tmp_path, "w", ewc_lambda=1e6, ewc_batches=1, ewc_gamma=0.5)
    assert tr._joint.ewc.gamma == 0.5 and tr._ewc_batches == 1
    tr.train([_host_batch(), _host_batch()], crit, 1)                # task 1, one epoch
    assert tr.writer.scalars("train/ewc_penalty") == []              # not active yet
    steps = tr.optimizer.steps
    assert tr.consolidate([_host_batch(), _host_batch()]) == 1       # at most "ewc_batches"
    assert tr.optimizer.steps == steps == 2 and tr._joint.ewc.active
    for epoch in (1, 2):                                             # task 2, two epochs
        tr.train([_host_batch(), _host_batch()], crit, epoch)
    logged = tr.writer.scalars("train/ewc_penalty")
    assert [e[2] for e in logged] == [1, 2] and all(e[1] > 0 for e in logged)           # once per epoch while active
    assert logged[-1][1] == tr._joint.current_penalty()
    tr.save()
    sd = torch.load(tmp_path / "w" / "ewc.pt", map_location="cpu", weights_only=True)   # tensors and plain numbers only
    assert set(sd) == {"tasks", "gamma", "fisher", "numel", "anchor", "F"} and sd["tasks"] == 1
    fresh = _trainer(tmp_path, "w", ewc_lambda=1e6)
    assert not fresh._joint.ewc.active
    fresh.load()
    e0, e1 = tr._joint.ewc, fresh._joint.ewc
    assert e1.active and e1.tasks == 1 and e1.gamma == 0.5
    assert torch.equal(_bits(e1.F), _bits(e0.F)) and torch.equal(_bits(e1.anchor), _bits(e0.anchor))
    assert torch.equal(_bits(fresh.optimizer.flat_p), _bits(tr.optimizer.flat_p))
    # a file of another size is refused, and nothing of it is taken
    torch.save(dict(sd, F=sd["F"][:-4]), tmp_path / "w" / "ewc.pt")
    other = _trainer(tmp_path, "w", ewc_lambda=1e6)
    with pytest.raises(ValueError, match="elements"):
        other.load()
    assert not other._joint.ewc.active and other._joint.ewc.F is None
    # without the option nothing is written, and consolidate is refused
    plain = _trainer(tmp_path, "p")
    plain.train([_host_batch()], crit, 1)
    plain.save()
    assert not os.path.exists(tmp_path / "p" / "ewc.pt") and plain.writer.scalars("train/ewc_penalty") == []
    with pytest.raises(ValueError, match="ewc_lambda"):
        plain.consolidate([_host_batch()])
