"""A-GEM in the joint trainers with the REAL HIP kernels, on the small models and helpers of
tests/test_logit_scale_gpu.py (ResNet-50 at 64 px, a 2-layer 128-wide CXR-BERT, 8 pairs).

`JointContrastiveTrainer(agem_memory=...)`: before the first `remember` a step is the plain step bit for bit; with the memory equal
to the step's batch the gradients agree and nothing is projected; with a conflicting memory the gradient buffer after the step is the
float64 projection (tests/agem_ref.py) of the two gradients the plain trainer computes at the same parameters, whichever branch was
taken.  Then `agem_every`, micro-batching, and `Trainer`: a two-task loop, the epoch log, `agem.pt`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import agem_ref as A  # noqa: E402
from test_logit_scale_gpu import _batch, _bits, _host_batch, _joint, _trainer  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

LR = 1e-2
ROWS = 8


def _f64(t):
    return t.detach().double().cpu()


def _rotated(batch):
    """the images of a batch paired with the reports of the row before"""
    images, ids, mask = batch
    return images, torch.roll(ids, 1, dims=0), torch.roll(mask, 1, dims=0)


def test_before_remember_a_step_is_the_plain_step():
    images, ids, mask = _batch()
    P, Q = _joint(lr=LR, optim="sgd"), _joint(lr=LR, optim="sgd", agem_memory=ROWS)
    assert P.agem is None and P.memory is None and P.current_interference() is None
    assert Q.agem is not None and len(Q.memory) == 0
    for _ in range(2):
        lp, lq = P.step(images, ids, mask), Q.step(images, ids, mask)
        assert torch.equal(_bits(lp), _bits(lq)) and torch.equal(_bits(P.optimizer.flat_p), _bits(Q.optimizer.flat_p))
    assert Q.agem.gref is None and Q.agem._partials is None and Q.current_interference() is None and Q.agem_steps == 0
    with pytest.raises(ValueError, match="agem_memory"):
        P.remember([(images, ids, mask)])


def test_memory_equal_to_the_batch_projects_nothing():
    """the reference batch is the step's batch (its rows in the sampler's order): g_ref = g up to the order of the rows, the dot is
    |g|^2 > 0, the gradient buffer is not touched and the parameters stay bit-identical to the plain trainer's"""
    images, ids, mask = _batch()
    P, Q = _joint(lr=LR, optim="sgd"), _joint(lr=LR, optim="sgd", agem_memory=ROWS)
    assert Q.remember([(images, ids, mask)]) == ROWS and len(Q.memory) == ROWS
    for k in range(2):
        lp, lq = P.step(images, ids, mask), Q.step(images, ids, mask)
        info = Q.current_interference()
        g2 = float((_f64(P.optimizer.flat_g) ** 2).sum())
        print(f"step {k + 1}: dot {info['dot']:.6e}, |g|^2 {g2:.6e}, |gref|^2 {info['ref_sqnorm']:.6e}")
        assert info["dot"] > 0 and info["coef"] == 0.0 and (info["projected"], info["applied"]) == (0, k + 1)
        assert info["dot"] == pytest.approx(g2, rel=1e-2)             # the same rows in another order: the same gradient, nearly
        assert torch.equal(_bits(lp), _bits(lq))                      # the step still returns the current batch's loss
        assert torch.equal(_bits(P.optimizer.flat_g), _bits(Q.optimizer.flat_g))
        assert torch.equal(_bits(P.optimizer.flat_p), _bits(Q.optimizer.flat_p))
    assert Q.optimizer.steps == 2 and Q.agem_steps == 2               # the reference pass advances no optimiser state


# the steps of the conflicting sequence: True = M's images with M's reports rotated by one row, False = M itself
SEQUENCE = (True, True, False, True)


def test_a_conflicting_memory_against_the_float64_projection():
    """Remember batch M, then step on M's images paired with M's reports rotated by one row (and on M itself in between).  Before
    every step the plain trainer takes the A-GEM trainer's parameters and computes the two gradients (the memory rows the sampler
    will draw, then the step's batch); the A-GEM trainer's gradient buffer after its step is compared with their float64 projection:
    projected -> within gamma_1 (|g| + |coef gref|) of g - coef gref with the kernel's own coef, and coef within its bound of
    float64; not projected -> g bit for bit.  The reported dot agrees with float64 within the dot's bound, and the branch is the
    float64 one wherever |dot| exceeds that bound.  Over the sequence at least one step is projected and at least one is not.

    A negative parameter-space dot is expected of the rotated batch but not guaranteed: in logit space the two gradients oppose row
    by row, in parameter space the first rotated steps still agree with the memory.  Dots observed on an MI355X for the four steps
    (rotated, rotated, M, rotated), against bounds of 3e-5 .. 2e-4:
        fp32:       +3.495404e+01, +4.182356e+01, +3.341798e+01, -1.928276e-01 (coef -1.410801e-02)
        split_bf16: +3.495877e+01, +4.114176e+01, +3.480397e+01, -5.353042e-01 (coef -4.105755e-02)
    so the fourth step is projected, thousands of bounds below zero, and the others are not."""
    M = _batch()
    P, Q = _joint(lr=LR, optim="sgd"), _joint(lr=LR, optim="sgd", agem_memory=ROWS)
    Q.remember([M])
    n = Q.optimizer.numel
    nparts = K.agem_dots_nparts(n)
    taken = []
    for k, rotate in enumerate(SEQUENCE):
        batch = _rotated(M) if rotate else M
        P.optimizer.flat_p.copy_(Q.optimizer.flat_p)
        ref_rows = Q.memory.sample(ROWS, step=Q.agem_steps)
        P._gradient(*ref_rows[:3], None, None)
        gref = P.optimizer.flat_g.detach().clone().cpu()
        P._gradient(*batch, None, None)
        g = P.optimizer.flat_g.detach().clone().cpu()
        Q.step(*batch)
        info = Q.current_interference()
        assert torch.equal(_bits(Q.agem.gref), _bits(gref)), "the reference pass is not the plain gradient of the memory rows"
        D, RR, S = A.dots(g, gref)
        dbound = A.dot_bound(g, gref, nparts)
        projected = info["projected"] - sum(taken)
        taken.append(projected)
        print(f"step {k + 1} ({'rotated' if rotate else 'M'}): dot {info['dot']:.6e} (float64 {D:.6e}, bound {dbound:.2e}), |gref|^2 {RR:.4e}, "
              f"coef {info['coef']:.6e}, projected {projected}")
        assert projected in (0, 1) and info["applied"] == k + 1
        assert abs(info["dot"] - D) <= dbound and abs(info["ref_sqnorm"] - RR) <= A.rr_rtol(n, nparts) * RR
        if abs(D) > dbound:
            assert projected == int(D < 0), "the branch taken is not the one the float64 dot asks for"
        got = Q.optimizer.flat_g.detach().cpu()
        if projected:
            coef = info["coef"]
            assert abs(coef - D / RR) <= A.coef_bound(g, gref, nparts)
            err, bound = (got.double() - A.project(g, gref, coef)).abs(), A.axpy_bound(g, gref, coef)
            print(f"         worst |err| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}; |g' . gref| "
                  f"{abs(A.dots(got, gref)[0]):.3e}")
            assert bool((err <= bound).all())
            assert abs(A.dots(got, gref)[0]) <= dbound
        else:
            assert info["coef"] == 0.0 and torch.equal(_bits(got), _bits(g))
    print("projected:", taken)
    assert any(taken) and not all(taken), f"the sequence must hold a projected and an unprojected step, got {taken}"


def test_agem_every_reuses_the_reference():
    """agem_every=2: the reference pass runs on steps 0, 2, ... of the steps with a memory; in between no second `_gradient`"""
    M = _batch()
    Q = _joint(lr=LR, optim="sgd", agem_memory=ROWS, agem_every=2)
    Q.remember([M])
    calls = []
    inner = Q._gradient
    Q._gradient = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    refs = []
    for k in range(5):
        del calls[:]
        Q.step(*(_rotated(M) if k % 2 else M))
        assert len(calls) == (2 if k % 2 == 0 else 1), f"step {k}: {len(calls)} gradient computations"
        refs.append(_bits(Q.agem.gref))
    assert torch.equal(refs[0], refs[1]) and torch.equal(refs[2], refs[3]) and not torch.equal(refs[1], refs[2])
    assert Q.current_interference()["applied"] == 5 and Q.agem_steps == 5
    del calls[:]
    Q.remember([_rotated(M)])                                         # new rows: the stored reference is dropped, although the
    Q.step(*M)                                                        # sixth step would have reused it
    assert len(calls) == 2 and len(Q.memory) == 2 * ROWS


def test_micro_batched_agem_step_is_the_unchunked_one():
    """the gradient buffer after an A-GEM step, chunked against whole, by the criterion tests/test_microbatch_gpu.py applies to a
    chunked against a whole step (> 99 % of a strided sample within 2e-6 + 1e-2 |reference|); the reference pass is chunked too"""
    M = _batch()
    res, dots = [], []
    for mb in (4, None):
        Q = _joint(lr=LR, optim="sgd", agem_memory=ROWS, micro_batch=mb)
        Q.remember([M])
        Q.step(*_rotated(M))
        g = Q.optimizer.flat_g
        res.append(g[:: max(1, g.numel() // 4096)].detach().double().cpu().numpy())
        dots.append(Q.current_interference())
    agree = float(np.mean(np.abs(res[0] - res[1]) <= 2e-6 + 1e-2 * np.abs(res[1])))
    print(f"micro_batch=4 against the whole batch: agreement {agree:.5f}; dots {dots[0]['dot']:.6e} / {dots[1]['dot']:.6e}")
    assert np.abs(res[1]).max() > 1e-4 and agree > 0.99, agree
    assert dots[0]["projected"] == dots[1]["projected"] and dots[0]["dot"] == pytest.approx(dots[1]["dot"], rel=1e-2, abs=1e-6)


def test_the_reference_pass_never_augments_and_composes_with_ewc():
    M = _batch()
    Q = _joint(lr=LR, optim="sgd", agem_memory=ROWS, augment=True, augment_seed=7, ewc_lambda=10.0, ewc_fisher="identity")
    Q.remember([M])
    Q.consolidate(iter(()))
    assert Q.augment_state == (7, 0)
    Q.step(*M)
    assert Q.augment_state == (7, 1)                                  # one draw per step: the reference pass took none
    Q.step(*_rotated(M))
    assert Q.augment_state == (7, 2) and Q.current_interference()["applied"] == 2 and Q.current_penalty() > 0


def test_trainer_two_tasks_log_and_checkpoint(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    tr = _trainer(tmp_path, "w", agem_memory=6, agem_batch=4, agem_seed=3)
    j = tr._joint
    assert (j.agem_memory, j.agem_batch, j.agem_every, j.agem_seed) == (6, 4, 1, 3)
    tr.train([_host_batch(), _host_batch()], crit, 1)                # task 1, one epoch
    assert tr.writer.scalars("train/agem_projected") == [] and tr.writer.scalars("train/agem_dot") == []      # not active yet
    steps = tr.optimizer.steps
    assert tr.remember([_host_batch(), _host_batch()]) == 6           # six of the sixteen rows
    assert tr.optimizer.steps == steps == 2 and len(j.memory) == 6
    for epoch in (1, 2):                                             # task 2, two epochs
        tr.train([_host_batch(), _host_batch()], crit, epoch)
    frac, dot = tr.writer.scalars("train/agem_projected"), tr.writer.scalars("train/agem_dot")
    assert [e[2] for e in frac] == [1, 2] == [e[2] for e in dot] and all(0.0 <= e[1] <= 1.0 for e in frac)  # once per epoch while active
    info = j.current_interference()
    assert info["applied"] == 4 == j.agem_steps and dot[-1][1] == info["dot"] and tuple(j.agem.gref.shape) == (tr.optimizer.numel,)
    tr.save()
    sd = torch.load(tmp_path / "w" / "agem.pt", map_location="cpu", weights_only=True)   # tensors, lists and plain numbers only
    assert set(sd) == {"memory", "agem", "steps"} and sd["steps"] == 4 and len(sd["memory"]["tasks"]) == 1
    fresh = _trainer(tmp_path, "w", agem_memory=6, agem_batch=4, agem_seed=3)
    assert len(fresh._joint.memory) == 0
    fresh.load()
    f = fresh._joint
    assert len(f.memory) == 6 and f.agem_steps == 4 and f.agem.applied == 4 and not f.agem.valid and f.agem.gref is None
    assert f.memory.tasks[0]["images"].device.type == "cuda"
    for a, b in zip(j.memory.sample(4, step=9), f.memory.sample(4, step=9)):
        assert torch.equal(a, b)
    assert f.current_interference() == info
    assert torch.equal(_bits(fresh.optimizer.flat_p), _bits(tr.optimizer.flat_p))
    # the reloaded run recomputes its reference at its first step, from the rows the saved run would draw (step index 4)
    fresh.train([_host_batch()], crit, 3)
    assert f.agem.valid and f.agem.gref is not None and f.agem_steps == 5 and f.current_interference()["applied"] == 5
    # a state written with another memory size is refused
    other = _trainer(tmp_path, "w", agem_memory=5)
    with pytest.raises(ValueError, match="rows_per_task"):
        other.load()
    assert len(other._joint.memory) == 0
    # without the option nothing is written, and remember is refused
    plain = _trainer(tmp_path, "p")
    plain.train([_host_batch()], crit, 1)
    plain.save()
    assert not os.path.exists(tmp_path / "p" / "agem.pt") and plain.writer.scalars("train/agem_projected") == []
    with pytest.raises(ValueError, match="agem_memory"):
        plain.remember([_host_batch()])
