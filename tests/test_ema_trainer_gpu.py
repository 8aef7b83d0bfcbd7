"""The parameter average in the joint trainers with the REAL HIP kernels, on the small models and helpers of
tests/test_logit_scale_gpu.py (ResNet-50 at 64 px, a 2-layer 128-wide CXR-BERT, 8 pairs).

`JointContrastiveTrainer(ema_decay=...)`: training is bit for bit that of the trainer without it while the average follows the
recurrence within the kernel's elementwise bound (tests/ema_ref.py); `averaged()` makes the encoders read the average and puts both
buffers back; the momentum teacher (`ema_teacher`) is the average itself -- a student that does not move is distilled against
itself at exactly zero, a stationary average (decay 1) is the frozen teacher bit for bit, a moving one is not.  Then `Trainer`:
`"ema_eval"`, the epoch log, `ema.pt`."""
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ema_ref as E  # noqa: E402
from test_logit_scale_gpu import _batch, _bits, _host_batch, _joint, _trainer  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

LR = 1e-3            # Adam: every parameter moves by about LR per step, far above the fp32 spacing of the weights


def test_three_steps_train_as_without_the_average_and_the_average_follows_the_recurrence():
    images, ids, mask = _batch()
    A, B = _joint(lr=LR), _joint(lr=LR, ema_decay=0.9)
    assert A.ema is None and A.current_ema() is None
    assert B.ema is not None and B.ema.avg is None and B.current_ema() == {"updates": 0, "decay": 0.9, "last_decay": None}
    avg = B.optimizer.flat_p.detach().clone()                        # the average begins at the entry of the first step
    for t in (1, 2, 3):
        la, lb = A.step(images, ids, mask), B.step(images, ids, mask)
        assert torch.equal(_bits(la), _bits(lb)), f"step {t}: the losses differ"
        assert torch.equal(_bits(A.optimizer.flat_p), _bits(B.optimizer.flat_p)), f"step {t}: the parameters differ"
        d = B.current_ema()["last_decay"]
        assert d == E.decay_at(0.9, t) == (1 + t) / (10 + t) and B.current_ema()["updates"] == t
        worst = E.within(B.ema.avg, avg, B.optimizer.flat_p, d)      # float64 on the device, from the recorded snapshots
        print(f"step {t}: d_t {d:.6f}, worst |err| / bound {worst:.3f}")
        assert worst <= 1.0
        avg = B.ema.avg.detach().clone()
    assert B.ema.avg.data_ptr() != B.optimizer.flat_p.data_ptr() and B.ema.avg.shape == B.optimizer.flat_p.shape
    moved = float((B.ema.avg.double() - B.optimizer.flat_p.double()).abs().max())
    print(f"largest |avg - p| after three steps: {moved:.3e}")
    assert moved > 1e-4 and not torch.equal(_bits(B.ema.avg), _bits(B.optimizer.flat_p))


def _embed(tr, images, ids, mask):
    with torch.no_grad():
        return tr.image_model(images), tr.text_model.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)


def test_averaged_reads_the_average_and_restores_both_buffers():
    images, ids, mask = _batch()
    tr = _joint(lr=LR, ema_decay=0.5, ema_warmup=False, learn_temperature=True)
    for _ in range(3):
        tr.step(images, ids, mask)
    p0, a0 = _bits(tr.optimizer.flat_p), _bits(tr.ema.avg)
    raw, tau_raw = _embed(tr, images, ids, mask), tr.current_temperature()
    other = _joint(lr=LR, learn_temperature=True)                    # a second trainer whose parameters ARE the first one's average
    with torch.no_grad():
        other.optimizer.flat_p.copy_(tr.ema.avg)
    want, tau_want = _embed(other, images, ids, mask), other.current_temperature()
    with tr.averaged():
        assert tr.ema.swapped and torch.equal(_bits(tr.optimizer.flat_p), a0) and torch.equal(_bits(tr.ema.avg), p0)
        got, tau_got = _embed(tr, images, ids, mask), tr.current_temperature()
        with pytest.raises(RuntimeError, match=r"inside averaged\(\)"):
            with tr.averaged():
                pass
    for k in (0, 1):
        assert torch.equal(_bits(got[k]), _bits(want[k])), ("image", "text")[k]
        assert not torch.equal(_bits(got[k]), _bits(raw[k]))
    assert tau_got == tau_want != tau_raw                            # the averaged theta
    assert not tr.ema.swapped and torch.equal(_bits(tr.optimizer.flat_p), p0) and torch.equal(_bits(tr.ema.avg), a0)
    again = _embed(tr, images, ids, mask)
    assert all(torch.equal(_bits(again[k]), _bits(raw[k])) for k in (0, 1)) and tr.current_temperature() == tau_raw
    with pytest.raises(RuntimeError, match=r"inside averaged\(\)"):  # a step inside raises, and the buffers are still put back
        with tr.averaged():
            tr.step(images, ids, mask)
    assert not tr.ema.swapped and tr.optimizer.steps == 3 and tr.ema.updates == 3
    assert torch.equal(_bits(tr.optimizer.flat_p), p0) and torch.equal(_bits(tr.ema.avg), a0)
    with pytest.raises(ValueError, match="without ema_decay"):
        with other.averaged():
            pass


def test_the_momentum_teacher_of_a_student_that_does_not_move_is_the_student():
    """sgd at lr 0: the parameters stay, so does their average bit for bit (the lerp form), and the distillation loss against it is
    exactly zero"""
    images, ids, mask = _batch()
    tr = _joint(optim="sgd", lr=0.0, ema_decay=0.9, ema_teacher=True, distill_weight=1.0)
    assert tr.teacher is None and tr.ema.avg is None
    tr.snapshot_teacher()
    assert tr.teacher.flat.data_ptr() == tr.ema.avg.data_ptr() != tr.optimizer.flat_p.data_ptr()
    p0 = _bits(tr.optimizer.flat_p)
    for t in (1, 2, 3):
        tr.step(images, ids, mask)
        assert tr.current_distill() == 0.0, t                         # exactly
        assert torch.equal(_bits(tr.ema.avg), _bits(tr.optimizer.flat_p)) and torch.equal(_bits(tr.optimizer.flat_p), p0), t
    assert tr.ema.updates == 3 and tr.teacher.flat.data_ptr() == tr.ema.avg.data_ptr()
    assert float(tr.optimizer.flat_g.abs().max()) > 0                 # the steps did compute gradients


_FROZEN = {}


def _digest(t):
    return hashlib.sha256(_bits(t).numpy().tobytes()).hexdigest()


@pytest.fixture
def frozen_run(precision):
    """three steps of a plain `distill_weight` trainer with a frozen teacher taken before step 1: (loss bits, L_d, digest of the
    parameter bits) per step; computed once per contraction precision and shared by the two tests below, which leave it unchanged"""
    if precision not in _FROZEN:
        images, ids, mask = _batch()
        tr = _joint(lr=LR, distill_weight=1.0)
        tr.snapshot_teacher()
        out = []
        for _ in range(3):
            loss = tr.step(images, ids, mask)
            out.append((_bits(loss), tr.current_distill(), _digest(tr.optimizer.flat_p)))
        _FROZEN[precision] = out
    return _FROZEN[precision]


def test_a_stationary_average_is_a_frozen_teacher(frozen_run):
    images, ids, mask = _batch()
    tr = _joint(lr=LR, distill_weight=1.0, ema_decay=1.0, ema_warmup=False, ema_teacher=True)
    tr.snapshot_teacher()
    a0 = _bits(tr.ema.avg)
    for t, (loss_bits, distill, p_digest) in enumerate(frozen_run, 1):
        loss = tr.step(images, ids, mask)
        assert torch.equal(_bits(loss), loss_bits) and tr.current_distill() == distill and _digest(tr.optimizer.flat_p) == p_digest, t
        assert torch.equal(_bits(tr.ema.avg), a0) and tr.current_ema()["last_decay"] == 1.0
    assert frozen_run[0][1] == 0.0 and frozen_run[2][1] > 0          # the yardstick itself: silent at the snapshot, then not


def test_a_moving_average_is_not(frozen_run):
    images, ids, mask = _batch()
    tr = _joint(lr=LR, distill_weight=1.0, ema_decay=0.5, ema_teacher=True)
    tr.snapshot_teacher()
    seen = []
    for t, (loss_bits, distill, p_digest) in enumerate(frozen_run, 1):
        tr.step(images, ids, mask)
        seen.append(tr.current_distill())
        if t == 1:                                                    # the teacher of step 1 is the snapshot in both runs
            assert seen[0] == distill == 0.0 and _digest(tr.optimizer.flat_p) == p_digest
        else:                                                         # from step 2 on it has moved towards the student
            assert seen[-1] > 0 and seen[-1] != distill, (t, seen, distill)
    print(f"L_d against the moving teacher {seen}, against the frozen one {[r[1] for r in frozen_run]}")
    kept = _bits(tr.ema.avg)
    tr.snapshot_teacher()                                             # a later snapshot leaves the average alone
    assert torch.equal(_bits(tr.ema.avg), kept) and tr.teacher.flat.data_ptr() == tr.ema.avg.data_ptr()


def _val_losses(tr):
    return [v for _, v, _ in tr.writer.scalars("val/Loss")]


def test_trainer_evaluates_the_average_logs_and_checkpoints(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    je = dict(ema_decay=0.5, ema_warmup=False)
    raw, avg = _trainer(tmp_path, "r", **je), _trainer(tmp_path, "a", ema_eval=True, retrieval=True, **je)
    assert raw._joint.ema_eval is False and avg._joint.ema_eval is True
    for tr in (raw, avg):
        tr.train([_host_batch(), _host_batch()], crit, 1)            # one epoch of two steps
        assert tr.writer.scalars("train/ema_decay") == [("train/ema_decay", 0.5, 1)]        # once per epoch
    assert torch.equal(_bits(raw.optimizer.flat_p), _bits(avg.optimizer.flat_p)) and torch.equal(_bits(raw._joint.ema.avg), _bits(avg._joint.ema.avg))
    p0, a0 = _bits(avg.optimizer.flat_p), _bits(avg._joint.ema.avg)
    m_raw, m_avg = raw.val([_host_batch()], crit, 1, 1), avg.val([_host_batch()], crit, 1, 1)
    assert set(m_raw) <= set(m_avg) and any(k.startswith("Retrieval/") for k in m_avg)       # the tags are the same
    l_raw, l_avg = _val_losses(raw), _val_losses(avg)
    print(f"val/Loss raw {l_raw}, averaged {l_avg}")
    assert len(l_raw) == len(l_avg) == 1 and l_raw != l_avg          # the averaged model's numbers
    assert torch.equal(_bits(avg.optimizer.flat_p), p0) and torch.equal(_bits(avg._joint.ema.avg), a0) and not avg._joint.ema.swapped
    inside = {}
    with avg._joint.averaged():                                       # what `val` read: the same loss from the swapped trainer by hand
        avg._joint.ema_eval = False
        try:
            avg._bert_cache.clear()
            avg.val([_host_batch()], crit, 2, 2)
            inside["loss"] = _val_losses(avg)[-1]
        finally:
            avg._joint.ema_eval = True
            avg._bert_cache.clear()
    assert inside["loss"] == l_avg[0]
    avg.test([_host_batch()], None, 1, 1)
    assert torch.equal(_bits(avg.optimizer.flat_p), p0) and torch.equal(_bits(avg._joint.ema.avg), a0)
    # save / load: the model files are the raw weights, the average travels as ema.pt
    avg.save()
    sd = torch.load(tmp_path / "a" / "ema.pt", map_location="cpu", weights_only=True)       # tensors and plain numbers only
    assert set(sd) == {"numel", "decay", "warmup", "updates", "avg"} and sd["updates"] == 2 and sd["decay"] == 0.5 and sd["warmup"] is False
    fresh = _trainer(tmp_path, "a", ema_eval=True, **je)
    assert fresh._joint.ema.avg is None
    fresh.load()
    assert torch.equal(_bits(fresh.optimizer.flat_p), p0) and torch.equal(_bits(fresh._joint.ema.avg), a0)
    assert fresh._joint.current_ema() == avg._joint.current_ema() == {"updates": 2, "decay": 0.5, "last_decay": 0.5}
    torch.save(dict(sd, avg=sd["avg"][:-4]), tmp_path / "a" / "ema.pt")                      # another size: refused, nothing taken
    other = _trainer(tmp_path, "a", **je)
    with pytest.raises(ValueError, match="elements"):
        other.load()
    assert other._joint.ema.avg is None and other._joint.ema.updates == 0
    plain = _trainer(tmp_path, "p")                                   # without the option nothing is written or logged
    plain.train([_host_batch()], crit, 1)
    plain.save()
    assert not os.path.exists(tmp_path / "p" / "ema.pt") and plain.writer.scalars("train/ema_decay") == [] and plain._joint.ema is None


def test_trainer_checkpoint_of_a_momentum_teacher(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    je = dict(ema_decay=0.5, ema_teacher=True, distill_weight=1.0)
    tr = _trainer(tmp_path, "w", **je)
    tr.train([_host_batch()], crit, 1)                               # task 1
    tr.end_task([_host_batch()])                                     # -> snapshot_teacher(): the teacher is the average so far
    assert tr._joint.teacher.flat.data_ptr() == tr._joint.ema.avg.data_ptr()
    tr.train([_host_batch(), _host_batch()], crit, 1)                # task 2
    assert tr._joint.current_distill() > 0 and tr._joint.ema.updates == 3
    tr.save()
    for name in ("ema.pt", "teacher.pt"):
        assert os.path.exists(tmp_path / "w" / name)
    fresh = _trainer(tmp_path, "w", **je)
    fresh.load()
    j0, j1 = tr._joint, fresh._joint
    assert j1.teacher is not None and j1.teacher.flat.data_ptr() == j1.ema.avg.data_ptr()   # both loads landed in one storage
    assert torch.equal(_bits(j1.ema.avg), _bits(j0.ema.avg)) and j1.ema.updates == 3 and j1.ema.last_decay == j0.ema.last_decay
    assert torch.equal(_bits(fresh.optimizer.flat_p), _bits(tr.optimizer.flat_p))
    for t in (tr, fresh):                                            # the next step: L_d and the gradient buffer bit-identical
        t.train([_host_batch()], crit, 2)
    assert torch.equal(_bits(fresh.optimizer.flat_g), _bits(tr.optimizer.flat_g))
    assert j1.current_distill() == j0.current_distill() > 0
