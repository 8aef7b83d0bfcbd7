"""What the parameter average promises without a device: the float64 reference and its bound (tests/ema_ref.py)
against an fp32 emulation of the kernel's two roundings, the entry points in the header and the ctypes table, the life-cycle and every
refusal of `optim.EMA` on CPU buffers with the test-only emulation of the kernel wrappers (tests/cpu_kernels_ema.py), the ValueError /
SystemExit paths of the trainers and the drivers that need no kernel, and `JointContrastiveTrainer(ema_decay=...)` itself on two
small CPU stand-ins for the encoders."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_ema as CK  # noqa: E402
import ema_ref as E  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, functional as Fh, optim as O  # noqa: E402

ENTRY_POINTS = {"cxrk_ema_update": 5, "cxrk_flat_swap": 4}
SHAPES = [(1,), (7, 3), (2,), (5,), (4, 3, 3, 3), (6,)]
NUMEL = 4 + 24 + 4 + 8 + 108 + 8


def bits(t):
    return t.detach().reshape(-1).view(torch.int32).clone()


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached")


@pytest.fixture
def emulated(monkeypatch):
    for mod in (O, C, Fh):
        monkeypatch.setattr(mod, "K", CK)


def _opt(seed=3, lr=0.1):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    ps[4].data = ps[4].data.contiguous(memory_format=torch.channels_last)
    opt = O.SGD(ps, lr=lr)
    assert opt.numel == NUMEL
    return opt


def _mixed(n, seed):
    """n fp32 numbers of both signs with magnitudes from 1e-30 to 1e30"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 60 - 30)
    return (mag * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 1.0])
def test_the_bound_holds_for_the_two_roundings_and_is_tight(decay):
    """the kernel's operations restated in numpy fp32 (d rounded, then one rounding of c d + e taken in float64, where the product is
    exact) stay within the bound, and the bound is not loose: the worst element uses more than a quarter of it"""
    avg, p = _mixed(4099, 1), _mixed(4099, 2)
    p[::3] = avg[::3] * (1 + 2.0 ** -12)                            # neighbours: the lerp of close numbers
    c = E.coef(decay)
    d = (p.numpy() - avg.numpy()).astype(np.float32)
    got = torch.from_numpy((c * d.astype(np.float64) + avg.numpy().astype(np.float64)).astype(np.float32))
    worst = E.within(got, avg, p, decay)
    print(f"decay {decay}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
    if 0.0 < decay < 1.0:
        assert worst > 0.25
    off = got.clone()
    off[5] = torch.nextafter(torch.nextafter(got[5], torch.tensor(float("inf"))), torch.tensor(float("inf")))
    assert E.within(off, avg, p, decay) > 1.0                      # two units in the last place off is outside
    assert E.coef(0.999) == float(np.float32(1) - np.float32(0.999)) != 1 - 0.999 and E.coef(1.0) == 0.0 and E.coef(0.0) == 1.0


def test_decay_sequence():
    """with warmup 2/11, 3/12, ... until it crosses the decay, then the decay; without warmup the decay from the first update on"""
    opt = _opt()
    e = O.EMA(opt, 0.999)
    seq = [e.decay_at(t) for t in range(1, 9000)]
    assert seq[:3] == [2 / 11, 3 / 12, 4 / 13]
    cross = next(t for t in range(1, 9000) if (1 + t) / (10 + t) >= 0.999)
    assert cross == 8990 and seq[cross - 2] == (cross) / (cross + 9) < 0.999 and seq[cross - 1] == 0.999 == seq[-1]
    assert all(a <= b for a, b in zip(seq, seq[1:]))
    assert [E.decay_at(0.999, t) for t in (1, 2, 100, 8998)] == [seq[0], seq[1], seq[99], 0.999]
    flat = O.EMA(opt, 0.999, warmup=False)
    assert [flat.decay_at(t) for t in (1, 2, 500)] == [0.999] * 3
    assert O.EMA(opt, 0.1).decay_at(1) == 0.1                       # a decay below 2/11 is never raised


# ---------------------------------------------------------------------------------------------------------------- the C interface
def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert args[-1] == "hipStream_t stream" and not any("ws" in a.split()[-1] for a in args)
        assert not re.search(r"\b" + name + r"\w*_bytes\b", code) and not any(k.startswith(name) and k.endswith("_bytes") for k in _lib.SIGNATURES)
    assert "ema_update:" in hdr and "flat_swap:" in hdr                                                  # the contract comments
    assert "ema.hip" in open(os.path.join(ROOT, "incremental_multimodal_medical_learning_ii_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ENTRY_POINTS)
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert callable(kernels.ema_update) and callable(kernels.flat_swap)


# ---------------------------------------------------------------------------------------------------------------- optim.EMA
def test_constructor_refusals():
    opt = _opt()
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, False, "0.9", None):
        with pytest.raises(ValueError, match="decay"):
            O.EMA(opt, bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="warmup"):
            O.EMA(opt, 0.9, warmup=bad)
    e = O.EMA(opt, 1)
    assert (e.decay, e.warmup, e.updates, e.last_decay, e.swapped, e.avg) == (1.0, True, 0, None, False, None)
    assert O.EMA(opt, 0.0, warmup=False).decay == 0.0


def test_nothing_is_allocated_or_launched_before_begin(monkeypatch):
    monkeypatch.setattr(O, "K", NoKernels())
    opt = _opt()
    e = O.EMA(opt, 0.9)
    assert e.avg is None
    for call in (e.update, e.swap):
        with pytest.raises(ValueError, match="begin"):
            call()
    assert e.updates == 0 and not e.swapped
    e.begin()                                                        # a copy, no kernel
    first = e.avg
    assert torch.equal(bits(first), bits(opt.flat_p)) and first.data_ptr() != opt.flat_p.data_ptr()
    opt.flat_p.add_(1.0)
    e.begin()                                                        # idempotent: the same buffer, its values kept
    assert e.avg is first and not torch.equal(first, opt.flat_p)


def test_life_cycle_on_the_emulation(emulated):
    opt = _opt()
    e = O.EMA(opt, 0.9)
    e.begin()
    e.update()                                                       # the parameters have not moved: the average is the parameters
    assert torch.equal(bits(e.avg), bits(opt.flat_p)) and (e.updates, e.last_decay) == (1, 2 / 11)
    p_bits = bits(opt.flat_p)
    for t in (2, 3, 4):
        opt.flat_p.add_(torch.randn(NUMEL, generator=torch.Generator().manual_seed(t)) * 0.1)
        before = e.avg.clone()
        e.update()
        assert e.updates == t and e.last_decay == (1 + t) / (10 + t)
        assert E.within(e.avg, before, opt.flat_p, e.last_decay) <= 1.0
        assert not torch.equal(e.avg, before)
    assert not torch.equal(bits(opt.flat_p), p_bits)
    a0, p0 = bits(e.avg), bits(opt.flat_p)
    e.swap()
    assert e.swapped and torch.equal(bits(opt.flat_p), a0) and torch.equal(bits(e.avg), p0)
    with pytest.raises(ValueError, match="swapped"):
        e.update()
    with pytest.raises(ValueError, match="swapped"):
        e.state_dict()
    with pytest.raises(ValueError, match="swapped"):
        e.load_state_dict({"numel": NUMEL, "decay": 0.9, "warmup": True, "updates": 0})
    assert e.updates == 4
    e.swap()
    assert not e.swapped and torch.equal(bits(opt.flat_p), p0) and torch.equal(bits(e.avg), a0)
    one = O.EMA(opt, 1.0, warmup=False)                             # a stationary average
    one.begin()
    opt.flat_p.mul_(3.0)
    kept = bits(one.avg)
    one.update()
    assert torch.equal(bits(one.avg), kept) and one.last_decay == 1.0
    zero = O.EMA(opt, 0.0)                                          # no memory: the average is the last iterate (d rounds once)
    zero.begin()
    opt.flat_p.add_(0.5)
    before = zero.avg.clone()
    zero.update()
    assert zero.last_decay == 0.0 and E.within(zero.avg, before, opt.flat_p, 0.0) <= 1.0
    torch.testing.assert_close(zero.avg, opt.flat_p, rtol=2 ** -22, atol=0)


def test_the_emulation_keeps_the_bits_of_an_average_that_equals_its_result():
    """include/cxrk.h, "ema_update": a negative zero stays a negative zero, whatever the decay (fma(c, d, -0) alone gives +0)"""
    for decay in (0.0, 0.5, 1.0):
        avg, p = torch.tensor([-0.0, 0.0, -0.0, 1.5, -0.0]), torch.tensor([-0.0, -0.0, 0.0, 1.5, -0.0])
        want = bits(avg)
        CK.ema_update(avg, p, decay)
        assert torch.equal(bits(avg), want), decay
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cxrk code -1"):
            CK.ema_update(torch.zeros(4), torch.zeros(4), bad)
    a = torch.arange(8.0)
    for x, y in ((a, a), (a[:6], a[2:])):
        with pytest.raises(ValueError, match="cxrk code -1"):
            CK.flat_swap(x, y)


def test_state_dict_round_trip_and_refusals(emulated):
    opt = _opt()
    e = O.EMA(opt, 0.75, warmup=False)
    sd0 = e.state_dict()
    assert sd0 == {"numel": NUMEL, "decay": 0.75, "warmup": False, "updates": 0}
    e.begin()
    opt.flat_p.add_(0.25)
    e.update()
    e.update()
    sd = e.state_dict()
    assert set(sd) == {"numel", "decay", "warmup", "updates", "avg"} and sd["updates"] == 2
    assert all(isinstance(v, (bool, int, float, torch.Tensor)) for v in sd.values())             # tensors and plain numbers only
    other = O.EMA(_opt(seed=8), 0.75, warmup=False)
    other.load_state_dict(sd)
    assert (other.updates, other.last_decay, other.swapped) == (2, 0.75, False)
    assert torch.equal(bits(other.avg), bits(e.avg)) and other.avg.data_ptr() != sd["avg"].data_ptr()
    begun = O.EMA(_opt(seed=9), 0.75, warmup=False)                  # an average that exists is filled in place: views of it stay valid
    begun.begin()
    held = begun.avg
    begun.load_state_dict(sd)
    assert begun.avg is held and torch.equal(bits(held), bits(e.avg))
    fresh = O.EMA(_opt(), 0.75, warmup=False)
    fresh.load_state_dict(sd0)
    assert fresh.avg is None and fresh.updates == 0 and fresh.last_decay is None
    for bad, what in ((dict(sd, avg=sd["avg"][:-4]), "elements"), (dict(sd, avg=sd["avg"].reshape(2, -1)), "elements"),
                      (dict(sd, avg=sd["avg"].double()), "float32"), (dict(sd, decay=0.5), "decay"), (dict(sd, warmup=True), "warmup"),
                      (dict(sd, extra=1), "keys"), ({k: v for k, v in sd.items() if k != "updates"}, "keys"),
                      ({k: v for k, v in sd.items() if k != "avg"}, "need the tensor"), (dict(sd, numel=NUMEL + 4), "flat buffer"),
                      (dict(sd, updates=-1), "updates"), (dict(sd, updates=True), "updates"), ([1, 2], "dict")):
        target = O.EMA(_opt(), 0.75, warmup=False)
        with pytest.raises(ValueError, match=what):
            target.load_state_dict(bad)
        assert target.avg is None and target.updates == 0 and target.last_decay is None          # a refused state changes nothing
    small = O.EMA(O.SGD([torch.nn.Parameter(torch.zeros(8))], lr=0.1), 0.75, warmup=False)
    with pytest.raises(ValueError, match="flat buffer"):
        small.load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------- options
def test_joint_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    for kw in ({"ema_warmup": False}, {"ema_eval": True}, {"ema_teacher": True}, {"ema_teacher": False, "distill_weight": 1.0}):
        with pytest.raises(ValueError, match="without ema_decay"):
            C.JointContrastiveTrainer(None, None, **kw)
    with pytest.raises(ValueError, match="without distill_weight"):
        C.JointContrastiveTrainer(None, None, ema_decay=0.9, ema_teacher=True)
    for bad in (-0.1, 1.01, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match="ema_decay"):
            C.JointContrastiveTrainer(None, None, ema_decay=bad)
    for name in ("ema_warmup", "ema_eval", "ema_teacher"):
        with pytest.raises(ValueError, match=name):
            C.JointContrastiveTrainer(None, None, ema_decay=0.9, distill_weight=1.0, **{name: 1})
    assert C.check_ema_options(None, None, None, None) == (None, None, None, None)
    assert C.check_ema_options(1, None, None, None) == (1.0, True, False, False)
    assert C.check_ema_options(0.5, False, True, True, 0.0) == (0.5, False, True, True)


def test_joint_options_pass_the_four_keys():
    im = object()
    je = {"image_model": im, "ema_decay": 0.99, "ema_warmup": False, "ema_eval": True, "ema_teacher": True, "distill_weight": 1.0}
    step, own = TR.joint_options(je)
    assert {k: step[k] for k in ("ema_decay", "ema_warmup", "ema_eval", "ema_teacher")} == {
        "ema_decay": 0.99, "ema_warmup": False, "ema_eval": True, "ema_teacher": True}
    assert own == {"image_model": im, "retrieval": None, "ewc_batches": None}
    assert {"ema_decay", "ema_warmup", "ema_eval", "ema_teacher"} <= set(TR.JOINT_STEP_KEYS)
    assert not any(k.startswith("ema") for g in TR.JOINT_GROUPS for k in (g[0],) + g[1]) and not any(k.startswith("ema") for k in TR.JOINT_OWN_KEYS)
    assert not any(k.startswith("ema") for k in TR.joint_options({"image_model": im, "ema_decay": None, "ema_eval": None})[0])
    # refused before anything is built: `object()` as the text engine proves that the engine is never touched
    for bad, what in (({"ema_eval": True}, "without ema_decay"), ({"ema_decay": 0.9, "ema_teacher": True}, "without distill_weight"),
                      ({"ema_decay": 2.0}, "ema_decay"), ({"ema_decay": 0.9, "ema_eval": "yes"}, "ema_eval")):
        with pytest.raises(ValueError, match=what):
            TR.Trainer(True, [], [], "standard", 1e-3, "cpu", None, bert_encoder=object(), joint_encoders={"image_model": im, **bad})


def test_drivers_arguments():
    im = object()
    a = drivers.parse_args(["class-inc", "--joint"])
    assert drivers.ema_from_args(a) == {} and not any(k.startswith("ema") for k in drivers.joint_encoders_from_args(a, im))
    a = drivers.parse_args(["zero-joint", "--joint", "--ema-decay", "0.999"])
    assert drivers.ema_from_args(a) == {"ema_decay": 0.999}
    a = drivers.parse_args(["data-inc", "--joint", "--cl", "lwf", "--ema-decay", "0.99", "--ema-no-warmup", "--ema-eval", "--ema-teacher"])
    want = {"ema_decay": 0.99, "ema_warmup": False, "ema_eval": True, "ema_teacher": True}
    assert drivers.ema_from_args(a) == want
    je = drivers.joint_encoders_from_args(a, im)
    assert {k: v for k, v in je.items() if k.startswith("ema")} == want and je["distill_weight"] == drivers.DISTILL_WEIGHT
    step, _ = TR.joint_options(je)                                  # and `Trainer` accepts the dict
    assert {k: v for k, v in step.items() if k.startswith("ema")} == want
    for argv in (["zero-joint", "--ema-decay", "0.9"],                                   # needs --joint
                 ["zero-joint", "--joint", "--ema-eval"],                                # the options need --ema-decay
                 ["zero-joint", "--joint", "--ema-no-warmup"],
                 ["class-inc", "--joint", "--cl", "lwf", "--ema-teacher"],
                 ["class-inc", "--joint", "--ema-decay", "0.9", "--ema-teacher"],        # the momentum teacher needs --cl lwf
                 ["class-inc", "--joint", "--cl", "ewc", "--ema-decay", "0.9", "--ema-teacher"],
                 ["zero-joint", "--joint", "--ema-decay", "1.5"],
                 ["zero-joint", "--joint", "--ema-decay", "-0.1"],
                 ["zero-joint", "--joint", "--ema-decay", "nan"]):
        with pytest.raises(SystemExit):
            drivers.parse_args(argv)
        with pytest.raises(SystemExit):
            drivers.main(argv)


# ---------------------------------------------------------------------------------------------------------------- the joint trainer
D_EMB, VOCAB, B_CPU = 16, 50, 8


class _Image(torch.nn.Module):
    """what `JointContrastiveTrainer` asks of an image encoder, as one linear layer on the CPU"""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(12, D_EMB)
        self.register_buffer("running", torch.ones(3))
        self.grad_ready_hook, self.augment_call, self.save_free = None, None, False

    def prepare_(self):
        return self

    def forward(self, x):
        return self.lin(x.reshape(x.shape[0], -1))


class _Text(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(VOCAB, D_EMB)
        self.proj = torch.nn.Linear(D_EMB, D_EMB)
        self.grad_ready_hook, self.save_free = None, False

    def prepare_(self):
        return self

    def get_projected_text_embeddings(self, ids, mask, normalize_embeddings=False):
        m = mask.unsqueeze(-1).float()
        return self.proj((self.emb(ids) * m).sum(1) / m.sum(1))


def _cpu_joint(**kw):
    torch.manual_seed(11)
    return C.JointContrastiveTrainer(_Image(), _Text(), lr=kw.pop("lr", 0.5), temperature=0.5, optim="sgd", **kw)


def _cpu_batch(k=0):
    g = torch.Generator().manual_seed(100 + k)
    return torch.randn(B_CPU, 3, 2, 2, generator=g), torch.randint(0, VOCAB, (B_CPU, 5), generator=g), torch.ones(B_CPU, 5, dtype=torch.int64)


def test_a_run_with_the_average_trains_bit_for_bit_as_the_run_without(emulated):
    A, B = _cpu_joint(), _cpu_joint(ema_decay=0.9)
    assert A.ema is None and A.current_ema() is None and B.ema is not None and B.ema.avg is None       # no buffer at construction
    assert B.current_ema() == {"updates": 0, "decay": 0.9, "last_decay": None}
    with torch.no_grad():                                            # what a broadcast or a checkpoint does after construction
        for tr in (A, B):
            tr.optimizer.flat_p.mul_(1.25)
    avg = B.optimizer.flat_p.detach().clone()                       # begun at the entry of the first step: from the values of then
    snaps = []
    for k in range(3):
        la, lb = A.step(*_cpu_batch(k)), B.step(*_cpu_batch(k))
        assert torch.equal(bits(la), bits(lb)) and torch.equal(bits(A.optimizer.flat_p), bits(B.optimizer.flat_p)), k
        d = E.decay_at(0.9, k + 1)
        assert B.current_ema() == {"updates": k + 1, "decay": 0.9, "last_decay": d}
        assert E.within(B.ema.avg, avg, B.optimizer.flat_p, d) <= 1.0
        avg = B.ema.avg.clone()
        snaps.append(bits(B.optimizer.flat_p))
    assert not torch.equal(snaps[0], snaps[2]) and not torch.equal(bits(B.ema.avg), snaps[2])


def test_averaged_swaps_restores_and_refuses(emulated):
    tr = _cpu_joint(ema_decay=0.5, ema_warmup=False, learn_temperature=True, ewc_lambda=1.0, ewc_fisher="identity", distill_weight=0.0,
                    agem_memory=4)
    with pytest.raises(ValueError, match="without ema_decay"):
        with _cpu_joint().averaged():
            pass
    for k in range(2):
        tr.step(*_cpu_batch(k))
    p0, a0 = bits(tr.optimizer.flat_p), bits(tr.ema.avg)
    assert not torch.equal(p0, a0)
    tau_raw = tr.current_temperature()
    w = tr.image_model.lin.weight
    off = (w.data_ptr() - tr.optimizer.flat_p.data_ptr()) // 4
    raw_w = w.detach().clone()
    with tr.averaged() as inside:
        assert inside is tr and tr.ema.swapped
        assert torch.equal(bits(tr.optimizer.flat_p), a0) and torch.equal(bits(tr.ema.avg), p0)
        assert torch.equal(bits(w), a0[off:off + w.numel()]) and not torch.equal(w, raw_w)        # the modules view flat_p
        assert tr.current_temperature() != tau_raw                                               # the averaged theta
        for call in (lambda: tr.step(*_cpu_batch(5)), lambda: tr.consolidate([]), lambda: tr.remember([]), tr.snapshot_teacher,
                     lambda: tr.averaged().__enter__()):
            with pytest.raises(RuntimeError, match=r"inside averaged\(\)"):
                call()
        assert tr.ema.swapped and tr.ema.updates == 2 and tr.optimizer.steps == 2
    assert not tr.ema.swapped and torch.equal(bits(tr.optimizer.flat_p), p0) and torch.equal(bits(tr.ema.avg), a0)
    with pytest.raises(RuntimeError, match="inside"):               # a step inside raises, and the buffers are still put back
        with tr.averaged():
            tr.step(*_cpu_batch(5))
    assert not tr.ema.swapped and not tr._averaging
    assert torch.equal(bits(tr.optimizer.flat_p), p0) and torch.equal(bits(tr.ema.avg), a0) and tr.current_temperature() == tau_raw
    tr.step(*_cpu_batch(2))                                          # and training goes on
    assert tr.ema.updates == 3
    early = _cpu_joint(ema_decay=0.5)                                # before any step: the average begins as the parameters
    q0 = bits(early.optimizer.flat_p)
    with early.averaged():
        assert torch.equal(bits(early.optimizer.flat_p), q0) and torch.equal(bits(early.ema.avg), q0)
    assert early.ema.updates == 0


def test_the_momentum_teacher_is_the_average_itself(emulated):
    tr = _cpu_joint(ema_decay=0.5, ema_teacher=True, distill_weight=1.0)
    assert tr.teacher is None and tr.ema.avg is None
    tr.snapshot_teacher()                                            # before any step: the average begins here
    t = tr.teacher
    assert t.flat is tr.ema.avg and t.flat.data_ptr() == tr.ema.avg.data_ptr() != tr.optimizer.flat_p.data_ptr()
    tw, sw = t.image_model.lin.weight, tr.image_model.lin.weight
    off = (sw.data_ptr() - tr.optimizer.flat_p.data_ptr()) // 4
    assert tw.data_ptr() == tr.ema.avg.data_ptr() + 4 * off and torch.equal(tw, sw) and not tw.requires_grad
    with torch.no_grad():
        tr.optimizer.flat_p.add_(1.0)
        tr.image_model.running.add_(2.0)
    tr.ema.update()                                                  # the teacher moves with the average ...
    assert torch.equal(bits(tw), bits(tr.ema.avg[off:off + tw.numel()])) and not torch.equal(tw, sw)
    assert float((tw - (sw - 1.0)).detach().abs().max()) > 0.1
    kept = bits(tr.ema.avg)
    tr.snapshot_teacher()                                            # ... and a later snapshot refreshes only the cloned tensors
    assert tr.teacher is t and torch.equal(bits(tr.ema.avg), kept) and torch.equal(t.image_model.running, tr.image_model.running)
    sd = t.state_dict()                                              # teacher.pt as ever; loading lands in the average's storage
    want = sd["flat"].clone() + 1.0                                  # (on the CPU `state_dict()["flat"]` shares the average's storage)
    t.load_state_dict(dict(sd, flat=want))
    assert torch.equal(tr.ema.avg, want) and tr.ema.avg.data_ptr() == t.flat.data_ptr()
    frozen = _cpu_joint(distill_weight=1.0)                         # without the option: a clone, refreshed by a later snapshot
    frozen.snapshot_teacher()
    with torch.no_grad():
        frozen.optimizer.flat_p.add_(1.0)
    assert not torch.equal(frozen.teacher.flat, frozen.optimizer.flat_p)
    frozen.snapshot_teacher()
    assert torch.equal(frozen.teacher.flat, frozen.optimizer.flat_p)
    with pytest.raises(ValueError, match="flat"):
        C.FrozenTeacher(frozen.image_model, frozen.text_model, frozen.optimizer, flat=frozen.optimizer.flat_p)
    with pytest.raises(ValueError, match="flat"):
        C.FrozenTeacher(frozen.image_model, frozen.text_model, frozen.optimizer, flat=torch.zeros(8))
