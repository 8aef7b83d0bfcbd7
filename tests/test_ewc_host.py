"""What elastic weight consolidation promises without a device: the float64 reference (tests/ewc_ref.py) pinned to
autograd, the entry points in the header and the ctypes table, the life-cycle and every refusal of `optim.EWC` on CPU buffers with
the test-only emulation of the kernel wrappers (tests/cpu_kernels_ewc.py), and the ValueError / SystemExit paths of the trainers and
the drivers that need no kernel."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_ewc as CK  # noqa: E402
import ewc_ref as E  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, optim as O  # noqa: E402

ENTRY_POINTS = {"cxrk_fisher_accumulate": 5, "cxrk_ewc_consolidate": 8, "cxrk_ewc_penalty_partials_bytes": 1, "cxrk_ewc_penalty": 9}
SHAPES = [(1,), (7, 3), (2,), (5,), (4, 3, 3, 3), (6,)]
NUMEL = 4 + 24 + 4 + 8 + 108 + 8


def bits(t):
    return t.detach().reshape(-1).view(torch.int32)


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached")


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(O, "K", CK)


def _opt(seed=3, lr=0.1):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    ps[4].data = ps[4].data.contiguous(memory_format=torch.channels_last)
    opt = O.SGD(ps, lr=lr)
    assert opt.numel == NUMEL
    return opt


def _set_grad(opt, seed):
    opt.zero_grad()
    opt.flat_g.copy_(torch.randn(opt.numel, generator=torch.Generator().manual_seed(seed)))


def test_reference_gradient_is_autograd_of_the_penalty():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(37, generator=g, dtype=torch.float64, requires_grad=True)
    a, F, g0 = torch.randn(37, generator=g, dtype=torch.float64), torch.rand(37, generator=g, dtype=torch.float64), torch.randn(37, generator=g, dtype=torch.float64)
    for Fk in (F, None):
        pen = 0.5 * 8.0 * ((1.0 if Fk is None else Fk) * (p - a) ** 2).sum()
        (dp,) = torch.autograd.grad(pen, p)
        torch.testing.assert_close(E.penalty_grad(g0, p.detach(), a, Fk, 8.0), g0 + dp, rtol=1e-14, atol=1e-15)
        assert E.penalty_value(p.detach(), a, Fk, 8.0) == pytest.approx(float(pen.detach()), rel=1e-14)
        for nparts in (1, 3):
            assert E.penalty_partials(p.detach(), a, Fk, nparts).sum() == pytest.approx(float(pen.detach()) / 4.0, rel=1e-14)
    assert E.block_of(36, 37, 1) == 0 and E.block_of(4 * 256, 4 * 600, 2) == 1 and E.block_of(4 * 512, 4 * 600, 2) == 0


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        if nargs > 1:
            assert args[-1] == "hipStream_t stream"
    assert "fisher_accumulate:" in hdr and "ewc_consolidate:" in hdr and "ewc_penalty:" in hdr          # the contract comments
    assert "consolidate.hip" in open(os.path.join(ROOT, "incremental_multimodal_medical_learning_ii_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    for n in (1, 3, 4096, 4100, 65923, 4 * (1 << 20) + 3, 135_000_000):      # one partition for the norm and the penalty
        assert lib.cxrk_ewc_penalty_partials_bytes(n) == lib.cxrk_grad_sqnorm_partials_bytes(n) == 4 * CK.ewc_penalty_nparts(n), n
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert all(callable(getattr(kernels, f)) for f in ("fisher_accumulate", "ewc_consolidate", "ewc_penalty"))
    assert kernels.ewc_penalty_nparts(4100) == 2


def test_constructor_refusals():
    opt = _opt()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            O.EWC(opt, bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            O.EWC(opt, 1.0, gamma=bad)
    with pytest.raises(ValueError, match="fisher"):
        O.EWC(opt, 1.0, fisher="kfac")
    e = O.EWC(opt, 0.0, gamma=0.0)
    assert (e.strength, e.gamma, e.fisher, e.tasks, e.active) == (0.0, 0.0, "empirical", 0, False)


def test_life_cycle_and_refusals(emulated):
    opt = _opt()
    e = O.EWC(opt, 50.0)
    with pytest.raises(ValueError, match="begin_estimate"):
        e.accumulate()                                               # outside an estimate
    with pytest.raises(ValueError, match="accumulate"):
        e.consolidate()                                              # empirical, no estimate at all
    e.begin_estimate()
    with pytest.raises(ValueError, match="accumulate"):
        e.consolidate()                                              # empirical, zero samples: refused, nothing changes
    assert (e.tasks, e.active, e.F, e.anchor) == (0, False, None, None) and e._acc is not None and e.current_penalty() is None
    grads = []
    for seed in (1, 2):
        _set_grad(opt, seed)
        grads.append(opt.flat_g.clone())
        e.accumulate()
    assert e.samples == 2
    p_before = opt.flat_p.clone()
    e.consolidate()
    assert (e.tasks, e.active, e.samples, e._acc) == (1, True, 0, None)
    assert torch.equal(bits(e.anchor), bits(p_before)) and torch.equal(bits(opt.flat_p), bits(p_before))
    acc = E.fisher_accumulate(E.fisher_accumulate(torch.zeros(NUMEL), grads[0]), grads[1])
    ref, _ = E.consolidate(torch.zeros(NUMEL), acc, p_before, 1.0, 0.5)
    assert bool(((e.F.double() - ref).abs() <= 4 * E.gamma_k(2) * ref.abs()).all())      # two accumulations and the merge
    with pytest.raises(ValueError, match="begin_estimate"):
        e.accumulate()                                               # the estimate ended with the consolidation


def test_apply_before_consolidation_issues_no_kernel_call(monkeypatch):
    monkeypatch.setattr(O, "K", NoKernels())
    opt = _opt()
    for fisher in O.FISHERS:
        e = O.EWC(opt, 10.0, fisher=fisher)
        g = opt.flat_g.clone()
        e.apply()
        assert torch.equal(opt.flat_g, g) and e.current_penalty() is None and e._partials is None


def test_gamma_merges_two_consolidations(emulated):
    opt = _opt()
    e = O.EWC(opt, 1.0, gamma=0.25)
    fs = []
    for seed in (1, 2):
        e.begin_estimate()
        _set_grad(opt, seed)
        g = opt.flat_g.clone()
        e.accumulate()
        opt.flat_p.add_(0.01)                                        # the anchor is always the latest parameters
        e.consolidate()
        fs.append(g.double() ** 2)
        assert torch.equal(e.anchor, opt.flat_p)
    assert e.tasks == 2
    ref = 0.25 * fs[0] + fs[1]
    assert bool(((e.F.double() - ref).abs() <= 2 * E.gamma_k(2) * ref).all())
    assert float((e.F.double() - fs[1]).abs().max()) > 1e-3           # the first task's importance is still in there


def test_identity_is_all_ones_fisher_bit_for_bit(emulated):
    a, b = _opt(), _opt()
    ident, ones = O.EWC(a, 3.0, fisher="identity"), O.EWC(b, 3.0)
    ident.consolidate()                                              # no begin_estimate / accumulate needed
    assert ident.F is None and ident._acc is None and ident.active
    ones.begin_estimate()
    b.flat_g.fill_(1.0)
    ones.accumulate()
    ones.consolidate()
    assert bool((ones.F == 1.0).all())
    for opt in (a, b):
        opt.flat_p.add_(torch.randn(NUMEL, generator=torch.Generator().manual_seed(9)) * 0.1)
        _set_grad(opt, 5)
    ident.apply()
    ones.apply()
    assert torch.equal(bits(a.flat_g), bits(b.flat_g)) and torch.equal(bits(ident._partials), bits(ones._partials))
    assert ident.current_penalty() == ones.current_penalty() > 0
    want = E.penalty_value(a.flat_p, ident.anchor, None, 3.0)
    assert ident.current_penalty() == pytest.approx(want, rel=1e-5)


def test_at_the_anchor_the_gradient_is_unchanged_and_the_penalty_zero(emulated):
    opt = _opt()
    e = O.EWC(opt, 1e6)
    e.begin_estimate()
    _set_grad(opt, 1)
    e.accumulate()
    e.consolidate()
    _set_grad(opt, 2)
    g = opt.flat_g.clone()
    e.apply()
    assert bool((opt.flat_g == g).all()) and e.current_penalty() == 0.0


def test_sgd_on_a_zero_task_gradient_contracts_towards_the_anchor(emulated):
    """p' - a = (p - a) (1 - lr * lambda * F) per element: one rounding each for d, F d, the penalty gradient, lr * g and the update"""
    lr, lam = 0.1, 2.0
    opt = _opt(lr=lr)
    e = O.EWC(opt, lam)
    e.begin_estimate()
    _set_grad(opt, 1)
    e.accumulate()
    e.consolidate()
    opt.flat_p.add_(torch.randn(NUMEL, generator=torch.Generator().manual_seed(4)) * 0.05)
    d0, F, a = (opt.flat_p - e.anchor).double(), e.F.double(), e.anchor.double()
    opt.zero_grad()
    e.apply()
    opt.step()
    want = d0 * (1.0 - E.f32(lr) * E.f32(lam) * F)
    got = opt.flat_p.double() - a
    bound = E.gamma_k(4) * (d0.abs() + E.f32(lr) * E.f32(lam) * F * d0.abs()) + E.U * (a.abs() + d0.abs())     # + p' itself, rounded near a
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
    assert float((got - d0).abs().max()) > 1e-3                       # it did contract


def test_state_dict_round_trip_and_refusals(emulated):
    opt = _opt()
    e = O.EWC(opt, 5.0, gamma=0.5)
    sd0 = e.state_dict()
    assert set(sd0) == {"tasks", "gamma", "fisher", "numel"} and sd0["tasks"] == 0
    e.begin_estimate()
    _set_grad(opt, 1)
    e.accumulate()
    e.consolidate()
    sd = e.state_dict()
    assert set(sd) == {"tasks", "gamma", "fisher", "numel", "anchor", "F"}
    assert all(isinstance(v, (int, float, str, torch.Tensor)) for v in sd.values())            # tensors and plain numbers only
    other = O.EWC(_opt(seed=8), 5.0)
    other.load_state_dict(sd)
    assert (other.tasks, other.gamma, other.active) == (1, 0.5, True)
    assert torch.equal(bits(other.F), bits(e.F)) and torch.equal(bits(other.anchor), bits(e.anchor))
    assert other.F.data_ptr() != sd["F"].data_ptr()
    fresh = O.EWC(_opt(), 5.0)
    fresh.load_state_dict(sd0)
    assert not fresh.active and fresh.F is None
    for bad, what in ((dict(sd, F=sd["F"][:-4]), "elements"), (dict(sd, anchor=sd["anchor"].reshape(2, -1)), "elements"),
                      ({k: v for k, v in sd.items() if k != "F"}, "need exactly"), (dict(sd, extra=1), "keys"),
                      ({k: v for k, v in sd.items() if k != "gamma"}, "keys"), (dict(sd, fisher="identity"), "fisher"),
                      (dict(sd, numel=NUMEL + 4), "flat buffer"), (dict(sd, F=sd["F"].double()), "float32")):
        target = O.EWC(_opt(), 5.0)
        with pytest.raises(ValueError, match=what):
            target.load_state_dict(bad)
        assert not target.active and target.F is None and target.anchor is None               # a refused state changes nothing
    small = O.EWC(O.SGD([torch.nn.Parameter(torch.zeros(8))], lr=0.1), 5.0)
    with pytest.raises(ValueError, match="elements"):
        small.load_state_dict(sd)


def test_joint_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    with pytest.raises(ValueError, match="ewc_lambda"):
        C.JointContrastiveTrainer(None, None, ewc_gamma=0.5)
    with pytest.raises(ValueError, match="ewc_lambda"):
        C.JointContrastiveTrainer(None, None, ewc_fisher="identity")


def test_trainer_refuses_the_keys_without_joint_mode():
    for je in ({"ewc_lambda": 10.0}, {"ewc_batches": 4}, {"image_model": None, "ewc_fisher": "identity"}):
        with pytest.raises(ValueError, match="joint mode"):
            TR.Trainer(True, [], [], "standard", 1e-3, "cpu", None, bert_encoder=object(), joint_encoders=je)
    im = object()
    with pytest.raises(ValueError, match="ewc_lambda"):
        TR.joint_options({"image_model": im, "ewc_gamma": 0.5})
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="ewc_batches"):
            TR.joint_options({"image_model": im, "ewc_lambda": 1.0, "ewc_batches": bad})
    assert TR.joint_options({"image_model": im, "ewc_lambda": 1.0, "ewc_batches": 3})[1]["ewc_batches"] == 3
    assert TR.joint_options({"image_model": im})[1]["ewc_batches"] is None and TR.joint_options(None)[1]["ewc_batches"] is None


def test_drivers_arguments():
    a = drivers.parse_args(["class-inc", "--joint"])
    assert drivers.continual_from_args(a) == {}
    a = drivers.parse_args(["class-inc", "--joint", "--cl", "ewc"])
    assert drivers.continual_from_args(a) == {"ewc_lambda": drivers.EWC_LAMBDA}
    a = drivers.parse_args(["data-inc", "--joint", "--cl", "ewc", "--ewc-lambda", "3e5", "--ewc-batches", "8", "--ewc-gamma", "0.9",
                            "--ewc-fisher", "identity"])
    assert drivers.continual_from_args(a) == {"ewc_lambda": 3e5, "ewc_batches": 8, "ewc_gamma": 0.9, "ewc_fisher": "identity"}
    for argv in (["class-inc", "--cl", "ewc"],                                     # needs --joint
                 ["zero-joint", "--joint", "--cl", "ewc"],                          # a single task: nothing to consolidate between
                 ["class-inc", "--joint", "--ewc-lambda", "10"],                    # the options need --cl ewc
                 ["class-inc", "--joint", "--cl", "profCL", "--ewc-batches", "2"],
                 ["class-inc", "--joint", "--cl", "ewc", "--ewc-fisher", "kfac"],
                 ["class-inc", "--joint", "--cl", "ewc", "--ewc-gamma", "1.5"],
                 ["class-inc", "--joint", "--cl", "ewc", "--ewc-lambda", "-1"],
                 ["class-inc", "--joint", "--cl", "ewc", "--ewc-batches", "0"]):
        with pytest.raises(SystemExit):
            drivers.parse_args(argv)
        with pytest.raises(SystemExit):
            drivers.main(argv)
    assert math.isfinite(drivers.EWC_LAMBDA) and drivers.EWC_LAMBDA >= 1e3       # F is a squared mean gradient: strengths are large
