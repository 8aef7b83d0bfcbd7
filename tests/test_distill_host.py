"""What similarity distillation promises without a device: the fp32 restatement of the kernel's formulas against the
float64 reference (tests/distill_ref.py) with the two bounds the GPU tests use, exact zeros for identical blocks, the entry points in
the header and the ctypes table, `functional.distill_loss` on the emulated wrappers (tests/cpu_kernels_distill.py) against float64
autograd, and the ValueError / SystemExit paths of the trainers and the drivers that need no kernel."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_distill as CK  # noqa: E402
import distill_ref as R  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402

ENTRY_POINTS = {"cxrk_distill_row_stats": 13, "cxrk_distill_grad_inplace": 11}
#          rows cols
SHAPES = [(1, 1), (8, 8), (8, 24), (5, 7), (3, 1030), (4, 260)]
SCALES = [1.0, 1.0 / 0.07, 100.0]
TEACHERS = ["independent", "perturbed"]


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached")


@pytest.mark.parametrize("teacher", TEACHERS)
@pytest.mark.parametrize("scale", SCALES, ids=["x1", "tau0.07", "x100"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_fp32_formulas_against_float64(rows, cols, scale, teacher):
    """kl within 2e-5 of max_i(|lse| + |lse_t| + sum pt |St - S|), the gradient block within 2e-5 of max(p + q + pt + qt), and
    kl >= -bound (the true value is >= 0; fp32 gives values like -2e-6 where float64 gives 1e-14)"""
    S, St = R.block_pair(rows, cols, scale, teacher)
    lse64, lset64, kl64, mag = R.block_stats(S, St)
    lse, lse_t, kl = R.block_stats_fp32(S, St)
    bound = R.TOL * float(mag.max())
    err = float((kl.double() - kl64).abs().max())
    print(f"kl err {err:.3e} = {err / float(mag.max()):.3e} of the scale {float(mag.max()):.3e}; min kl {float(kl.min()):.3e}")
    assert err <= bound
    assert float(kl.min()) >= -bound and float(kl64.min()) >= -1e-12
    assert float((lse.double() - lse64).abs().max()) <= R.TOL * float(lse64.abs().max().clamp_min(1e-20))
    assert float((lse_t.double() - lset64).abs().max()) <= R.TOL * float(lset64.abs().max().clamp_min(1e-20))
    lc, ltc = R.column_lses(S, St)
    G64, gmag = R.block_grad(S, St, lse, lc, lse_t, ltc)
    G = R.block_grad_fp32(S, St, lse, lc, lse_t, ltc)
    gerr = float((G.double() - G64).abs().max())
    print(f"grad err {gerr:.3e} = {gerr / gmag:.3e} of the scale {gmag:.3e}")
    assert gerr <= R.TOL * gmag


@pytest.mark.parametrize("scale", SCALES, ids=["x1", "tau0.07", "x100"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_identical_blocks_give_exact_zeros(rows, cols, scale):
    S, St = R.block_pair(rows, cols, scale, "identical")
    assert torch.equal(S, St)
    lse, lse_t, kl = R.block_stats_fp32(S, St)
    assert torch.equal(lse, lse_t) and bool((kl == 0.0).all())
    lc, ltc = R.column_lses(S, St)
    assert torch.equal(lc, ltc)
    assert bool((R.block_grad_fp32(S, St, lse, lc, lse_t, ltc) == 0.0).all())
    kl_e = CK.distill_row_stats(S, St)[2]
    assert bool((kl_e == 0.0).all()) and bool((CK.distill_grad_inplace(S.clone(), St, lse, lc, lse_t, ltc) == 0.0).all())


def test_reference_gradient_is_the_closed_form():
    """dL_d/dS_ij = (p - pt + q - qt) / (2 Bg): autograd of the float64 loss against the formula of the issue"""
    g = torch.Generator().manual_seed(5)
    S = torch.randn(6, 6, generator=g, dtype=torch.float64, requires_grad=True)
    St = torch.randn(6, 6, generator=g, dtype=torch.float64)
    L = ((torch.softmax(St, 1) * (torch.log_softmax(St, 1) - torch.log_softmax(S, 1))).sum()
         + (torch.softmax(St, 0) * (torch.log_softmax(St, 0) - torch.log_softmax(S, 0))).sum()) / 12
    (dS,) = torch.autograd.grad(L, S)
    Sd = S.detach()
    G, _ = R.block_grad(Sd, St, torch.logsumexp(Sd, 1), torch.logsumexp(Sd, 0), torch.logsumexp(St, 1), torch.logsumexp(St, 0))
    torch.testing.assert_close(dS, G / 12, rtol=1e-12, atol=1e-14)
    _, _, kl, _ = R.block_stats(Sd, St)
    _, _, klT, _ = R.block_stats(Sd.T, St.T)
    assert float(L.detach()) == pytest.approx(float((kl.sum() + klT.sum()) / 12), rel=1e-12)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert args[-1] == "hipStream_t stream"
    assert " * distill:" in hdr and "IDENTICAL INPUTS GIVE EXACT ZEROS" in hdr                     # the contract comment
    assert "distill.hip" in open(os.path.join(ROOT, "incremental_multimodal_medical_learning_ii_amd", "csrc", "Makefile")).read()
    assert not [n for n in _lib.SIGNATURES if "distill" in n and (n.endswith("_ws_bytes") or n.endswith("_bytes"))]   # no scratch memory
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ENTRY_POINTS)
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert callable(kernels.distill_row_stats) and callable(kernels.distill_grad_inplace)


@pytest.mark.parametrize("B", [8, 12])
def test_functional_on_the_emulated_wrappers(monkeypatch, B):
    """single process, emulated wrappers: weight * L_d and both gradients against float64 autograd; `weight` scales linearly; the
    teacher gets no gradient and one that requires grad is refused; shape refusals; no collective is reached"""
    import torch.distributed as dist
    monkeypatch.setattr(Fh, "K", CK)
    for name in ("all_reduce", "all_gather_into_tensor"):
        monkeypatch.setattr(dist, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("a collective in the single-process path")))
    D, tau = 128, 0.07
    mk = lambda tag: torch.from_numpy(syn._normal(f"distill.host.{tag}", (B, D)))   # noqa: E731
    img, txt, it, tt = mk("I"), mk("T"), mk("It"), mk("Tt")
    ref = R.distill_grads(img, txt, it, tt, tau)
    assert ref["loss"] > 1e-3
    for weight in (1.0, 2.5):
        a, b = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        d = Fh.distill_loss(a, b, it, tt, tau, weight=weight)
        assert d.shape == () and float(d.detach()) == pytest.approx(weight * ref["loss"], rel=2e-5)
        d.backward()
        for got, want in ((a.grad, ref["dimg"]), (b.grad, ref["dtxt"])):
            err = float((got.double() - weight * want).abs().max() / (weight * want).abs().max())
            assert err < 2e-5, err
    w, u = Fh._distill_pair(img.clone().requires_grad_(True), txt, it, tt, tau, 0.0)
    assert float(w) == 0.0 and float(u) == pytest.approx(ref["loss"], rel=2e-5) and not u.requires_grad
    z = Fh.distill_loss(img.clone().requires_grad_(True), txt.clone(), img.clone(), txt.clone(), tau)     # the teacher IS the student
    assert float(z.detach()) == 0.0
    with pytest.raises(ValueError, match="requires grad"):
        Fh.distill_loss(img, txt, it.clone().requires_grad_(True), tt, tau)
    with pytest.raises(ValueError, match="requires grad"):
        Fh.distill_loss(img, txt, it, tt.clone().requires_grad_(True), tau)
    monkeypatch.setattr(Fh, "K", NoKernels())           # the refusals below are raised before any kernel
    with pytest.raises(ValueError, match="multiples of 4"):
        Fh.distill_loss(img[:B - 1], txt[:B - 1], it[:B - 1], tt[:B - 1], tau)
    with pytest.raises(ValueError, match="multiples of 4"):
        Fh.distill_loss(img[:, :126], txt[:, :126], it[:, :126], tt[:, :126], tau)
    with pytest.raises(ValueError, match="text embeddings"):
        Fh.distill_loss(img, txt[:4], it, tt, tau)
    with pytest.raises(ValueError, match="teacher"):
        Fh.distill_loss(img, txt, it[:4], tt[:4], tau)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            Fh.distill_loss(img, txt, it, tt, tau, weight=bad)
    for bad in (0.0, -0.07, float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            Fh.distill_loss(img, txt, it, tt, bad)


def test_joint_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    with pytest.raises(ValueError, match="without distill_weight"):
        C.JointContrastiveTrainer(None, None, distill_temperature=0.1)
    for bad in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="distill_weight"):
            C.JointContrastiveTrainer(None, None, distill_weight=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="distill_temperature"):
            C.JointContrastiveTrainer(None, None, distill_weight=1.0, distill_temperature=bad)
    assert C.check_distill_options(None, None) == (None, None)
    assert C.check_distill_options(0, None) == (0.0, None) and C.check_distill_options(2, 0.5) == (2.0, 0.5)


def test_current_distill_is_none_before_a_snapshot():
    """the accessors and `snapshot_teacher`'s refusal on a bare object: nothing here needs the encoders"""
    t = C.JointContrastiveTrainer.__new__(C.JointContrastiveTrainer)
    t.distill_weight, t.teacher, t._last_distill, t._distill_off = None, None, None, False
    assert t.current_distill() is None and not t._distilling()
    with pytest.raises(ValueError, match="without distill_weight"):
        t.snapshot_teacher()
    t.distill_weight = 1.0
    assert t.current_distill() is None and not t._distilling()          # a weight alone runs no teacher
    t._last_distill = torch.tensor(0.25)
    assert t.current_distill() == 0.25


def test_trainer_refuses_the_keys_without_joint_mode():
    for je in ({"distill_weight": 1.0}, {"distill_temperature": 0.1}, {"image_model": None, "distill_weight": 0.5}):
        with pytest.raises(ValueError, match="joint mode"):
            TR.Trainer(True, [], [], "standard", 1e-3, "cpu", None, bert_encoder=object(), joint_encoders=je)
    im = object()
    with pytest.raises(ValueError, match="without it"):
        TR.joint_options({"image_model": im, "distill_temperature": 0.1})
    with pytest.raises(ValueError, match="distill_weight"):
        TR.joint_options({"image_model": im, "distill_weight": -2.0})
    with pytest.raises(ValueError, match="distill_temperature"):
        TR.joint_options({"image_model": im, "distill_weight": 1.0, "distill_temperature": 0.0})
    # (the removed checker returned None for what it accepted; the one function returns what it passes on)
    step, own = TR.joint_options({"image_model": im, "distill_weight": 0.0, "distill_temperature": 0.1})
    assert (step["distill_weight"], step["distill_temperature"]) == (0.0, 0.1) and own["image_model"] is im
    assert "distill_weight" not in TR.joint_options({"image_model": im})[0] and TR.joint_options(None)[0] == {}
    t = TR.Trainer.__new__(TR.Trainer)
    t._joint = None
    with pytest.raises(ValueError, match="distill_weight"):
        t.snapshot_teacher()


def test_drivers_arguments():
    a = drivers.parse_args(["class-inc", "--joint"])
    assert drivers.continual_from_args(a) == {}
    a = drivers.parse_args(["class-inc", "--joint", "--cl", "lwf"])
    assert drivers.continual_from_args(a) == {"distill_weight": 1.0} and drivers.DISTILL_WEIGHT == 1.0     # the whole dict: no "ewc_*" key
    a = drivers.parse_args(["data-inc", "--joint", "--cl", "lwf", "--distill-weight", "0.5", "--distill-temperature", "0.2"])
    assert drivers.continual_from_args(a) == {"distill_weight": 0.5, "distill_temperature": 0.2}
    a = drivers.parse_args(["data-inc", "--joint", "--cl", "lwf", "--distill-weight", "0"])
    assert drivers.continual_from_args(a) == {"distill_weight": 0.0}
    for argv in (["class-inc", "--cl", "lwf"],                                      # needs --joint
                 ["zero-joint", "--joint", "--cl", "lwf"],                           # a single task: no teacher to take between tasks
                 ["class-inc", "--joint", "--distill-weight", "1"],                  # the options need --cl lwf
                 ["class-inc", "--joint", "--cl", "ewc", "--distill-temperature", "0.1"],
                 ["class-inc", "--joint", "--cl", "lwf", "--distill-weight", "-1"],
                 ["class-inc", "--joint", "--cl", "lwf", "--distill-weight", "inf"],
                 ["class-inc", "--joint", "--cl", "lwf", "--distill-temperature", "0"]):
        with pytest.raises(SystemExit) as e:
            drivers.parse_args(argv)
        assert e.value.code == 2                                                     # a parser error
        with pytest.raises(SystemExit):
            drivers.main(argv)
