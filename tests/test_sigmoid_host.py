"""What the pairwise sigmoid loss promises without a device: the float64 reference's identities (tests/sigmoid_ref.py), the
cancellation the positive branch must avoid, the two entry points in the header and the ctypes table, `drivers --contrastive-loss`
parsing, the ValueError paths before any kernel or collective, and the CPU emulation of the kernels against the reference."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_sigmoid as CK  # noqa: E402
import sigmoid_ref as R  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, functional as Fh  # noqa: E402

ENTRY_POINTS = {"cxrk_sigmoid_pairs_fwd_bwd_inplace": 11, "cxrk_sigmoid_pairs_loss": 6}
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
THETA0, BIAS0 = F32(math.log(1 / 0.07)), -10.0


def batch_keys(Bg):
    keys = torch.arange(Bg, dtype=torch.int64) * 7 - 3
    keys[0] = keys[3] = keys[Bg - 1] = 5
    keys[1] = keys[2] = (1 << 40)
    return keys


@pytest.mark.parametrize("Bg", [8, 24, 260])
@pytest.mark.parametrize("keyed", [False, True])
def test_reference_identities_and_cpu_emulation(Bg, keyed):
    """float64: the closed forms and the BCE identity (asserted inside `sigmoid_grads`); and the single-process head on the emulated
    kernels reproduces loss, d theta, d b and the embedding gradients"""
    gen = torch.Generator().manual_seed(Bg)
    img, txt = torch.randn(Bg, 32, generator=gen), torch.randn(Bg, 32, generator=gen)
    keys = batch_keys(Bg) if keyed else None
    for theta0, b0 in ((THETA0, BIAS0), (0.0, 3.0)):
        ref = R.sigmoid_grads(img, txt, theta0, b0, keys)
        assert abs(ref["dtheta"]) <= ref["mag_theta"] and abs(ref["db"]) <= ref["mag_b"]
        assert int(ref["pos"].sum()) == (Bg + 8 if keyed else Bg)            # a group of 3 and a group of 2: 9 + 4 + (Bg - 5)
        old = Fh.K
        Fh.K = CK
        try:
            i, t = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
            th, b = torch.tensor([theta0], requires_grad=True), torch.tensor([b0], requires_grad=True)
            out = Fh.sigmoid_pairs_loss(i, t, th, b, keys=keys)
            out.backward()
        finally:
            Fh.K = old
        assert abs(out.item() - ref["loss"]) <= 1e-5 * abs(ref["loss"])
        assert abs(float(th.grad) - ref["dtheta"]) <= 2e-5 * ref["mag_theta"]
        assert abs(float(b.grad) - ref["db"]) <= 2e-5 * ref["mag_b"]
        torch.testing.assert_close(i.grad.double(), ref["dimg"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(t.grad.double(), ref["dtxt"], rtol=1e-4, atol=1e-6)


def test_block_reference_with_a_row_that_has_no_positive():
    gen = torch.Generator().manual_seed(3)
    Cb = torch.rand(5, 7, generator=gen) * 2 - 1
    kc = torch.tensor([4, 9, 4, -1, 1 << 40, 9, 7], dtype=torch.int64)
    kr = torch.tensor([4, 9, 1 << 40, 12345, -1], dtype=torch.int64)          # row 3 matches no column
    tg, l, gx, g = R.block(Cb, THETA0, BIAS0, 0, kr, kc)
    pos = R.positives(5, 7, 0, kr, kc)
    assert pos.sum(1).tolist() == [2, 2, 1, 0, 1]
    assert bool((g[3] > 0).all()) and bool((g[pos] < 0).all()) and bool((g[~pos] > 0).all())
    t = math.exp(THETA0)
    torch.testing.assert_close(gx, g * t * Cb.double(), rtol=1e-14, atol=0)
    torch.testing.assert_close(tg, t * g, rtol=1e-14, atol=0)
    for a, want in zip(R.block_fp32(Cb, THETA0, BIAS0, 0, kr, kc), (tg, l, gx, g)):   # the kernel's formulas in fp32
        assert float((a.double() - want).abs().max()) <= 5.8e-6 * float(want.abs().max())


def test_positive_branch_does_not_cancel():
    """x > 20 on a positive pair: -sigmoid(-x) is a non-zero gradient; sigmoid(x) - 1 is exactly 0 in fp32"""
    x = torch.tensor([[21.0, 30.0, 60.0]], dtype=torch.float64)
    pos = torch.ones(1, 3, dtype=torch.bool)
    _, g = R.closed_form(x, pos)
    assert bool((g < 0).all())
    torch.testing.assert_close(g, -torch.exp(-x), rtol=1e-8, atol=0)
    assert (torch.sigmoid(x.float()) - 1.0).tolist() == [[0.0, 0.0, 0.0]]                # what the kernel must not compute
    Cb = torch.tensor([[1.0]])                                                          # the kernel's formulas: cos = 1, t = 31, b = -10
    tg, l, _, g32 = R.block_fp32(Cb, F32(math.log(31.0)), -10.0)
    assert float(g32) < 0 and abs(float(g32) / -math.exp(-21.0) - 1) < 1e-4 and float(l) > 0


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert args[-1] == "hipStream_t stream"
        assert not any(re.search(r"\bws(_bytes)?\b", a) for a in args), name             # no workspace: the partial sums are an output
    assert not [n for n in _lib.SIGNATURES if n.endswith("_ws_bytes") and "sigmoid" in n]
    assert "3 * rows * nchunk" in hdr and "nchunk = ceil(cols / 1024)" in hdr            # the size of the partials is documented
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert kernels.sigmoid_partials_numel(3, 1030) == 3 * 3 * 2 and kernels.sigmoid_partials_numel(8, 1024) == 24


def test_drivers_arguments():
    ap = drivers.make_parser()
    a = ap.parse_args(["class-inc", "--joint"])
    assert a.contrastive_loss is None and a.sigmoid_bias is None
    a = ap.parse_args(["zero-joint", "--joint", "--contrastive-loss", "sigmoid", "--sigmoid-bias", "-4.5", "--learn-temperature"])
    assert a.contrastive_loss == "sigmoid" and a.sigmoid_bias == -4.5 and a.learn_temperature
    with pytest.raises(SystemExit):
        ap.parse_args(["zero-joint", "--joint", "--contrastive-loss", "softmax"])
    with pytest.raises(SystemExit, match="--joint"):
        drivers.main(["class-inc", "--contrastive-loss", "sigmoid"])
    with pytest.raises(SystemExit, match="--joint"):
        drivers.main(["class-inc", "--sigmoid-bias", "-10"])
    with pytest.raises(SystemExit, match="--contrastive-loss sigmoid"):
        drivers.main(["class-inc", "--joint", "--sigmoid-bias", "-10"])
    with pytest.raises(SystemExit, match="--contrastive-loss sigmoid"):
        drivers.main(["class-inc", "--joint", "--contrastive-loss", "infonce", "--sigmoid-bias", "-10"])


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached before the arguments were validated")


def test_functional_arguments_are_validated_before_anything_runs(monkeypatch):
    monkeypatch.setattr(Fh, "K", NoKernels())
    img, txt = torch.zeros(8, 16), torch.zeros(8, 16)
    th, b = torch.zeros(1), torch.zeros(1)
    bad_scalars = (torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64), torch.zeros(2), torch.zeros(1, 1),
                   torch.zeros(1, device="meta"), 2.66, [2.66], None)
    for bad in bad_scalars:
        with pytest.raises(ValueError, match="log_scale"):
            Fh.sigmoid_pairs_loss(img, txt, bad, b)
        with pytest.raises(ValueError, match="logit_bias"):
            Fh.sigmoid_pairs_loss(img, txt, th, bad)
    with pytest.raises(ValueError, match="text embeddings"):
        Fh.sigmoid_pairs_loss(img, torch.zeros(8, 12), th, b)
    with pytest.raises(ValueError, match="multiples of 4"):
        Fh.sigmoid_pairs_loss(torch.zeros(6, 16), torch.zeros(6, 16), th, b)
    with pytest.raises(ValueError, match="multiples of 4"):
        Fh.sigmoid_pairs_loss(torch.zeros(8, 18), torch.zeros(8, 18), th, b)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.int64), torch.zeros(8, dtype=torch.int64, device="meta"), [0] * 8):
        with pytest.raises(ValueError, match="keys"):
            Fh.sigmoid_pairs_loss(img, txt, th, b, keys=bad)


def test_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    monkeypatch.setattr(Fh, "K", NoKernels())
    with pytest.raises(ValueError, match="loss must be"):
        C.JointContrastiveTrainer(None, None, loss="softmax")
    with pytest.raises(ValueError, match="sigmoid_bias"):
        C.JointContrastiveTrainer(None, None, sigmoid_bias=-10.0)
    with pytest.raises(ValueError, match="sigmoid_bias"):
        C.JointContrastiveTrainer(None, None, loss="infonce", sigmoid_bias=0.0)
    with pytest.raises(ValueError, match="sigmoid_bias"):
        C.JointContrastiveTrainer(None, None, loss="sigmoid", sigmoid_bias=float("nan"))
    with pytest.raises(ValueError, match="temperature"):
        C.JointContrastiveTrainer(None, None, loss="sigmoid", temperature=0.0)
    with pytest.raises(ValueError, match="log_scale_bounds"):
        C.JointContrastiveTrainer(None, None, loss="sigmoid", learn_temperature=True, log_scale_bounds=(2.0, 1.0))
    assert C.LOSSES == ("infonce", "sigmoid") and C.SIGMOID_BIAS == -10.0
    t = object.__new__(C.JointContrastiveTrainer)
    t.loss, t.logit_scale, t.logit_bias, t.temperature = "infonce", None, None, 0.07
    assert t.current_bias() is None and t.current_temperature() == 0.07
    t.loss, t._sigmoid_consts = "sigmoid", (torch.tensor([THETA0]), torch.tensor([-10.0]))
    assert t.current_bias() == -10.0 and t.current_temperature() == 0.07
    t.logit_scale, t.logit_bias = torch.nn.Parameter(torch.tensor([math.log(50.0)])), torch.nn.Parameter(torch.tensor([-2.5]))
    assert t.current_bias() == -2.5 and abs(t.current_temperature() - 0.02) < 1e-8
