"""What the learnable-temperature feature promises without a device: `drivers --learn-temperature` parsing, the ValueError paths before
any kernel or collective, the new entry points in the header and the ctypes table, the float64 identity d L / d theta = sum dL/dS o S
of tests/logit_scale_ref.py, and the CPU emulation of the kernels against it."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cpu_kernels_logit_scale as CK  # noqa: E402
import logit_scale_ref as R  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, functional as Fh  # noqa: E402

ENTRY_POINTS = {"cxrk_infonce_row_lse_scaled": 12, "cxrk_infonce_grad_scaled_inplace": 10, "cxrk_multipos_row_stats_scaled": 14,
                "cxrk_multipos_grad_scaled_inplace": 12, "cxrk_logit_scale_grad": 9, "cxrk_clamp_inplace": 5}


def test_drivers_learn_temperature_argument():
    ap = drivers.make_parser()
    assert ap.parse_args(["class-inc", "--joint"]).learn_temperature is False
    assert ap.parse_args(["class-inc", "--joint", "--learn-temperature"]).learn_temperature is True
    with pytest.raises(SystemExit, match="--joint"):                                 # rejected the way --positives is
        drivers.main(["class-inc", "--learn-temperature"])


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert args[-1] == "hipStream_t stream"
        assert not any(re.search(r"\bws(_bytes)?\b", a) for a in args), name         # no workspace: the partial sums are an output
    assert not [n for n in _lib.SIGNATURES if n.endswith("_ws_bytes") and ("scale" in n or "clamp" in n)]
    assert "ceil(cols / 1024)" in hdr                                                # the size of the partials is documented


def test_log_scale_is_validated_before_anything_runs(monkeypatch):
    class NoKernels:
        def __getattr__(self, name):
            raise AssertionError(f"kernel wrapper {name} was reached before log_scale was validated")
    monkeypatch.setattr(Fh, "K", NoKernels())
    img, txt = torch.zeros(8, 16), torch.zeros(8, 16)
    for bad in (torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64), torch.zeros(2), torch.zeros(1, 1),
                torch.zeros(1, device="meta"), 2.66, [2.66]):
        with pytest.raises(ValueError, match="log_scale"):
            Fh.infonce_loss(img, txt, 0.07, None, log_scale=bad)


def test_trainer_arguments():
    with pytest.raises(ValueError, match="log_scale_bounds"):
        C.JointContrastiveTrainer(None, None, learn_temperature=True, log_scale_bounds=(2.0, 1.0))
    with pytest.raises(ValueError, match="log_scale_bounds"):
        C.JointContrastiveTrainer(None, None, learn_temperature=True, log_scale_bounds=(0.0, float("nan")))
    with pytest.raises(ValueError, match="temperature"):
        C.JointContrastiveTrainer(None, None, temperature=0.0, learn_temperature=True)
    assert C.LOG_SCALE_BOUNDS == (0.0, math.log(100.0))
    t = object.__new__(C.JointContrastiveTrainer)
    t.logit_scale, t.temperature = None, 0.07
    assert t.current_temperature() == 0.07
    t.logit_scale = torch.nn.Parameter(torch.tensor([math.log(50.0)]))
    assert abs(t.current_temperature() - 0.02) < 1e-8


@pytest.mark.parametrize("Bg", [8, 24, 64, 260])
@pytest.mark.parametrize("keyed", [False, True])
def test_reference_identity_and_cpu_emulation(Bg, keyed):
    """float64: autograd's d theta equals sum_ij dL/dS_ij S_ij (asserted inside `scaled_grads`); and the single-process head on the
    emulated kernels reproduces loss and d theta"""
    g = torch.Generator().manual_seed(Bg)
    img, txt = torch.randn(Bg, 32, generator=g), torch.randn(Bg, 32, generator=g)
    keys = None
    if keyed:
        keys = torch.arange(Bg, dtype=torch.int64) * 7 - 3
        keys[0] = keys[3] = keys[Bg - 1] = 5
        keys[1] = keys[2] = (1 << 40)
    theta0 = float(torch.tensor(math.log(1 / 0.07), dtype=torch.float32))
    loss, di, dt, dth, mag = R.scaled_grads(img, txt, theta0, keys)
    assert abs(dth) <= mag
    import incremental_multimodal_medical_learning_ii_amd.functional as F2
    old = F2.K
    F2.K = CK
    try:
        i, t = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        th = torch.tensor([theta0], requires_grad=True)
        out = F2.infonce_loss(i, t, 99.0, keys=keys, log_scale=th)
        out.backward()
    finally:
        F2.K = old
    assert abs(out.item() - loss) < 1e-5
    assert abs(float(th.grad) - dth) <= 2e-5 * mag                                   # fp32 sums: the kernel tests' bound for d theta
    torch.testing.assert_close(i.grad.double(), di, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(t.grad.double(), dt, rtol=1e-4, atol=1e-6)
    x = torch.tensor([-1.0, 0.0, 2.0, 9.0, float("nan")])
    CK.clamp_inplace(x, 0.0, math.log(100.0))
    assert x[:4].tolist() == [0.0, 0.0, 2.0, float(torch.tensor(math.log(100.0)))] and math.isnan(x[4].item())
