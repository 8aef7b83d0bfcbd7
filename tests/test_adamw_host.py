"""What clipping, decoupled decay and the schedule promise without a device: the float64 reference
(tests/optim_ref.py) pinned to `torch.optim.AdamW` + `torch.nn.utils.clip_grad_norm_`, the entry points in the header and the ctypes
table, `optim.LRSchedule` against its closed form, the decay mask of a CPU-built `optim.AdamW`, and the ValueError / SystemExit paths
that need no kernel."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import optim_ref as R  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, optim as O  # noqa: E402

ENTRY_POINTS = {"cxrk_grad_sqnorm_partials_bytes": 1, "cxrk_grad_sqnorm": 5, "cxrk_adamw_clipped": 18}
SHAPES = [(1,), (2,), (5,), (21,), (4, 3, 3, 3)]
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.999, 1e-8, 0.1


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]


@pytest.mark.parametrize("clip", ["active", "inactive", "none"])
def test_reference_is_torch_adamw_behind_clip_grad_norm(clip):
    """float64, three steps, two param groups (decay: the tensors with ndim >= 2 and the 21-vector; none: the rest)"""
    params = [torch.nn.Parameter(t.clone()) for t in _tensors(0)]
    decays = [False, False, False, True, True]
    opt = torch.optim.AdamW([{"params": [p for p, d in zip(params, decays) if d], "weight_decay": WD},
                             {"params": [p for p, d in zip(params, decays) if not d], "weight_decay": 0.0}],
                            lr=LR, betas=(B1, B2), eps=EPS)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
    mask = torch.cat([torch.full((math.prod(s),), d) for s, d in zip(SHAPES, decays)])
    p, m, v = flat(params), torch.zeros(mask.numel(), dtype=torch.float64), torch.zeros(mask.numel(), dtype=torch.float64)
    for step in range(1, 4):
        grads = _tensors(step)
        total = math.sqrt(sum(float((g ** 2).sum()) for g in grads))
        max_norm = {"active": 0.5 * total, "inactive": 2.0 * total, "none": None}[clip]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        p, m, v, norm, coef = R.adamw_step(p, flat(grads), m, v, mask, LR, B1, B2, EPS, WD, step, max_norm=max_norm)
        if max_norm is not None:
            assert abs(norm - float(tn)) <= 1e-14 * norm
            assert (coef == 1.0) if clip == "inactive" else abs(coef - 0.5) < 1e-6
        else:
            assert coef == 1.0
        torch.testing.assert_close(p, flat(params), rtol=1e-13, atol=1e-15)
    # grad_scale multiplies the gradient before the norm is taken
    a = R.adamw_step(p, flat(grads), m, v, mask, LR, B1, B2, EPS, WD, 4, grad_scale=0.5, max_norm=0.1)
    b = R.adamw_step(p, 0.5 * flat(grads), m, v, mask, LR, B1, B2, EPS, WD, 4, max_norm=0.1)
    assert a[3] == 0.5 * R.grad_norm(flat(grads)) and abs(a[3] - b[3]) <= 1e-15 * a[3]
    torch.testing.assert_close(a[0], b[0], rtol=1e-13, atol=1e-15)


def test_reference_non_finite_coefficients():
    assert R.clip_coef(float("inf"), 1.0) == 0.0 and math.isnan(R.clip_coef(float("nan"), 1.0))
    assert R.clip_coef(3.0, float("inf")) == 1.0 and R.clip_coef(3.0, None) == 1.0 and R.clip_coef(3.0, 0.0) == 1.0
    g = torch.tensor([1.0, float("inf")], dtype=torch.float64).requires_grad_(True)
    g.grad = g.detach().clone()
    torch.nn.utils.clip_grad_norm_([g], 1.0, error_if_nonfinite=False)
    assert g.grad[0] == 0.0 and math.isnan(float(g.grad[1]))          # what the kernel must reproduce: coef 0, inf * 0


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
    assert "grad_sqnorm:" in hdr and "adamw_clipped:" in hdr                             # the contract comments
    lib = _lib.load()
    # the partition is a function of n alone: one block per 1024 groups of four, at most 1024
    for n, parts in ((1, 1), (3, 1), (4096, 1), (4100, 2), (65923, 17), (4 * (1 << 20) + 3, 1024), (135_000_000, 1024)):
        assert lib.cxrk_grad_sqnorm_partials_bytes(n) == 4 * parts, n
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert callable(kernels.grad_sqnorm) and callable(kernels.adamw_clipped) and kernels.grad_sqnorm_nparts(4100) == 2


SCHEDULES = [dict(warmup_steps=0), dict(warmup_steps=4), dict(warmup_steps=4, total_steps=20, decay="linear"),
             dict(warmup_steps=4, total_steps=20, decay="cosine", min_lr_ratio=0.1), dict(total_steps=11, decay="cosine"),
             dict(warmup_steps=6, total_steps=6, decay="linear", min_lr_ratio=0.5)]


@pytest.mark.parametrize("kw", SCHEDULES)
def test_lr_schedule_against_the_closed_form(kw):
    base = 3e-4
    s = O.LRSchedule(base, **kw)
    w, total = kw.get("warmup_steps", 0), kw.get("total_steps") or 40
    for step in sorted({1, max(w, 1), w + 1, (w + total) // 2, total, total + 5}):
        assert s(step) == pytest.approx(R.lr_at(step, base, **kw), rel=1e-15, abs=0), step
    if w:
        assert s(1) == base / w and s(w) == base
    kind, mn = kw.get("decay", "constant"), kw.get("min_lr_ratio", 0.0)
    if kind == "constant":
        assert s(w + 1) == base and s(total + 5) == base
    else:
        mid = w + (total - w) // 2
        if (total - w) % 2 == 0 and total > w:
            assert s(mid) == pytest.approx(base * (mn + (1 - mn) * 0.5), rel=1e-12)  # both kinds pass through the middle at t = 1/2
        last = total if total > w else total + 1                            # warmup up to the last step: the floor follows it
        assert s(last) == pytest.approx(base * mn, abs=1e-20) and s(total + 5) == s(last)
        assert all(s(k + 1) <= s(k) * (1 + 1e-15) for k in range(max(w, 1), total + 3))
    with pytest.raises(ValueError):
        s(0)


def test_lr_schedule_refusals():
    for kind in ("linear", "cosine"):
        with pytest.raises(ValueError, match="total_steps"):
            O.LRSchedule(1e-3, decay=kind)
    with pytest.raises(ValueError, match="warmup_steps"):
        O.LRSchedule(1e-3, warmup_steps=11, total_steps=10)
    with pytest.raises(ValueError, match="decay"):
        O.LRSchedule(1e-3, decay="exponential")
    with pytest.raises(ValueError, match="min_lr_ratio"):
        O.LRSchedule(1e-3, min_lr_ratio=1.5)
    with pytest.raises(ValueError, match="warmup_steps"):
        O.LRSchedule(1e-3, warmup_steps=-1)


def _cpu_params():
    g = torch.Generator().manual_seed(3)
    shapes = [(1,), (7, 3), (2,), (5,), (4, 3, 3, 3), (6,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    ps[4].data = ps[4].data.contiguous(memory_format=torch.channels_last)
    return ps


def _expected_mask(opt, decays):
    want = torch.zeros(opt.numel // 4, dtype=torch.uint8)
    base = opt.flat_p.data_ptr()
    for p, d in zip(opt.params, decays):
        o = (p.data_ptr() - base) // 4
        assert o % 4 == 0
        want[o // 4:o // 4 + (p.numel() + 3) // 4] = int(d)
    return want


def test_decay_mask_of_a_cpu_optimiser():
    ps = _cpu_params()
    opt = O.AdamW(ps, lr=1e-3)
    assert opt.weight_decay == 0.01 and opt.max_grad_norm is None
    assert opt.decay_mask.dtype == torch.uint8 and opt.decay_mask.numel() == opt.numel // 4 == (4 + 24 + 4 + 8 + 108 + 8) // 4
    want = _expected_mask(opt, [p.ndim >= 2 for p in ps])
    assert torch.equal(opt.decay_mask, want)
    assert int(want.sum()) == 6 + 27                         # the 21 elements of the 7x3 take 6 groups: its padding group follows it
    assert tuple(opt.last_grad_norm.shape) == (1,) and opt.last_clip_coef.data_ptr() == opt.last_grad_norm.data_ptr() + 4
    assert float(opt.last_clip_coef) == 1.0 and opt.current_grad_norm() is None
    assert set(opt.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "lr"}
    # an explicit no_decay list is honoured, ndim or not
    ps = _cpu_params()
    opt = O.AdamW(ps, lr=1e-3, no_decay=[ps[1], ps[5]])
    assert torch.equal(opt.decay_mask, _expected_mask(opt, [True, False, True, True, True, False]))
    opt = O.AdamW(_cpu_params(), lr=1e-3, no_decay=[])
    assert bool(opt.decay_mask.all())
    with pytest.raises(ValueError, match="no_decay"):
        O.AdamW(_cpu_params(), lr=1e-3, no_decay=[torch.nn.Parameter(torch.zeros(3))])


def test_optimiser_refusals():
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            O.AdamW(_cpu_params(), weight_decay=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            O.AdamW(_cpu_params(), max_grad_norm=bad)
    assert O.AdamW(_cpu_params(), max_grad_norm=float("inf")).max_grad_norm == float("inf")
    with pytest.raises(ValueError, match="GPU"):                    # the kernels have no CPU fallback
        O.AdamW(_cpu_params()).step()


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached before the arguments were validated")


def test_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    assert C.OPTIMS == ("adam", "sgd", "adamw")
    for optim in ("adam", "sgd"):
        with pytest.raises(ValueError, match="adamw"):
            C.JointContrastiveTrainer(None, None, optim=optim, weight_decay=0.01)
        with pytest.raises(ValueError, match="adamw"):
            C.JointContrastiveTrainer(None, None, optim=optim, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="optim must be"):
        C.JointContrastiveTrainer(None, None, optim="lamb")
    with pytest.raises(ValueError, match="total_steps"):
        C.JointContrastiveTrainer(None, None, lr_decay="cosine")
    with pytest.raises(ValueError, match="warmup_steps"):
        C.JointContrastiveTrainer(None, None, optim="sgd", warmup_steps=9, total_steps=3)


def test_drivers_arguments():
    ap = drivers.make_parser()
    a = ap.parse_args(["zero-joint", "--joint"])
    assert drivers.optimiser_from_args(a) == {}
    a = ap.parse_args(["zero-joint", "--joint", "--optim", "adamw", "--weight-decay", "0.05", "--clip-grad-norm", "inf", "--warmup-steps", "10",
                       "--lr-decay", "cosine", "--min-lr-ratio", "0.1", "--epochs", "3"])
    assert a.clip_grad_norm == float("inf")
    je = drivers.optimiser_from_args(a, "joint", range(7))                  # one loader of 7 steps per epoch
    assert je == {"optim": "adamw", "weight_decay": 0.05, "max_grad_norm": float("inf"), "warmup_steps": 10, "lr_decay": "cosine",
                  "min_lr_ratio": 0.1, "total_steps": 21}
    assert drivers.run_steps(a, "class", [[None] * 4, [None] * 5]) == 3 * 9    # the schedule spans every task of the run
    with pytest.raises(SystemExit):
        ap.parse_args(["zero-joint", "--joint", "--optim", "lamb"])
    for flags in (["--optim", "adamw"], ["--warmup-steps", "5"], ["--lr-decay", "linear"]):
        with pytest.raises(SystemExit, match="--joint"):
            drivers.main(["class-inc"] + flags)
    for flags in (["--weight-decay", "0.1"], ["--clip-grad-norm", "1.0"], ["--optim", "adam", "--clip-grad-norm", "1.0"]):
        with pytest.raises(SystemExit, match="--optim adamw"):
            drivers.main(["class-inc", "--joint"] + flags)
