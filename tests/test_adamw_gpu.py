"""Gradient clipping and decoupled weight decay on the GPU (include/cxrk.h "grad_sqnorm" / "adamw_clipped"): the norm
kernel against float64 within the bound of its own summation tree, its memory contract; the step kernel against torch's CPU
`AdamW` behind `clip_grad_norm_` at the existing Adam test's 1e-6, its bit-identities (no clipping == no partials; no decay, no
clipping == `adam_fused`), memory contract, bad arguments and non-finite gradients; `optim.AdamW` end to end.  The kernels hold no
GEMM: nothing here depends on the contraction precision."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import memguard as MG  # noqa: E402
import optim_ref as R  # noqa: E402

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import optim as O  # noqa: E402

DEV = "cuda"
Out = MG.Out
TOL = 1e-6                       # tests/test_kernels_gpu.py::test_adam_sgd_weight_reset's bound, same measure
N_ADAM = 65920 + 3               # ... and its size
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.1
SWEEP = 1024 * 256 * 4 * 4       # elements one pass of the full grid covers: 1024 blocks x 256 threads x 4 groups x 4 elements
NORM_SIZES = [1, 3, 4, 5, 1023, 4097, N_ADAM, 4 * (1 << 20) + 3, 2 * SWEEP + 4 * 37 + 3]


def close(a, b, what="", tol=TOL):
    """max |a - b| / max |b| < tol (tests/test_kernels_gpu.py's measure), printed before it is asserted"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    print(f"{what}: rel-to-max err {err:.3e} (tol {tol})")
    assert torch.isfinite(a).all(), what
    assert err < tol, f"{what}: rel-to-max err {err:.3e} (tol {tol})"


def rnd(n, seed=0, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * scale


def bits(t):
    return t.detach().reshape(-1).view(torch.int32).cpu()


def partials_ref(g: torch.Tensor, nparts: int) -> np.ndarray:
    """float64 partial sums of g^2 over the kernel's partition (`optim_ref.by_block`)"""
    return R.by_block(g.double().numpy() ** 2, nparts)


# ------------------------------------------------------------------------------------------------ the norm kernel
@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_sqnorm_against_float64_and_memory_contract(n):
    """Every partial sum and their total against float64.  Bound, derived in tests/optim_ref.py (`sqnorm_depth`): a term passes through
    k = 4 * ceil(groups per thread / 4) + n % 4 + 2 + 6 + 4 fp32 additions, and a sum of non-negative terms through k additions is
    within k u / (1 - k u), u = 2^-24, of the exact one.  Two calls, an exact-size workspace poisoned with NaN and with +-1e30: the same
    bits; guards intact; g unmodified; a short workspace is refused with nothing written."""
    g = rnd(n, seed=1)
    nparts = K.grad_sqnorm_nparts(n)
    assert nparts == min(1024, max(1, -(-(n // 4) // 1024)))
    ref = partials_ref(g, nparts)
    tol = R.sqnorm_rtol(n, nparts)
    gd = MG.Guarded((n,), device=DEV, name="g").load(g)
    before = gd.bits()

    def call(o):
        o["partials"].copy_(K.grad_sqnorm(gd.t))

    outs = {"partials": Out((nparts,))}
    o = MG.run_contract(call, outs, {"partials": torch.from_numpy(ref)}, tol, module=K, device=DEV)
    got = o["partials"].t.double().cpu().numpy()
    err_total = abs(got.sum() - ref.sum()) / ref.sum()
    print(f"n={n}: nparts {nparts}, depth {R.sqnorm_depth(n, nparts)}, total rel err {err_total:.3e} (bound {tol:.3e})")
    assert err_total <= tol
    again = K.grad_sqnorm(gd.t).clone()
    own = torch.full((nparts + 3,), 7.0, device=DEV)                 # a caller-owned buffer: only the first nparts are written
    K.grad_sqnorm(gd.t, out=own)
    assert torch.equal(bits(again), bits(o["partials"].t)) and torch.equal(bits(own[:nparts]), bits(again))
    assert bool((own[nparts:] == 7.0).all())
    gd.check()
    assert torch.equal(gd.bits(), before), "g was modified"
    MG.refuses_short_workspace(call, outs, module=K, device=DEV)
    if nparts > 1:
        short = torch.full((nparts - 1,), 7.0, device=DEV)
        with pytest.raises(RuntimeError, match="cxrk code -2"):
            K.grad_sqnorm(gd.t, out=short)
        assert bool((short == 7.0).all())


def test_grad_sqnorm_refuses_bad_arguments():
    flat = torch.zeros(12, device=DEV)
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.grad_sqnorm(flat[1:9])                                     # 4 bytes off 16-byte alignment
    with pytest.raises(ValueError):
        K.grad_sqnorm(flat[:0])
    with pytest.raises(ValueError):
        K.grad_sqnorm(torch.zeros(2, 4, device=DEV))


# ------------------------------------------------------------------------------------------------ the step kernel
def segment_mask(n):
    """decay bytes of a flat buffer of "tensors" of 1024, 4, 20000, 8, ... elements (every one a multiple of four, the last one ragged),
    alternating decay / no decay -> (uint8 [ceil(n / 4)], bool [n])"""
    sizes, left = [], n
    for s in (1024, 4, 20000, 8, 40000, 12):
        if left <= s:
            break
        sizes.append(s)
        left -= s
    sizes.append(left)
    mb = torch.cat([torch.full(((s + 3) // 4,), (k + 1) % 2, dtype=torch.uint8) for k, s in enumerate(sizes)])
    assert mb.numel() == (n + 3) // 4
    return mb, R.expand_mask(mb, n)


class TorchRef:
    """torch's CPU AdamW (fp32, two param groups: decay / none) behind clip_grad_norm_ over a flat buffer with a per-element mask"""

    def __init__(self, p0, decay, wd=WD, lr=LR):
        self.decay = decay
        self.a = torch.nn.Parameter(p0[decay].clone())
        self.b = torch.nn.Parameter(p0[~decay].clone())
        self.opt = torch.optim.AdamW([{"params": [self.a], "weight_decay": wd}, {"params": [self.b], "weight_decay": 0.0}],
                                     lr=lr, betas=(B1, B2), eps=EPS)

    def step(self, g, max_norm=None):
        self.a.grad, self.b.grad = g[self.decay].clone(), g[~self.decay].clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([self.a, self.b], max_norm, error_if_nonfinite=False)
        self.opt.step()
        p = torch.empty(self.decay.numel())
        p[self.decay], p[~self.decay] = self.a.detach(), self.b.detach()
        return p


class Dev:
    """p, m, v, mask, stats of one flat buffer on the device"""

    def __init__(self, p0, mask_bytes):
        n = p0.numel()
        self.p, self.m, self.v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.mask = None if mask_bytes is None else mask_bytes.to(DEV)
        self.stats = torch.full((2,), -7.0, device=DEV)

    def step(self, g, step, max_norm=0.0, wd=WD, grad_scale=1.0, partials=True):
        gd = g.to(DEV)
        part = K.grad_sqnorm(gd) if partials else None
        K.adamw_clipped(self.p, gd, self.m, self.v, LR, B1, B2, EPS, wd, step, grad_scale, max_norm, decay_mask=self.mask,
                        partials=part, stats=self.stats)
        return self.stats.cpu()


def check_stats(stats, g, n, max_norm, grad_scale=1.0):
    norm = R.grad_norm(g, grad_scale)
    coef = R.clip_coef(norm, max_norm)
    tol = R.norm_rtol(n, K.grad_sqnorm_nparts(n))
    e_n, e_c = abs(float(stats[0]) - norm) / norm, abs(float(stats[1]) - coef) / coef
    print(f"stats: norm {float(stats[0]):.9e} ref {norm:.9e} err {e_n:.2e}; coef {float(stats[1]):.9e} ref {coef:.9e} err {e_c:.2e} (bound {tol:.2e})")
    assert e_n <= tol and e_c <= tol + 3 * R.U          # coef: one addition, one division and the norm's own error


def test_clipped_step_against_torch():
    """case 1: clipping active, max_norm = half of each step's norm; three steps; stats against float64"""
    n = N_ADAM
    mb, decay = segment_mask(n)
    p0, gs = rnd(n), [rnd(n, seed=s) for s in (1, 2, 3)]
    ref, dev = TorchRef(p0, decay), Dev(p0, mb)
    for step, g in enumerate(gs, 1):
        max_norm = 0.5 * R.grad_norm(g)
        want = ref.step(g, max_norm)
        stats = dev.step(g, step, max_norm)
        check_stats(stats, g, n, max_norm)
        assert abs(float(stats[1]) - 0.5) < 1e-6
        close(dev.p, want, f"clipped AdamW step {step}")
    nodecay = TorchRef(p0, torch.zeros(n, dtype=torch.bool))         # the decay is far above the bound: lr * wd = 1e-4 of a parameter
    for g in gs:
        other = nodecay.step(g, 0.5 * R.grad_norm(g))
    assert float((want - other).abs().max() / want.abs().max()) > 50 * TOL


def test_inactive_clipping_is_bit_identical_to_no_partials():
    """case 2: max_norm = 1e30 and inf give coef == 1.0 exactly and the bits of max_norm = 0 with partials = NULL; against torch too"""
    n = N_ADAM
    mb, decay = segment_mask(n)
    p0, gs = rnd(n), [rnd(n, seed=s) for s in (1, 2, 3)]
    ref = TorchRef(p0, decay)
    runs = {"1e30": Dev(p0, mb), "inf": Dev(p0, mb), "monitor": Dev(p0, mb), "none": Dev(p0, mb)}
    for step, g in enumerate(gs, 1):
        want = ref.step(g, 1e30)
        for tag, mx in (("1e30", 1e30), ("inf", float("inf"))):
            stats = runs[tag].step(g, step, mx)
            assert float(stats[1]) == 1.0, (tag, float(stats[1]))
            check_stats(stats, g, n, mx)
        stats = runs["monitor"].step(g, step, 0.0)                   # partials given, max_norm <= 0: the norm is reported, nothing clipped
        assert float(stats[1]) == 1.0 and float(stats[0]) > 0
        stats = runs["none"].step(g, step, 0.0, partials=False)
        assert stats.tolist() == [0.0, 1.0]
        for tag in ("1e30", "inf", "monitor"):
            for name in ("p", "m", "v"):
                assert torch.equal(bits(getattr(runs[tag], name)), bits(getattr(runs["none"], name))), (tag, name, step)
        close(runs["none"].p, want, f"unclipped AdamW step {step}")


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
@pytest.mark.parametrize("n", [N_ADAM, N_ADAM - 1, N_ADAM - 2, N_ADAM - 3, 7, 5, 2, 1])
def test_no_decay_no_clipping_is_adam_fused_bit_for_bit(n, masked):
    """case 3: weight_decay = 0 without clipping (and with max_norm = inf) against K.adam_fused(weight_decay = 0), three steps, with a
    gradient scale away from 1; every length of the scalar tail (n % 4 = 3, 2, 1, 0)"""
    mb, _ = segment_mask(n)
    p0, gs = rnd(n), [rnd(n, seed=s) for s in (1, 2, 3)]
    a, b = Dev(p0, mb if masked else None), Dev(p0, mb if masked else None)
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step, g in enumerate(gs, 1):
        K.adam_fused(pd, g.to(DEV), m, v, LR, B1, B2, EPS, 0.0, step, 0.75)
        a.step(g, step, 0.0, wd=0.0, grad_scale=0.75, partials=False)
        b.step(g, step, float("inf"), wd=0.0, grad_scale=0.75)
        for d in (a, b):
            assert torch.equal(bits(d.p), bits(pd)) and torch.equal(bits(d.m), bits(m)) and torch.equal(bits(d.v), bits(v)), step


def test_grad_scale_scales_the_norm_exactly_and_the_update():
    """case 4: grad_scale = 0.5 halves the reported norm exactly (a power of two) and the step is torch's on the halved gradient"""
    n = N_ADAM
    mb, decay = segment_mask(n)
    p0, g = rnd(n), rnd(n, seed=1)
    max_norm = 0.3 * R.grad_norm(g)
    one, half = Dev(p0, mb), Dev(p0, mb)
    s1 = one.step(g, 1, max_norm)
    s2 = half.step(g, 1, max_norm, grad_scale=0.5)
    assert float(s2[0]) == 0.5 * float(s1[0])
    check_stats(s2, g, n, max_norm, grad_scale=0.5)
    close(half.p, TorchRef(p0, decay).step(0.5 * g, max_norm), "grad_scale 0.5")
    neg = Dev(p0, mb)
    s3 = neg.step(g, 1, max_norm, grad_scale=-0.5)                   # the norm takes |grad_scale|
    assert float(s3[0]) == float(s2[0]) and float(s3[1]) == float(s2[1])


@pytest.mark.parametrize("n", [1, 5, 7])
def test_scalar_tail_and_short_masks(n):
    """the n % 4 tail of both kernels, a mask of ceil(n / 4) bytes (decay in the first group only), three clipped steps against float64"""
    mb = torch.tensor([1, 0][:(n + 3) // 4], dtype=torch.uint8)
    decay = R.expand_mask(mb, n)
    p0, gs = rnd(n, seed=5), [rnd(n, seed=s) for s in (6, 7, 8)]
    lr, b1, b2, eps, wd = (float(np.float32(t)) for t in (LR, B1, B2, EPS, WD))     # the hyper-parameters as the kernel sees them
    dev = Dev(p0, mb)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(gs, 1):
        max_norm = 0.5 * R.grad_norm(g)
        p, m, v, norm, coef = R.adamw_step(p, g, m, v, decay, lr, b1, b2, eps, wd, step, max_norm=max_norm)
        stats = dev.step(g, step, max_norm)
        check_stats(stats, g, n, max_norm)
        close(dev.p, p, f"n={n} step {step} p")
        close(dev.m, m, f"n={n} step {step} m")
        close(dev.v, v, f"n={n} step {step} v")


# ------------------------------------------------------------------------------------------------ memory contract
@pytest.mark.parametrize("n", [3, 1027])
def test_step_memory_contract(n):
    """guards around p, g, m, v, the mask, the partials and the stats; g, mask and partials unmodified; p, m, v, stats against float64"""
    mb = torch.tensor([1, 0, 0, 1] * ((n + 15) // 16), dtype=torch.uint8)[:(n + 3) // 4]
    decay = R.expand_mask(mb, n)
    p0, g, m0, v0 = rnd(n), rnd(n, seed=1), 0.1 * rnd(n, seed=2), 0.01 * rnd(n, seed=3).abs()
    lr, b1, b2, eps, wd, gs = (float(np.float32(t)) for t in (1e-2, 0.9, 0.999, 1e-8, 0.05, 0.5))
    step, max_norm = 3, 0.25 * R.grad_norm(g, 0.5)
    pref, mref, vref, norm, coef = R.adamw_step(p0, g, m0, v0, decay, lr, b1, b2, eps, wd, step, grad_scale=gs, max_norm=max_norm)
    nparts = K.grad_sqnorm_nparts(n)
    gd = MG.Guarded((n,), device=DEV, name="g").load(g)
    md = MG.Guarded(((n + 3) // 4,), torch.uint8, device=DEV, name="mask").load(mb)
    pd = MG.Guarded((nparts,), device=DEV, name="partials")
    K.grad_sqnorm(gd.t, out=pd.t)
    pd.must_write = False
    keep = (gd.bits(), md.bits(), pd.bits())

    def call(o):
        K.adamw_clipped(o["p"], gd.t, o["m"], o["v"], lr, b1, b2, eps, wd, step, gs, max_norm, decay_mask=md.t, partials=pd.t, stats=o["stats"])

    outs = {"p": Out((n,), init=p0), "m": Out((n,), init=m0), "v": Out((n,), init=v0), "stats": Out((2,))}
    MG.run_contract(call, outs, {"p": pref, "m": mref, "v": vref, "stats": torch.tensor([norm, coef], dtype=torch.float64)}, TOL,
                    module=K, device=DEV, runs=("session", "nan"))
    for gdd, was in zip((gd, md, pd), keep):
        gdd.check()
        assert torch.equal(gdd.bits(), was), f"{gdd.name} was modified"


def test_step_refuses_bad_arguments_and_touches_nothing():
    n = 1027
    flat = {k: torch.full((n + 5,), 3.0, device=DEV) for k in "pgmv"}
    t = {k: f[:n] for k, f in flat.items()}
    stats = torch.full((2,), -7.0, device=DEV)
    part = K.grad_sqnorm(t["g"]).clone()
    args = (LR, B1, B2, EPS, WD)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((f == 3.0).all()) for k, f in flat.items()) and stats.tolist() == [-7.0, -7.0]

    with pytest.raises(ValueError, match="cxrk code -1"):            # p 4 bytes off 16-byte alignment
        K.adamw_clipped(flat["p"][1:n + 1], t["g"], t["m"], t["v"], *args, 1, 1.0, 1.0, partials=part, stats=stats)
    untouched()
    with pytest.raises(ValueError, match="cxrk code -1"):            # n = 0
        K.adamw_clipped(t["p"][:0], t["g"][:0], t["m"][:0], t["v"][:0], *args, 1, stats=stats)
    untouched()
    with pytest.raises(ValueError, match="cxrk code -1"):            # step = 0
        K.adamw_clipped(t["p"], t["g"], t["m"], t["v"], *args, 0, 1.0, 1.0, partials=part, stats=stats)
    untouched()
    for mx in (1.0, float("inf")):                                   # clipping or monitoring without the partial sums
        with pytest.raises(ValueError, match="cxrk code -1"):
            K.adamw_clipped(t["p"], t["g"], t["m"], t["v"], *args, 1, 1.0, mx, stats=stats)
        untouched()
    with pytest.raises(RuntimeError, match="cxrk code -2"):          # partials shorter than nparts(n)
        K.adamw_clipped(torch.zeros(8192, device=DEV), torch.zeros(8192, device=DEV), torch.zeros(8192, device=DEV),
                        torch.zeros(8192, device=DEV), *args, 1, 1.0, 1.0, partials=torch.zeros(1, device=DEV), stats=stats)
    untouched()
    with pytest.raises(ValueError, match="decay_mask"):
        K.adamw_clipped(t["p"], t["g"], t["m"], t["v"], *args, 1, decay_mask=torch.zeros(n // 4, dtype=torch.uint8, device=DEV))
    untouched()


# ------------------------------------------------------------------------------------------------ non-finite gradients
def test_nan_gradient_reaches_norm_coefficient_and_every_parameter():
    n = 1027
    mb, decay = segment_mask(n)
    p0, g0, g = rnd(n), rnd(n, seed=1), rnd(n, seed=2)
    g[700] = float("nan")
    ref, dev = TorchRef(p0, decay), Dev(p0, mb)
    ref.step(g0, 1.0)
    dev.step(g0, 1, 1.0)
    want = ref.step(g, 1.0)
    stats = dev.step(g, 2, 1.0)
    assert math.isnan(float(stats[0])) and math.isnan(float(stats[1]))
    assert bool(torch.isnan(want).all()) and bool(torch.isnan(dev.p).all())          # torch with error_if_nonfinite=False does the same


def test_inf_gradient_zeroes_the_coefficient():
    """norm inf, coef 0: the element with the inf takes inf * 0 = NaN, every other element a zero-gradient step (moments decay, the
    parameter follows the first moment, weight decay applies), as torch"""
    n = 1027
    mb, decay = segment_mask(n)
    p0, g0, g = rnd(n), rnd(n, seed=1), rnd(n, seed=2)
    g[700] = float("inf")
    ref, dev = TorchRef(p0, decay), Dev(p0, mb)
    ref.step(g0, 1.0)
    dev.step(g0, 1, 1.0)
    want = ref.step(g, 1.0)
    stats = dev.step(g, 2, 1.0)
    assert float(stats[0]) == float("inf") and float(stats[1]) == 0.0
    got = dev.p.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[700]))
    fin = ~torch.isnan(want)
    close(got[fin], want[fin], "the finite elements after the inf step")
    assert float((got[fin] - p0[fin]).abs().max()) > 1e-5                            # they did move


# ------------------------------------------------------------------------------------------------ optim.AdamW end to end
def test_optimiser_end_to_end_against_torch():
    """parameters of 1, 2, 5, 7x3 elements and a channels_last 4-D filter; three steps against torch with decay / no-decay groups
    (ndim >= 2 decays) and clipping at 1.0 (the gradient norm is about 12), at 1e-6; the reported norm against float64"""
    g = torch.Generator().manual_seed(11)
    shapes = [(1,), (2,), (5,), (7, 3), (4, 3, 3, 3)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    mine = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    mine[4].data = mine[4].data.contiguous(memory_format=torch.channels_last)
    theirs = [torch.nn.Parameter(t.clone()) for t in init]
    opt = O.AdamW(mine, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    assert mine[4].is_contiguous(memory_format=torch.channels_last) and opt.numel == 4 + 4 + 8 + 24 + 108
    assert int(opt.decay_mask.sum()) == 6 + 27 and opt.current_grad_norm() == 0.0
    ref = torch.optim.AdamW([{"params": theirs[3:], "weight_decay": WD}, {"params": theirs[:3], "weight_decay": 0.0}], lr=LR,
                            betas=(B1, B2), eps=EPS)
    for step in range(1, 4):
        grads = [torch.randn(*s, generator=g) for s in shapes]
        opt.zero_grad()
        for p, q, gr in zip(mine, theirs, grads):
            p.grad.copy_(gr)
            q.grad = gr.clone()
        tn = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        ref.step()
        opt.step()
        norm = math.sqrt(sum(float((gr.double() ** 2).sum()) for gr in grads))
        tol = R.norm_rtol(opt.numel, K.grad_sqnorm_nparts(opt.numel))
        got = opt.current_grad_norm()
        print(f"step {step}: norm {got:.9e} float64 {norm:.9e} torch {float(tn):.9e} (bound {tol:.2e}); coef {float(opt.last_clip_coef):.6f}")
        assert abs(got - norm) <= tol * norm and abs(float(opt.last_clip_coef) - 1.0 / (norm + 1e-6)) <= (tol + 3 * R.U) / norm
        assert opt.steps == step
        for k, (p, q) in enumerate(zip(mine, theirs)):
            close(p, q, f"step {step} parameter {k}")
        assert torch.equal(opt.flat_g[:1].cpu(), grads[0]), "the gradient buffer is left unclipped"
    unclipped = O.AdamW([torch.nn.Parameter(torch.ones(5, device=DEV))], lr=LR)
    unclipped.step()
    assert unclipped.current_grad_norm() is None and float(unclipped.last_clip_coef) == 1.0 and unclipped._partials is None
