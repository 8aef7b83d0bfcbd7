"""A-GEM's two kernels on the GPU (include/cxrk.h "agem_dots" / "agem_project"): the partial sums against float64
within the bounds of grad_sqnorm's summation tree (absolute for the signed dot, relative for the squared norm; tests/agem_ref.py),
the memory contract (exact-size poisoned partials, guards, read-only inputs, a short workspace refused with nothing written), the
projection taken and not taken, where a non-finite value goes, and bad arguments.  The kernels hold no GEMM: nothing here depends
on the contraction precision."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import agem_ref as A  # noqa: E402
import memguard as MG  # noqa: E402
from test_adamw_gpu import NORM_SIZES  # noqa: E402

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
NOISE = 0.1


def rnd(n, seed=0, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * scale


def bits(t):
    return t.detach().reshape(-1).view(torch.int32).cpu()


def within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (float64, on the host); the worst ratio is printed before it is asserted"""
    got, ref, bound = got.detach().double().cpu(), ref.double().cpu(), bound.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |err| / bound {worst:.3f} (largest |err| {float(err.max()):.3e})")
    assert bool((err <= bound).all()), f"{what}: worst |err| / bound {worst:.3f}"


def inputs(n, sign):
    """gref and g = sign * 0.5 * gref + noise on the host: a dot of about sign * |gref|^2 / 2, far from zero"""
    r = rnd(n, seed=2)
    return sign * 0.5 * r + NOISE * rnd(n, seed=1), r


def guarded(t, name):
    return MG.Guarded((t.numel(),), device=DEV, name=name).load(t)


def run(g, r, stats):
    """both launches on device copies -> (g', partials, stats, the guarded pair)"""
    gd, rd = guarded(g, "g"), guarded(r, "gref")
    part = K.agem_dots(gd.t, rd.t).clone()
    K.agem_project(gd.t, rd.t, part, stats)
    torch.cuda.synchronize()
    gd.check()
    rd.check()
    assert torch.equal(rd.bits().cpu(), bits(r)), "gref was modified"
    return gd.t, part, stats.cpu().double(), (gd, rd)


# ------------------------------------------------------------------------------------------------ agem_dots
@pytest.mark.parametrize("n", NORM_SIZES)
def test_dots_against_float64_and_memory_contract(n):
    """Both partial vectors against float64 over the kernel's own partition: the dot's share of each block within
    gamma_depth * (the block's sum of |g * gref|), absolute; gref . gref's within gamma_depth, relative.  Three poisons of an
    exact-size workspace: the same bits; guards intact; g and gref unmodified; a short workspace is refused with nothing written."""
    g, r = inputs(n, -1.0)
    nparts = K.agem_dots_nparts(n)
    assert nparts == K.grad_sqnorm_nparts(n) == min(1024, max(1, -(-(n // 4) // 1024)))
    dref, rref, aref = A.dots_partials(g, r, nparts)
    gd, rd = guarded(g, "g"), guarded(r, "gref")
    keep = (gd.bits(), rd.bits())

    def call(o):
        o["partials"].copy_(K.agem_dots(gd.t, rd.t))

    outs = {"partials": Out((2 * nparts,))}
    o = MG.run_contract(call, outs, module=K, device=DEV)
    got = o["partials"].t.double().cpu()
    within(got[:nparts], torch.from_numpy(dref), torch.from_numpy(A.dot_partial_bound(aref, n, nparts)), f"agem_dots g.gref n={n}")
    within(got[nparts:], torch.from_numpy(rref), A.rr_partial_rtol(n, nparts) * torch.from_numpy(rref), f"agem_dots gref.gref n={n}")
    own = torch.full((2 * nparts + 3,), 7.0, device=DEV)               # a caller-owned buffer: only the first 2 * nparts are written
    ret = K.agem_dots(gd.t, rd.t, out=own)
    assert ret.data_ptr() == own.data_ptr() and ret.numel() == 2 * nparts
    assert torch.equal(bits(own[:2 * nparts]), bits(o["partials"].t)) and bool((own[2 * nparts:] == 7.0).all())
    for d, was in zip((gd, rd), keep):
        d.check()
        assert torch.equal(d.bits(), was), f"{d.name} was modified"
    MG.refuses_short_workspace(call, outs, module=K, device=DEV)
    short = torch.full((2 * nparts - 1,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="cxrk code -2"):
        K.agem_dots(gd.t, rd.t, out=short)
    torch.cuda.synchronize()
    assert bool((short == 7.0).all())


# ------------------------------------------------------------------------------------------------ agem_project
@pytest.mark.parametrize("n", NORM_SIZES)
def test_projection_taken(n):
    """g = -0.5 gref + noise: the dot is negative by at least 10^3 of its bounds (asserted: no sign decided by rounding).  coef
    against float64; g' elementwise against the float64 axpy with the kernel's own fp32 coef within gamma_1 (|g| + |coef gref|); the
    invariant g' . gref = 0 within the dot's bound; gref unchanged; the count incremented on the device."""
    g, r = inputs(n, -1.0)
    nparts = K.agem_dots_nparts(n)
    D, RR, _ = A.dots(g, r)
    dbound = A.dot_bound(g, r, nparts)
    print(f"n={n}: dot {D:.6e}, bound {dbound:.3e}, |dot| / bound {abs(D) / dbound:.3e}")
    assert D < 0 and abs(D) >= 1e3 * dbound
    gnew, _, st, _ = run(g, r, torch.tensor([9.0, 9.0, 9.0, 5.0], device=DEV))
    dot, rr, coef, count = (float(v) for v in st)
    print(f"n={n}: dot err / bound {abs(dot - D) / dbound:.3f}, rr rel err {abs(rr - RR) / RR:.3e} (bound {A.rr_rtol(n, nparts):.3e}), "
          f"coef err / bound {abs(coef - D / RR) / A.coef_bound(g, r, nparts):.3f}")
    assert abs(dot - D) <= dbound and abs(rr - RR) <= A.rr_rtol(n, nparts) * RR
    assert abs(coef - D / RR) <= A.coef_bound(g, r, nparts)
    assert count == 6.0
    within(gnew, A.project(g, r, coef), A.axpy_bound(g, r, coef), f"agem_project g' n={n}")
    left = abs(A.dots(gnew.cpu(), r)[0])
    print(f"n={n}: |g' . gref| {left:.3e} (the dot's bound {dbound:.3e})")
    assert left <= dbound


@pytest.mark.parametrize("n", NORM_SIZES)
def test_projection_not_taken(n):
    """g = +0.5 gref + noise: g stays bit for bit, stats = (dot, rr, 0, count unchanged)"""
    g, r = inputs(n, 1.0)
    nparts = K.agem_dots_nparts(n)
    D, RR, _ = A.dots(g, r)
    dbound = A.dot_bound(g, r, nparts)
    assert D > 0 and D >= 1e3 * dbound
    gnew, _, st, _ = run(g, r, torch.tensor([9.0, 9.0, 9.0, 5.0], device=DEV))
    assert torch.equal(bits(gnew), bits(g)), "g was touched although the gradients do not conflict"
    assert abs(float(st[0]) - D) <= dbound and abs(float(st[1]) - RR) <= A.rr_rtol(n, nparts) * RR
    assert float(st[2]) == 0.0 and float(st[3]) == 5.0


@pytest.mark.parametrize("n", [5, 4097])
def test_zero_reference_does_not_project(n):
    """dot == 0 exactly with rr == 0: no projection, no 0 / 0"""
    g = rnd(n, seed=1)
    gnew, part, st, _ = run(g, torch.zeros(n), torch.tensor([9.0, 9.0, 9.0, 5.0], device=DEV))
    assert bool((part == 0).all()) and torch.equal(bits(gnew), bits(g))
    assert st.tolist() == [0.0, 0.0, 0.0, 5.0]


def test_stale_partials_are_what_decides():
    """agem_project reads nothing but the partials to decide: partials of a conflicting pair project another g"""
    n = 4097
    g, r = inputs(n, -1.0)
    part = K.agem_dots(g.to(DEV), r.to(DEV)).clone()
    other = rnd(n, seed=7)
    od, stats = other.to(DEV), torch.zeros(4, device=DEV)
    K.agem_project(od, r.to(DEV), part, stats)
    coef = float(stats[2])
    assert coef < 0 and float(stats[3]) == 1.0
    within(od, A.project(other, r, coef), A.axpy_bound(other, r, coef), "projected with given partials")


# ------------------------------------------------------------------------------------------------ non-finite values
N_NF = 4 * 1024 * 3 + 2            # three blocks and a tail
SPOTS = [0, 4 * 600 + 1, N_NF - 1]       # the first element, the middle of a block, the tail


@pytest.mark.parametrize("where", ["g", "gref"])
@pytest.mark.parametrize("i", SPOTS)
@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["conflicting", "agreeing"])
def test_a_nan_reaches_every_element(where, i, sign):
    """one NaN in g or in gref makes its block's partial NaN, the dot NaN, the projection taken with a NaN coefficient,
    and every element of g NaN -- whichever way the finite part of the dot points"""
    g, r = inputs(N_NF, sign)
    (g if where == "g" else r)[i] = float("nan")
    nparts = K.agem_dots_nparts(N_NF)
    assert nparts == 3
    gd, rd, stats = g.to(DEV), r.to(DEV), torch.zeros(4, device=DEV)
    part = K.agem_dots(gd, rd).clone()
    K.agem_project(gd, rd, part, stats)
    pbad = torch.isnan(part.cpu())
    b = A.block_of(i, N_NF, nparts)
    want = torch.zeros(2 * nparts, dtype=torch.bool)
    want[b] = True
    want[nparts + b] = where == "gref"
    assert torch.equal(pbad, want), "the NaN left its block's partial sums or never reached them"
    assert bool(torch.isnan(gd).all()), "a NaN gradient must show in the step"
    st = stats.cpu()
    assert bool(torch.isnan(st[0])) and bool(torch.isnan(st[2])) and float(st[3]) == 1.0
    assert torch.equal(bits(rd), bits(r))


# ------------------------------------------------------------------------------------------------ bad arguments
def test_refuses_bad_arguments_and_touches_nothing():
    n = 1027
    flat = {k: torch.full((n + 5,), 3.0, device=DEV) for k in ("g", "r")}
    t = {k: f[:n] for k, f in flat.items()}
    part = torch.full((2,), -7.0, device=DEV)
    stats = torch.full((4,), -7.0, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        assert all(bool((f == 3.0).all()) for f in flat.values()) and bool((part == -7.0).all()) and bool((stats == -7.0).all())

    off = {k: f[1:n + 1] for k, f in flat.items()}                    # 4 bytes off 16-byte alignment
    for k in ("g", "r"):
        args = dict(t, **{k: off[k]})
        with pytest.raises(ValueError, match="cxrk code -1"):
            K.agem_dots(args["g"], args["r"], out=part)
        untouched()
        with pytest.raises(ValueError, match="cxrk code -1"):
            K.agem_project(args["g"], args["r"], part, stats)
        untouched()
    empty, two_d = t["g"][:0], torch.zeros(2, 4, device=DEV)
    for bad in (empty, two_d, t["g"][:8]):                            # empty, 2-D, another length
        for a, b in ((bad, t["r"]), (t["g"], bad)):
            with pytest.raises(ValueError):
                K.agem_dots(a, b, out=part)
            with pytest.raises(ValueError):
                K.agem_project(a, b, part, stats)
        untouched()
    with pytest.raises(ValueError):                                   # partials of another n
        K.agem_project(t["g"], t["r"], torch.zeros(4, device=DEV), stats)
    with pytest.raises(ValueError):
        K.agem_project(t["g"], t["r"], part, torch.zeros(2, device=DEV))
    untouched()
    with pytest.raises(RuntimeError, match="cxrk code -2"):           # partials shorter than 2 * nparts(n)
        K.agem_dots(torch.zeros(8192, device=DEV), torch.zeros(8192, device=DEV), out=torch.zeros(3, device=DEV))
    untouched()
