"""The geometry contract of the three convolution entry points (include/cxrk.h), off ResNet's own grid: pad above and below "same",
R != S, stride 2 with a left-over row or column, stride 2 / pad 0 with a 3-wide filter (the data gradient's tap offset of -1),
images of one pixel with hundreds per tile, channel counts that leave the tap-wise gather -- and what each entry point refuses.

Every geometry of tests/test_conv_geometry_host.py runs forward (shift, residual, ReLU; the decision bits in the planes form), data
gradient (plain; with residual, mask and fused column sums where the library takes them) and weight gradient with the BatchNorm
gradients (fresh and accumulated), through the wrappers of kernels.py, against float64 `F.conv2d` / `conv2d_input` / `conv2d_weight`
on the values the kernel sees (that file checks those references against the definition).  Bounds are those of
tests/test_kernels_gpu.py: 2e-5 / 5e-5 (fp32 forward / gradients), 2e-4 / 3e-4 (planes), dgamma 2e-3 / 2e-2; the reductions here
are shorter than where those bounds were set.

Memory: every INPUT sits in a `memguard.Guarded` allocation, NaN sentinels in front and behind; the two planes of a planes input are
more than one image row (plus a pixel) of sentinels apart, so a read of row -1 of the lo plane does not land in the hi plane's data.
Every output goes through `memguard.run_contract` or a `Guarded` allocation of its own.  A gather that leaves its tensor therefore reads a NaN, which no comparison accepts,
and cannot leave memory the test owns: the guards are 4 MiB or a 256-row tile, whichever is larger."""
import numpy as np
import pytest
import torch

import memguard as MG
import test_conv_geometry_host as G

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
BF, U8 = torch.bfloat16, torch.uint8
ARG, UNSUPPORTED = -1, -4      # CXRK_ERR_ARG, CXRK_ERR_UNSUPPORTED (include/cxrk.h)


def plane_gap(shape) -> int:
    """sentinel elements between the hi and the lo plane of a guarded planes input: at least one row of the tensor's second
    dimension (an image row of [N, H, W, C]) plus one pixel, in multiples of 64 (the lo plane stays 16-byte aligned)"""
    row = 1
    for v in shape[2:]:
        row *= int(v)
    return (max(64, row + int(shape[-1])) + 63) // 64 * 64


def _split() -> bool:
    return _cxr_lib.get_precision() == "split_bf16"


def tl(t: float) -> float:
    """the bound tests/test_kernels_gpu.py's close() applies: `t` of the output scale, at least 3e-4 in split-bf16 mode"""
    return max(t, 3e-4) if _split() else t


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


class Inputs:
    """the guarded inputs of one test; `check()` once the kernels have run"""

    def __init__(self):
        self.guards = []

    def f32(self, t, name):
        """fp32 CPU tensor -> (guarded device copy, float64 values)"""
        g = MG.Guarded(t.shape, torch.float32, device=DEV, name=name).load(t.float())
        self.guards.append(g)
        return g.t, t.double()

    def planes(self, t, name):
        """fp32 CPU tensor -> (guarded Planes, the float64 values the kernels see)"""
        p = K.split_planes(t.float().contiguous().to(DEV))
        g = MG.Guarded((2,) + tuple(t.shape), BF, gap=plane_gap(t.shape), device=DEV, name=name).load(p.t)
        self.guards.append(g)
        gp = K.Planes(g.t)
        return gp, gp.float().cpu().double()

    def bits(self, dec, name):
        """bool [rows, C] -> guarded packed ReLU decision bits [rows, C / 8]"""
        b = torch.from_numpy(np.packbits(dec.numpy(), axis=1, bitorder="little"))
        g = MG.Guarded(b.shape, U8, device=DEV, name=name).load(b)
        self.guards.append(g)
        return g.t

    def check(self):
        for g in self.guards:
            g.check()


def _id(cfg):
    return "x".join(str(v) for v in cfg)


def contract(call, outs, ref, tol, report=None):
    return MG.run_contract(call, outs, ref, tol, module=K, device=DEV, report=report)


def refused(call, outputs, code):
    """`call` raises ValueError with exactly the code include/cxrk.h states for it (ARG or UNSUPPORTED) and leaves every byte of its
    outputs and their guards alone"""
    outs = {n: s.make(n, DEV, None, MG.BYTE_SENTINELS[0]) for n, s in outputs.items()}
    before = {n: g.backing.clone() for n, g in outs.items()}
    assert code in (ARG, UNSUPPORTED)
    with pytest.raises(ValueError, match=rf"\(cxrk code {code}\)"):
        call({n: g.t for n, g in outs.items()})
    torch.cuda.synchronize()
    for n, g in outs.items():
        assert torch.equal(g.backing, before[n]), f"{n}: written by a call that was refused"


def _show(tag, report):
    print(f"{tag}: " + ", ".join(f"{n} {err:.2e}/{bound:.0e}" for n, err, bound in report))


def _case(cfg, cpad=None):
    """random operands of one geometry, NHWC / [Ko, R, S, C] on the CPU; with `cpad` the input and the scaled filter carry zero
    channels up to cpad (the stem's layout) while the raw filter and its gradient keep the real count"""
    N, H, W, C, Ko, R, S, stride, pad = cfg
    Cp = cpad or C
    Ho, Wo = G.conv_out(H, W, R, S, stride, pad)
    x = torch.zeros(N, H, W, Cp)
    x[..., :C] = rnd(N, H, W, C)
    w = rnd(Ko, R, S, C, seed=1, scale=1.0 / (C * R * S) ** 0.5)
    wp = torch.zeros(Ko, R, S, Cp)
    wp[..., :C] = w
    return dict(N=N, H=H, W=W, C=C, Cp=Cp, Ko=Ko, R=R, S=S, stride=stride, pad=pad, Ho=Ho, Wo=Wo, x=x, w=w, wp=wp,
                dy=rnd(N, Ho, Wo, Ko, seed=2), res=rnd(N, Ho, Wo, Ko, seed=3), add=rnd(N, H, W, Cp, seed=4), src=rnd(N, H, W, Cp, seed=5),
                shift=0.1 * rnd(Ko, seed=6), scale=1 + 0.1 * rnd(Ko, seed=7), rstd=0.5 + rnd(Ko, seed=8).abs(), rmean=0.1 * rnd(Ko, seed=9),
                base_w=rnd(Ko, R, S, C, seed=10), base_g=rnd(Ko, seed=11), base_b=rnd(Ko, seed=12))


def _wgrad_refs(c, x64, dy64):
    raw = G.wgrad_ref(x64, dy64, c["R"], c["S"], c["stride"], c["pad"])[..., :c["C"]]
    sumdy = dy64.reshape(-1, c["Ko"]).sum(0)
    dgam = c["rstd"].double() * ((c["w"].double() * raw).sum((1, 2, 3)) - c["rmean"].double() * sumdy)
    return c["scale"].double()[:, None, None, None] * raw, dgam, sumdy


def _run_wgrad(c, fn, x64, dy64, tw, tg, tag):
    """weight gradient + BatchNorm gradients, fresh and accumulated; `fn(sumdy, dw, dg, db, accumulate)`"""
    Ko, R, S, C = c["Ko"], c["R"], c["S"], c["C"]
    dw64, dg64, sumdy64 = _wgrad_refs(c, x64, dy64)
    sumdy = sumdy64.float().to(DEV)
    sd64 = sumdy.cpu().double()
    rep = []
    contract(lambda o: fn(sumdy, o["dw"], o["dg"], o["db"], False), {"dw": Out((Ko, R, S, C)), "dg": Out((Ko,)), "db": Out((Ko,))},
             {"dw": dw64, "dg": dg64, "db": sd64}, {"dw": tw, "dg": tg, "db": tw}, rep)
    bw, bg, bb = c["base_w"], c["base_g"], c["base_b"]
    contract(lambda o: fn(sumdy, o["dw"], o["dg"], o["db"], True),
             {"dw": Out((Ko, R, S, C), init=bw), "dg": Out((Ko,), init=bg), "db": Out((Ko,), init=bb)},
             {"dw": bw.double() + dw64, "dg": bg.double() + dg64, "db": bb.double() + sd64}, {"dw": tw, "dg": tg, "db": tw}, rep)
    _show(tag + " wgrad", rep)


def _fp32_all(cfg, cpad=None, dgrad=True):
    c = _case(cfg, cpad)
    N, H, W, C, Cp, Ko, R, S, stride, pad, Ho, Wo = (c[k] for k in ("N", "H", "W", "C", "Cp", "Ko", "R", "S", "stride", "pad", "Ho", "Wo"))
    inp = Inputs()
    xd, x64 = inp.f32(c["x"], "x")
    wd, w64 = inp.f32(c["wp"], "w_scaled")
    wraw, _ = inp.f32(c["w"], "w")
    dyd, dy64 = inp.f32(c["dy"], "dy")
    resd, res64 = inp.f32(c["res"], "residual")
    shd, sh64 = inp.f32(c["shift"], "shift")
    geo = (N, H, W, Cp, Ko, R, S, stride, pad)
    tag = f"fp32 {cfg}"
    rep = []
    # forward: shift + residual + ReLU
    yref = torch.relu(G.fwd_ref(x64, w64, stride, pad) + sh64 + res64)
    contract(lambda o: K.conv_fwd(xd, wd, shd, resd, o["y"], *geo, True), {"y": Out((N, Ho, Wo, Ko))}, {"y": yref}, tl(2e-5), rep)
    if dgrad:
        g64 = G.dgrad_ref(dy64, w64, H, W, stride, pad)
        contract(lambda o: K.conv_bwd_data(dyd, wd, None, None, o["dx"], *geo), {"dx": Out((N, H, W, Cp))}, {"dx": g64}, tl(5e-5), rep)
        addd, add64 = inp.f32(c["add"], "dgrad residual")
        srcd, _ = inp.f32(c["src"], "relu source")
        full = (g64 + add64) * (c["src"] > 0)
        if G.dgrad_side_ok(H, W, R, S, stride, pad):
            contract(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *geo), {"dx": Out((N, H, W, Cp))}, {"dx": full}, tl(5e-5), rep)
        else:
            refused(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *geo), {"dx": Out((N, H, W, Cp))}, ARG)
        spec = {"dx": Out((N, H, W, Cp)), "sums": Out((Cp,))}
        if G.dgrad_sums_ok(H, W, R, S, stride, pad):
            contract(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *geo, sums=o["sums"]), spec,
                     {"dx": full, "sums": full.reshape(-1, Cp).sum(0)}, tl(5e-5), rep)
        else:
            refused(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *geo, sums=o["sums"]), spec, ARG)
    _show(tag, rep)
    sd, rd, md = (c[k].to(DEV) for k in ("scale", "rstd", "rmean"))
    _run_wgrad(c, lambda sumdy, dw, dg, db, acc: K.conv_bwd_params(xd, dyd, wraw, sd, rd, md, sumdy, dw, dg, db, acc, N, H, W, C, Cp, Ko, R, S,
                                                                  stride, pad),
               x64, dy64, tl(5e-5), 2e-2 if _split() else 2e-3, tag)
    inp.check()


def _planes_all(cfg):
    c = _case(cfg)
    N, H, W, C, Ko, R, S, stride, pad, Ho, Wo = (c[k] for k in ("N", "H", "W", "C", "Ko", "R", "S", "stride", "pad", "Ho", "Wo"))
    inp = Inputs()
    xp, x64 = inp.planes(c["x"], "x")
    wp, w64 = inp.planes(c["w"].reshape(Ko, -1), "w_scaled")
    w64 = w64.view(Ko, R, S, C)
    wraw, _ = inp.f32(c["w"], "w")
    dyp, dy64 = inp.planes(c["dy"], "dy")
    resp, res64 = inp.planes(c["res"], "residual")
    shd, sh64 = inp.f32(c["shift"], "shift")
    geo = (N, H, W, C, Ko, R, S, stride, pad)
    tag = f"planes {cfg}"
    rep = []
    # forward: shift + residual + ReLU, with the decision bits
    yref = torch.relu(G.fwd_ref(x64, w64, stride, pad) + sh64 + res64)
    fspec = {"y": Out((2, N, Ho, Wo, Ko), BF), "mask": Out((N * Ho * Wo, Ko // 8), U8)}
    if Ko % 64 == 0:
        o = contract(lambda o: K.conv_fwd_pl(xp, wp, shd, resp, K.Planes(o["y"]), o["mask"], *geo, True), fspec, {"y": yref}, tl(2e-4), rep)
        stored = K.Planes(o["y"].t).float().view(-1, Ko)
        assert torch.equal(K.unpack_mask(o["mask"].t.contiguous(), Ko).view(-1, Ko).to(DEV), stored > 0), "decision bits != sign of the stored output"
    else:       # the decision bits are written 64 channels at a time (include/cxrk.h): refused, and the forward runs without them
        refused(lambda o: K.conv_fwd_pl(xp, wp, shd, resp, K.Planes(o["y"]), o["mask"], *geo, True), fspec, ARG)
        contract(lambda o: K.conv_fwd_pl(xp, wp, shd, resp, K.Planes(o["y"]), None, *geo, True), {"y": fspec["y"]}, {"y": yref}, tl(2e-4), rep)
    # data gradient
    g64 = G.dgrad_ref(dy64, w64, H, W, stride, pad)
    contract(lambda o: K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(o["dx"]), *geo), {"dx": Out((2, N, H, W, C), BF)}, {"dx": g64}, tl(3e-4), rep)
    addp, add64 = inp.planes(c["add"], "dgrad residual")
    dec = c["src"].view(-1, C) > 0
    mbits = inp.bits(dec, "mask bits")
    full = (g64 + add64) * dec.view(N, H, W, C)
    if G.dgrad_side_ok(H, W, R, S, stride, pad):
        contract(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *geo), {"dx": Out((2, N, H, W, C), BF)}, {"dx": full},
                 tl(3e-4), rep)
    else:
        refused(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *geo), {"dx": Out((2, N, H, W, C), BF)}, ARG)
    spec = {"dx": Out((2, N, H, W, C), BF), "sums": Out((C,))}
    if G.dgrad_sums_ok(H, W, R, S, stride, pad):
        contract(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *geo, sums=o["sums"]), spec,
                 {"dx": full, "sums": full.reshape(-1, C).sum(0)}, tl(3e-4), rep)
    else:
        refused(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *geo, sums=o["sums"]), spec, ARG)
    _show(tag, rep)
    sd, rd, md = (c[k].to(DEV) for k in ("scale", "rstd", "rmean"))
    _run_wgrad(c, lambda sumdy, dw, dg, db, acc: K.conv_bwd_params_pl(xp, dyp, wraw, sd, rd, md, sumdy, dw, dg, db, acc, *geo),
               x64, dy64, tl(3e-4), 2e-2, tag)
    inp.check()


# ------------------------------------------------------------------------------------------------ geometries that compute
@pytest.mark.parametrize("cfg", G.COMPUTES, ids=_id)
def test_geometry_fp32(cfg):
    _fp32_all(cfg)


@pytest.mark.parametrize("cfg", G.COMPUTES, ids=_id)
def test_geometry_planes(cfg, wide):
    _planes_all(cfg)


@pytest.mark.parametrize("cfg", G.CHANNEL_EDGES, ids=_id)
def test_channel_edges_fp32(cfg):
    """C = 8, 16, 48 and 7x7 at C = 32 leave the tap-wise gather of the forward (a K-tile no longer lies inside one filter tap); C = 5 in
    8 padded channels is the stem's layout: the weight gradient has the real channel count and nothing is written past it (the
    output's guards and its fully-written check see to both).  The data gradient runs where the library computes it."""
    N, H, W, C, Cpad, Ko, R, S, stride, pad = cfg
    _fp32_all((N, H, W, C, Ko, R, S, stride, pad), cpad=Cpad, dgrad=R * S <= 32)


def _s2_pad0_per_image(planes):
    """Stride 2 / 3x3 / pad 0: the tap at offset -1 of an image's first row or column would be the previous image's last one.  With
    image 0 of dy replaced, image 1 of dx must not change by a bit.  dx sits between guards of its own."""
    cfg = G.S2_PAD0[0]
    c = _case(cfg)
    N, H, W, C, Ko, R, S, stride, pad = cfg
    dy2 = c["dy"].clone()
    dy2[0] = 3.0 * rnd(*dy2[0].shape, seed=20) + 1.0
    inp = Inputs()
    outs = []
    for dy in (c["dy"], dy2):
        if planes:
            dyp, _ = inp.planes(dy, "dy")
            wp, _ = inp.planes(c["w"].reshape(Ko, -1), "w_scaled")
            dx = MG.Guarded((2, N, H, W, C), BF, device=DEV, name="dx")
            K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(dx.t), *cfg)
        else:
            dyd, _ = inp.f32(dy, "dy")
            wd, _ = inp.f32(c["w"], "w_scaled")
            dx = MG.Guarded((N, H, W, C), torch.float32, device=DEV, name="dx")
            K.conv_bwd_data(dyd, wd, None, None, dx.t, *cfg)
        dx.check()
        outs.append(dx.bits())
    inp.check()
    a, b = (o[:, 1] if planes else o[1] for o in outs)
    assert torch.equal(a, b), f"image 1 of dx depends on image 0 of dy in {int((a != b).sum())} element(s)"
    a, b = (o[:, 0] if planes else o[0] for o in outs)
    assert not torch.equal(a, b)


def test_s2_pad0_dgrad_is_per_image_fp32():
    _s2_pad0_per_image(False)


def test_s2_pad0_dgrad_is_per_image_planes(wide):
    _s2_pad0_per_image(True)


@pytest.mark.parametrize("N,H,W,C,Ko,R", G.COMPACT_RESIDUAL)
def test_compact_residual_on_a_rectangle(N, H, W, C, Ko, R, wide):
    """The compact stride-2 residual of tests/test_kernels_gpu.py::test_planes_dgrad_compact_stride2_residual with an odd extent in
    either direction: the 1x1 / stride-2 data gradient dense and compact, then the stride-1 data gradient that takes the compact
    form with mask bits and column sums, against float64."""
    He, We, Kd = (H + 1) // 2, (W + 1) // 2, 2 * C
    inp = Inputs()
    gd, gd64 = inp.planes(rnd(N, He, We, Kd, seed=1), "projection dy")
    wd, wd64 = inp.planes(rnd(Kd, C, seed=2, scale=0.05), "projection w")
    dense64 = G.dgrad_ref(gd64, wd64.view(Kd, 1, 1, C), H, W, 2, 0)
    o = contract(lambda o: K.conv_bwd_data_pl(gd, wd, None, None, K.Planes(o["dx"]), N, H, W, C, Kd, 1, 1, 2, 0), {"dx": Out((2, N, H, W, C), BF)},
                 {"dx": dense64}, tl(3e-4))
    dense = K.Planes(o["dx"].t).float()
    # the compact form allocates its own output: the product it is (a dense [N He We, Kd] x [Kd, C] GEMM) also runs into guarded
    # memory, and the wrapper's result must equal that bit for bit
    oc = contract(lambda o: K.linear_bwd_data_pl(gd.view(N * He * We, Kd), wd, out=K.Planes(o["c"])), {"c": Out((2, N * He * We, C), BF)},
                  {"c": dense64[:, ::2, ::2].reshape(-1, C)}, tl(3e-4))
    comp = K.conv1x1_s2_bwd_data_compact_pl(gd, wd, N, H, W, C, Kd)
    assert tuple(comp.shape) == (N, He, We, C) and torch.equal(dense[:, ::2, ::2], comp.float())
    assert torch.equal(comp.t.view(torch.int16).reshape(2, -1), oc["c"].bits().reshape(2, -1))
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert float(dense[:, odd.to(DEV)].abs().max()) == 0.0
    compg, comp64 = inp.planes(comp.float().cpu(), "compact residual")
    dyp, dy64 = inp.planes(rnd(N, H, W, Ko, seed=3), "dy")
    w1, w64 = inp.planes(rnd(Ko, R * R * C, seed=4, scale=0.05), "w_scaled")
    dec = rnd(N * H * W, C, seed=5) > 0
    mbits = inp.bits(dec, "mask bits")
    scat = torch.zeros(N, H, W, C, dtype=torch.float64)
    scat[:, ::2, ::2] = comp64
    ref = (G.dgrad_ref(dy64, w64.view(Ko, R, R, C), H, W, 1, R // 2) + scat) * dec.view(N, H, W, C)
    geo = (N, H, W, C, Ko, R, R, 1, R // 2)
    rep = []
    contract(lambda o: K.conv_bwd_data_pl(dyp, w1, compg, mbits, K.Planes(o["dx"]), *geo, sums=o["sums"], residual_s2=True),
             {"dx": Out((2, N, H, W, C), BF), "sums": Out((C,))}, {"dx": ref, "sums": ref.reshape(-1, C).sum(0)}, tl(3e-4), rep)
    _show(f"compact residual {geo}", rep)
    inp.check()


# ------------------------------------------------------------------------------------------------ geometries that are refused
@pytest.mark.parametrize("what,eps,code,cfg", G.REFUSED, ids=[r[0] for r in G.REFUSED])
def test_refused_geometry(what, eps, code, cfg):
    """ValueError with the code include/cxrk.h states, before anything is launched: outputs and their guards keep every sentinel.
    Each call is one that computes at a valid geometry with these very operands (no decision bits at Ko = 32, which would be refused
    for their own reason; test_geometry_planes runs that form), so the geometry rule of the row is the only ground for refusing.
    The operands are real, guarded tensors of the nearest valid size, so a library that did launch could not leave them either."""
    N, H, W, C, Ko, R, S, stride, pad = cfg
    Ho, Wo = (max(1, v) for v in G.conv_out(H, W, R, S, max(1, stride), pad))
    inp = Inputs()
    x, w, dy = rnd(N, H, W, C), rnd(Ko, R, S, C, seed=1), rnd(N, Ho, Wo, Ko, seed=2)
    vec = {k: (1 + 0.1 * rnd(Ko, seed=s)).to(DEV) for s, k in enumerate(("shift", "scale", "rstd", "rmean", "sumdy"))}
    xd, _ = inp.f32(x, "x")
    wd, _ = inp.f32(w, "w")
    dyd, _ = inp.f32(dy, "dy")
    y_pl, dx_pl = Out((2, N, Ho, Wo, Ko), BF), Out((2, N, H, W, C), BF)
    wspec = {"dw": Out((Ko, R, S, C)), "dg": Out((Ko,)), "db": Out((Ko,))}
    assert C % 8 == 0 and Ko % 8 == 0       # every row exists in both storage forms
    xp, _ = inp.planes(x, "x")
    wp, _ = inp.planes(w.reshape(Ko, -1), "w")
    dyp, _ = inp.planes(dy, "dy")
    if eps == "fdw":
        refused(lambda o: K.conv_fwd(xd, wd, vec["shift"], None, o["y"], *cfg, True), {"y": Out((N, Ho, Wo, Ko))}, code)
    if eps in ("fdw", "f_pl"):
        refused(lambda o: K.conv_fwd_pl(xp, wp, vec["shift"], None, K.Planes(o["y"]), None, *cfg, True), {"y": y_pl}, code)
    if eps in ("fdw", "d"):
        refused(lambda o: K.conv_bwd_data(dyd, wd, None, None, o["dx"], *cfg), {"dx": Out((N, H, W, C))}, code)
        refused(lambda o: K.conv_bwd_data(dyd, wd, None, None, o["dx"], *cfg, sums=o["sums"]), {"dx": Out((N, H, W, C)), "sums": Out((C,))}, code)
        refused(lambda o: K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(o["dx"]), *cfg), {"dx": dx_pl}, code)
        refused(lambda o: K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(o["dx"]), *cfg, sums=o["sums"]), {"dx": dx_pl, "sums": Out((C,))}, code)
    if eps == "fdw":
        refused(lambda o: K.conv_bwd_params(xd, dyd, wd, vec["scale"], vec["rstd"], vec["rmean"], vec["sumdy"], o["dw"], o["dg"], o["db"], False,
                                            N, H, W, C, C, Ko, R, S, stride, pad), wspec, code)
        refused(lambda o: K.conv_bwd_params_pl(xp, dyp, wd, vec["scale"], vec["rstd"], vec["rmean"], vec["sumdy"], o["dw"], o["dg"], o["db"], False,
                                               *cfg), wspec, code)
    inp.check()
