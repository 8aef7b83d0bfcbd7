"""Bit-exact probes of the split-bf16 ("planes") arithmetic on the device (tests/exact_ref.py holds the float64 reference, the
generators, their exactness guards and the compare functions; tests/test_exact_planes_host.py shows what those reject).

Part 2: every contraction entry point on INDEPENDENT small-integer hi / lo planes must give the three-term sum of DESIGN section 3
exactly (torch.equal / int16 bit patterns, no tolerance), term by term and all together, with every exact epilogue; the exact-fp32
MFMA paths on integer fp32 operands likewise; the plane readers that use no MFMA too.
Part 3: every planes writer produces canonical planes (hi = bf16(y), lo = bf16(y - hi), round-to-nearest-even twice).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
import exact_ref as X  # noqa: E402
from kernel_refs import attention_reference  # noqa: E402

DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- helpers
def PL(hi64, lo64=None):
    """float64 planes (values that are bf16 numbers) -> Planes on the device; lo = +0 when not given"""
    lo64 = torch.zeros_like(hi64) if lo64 is None else lo64
    hb, lb = hi64.bfloat16(), lo64.bfloat16()
    assert torch.equal(hb.double(), hi64) and torch.equal(lb.double(), lo64), "planes values must be bf16 numbers"
    return K.Planes(torch.stack([hb, lb]).contiguous().to(DEV))


def PLc(y32):
    """canonical planes of an fp32 CPU tensor, on the device"""
    return K.Planes(torch.stack(X.canonical_planes(y32)).contiguous().to(DEV))


def f32(v64):
    return X.to_f32_exact(v64).to(DEV)


def Z(t):
    return torch.zeros_like(t)


def label():
    return _lib.load().cxrk_last_launch_label().decode()


def last_split():
    return int(_lib.load().cxrk_last_launch_split_bf16())


def said_planes_gemm(wide, what):
    """the launch ran on the LDS-DMA planes kernel: the 256x256 tile exactly when the `wide` mode forces it (none of the shapes of
    this file reaches the 1 GFLOP from which the policy picks it on its own), a 128-class tile otherwise"""
    lb = label()
    assert lb.startswith("gemm_pw_kernel<") and last_split() == 1, (what, lb)
    assert lb.startswith("gemm_pw_kernel<Pw256,") == (wide == "wide"), (what, wide, lb)
    return lb


def pack_bits(dec):
    """bool [rows, C] -> uint8 [rows, C / 8] (bit c % 8 of byte c / 8)"""
    return torch.from_numpy(np.packbits(dec.numpy(), axis=1, bitorder="little")).to(DEV)


# the five launches of a term isolation: which planes are live in a and b
ISOLATION = [("hh", (1, 0), (1, 0)), ("hl", (1, 0), (0, 1)), ("lh", (0, 1), (1, 0)), ("ll", (0, 1), (0, 1)), ("all", (1, 1), (1, 1))]


def isolate(a, b, contract, run, what, check_out=X.assert_exact):
    """run(a planes, b planes) under the five plane selections; each result must equal the three-term sum of the planes given:
    exactly hh, hl, lh, 0 (lo x lo is dropped) and hh + hl + lh."""
    full = X.plane_terms(a[0], a[1], b[0], b[1], contract)
    X.guard_terms(a[0], a[1], b[0], b[1], contract, what=what)
    for name, ma, mb in ISOLATION:
        ah, al = (a[0] if ma[0] else Z(a[0])), (a[1] if ma[1] else Z(a[1]))
        bh, bl = (b[0] if mb[0] else Z(b[0])), (b[1] if mb[1] else Z(b[1]))
        terms = X.plane_terms(ah, al, bh, bl, contract)
        exp = X.three_term(terms)
        if name == "ll":
            assert float(exp.abs().max()) == 0.0 and float(terms["ll"].abs().max()) > 0.0
        elif name != "all":
            assert torch.equal(exp, full[name]) and float(exp.abs().max()) > 0.0
        check_out(run(PL(ah, al), PL(bh, bl)), exp, f"{what} [{name}]", terms)


# ================================================================================================ part 2: dense GEMMs
GEMM_SHAPES = [(33, 64, 8), (200, 136, 72), (300, 264, 520)]      # K tail of 8 inside a 16-wide MFMA, ragged M / N, > 1 tile each way
SPLITK_SHAPE = (1000, 64, 72)                                    # rows, N, K of a weight gradient the policy splits (3 slabs, the last shorter)


@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, Kd):
    """integer planes of every operand of the three GEMM forms of one layer shape; shared, never modified"""
    s = 7 * M + 3 * N + Kd
    return {"x": X.int_planes(M, Kd, seed=s), "w": X.int_planes(N, Kd, seed=s + 1), "dy": X.int_planes(M, N, seed=s + 2)}


def _nt(a, b):
    return a @ b.T


def _nn(a, b):
    return a @ b


def _tn(a, b):
    return a.T @ b


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_terms_nt(shape, precision, wide):
    c = _gemm_case(*shape)

    def run(xp, wp):
        out = K.linear_fwd_pl(xp, wp)
        said_planes_gemm(wide, "linear_fwd_pl")
        return out
    isolate(c["x"], c["w"], _nt, run, f"linear_fwd_pl {shape}")


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_terms_nn(shape, precision, wide):
    c = _gemm_case(*shape)

    def run(dyp, wp):
        out = K.linear_bwd_data_pl(dyp, wp)
        said_planes_gemm(wide, "linear_bwd_data_pl")
        return out
    isolate(c["dy"], c["w"], _nn, run, f"linear_bwd_data_pl {shape}")


@pytest.mark.parametrize("shape", GEMM_SHAPES + [SPLITK_SHAPE])
def test_gemm_terms_tn_fresh_and_accumulate(shape, precision, wide):
    M, N, Kd = shape
    c = _gemm_case(*shape)
    sk = K._wgrad_splitk(N, Kd, M, planes=True)
    if shape == SPLITK_SHAPE:
        assert sk > 1, "this shape is here for the policy's split-K"
    base = X.int_tensor(N, Kd, amax=50, seed=M)

    def run(dyp, xp):
        dw = torch.full((N, Kd), float("nan"), device=DEV)
        K.linear_bwd_weight_pl(dyp, xp, dw)
        said_planes_gemm(wide, "linear_bwd_weight_pl")
        return dw
    isolate(c["dy"], c["x"], _tn, run, f"linear_bwd_weight_pl {shape} splitk {sk}")
    terms = X.plane_terms(*c["dy"], *c["x"], _tn)
    X.guard_terms(*c["dy"], *c["x"], _tn, extra=base.abs(), what="accumulate")
    dw = f32(base)
    K.linear_bwd_weight_pl(PL(*c["dy"]), PL(*c["x"]), dw, accumulate=True)
    X.assert_exact(dw, base + X.three_term(terms), f"linear_bwd_weight_pl {shape} accumulate", terms)


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_pl_direct(shape, precision, wide):
    """gemm_pl itself: the NT form into a caller's buffer, and the TN form with an explicit split-K of 3"""
    M, N, Kd = shape
    c = _gemm_case(*shape)

    def run_nt(ap, bp):
        out = torch.full((M, N), float("nan"), device=DEV)
        K.gemm_pl(ap, bp, M, N, Kd, False, True, out=out)
        said_planes_gemm(wide, "gemm_pl NT")
        return out
    isolate(c["x"], c["w"], _nt, run_nt, f"gemm_pl NT {shape}")

    def run_tn(ap, bp):
        out = torch.full((N, Kd), float("nan"), device=DEV)
        K.gemm_pl(ap, bp, N, Kd, M, True, False, out=out, splitk=3)
        said_planes_gemm(wide, "gemm_pl TN splitk=3")
        return out
    isolate(c["dy"], c["x"], _tn, run_tn, f"gemm_pl TN splitk=3 {shape}")


def test_gemm_strided_rows(precision, wide):
    """the strided-row operand of test_planes_gemm_strided_rows (CLS rows: row stride L * H) at 16 rows, and a strided fp32 output"""
    B, L, H, N = 16, 4, 72, 64
    h = X.int_planes(B * L, H, seed=1)
    w = X.int_planes(N, H, seed=2)
    hp = PL(*h)
    cls = K.Planes(hp.t.view(2, B, L * H)[:, :, :H])
    a = tuple(p.view(B, L, H)[:, 0] for p in h)
    terms = X.plane_terms(*a, *w, _nt)
    X.guard_terms(*a, *w, _nt, what="strided rows")
    out = K.linear_fwd_pl(cls, PL(*w))
    said_planes_gemm(wide, "strided A")
    X.assert_exact(out, X.three_term(terms), "strided planes A", terms)
    dy = X.int_planes(B, N, seed=3)
    tn = X.plane_terms(*dy, *w, _nn)
    base = X.int_tensor(B * L, H, amax=9, seed=4)
    dx = f32(base)
    K.linear_bwd_data_pl(PL(*dy), PL(*w), out=dx.view(B, L * H)[:, :H], accumulate=True)
    exp = base.clone().view(B, L, H)
    exp[:, 0] += X.three_term(tn)
    X.assert_exact(dx.view(B, L, H), exp, "strided fp32 output rows, accumulate")
    src = X.int_planes(B, H, seed=5)
    K.planes_add_rows(PL(*src), dx.view(B, L * H)[:, :H])
    exp[:, 0] += src[0] + src[1]
    X.assert_exact(dx.view(B, L, H), exp, "planes_add_rows")


# ---- exact epilogues -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GEMM_SHAPES + [(200, 192, 72)])
def test_gemm_exact_epilogues(shape, precision, wide):
    """integer bias, integer fp32 and planes residual, ReLU with the decision bits, the bit mask on the way in, accumulate and the
    fused column sums: every one stays exact, into fp32 and into planes (GELU / GELU' are not exact: part 3)"""
    M, N, Kd = shape
    c = _gemm_case(*shape)
    xp, wp, dyp = PL(*c["x"]), PL(*c["w"]), PL(*c["dy"])
    t = X.plane_terms(*c["x"], *c["w"], _nt)
    z = X.three_term(t)
    bias = X.int_tensor(N, amax=40, seed=11)
    r32 = X.int_tensor(M, N, amax=60, seed=12)
    rp = X.int_planes(M, N, seed=13, amax_hi=60, amax_lo=5)
    X.guard_terms(*c["x"], *c["w"], _nt, extra=bias.abs()[None] + r32.abs() + rp[0].abs() + rp[1].abs(), what="NT epilogues")
    X.assert_exact(K.linear_fwd_pl(xp, wp, bias=f32(bias), residual=f32(r32)), z + bias + r32, "bias + fp32 residual -> fp32", t)
    X.assert_exact(K.linear_fwd_pl(xp, wp, bias=f32(bias), residual=PL(*rp)), z + bias + rp[0] + rp[1], "bias + planes residual -> fp32", t)
    y = K.linear_fwd_pl(xp, wp, bias=f32(bias), residual=PL(*rp), out_planes=True)
    said_planes_gemm(wide, "epilogue")
    X.assert_planes_exact(y.t, z + bias + rp[0] + rp[1], "bias + planes residual -> planes", t)
    X.assert_planes_exact(K.linear_fwd_pl(xp, wp, out_planes=True).t, z, "plain -> planes", t)
    X.assert_exact(K.linear_fwd_pl(xp, wp, bias=f32(bias), act=K.ACT_RELU), F.relu(z + bias), "bias + relu -> fp32", t)
    if N % 64 == 0:
        mask = torch.zeros(M, N // 8, dtype=torch.uint8, device=DEV)
        y = K.linear_fwd_pl(xp, wp, bias=f32(bias), act=K.ACT_RELU, out_planes=True, maskout=mask)
        X.assert_planes_exact(y.t, F.relu(z + bias), "bias + relu -> planes", t)
        assert torch.equal(K.unpack_mask(mask, N), (z + bias) > 0), "ReLU decision bits != (y > 0)"
        assert 0.2 < float(((z + bias) > 0).double().mean()) < 0.8
    # data-gradient form
    tn = X.plane_terms(*c["dy"], *c["w"], _nn)
    g = X.three_term(tn)
    ap = X.int_planes(M, Kd, seed=14, amax_hi=60, amax_lo=5)
    base = X.int_tensor(M, Kd, amax=60, seed=15)
    X.guard_terms(*c["dy"], *c["w"], _nn, extra=ap[0].abs() + ap[1].abs() + base.abs(), what="NN epilogues")
    X.assert_exact(K.linear_bwd_data_pl(dyp, wp, residual=PL(*ap)), g + ap[0] + ap[1], "dgrad + planes residual -> fp32", tn)
    dec = torch.rand(M, Kd, generator=torch.Generator().manual_seed(16)) > 0.5
    out = K.linear_bwd_data_pl(dyp, wp, maskin=pack_bits(dec), out_planes=True)
    X.assert_planes_exact(out.t, torch.where(dec, g, Z(g)), "dgrad bit mask -> planes", tn)      # a select: +0 where the bit is off
    out = f32(base)
    K.linear_bwd_data_pl(dyp, wp, out=out, accumulate=True)
    X.assert_exact(out, g + base, "dgrad accumulate", tn)
    X.guard_exact(g.abs().sum(0, keepdim=True) * 2 + 3.0, what="fused column sums")
    cs = torch.full((Kd,), 3.0, device=DEV)
    out = K.linear_bwd_data_pl(dyp, wp, out_planes=True, colsum=cs)
    X.assert_planes_exact(out.t, g, "dgrad -> planes beside the fused column sums", tn)
    X.assert_exact(cs, g.sum(0), "fused column sums")
    K.linear_bwd_data_pl(dyp, wp, maskin=pack_bits(dec), out_planes=True, colsum=cs, colsum_accumulate=True)
    X.assert_exact(cs, g.sum(0) + (g * dec).sum(0), "fused column sums of the masked gradient, accumulated")


# ================================================================================================ part 2: convolutions
# N, H, W, C, Ko, R, stride, pad, which mainloop the forward / data gradient / weight gradient takes under the policy
G_HALO = (2, 9, 7, 64, 64, 3, 1, 1)
CONV_GEOMS = {
    "3x3_64_halo": G_HALO,                                  # window-resident forward, data gradient, weight gradient (conv_halo*.h)
    "3x3_64_wide_row": (2, 3, 59, 64, 64, 3, 1, 1),         # rows of 59 pixels: the first the window kernels leave to the implicit GEMM
    "1x1_64_256": (2, 9, 7, 64, 256, 1, 1, 0),
    "1x1_s2_odd": (2, 7, 9, 64, 128, 1, 2, 0),
    "3x3_s2_128": (2, 7, 9, 128, 128, 3, 2, 1),
}


def _out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    N, H, W, C, Ko, R, stride, pad = CONV_GEOMS[name]
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    s = sum(ord(ch) for ch in name)
    return {"x": X.int_planes(N, H, W, C, seed=s), "w": X.int_planes(Ko, R, R, C, seed=s + 1), "dy": X.int_planes(N, Ho, Wo, Ko, seed=s + 2),
            "shift": X.int_tensor(Ko, amax=40, seed=s + 3), "res": X.int_planes(N, Ho, Wo, Ko, seed=s + 4, amax_hi=60, amax_lo=5),
            "add": X.int_planes(N, H, W, C, seed=s + 5, amax_hi=60, amax_lo=5), "w32": X.int_tensor(Ko, R, R, C, amax=3, seed=s + 6)}


def _contracts(geom):
    """float64 conv2d and its gradients on NHWC / [Ko][R][S][C] tensors (bilinear in their two operands)"""
    N, H, W, C, Ko, R, stride, pad = geom

    def fwd(x, w):
        return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()

    def dgrad(dy, w):
        return torch.nn.grad.conv2d_input((N, C, H, W), w.permute(0, 3, 1, 2).contiguous(), dy.permute(0, 3, 1, 2).contiguous(),
                                          stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()

    def wgrad(dy, x):
        return torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).contiguous(), (Ko, C, R, R), dy.permute(0, 3, 1, 2).contiguous(),
                                           stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    return fwd, dgrad, wgrad


def _expect_label(kind, name, wide, what):
    lb = label()
    if name == "3x3_64_halo" and kind in ("fwd", "dgrad") and wide != "wide":
        # the window kernels under the policy; the forced 256x256 mode sends this geometry to the implicit GEMM instead (the
        # process-wide CXRK_HALO switch is read once, so this is how one process runs both paths of the same geometry)
        assert lb == f"conv3x3_halo_kernel<{kind}>", (what, lb)
    elif name == "3x3_64_halo" and kind == "wgrad":
        assert lb == "conv3x3_wgrad_window_kernel", (what, lb)
    else:
        said_planes_gemm(wide, what)
    return lb


@pytest.mark.parametrize("name", list(CONV_GEOMS))
def test_conv_fwd_terms_and_epilogue(name, wide):
    geom = CONV_GEOMS[name]
    N, H, W, C, Ko, R, stride, pad = geom
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    c = _conv_case(name)
    fwd, _, _ = _contracts(geom)
    zero_shift = torch.zeros(Ko, device=DEV)

    def run(xp, wp):
        y = K.Planes.empty(N, Ho, Wo, Ko, device=DEV)
        K.conv_fwd_pl(xp, wp.view(Ko, R * R * C), zero_shift, None, y, None, N, H, W, C, Ko, R, R, stride, pad, False)
        _expect_label("fwd", name, wide, f"conv_fwd_pl {name}")
        return y.t
    isolate(c["x"], c["w"], fwd, run, f"conv_fwd_pl {name}", check_out=X.assert_planes_exact)
    # shift + planes residual + ReLU + decision bits
    t = X.plane_terms(*c["x"], *c["w"], fwd)
    pre = X.three_term(t) + c["shift"] + c["res"][0] + c["res"][1]
    X.guard_terms(*c["x"], *c["w"], fwd, extra=c["shift"].abs() + c["res"][0].abs() + c["res"][1].abs(), what="conv fwd epilogue")
    y = K.Planes.empty(N, Ho, Wo, Ko, device=DEV)
    mask = torch.zeros(N * Ho * Wo, Ko // 8, dtype=torch.uint8, device=DEV)
    K.conv_fwd_pl(PL(*c["x"]), PL(*c["w"]).view(Ko, R * R * C), f32(c["shift"]), PL(*c["res"]), y, mask, N, H, W, C, Ko, R, R, stride, pad, True)
    X.assert_planes_exact(y.t, F.relu(pre), f"conv_fwd_pl {name} shift + residual + relu", t)
    assert torch.equal(K.unpack_mask(mask, Ko), (pre > 0).view(-1, Ko)), "ReLU decision bits != (y > 0)"


@pytest.mark.parametrize("name", list(CONV_GEOMS))
def test_conv_bwd_data_terms_and_epilogue(name, wide):
    geom = CONV_GEOMS[name]
    N, H, W, C, Ko, R, stride, pad = geom
    c = _conv_case(name)
    _, dgrad, _ = _contracts(geom)

    def run(dyp, wp):
        dx = K.Planes.empty(N, H, W, C, device=DEV)
        K.conv_bwd_data_pl(dyp, wp.view(Ko, R * R * C), None, None, dx, N, H, W, C, Ko, R, R, stride, pad)
        _expect_label("dgrad", name, wide, f"conv_bwd_data_pl {name}")
        return dx.t
    isolate(c["dy"], c["w"], dgrad, run, f"conv_bwd_data_pl {name}", check_out=X.assert_planes_exact)
    t = X.plane_terms(*c["dy"], *c["w"], dgrad)
    g = X.three_term(t)
    if R == 1 and stride == 2:
        # the compact form: the even pixels only, a dense [N Ho Wo, Ko] x [Ko, C] product
        comp = K.conv1x1_s2_bwd_data_compact_pl(PL(*c["dy"]), PL(*c["w"]).view(Ko, C), N, H, W, C, Ko)
        said_planes_gemm(wide, "compact stride-2 data gradient")
        X.assert_planes_exact(comp.t, g[:, ::2, ::2].contiguous(), f"conv1x1_s2_bwd_data_compact_pl {name}",
                              {k: v[:, ::2, ::2].contiguous() for k, v in t.items()})
        odd = torch.ones(H, W, dtype=torch.bool)
        odd[::2, ::2] = False
        assert float(g[:, odd].abs().max()) == 0.0
        return
    # planes residual + bit mask + fused column sums
    dec = torch.rand(N * H * W, C, generator=torch.Generator().manual_seed(5)) > 0.5
    exp = torch.where(dec.view(N, H, W, C), g + c["add"][0] + c["add"][1], Z(g))       # a select: +0 where the bit is off
    X.guard_terms(*c["dy"], *c["w"], dgrad, extra=c["add"][0].abs() + c["add"][1].abs(), what="conv dgrad epilogue")
    X.guard_exact(exp.abs().sum((0, 1, 2)), what="conv dgrad column sums")
    dx = K.Planes.empty(N, H, W, C, device=DEV)
    sums = torch.full((C,), float("nan"), device=DEV)
    K.conv_bwd_data_pl(PL(*c["dy"]), PL(*c["w"]).view(Ko, R * R * C), PL(*c["add"]), pack_bits(dec), dx, N, H, W, C, Ko, R, R, stride, pad, sums=sums)
    X.assert_planes_exact(dx.t, exp, f"conv_bwd_data_pl {name} residual + bit mask", t)
    X.assert_exact(sums, exp.sum((0, 1, 2)), f"conv_bwd_data_pl {name} fused column sums")


@pytest.fixture
def window_wgrad_switch():
    """CXRK_HALO_WGRAD, read by the library on every call (as tests/test_conv3x3_wgrad_window_gpu.py switches it)"""
    old = os.environ.get("CXRK_HALO_WGRAD")

    def set_(v):
        if v is None:
            os.environ.pop("CXRK_HALO_WGRAD", None)
        else:
            os.environ["CXRK_HALO_WGRAD"] = v
    yield set_
    set_(old)


@pytest.mark.parametrize("name,window", [(n, None) for n in CONV_GEOMS] + [("3x3_64_halo", "0")])
def test_conv_bwd_params_terms(name, window, wide, window_wgrad_switch):
    """dW = scale * wgrad, dbeta = sumdy, dgamma = rstd * (<w, wgrad> - mean * sumdy) with scale = rstd = 1, mean = 0 and an integer
    w: all three stay integer.  ("3x3_64_halo", "0"): the same geometry with the window kernel switched off."""
    window_wgrad_switch(window)
    geom = CONV_GEOMS[name]
    N, H, W, C, Ko, R, stride, pad = geom
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    c = _conv_case(name)
    _, _, wgrad = _contracts(geom)
    ones, zeros = torch.ones(Ko, device=DEV), torch.zeros(Ko, device=DEV)
    w32 = c["w32"]
    outs = {}

    def run(dyp, xp, accumulate=False, dw=None):
        sumdy = K.colsum(dyp.view(N * Ho * Wo, Ko), torch.full((Ko,), float("nan"), device=DEV))
        dw = torch.full((Ko, R, R, C), float("nan"), device=DEV) if dw is None else dw
        dg, db = torch.full((Ko,), float("nan"), device=DEV), torch.full((Ko,), float("nan"), device=DEV)
        K.conv_bwd_params_pl(xp, dyp, f32(w32), ones, ones, zeros, sumdy, dw, dg, db, accumulate, N, H, W, C, Ko, R, R, stride, pad)
        if window == "0":
            lb = said_planes_gemm(wide, "window kernel switched off")
            assert "DmaConvIm2colMC" in lb, lb
        else:
            _expect_label("wgrad", name, wide, f"conv_bwd_params_pl {name}")
        outs["dg"], outs["db"], outs["dy"] = dg, db, dyp
        return dw

    def check(dw, exp, what, terms):
        X.assert_exact(dw, exp, what, terms)
        dy_val = outs["dy"].t.cpu().double().sum(0)
        X.guard_exact((w32.abs() * exp.abs()).sum((1, 2, 3)), what="dgamma")
        X.assert_exact(outs["dg"], (w32 * exp).sum((1, 2, 3)), what + ": dgamma")
        X.assert_exact(outs["db"], dy_val.sum((0, 1, 2)), what + ": dbeta")
    isolate(c["dy"], c["x"], wgrad, run, f"conv_bwd_params_pl {name} window={window}", check_out=check)
    t = X.plane_terms(*c["dy"], *c["x"], wgrad)
    base = X.int_tensor(Ko, R, R, C, amax=50, seed=3)
    X.guard_terms(*c["dy"], *c["x"], wgrad, extra=base.abs(), what="wgrad accumulate")
    dw = run(PL(*c["dy"]), PL(*c["x"]), accumulate=True, dw=f32(base))
    X.assert_exact(dw, base + X.three_term(t), f"conv_bwd_params_pl {name} accumulate", t)


# ---- the stem, fused with its max-pool -----------------------------------------------------------------------------------------
def _pool_ref(u):
    """3x3 / 2 / 1 max-pool of NHWC float64 values as maxpool_fwd_pl_kernel documents it: taps in (r, s) order, taps outside the
    image skipped, a later tap replaces only when strictly greater (the first valid tap wins ties) -> (best, tap index r * 3 + s)"""
    N, H, W, C = u.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    idx = torch.full((N, Ho, Wo, C), 255, dtype=torch.int64)
    hs, ws = torch.arange(Ho) * 2 - 1, torch.arange(Wo) * 2 - 1
    for r in range(3):
        for s in range(3):
            hi, wi = hs + r, ws + s
            vh, vw = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
            v = torch.full_like(best, float("-inf"))
            sub = u[:, hi[vh]][:, :, wi[vw]]
            v[:, vh.nonzero()[:, 0][:, None], vw.nonzero()[:, 0][None, :]] = sub
            valid = (vh[:, None] & vw[None, :])[None, :, :, None]
            take = valid & ((idx == 255) | (v > best))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, r * 3 + s), idx)
    return best, idx.to(torch.uint8)


def _planes_value(y32):
    """hi + lo of the canonical planes of y (what a planes tensor holds of y), float64"""
    hi, lo = X.canonical_planes(y32)
    return hi.double() + lo.double()


STEM_SMALL, STEM_BIG = [(2, 32, 32), (1, 38, 26)], (4, 224, 224)    # BIG: 1.26 GFLOP, where split-bf16 mode takes the bf16 mainloop


@functools.lru_cache(maxsize=None)
def _stem_case(shape, split):
    """(x, w, shift) float64 and the reference's pooled values / winner bytes.  Every eighth channel carries a shift so negative
    that all its stem values are 0: whole windows tie and the first valid tap must win."""
    N, H, W = shape
    C, Ko, R = 4, 64, 7
    seed = H + W

    def conv(x, w):
        return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=2, padding=3).permute(0, 2, 3, 1)
    if split:
        x, xh, xl = X.pq_values(N, H, W, C, seed=seed)
        w, wh, wl = X.pq_values(Ko, R, R, C, seed=seed + 1)
        for t_ in (x, xh, xl, w, wh, wl):
            t_[..., 3] = 0
        shift = X.int_tensor(Ko, amax=40, seed=seed + 2) * float(1 << 20)
        shift[::8] = -float((1 << 31) + (1 << 29))
        z = conv(xh, wh + wl) + conv(xl, wh)                       # hh + hl + lh, without lo * lo
        assert float(conv(xl, wl).abs().max()) > 0.0
        X.guard_exact(conv(xh.abs(), wh.abs() + wl.abs()) + conv(xl.abs(), wh.abs()) + shift.abs(), 256.0, "stem, split")
    else:
        x, w = X.int_f32(N, H, W, C, seed=seed, amax=15), X.int_f32(Ko, R, R, C, seed=seed + 1, amax=7)
        x[..., 3] = 0
        w[..., 3] = 0
        shift = X.int_tensor(Ko, amax=100, seed=seed + 2)
        shift[::8] = -100000.0
        z = conv(x, w)
        X.guard_exact(conv(x.abs(), w.abs()) + shift.abs(), 1.0, "stem, fp32")
    stem = F.relu(z + shift)
    assert float(stem[..., ::8].abs().max()) == 0.0 and float((stem[..., 1] > 0).double().mean()) > 0.2
    best, idx_ref = _pool_ref(_planes_value(X.to_f32_exact(stem)))
    return x, w, shift, best, idx_ref


@pytest.mark.parametrize("shape", STEM_SMALL + [STEM_BIG])
def test_stem_pool_exact(shape, precision):
    """stem_pool_fwd_pl reads an fp32 image and fp32 weights.  Under 1 GFLOP (either mode) and in fp32 mode it runs the exact-fp32
    mainloop: integer operands, expected = the plain convolution.  From 1 GFLOP in split-bf16 mode it splits both on the fly:
    operands x = 2^8 p + q (hi = 2^8 p, lo = q exactly), expected = the three-term convolution, at a granularity of 2^8.  The stem
    value passes through planes storage (hi + lo) before the pool; the pooled planes are canonical; the winner is the first tap."""
    N, H, W = shape
    split = precision == "split_bf16" and shape == STEM_BIG
    x, w, shift, best, idx_ref = _stem_case(shape, split)
    out = K.stem_pool_fwd_pl(f32(x), f32(w), f32(shift), N, H, W, 4, 64, 7, 7, 2, 3)
    assert out is not None
    assert label() == ("stem_pool_fwd_kernel<true>" if split else "stem_pool_fwd_kernel<false>") and last_split() == int(split), label()
    pooled, idx = out
    X.assert_planes_exact(pooled.t, best, f"stem_pool_fwd_pl {shape} split={split}")
    assert torch.equal(idx.cpu(), idx_ref), f"winner bytes differ at {(idx.cpu() != idx_ref).nonzero()[:4].tolist()}"
    # backward sums in pooled space: sum over the pooled pixels of g * [pooled > 0] (the sign is read off the hi plane)
    Hp, Wp = pooled.shape[1], pooled.shape[2]
    g = X.int_planes(N, Hp, Wp, 64, seed=H + 3)
    exp = ((g[0] + g[1]) * (pooled.t[0].cpu().double() > 0)).sum((0, 1, 2))
    X.guard_exact(((g[0] + g[1]).abs()).sum((0, 1, 2)), what="stem_pool_bwd_sums")
    X.assert_exact(K.stem_pool_bwd_sums(PL(*g), pooled), exp, f"stem_pool_bwd_sums {shape}")


# ================================================================================================ part 2: exact-fp32 MFMA paths
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_fp32_gemm_integer_operands(shape, precision):
    """kernels.gemm on integer fp32 operands, every transpose form and split-K: under 1 GFLOP the exact-fp32 MFMA in either mode"""
    M, N, Kd = shape
    x, w, dy = X.int_f32(M, Kd, seed=1), X.int_f32(N, Kd, seed=2), X.int_f32(M, N, seed=3)
    X.guard_exact(_nt(x.abs(), w.abs()))
    X.guard_exact(_tn(dy.abs(), x.abs()))
    xd, wd, dyd = f32(x), f32(w), f32(dy)
    X.assert_exact(K.linear_fwd(xd, wd), _nt(x, w), "gemm NT")
    assert label().startswith("gemm_f32_kernel<") and last_split() == 0, label()
    X.assert_exact(K.linear_bwd_data(dyd, wd), _nn(dy, w), "gemm NN")
    assert last_split() == 0
    dw = torch.full((N, Kd), float("nan"), device=DEV)
    X.assert_exact(K.linear_bwd_weight(dyd, xd, dw), _tn(dy, x), "gemm TN")
    X.assert_exact(K.linear_bwd_weight(dyd, xd, dw, accumulate=True), 2 * _tn(dy, x), "gemm TN accumulate")
    out = torch.full((N, Kd), float("nan"), device=DEV)
    X.assert_exact(K.gemm(dyd, xd, out, N, Kd, M, True, False, splitk=3), _tn(dy, x), "gemm TN splitk=3")
    assert last_split() == 0
    out = torch.full((M, N), float("nan"), device=DEV)
    X.assert_exact(K.gemm(xd, wd, out, M, N, Kd, False, True, splitk=2), _nt(x, w), "gemm NT splitk=2")


def test_fp32_gemm_large_launch_splits_on_the_fly(precision):
    """2048 x 1024 x 256 is 1.07 GFLOP: in split-bf16 mode the fp32 API splits its operands on the fly (gemm_x3_kernel) and the
    result is the three-term sum of the canonical planes of x = 2^8 p + q; in fp32 mode it is the plain product of integers."""
    M, N, Kd = 2048, 1024, 256
    if precision == "split_bf16":
        x, xh, xl = X.pq_values(M, Kd, seed=1)
        w, wh, wl = X.pq_values(N, Kd, seed=2)
        X.guard_exact(_nt(xh.abs(), wh.abs() + wl.abs()) + _nt(xl.abs(), wh.abs()), 256.0, "on-the-fly split")
        exp = _nt(xh, wh + wl) + _nt(xl, wh)
        assert float((_nt(xl, wl)).abs().max()) > 0.0
    else:
        x, w = X.int_f32(M, Kd, seed=1), X.int_f32(N, Kd, seed=2)
        X.guard_exact(_nt(x.abs(), w.abs()))
        exp = _nt(x, w)
    out = K.linear_fwd(f32(x), f32(w))
    assert last_split() == int(precision == "split_bf16"), label()
    assert label().startswith("gemm_x3_kernel<" if precision == "split_bf16" else "gemm_f32_kernel<"), label()
    X.assert_exact(out, exp, f"fp32 API at 1 GFLOP, {precision}")


@pytest.mark.parametrize("name", ["3x3_64_halo", "1x1_64_256"])
def test_fp32_conv_integer_operands(name, precision):
    geom = CONV_GEOMS[name]
    N, H, W, C, Ko, R, stride, pad = geom
    Ho, Wo = _out_hw(H, W, R, stride, pad)
    fwd, dgrad, wgrad = _contracts(geom)
    x, w, dy = X.int_f32(N, H, W, C, seed=1), X.int_f32(Ko, R, R, C, seed=2, amax=3), X.int_f32(N, Ho, Wo, Ko, seed=3)
    shift, res = X.int_tensor(Ko, amax=40, seed=4), X.int_tensor(N, Ho, Wo, Ko, amax=60, seed=5)
    X.guard_exact(fwd(x.abs(), w.abs()) + shift.abs() + res.abs())
    xd, wd, dyd = f32(x), f32(w), f32(dy)
    y = torch.full((N, Ho, Wo, Ko), float("nan"), device=DEV)
    K.conv_fwd(xd, wd, f32(shift), f32(res), y, N, H, W, C, Ko, R, R, stride, pad, True)
    assert label().startswith("gemm_f32_kernel<") and last_split() == 0, label()
    X.assert_exact(y, F.relu(fwd(x, w) + shift + res), f"conv_fwd {name}")
    X.guard_exact(dgrad(dy.abs(), w.abs()))
    dx = torch.full((N, H, W, C), float("nan"), device=DEV)
    K.conv_bwd_data(dyd, wd, None, None, dx, N, H, W, C, Ko, R, R, stride, pad)
    assert last_split() == 0
    X.assert_exact(dx, dgrad(dy, w), f"conv_bwd_data {name}")
    gw = wgrad(dy, x)
    X.guard_exact(wgrad(dy.abs(), x.abs()))
    X.guard_exact((w.abs() * gw.abs()).sum((1, 2, 3)))
    ones, zeros = torch.ones(Ko, device=DEV), torch.zeros(Ko, device=DEV)
    sumdy = K.colsum(dyd.view(-1, Ko), torch.full((Ko,), float("nan"), device=DEV))
    dw, dg, db = (torch.full(s, float("nan"), device=DEV) for s in ((Ko, R, R, C), (Ko,), (Ko,)))
    K.conv_bwd_params(xd, dyd, wd, ones, ones, zeros, sumdy, dw, dg, db, False, N, H, W, C, C, Ko, R, R, stride, pad)
    assert last_split() == 0
    X.assert_exact(dw, gw, f"conv_bwd_params {name}: dW")
    X.assert_exact(dg, (w * gw).sum((1, 2, 3)), f"conv_bwd_params {name}: dgamma")
    X.assert_exact(db, dy.sum((0, 1, 2)), f"conv_bwd_params {name}: dbeta")


def test_retrieval_ranks_integer_scores(precision):
    """scores of integer embeddings are exact integers with many ties: best positive, beaten-by and tied counts against float64"""
    Nq, Mg, D = 70, 300, 72
    Q, G = X.int_f32(Nq, D, seed=1, amax=3), X.int_f32(Mg, D, seed=2, amax=3)
    G[5] = G[7]
    X.guard_exact(_nt(Q.abs(), G.abs()))
    S = _nt(Q, G)
    for off in (0, 11):
        pos, greater, ties = K.retrieval_ranks(f32(Q), f32(G), diag_off=off)
        cols = torch.arange(Nq) + off
        p = S[torch.arange(Nq), cols]
        other = torch.ones(Nq, Mg, dtype=torch.bool)
        other[torch.arange(Nq), cols] = False
        X.assert_exact(pos, p, f"retrieval pos, diag_off {off}")
        assert torch.equal(greater.cpu().long(), ((S > p[:, None]) & other).sum(1)), "greater"
        assert torch.equal(ties.cpu().long(), ((S == p[:, None]) & other).sum(1)), "ties"
        assert int(ties.sum()) > 0


# ================================================================================================ part 2: plane readers without MFMA
@pytest.mark.parametrize("C", [8, 136])
@pytest.mark.parametrize("rows", [1, 5, 300])
def test_plane_readers_exact(rows, C):
    a, b = X.int_planes(rows, C, seed=rows + C, amax_hi=60, amax_lo=5), X.int_planes(rows, C, seed=rows + C + 1, amax_hi=60, amax_lo=5)
    av, bv = a[0] + a[1], b[0] + b[1]
    ap, bp = PL(*a), PL(*b)
    # Planes.float(): the merge kernel (contiguous, numel % 8 == 0) and the torch form (a strided row view)
    X.assert_exact(ap.float(), av, "merge kernel")
    if rows > 1:
        X.assert_exact(ap.rows(slice(0, rows, 2)).float(), av[::2], "Planes.float() of a strided view")
    X.guard_exact(av.abs().sum(0) + 7.0)
    X.assert_exact(K.colsum(ap, torch.full((C,), float("nan"), device=DEV)), av.sum(0), "colsum")
    X.assert_exact(K.colsum(ap, torch.full((C,), 7.0, device=DEV), accumulate=True), av.sum(0) + 7.0, "colsum accumulate")
    bs = X.int_tensor(C, amax=9, seed=C)
    X.guard_exact((av.abs() * (bv.abs() + bs.abs())).sum(0))
    X.assert_exact(K.coldot(ap, bp), (av * bv).sum(0), "coldot")
    X.assert_exact(K.coldot(ap, bp, f32(bs)), (av * (bv - bs)).sum(0), "coldot with bshift")
    X.assert_exact(K.coldot(ap, f32(bv)), (av * bv).sum(0), "coldot planes x fp32")
    # planes_add_rows into a row-strided fp32 view
    base = X.int_tensor(rows, 2 * C, amax=50, seed=3)
    dst = f32(base)
    K.planes_add_rows(ap, dst[:, :C])
    exp = base.clone()
    exp[:, :C] += av
    X.assert_exact(dst, exp, "planes_add_rows")
    # bn_apply with integer scale / shift (+ planes residual, ReLU and its bits), planes and fp32 storage
    sc, sh = X.int_tensor(C, amax=3, seed=4), X.int_tensor(C, amax=40, seed=5)
    pre = av * sc + sh + bv
    y, mask = K.bn_apply(ap, f32(sc), f32(sh), residual=bp, relu=True, want_mask=True)
    X.assert_planes_exact(y.t, F.relu(pre), "bn_apply planes")
    assert torch.equal(K.unpack_mask(mask, C), pre > 0)
    y32, _ = K.bn_apply(f32(av), f32(sc), f32(sh), residual=f32(bv), relu=False)
    X.assert_exact(y32, pre, "bn_apply fp32")


@pytest.mark.parametrize("C", [8, 136])
@pytest.mark.parametrize("rows", [1, 256])
def test_colstats_mean_exact_at_power_of_two_rows(rows, C):
    a = X.int_planes(rows, C, seed=rows + C, amax_hi=60, amax_lo=5)
    av = a[0] + a[1]
    mean, var = K.colstats(PL(*a))
    X.assert_exact(mean, av.sum(0) / rows, f"colstats mean, rows {rows}")
    if rows == 1:
        assert float(var.abs().max()) == 0.0


@pytest.mark.parametrize("C", [8, 136])
def test_maxpool_planes_exact(C):
    N, H, W = 2, 9, 7
    a = X.int_planes(N, H, W, C, seed=C, amax_hi=4, amax_lo=2)          # a narrow range: many ties
    u = a[0] + a[1]
    best, idx_ref = _pool_ref(u)
    y, idx = K.maxpool_fwd_pl(PL(*a))
    X.assert_planes_exact(y.t, best, "maxpool_fwd_pl")
    assert torch.equal(idx.cpu(), idx_ref), "first winner"
    assert float((idx_ref != 0).double().mean()) > 0.3
    # backward: the gradient goes to the winner, masked by the sign of the pooled value (read off its hi plane)
    Ho, Wo = best.shape[1], best.shape[2]
    g = X.int_planes(N, Ho, Wo, C, seed=C + 1)
    gv = (g[0] + g[1]) * (y.t[0].cpu().double() > 0)
    exp = torch.zeros(N, H, W, C, dtype=torch.float64)
    n_i, c_i = torch.arange(N)[:, None, None, None], torch.arange(C)[None, None, None, :]
    hh = (torch.arange(Ho) * 2 - 1)[None, :, None, None] + (idx_ref // 3).long()
    ww = (torch.arange(Wo) * 2 - 1)[None, None, :, None] + (idx_ref % 3).long()
    exp.index_put_((n_i.expand_as(hh), hh, ww, c_i.expand_as(hh)), gv, accumulate=True)
    X.assert_exact(K.maxpool_bwd_pl(PL(*g), idx, y, H, W), exp, "maxpool_bwd_pl")


# ================================================================================================ part 3: writers of known values
def test_split_planes_is_canonical():
    v = X.rounding_probe_values()
    p = K.split_planes(v.to(DEV))
    X.assert_planes_bits(p.t[0], p.t[1], v, "split_planes")
    y = X.canonical_planes(v)
    X.assert_exact(K.Planes(torch.stack(y).to(DEV)).float(), y[0].double() + y[1].double(), "merge of the probe planes")


def test_planes_range_up_to_the_largest_bf16():
    """every |x| up to the largest finite bf16 round-trips finite and exact (values of <= 16 bits); a finite fp32 value
    from the rounding threshold (2 - 2^-8) 2^127 up has hi = +-Inf, lo = -+Inf and reads back as NaN."""
    v = X.top_of_range_values()
    p = K.split_planes(v.to(DEV))
    X.assert_planes_bits(p.t[0], p.t[1], v, "top of the range")
    back = p.float().cpu()
    assert bool(torch.isfinite(p.t.float()).all()) and torch.equal(back, v)
    a = X.above_range_values()
    p = K.split_planes(a.to(DEV))
    X.assert_planes_bits(p.t[0], p.t[1], a, "above the range")
    assert bool(torch.isinf(p.t[0].float()).all()) and bool(torch.isnan(p.float()).all())


def _probe_matrix(M, N):
    v = X.rounding_probe_values()
    return v.repeat((M * N + v.numel() - 1) // v.numel())[:M * N].view(M, N).contiguous()


def test_epilogue_writers_round_like_the_canonical_split(precision, wide):
    """the GEMM epilogue (fp32 residual added to a zero product) and the convolution epilogue (planes residual) store the rounding
    probes as canonical planes; bn_apply and spatial_mean_bwd_pl too"""
    M, N, Kd = 200, 192, 72
    r = _probe_matrix(M, N)
    exp = torch.zeros(M, N) + r                                   # the accumulator is +0: -0 arrives as +0
    y = K.linear_fwd_pl(K.Planes.zeros(M, Kd, device=DEV), PL(*X.int_planes(N, Kd, seed=1)), residual=r.to(DEV), out_planes=True)
    said_planes_gemm(wide, "epilogue probe")
    X.assert_planes_bits(y.t[0], y.t[1], exp, "GEMM epilogue -> planes")
    # convolution epilogue, window kernel and implicit GEMM
    for name in ("3x3_64_halo", "1x1_64_256"):
        Nn, H, W, C, Ko, R, stride, pad = CONV_GEOMS[name]
        rp = PLc(_probe_matrix(Nn * H * W, Ko))
        val = rp.t[0].cpu().float() + rp.t[1].cpu().float()
        yc = K.Planes.empty(Nn, H, W, Ko, device=DEV)
        K.conv_fwd_pl(K.Planes.zeros(Nn, H, W, C, device=DEV), PL(*_conv_case(name)["w"]).view(Ko, R * R * C), torch.zeros(Ko, device=DEV),
                      rp.view(Nn, H, W, Ko), yc, None, Nn, H, W, C, Ko, R, R, stride, pad, False)
        X.assert_planes_bits(yc.t[0].view(-1, Ko), yc.t[1].view(-1, Ko), torch.zeros_like(val) + val, f"conv epilogue {name} -> planes")
    # bn_apply: z in planes storage, scale 1, shift 0
    zp = PLc(_probe_matrix(40, 64))
    zv = zp.t[0].cpu().float() + zp.t[1].cpu().float()
    yb, _ = K.bn_apply(zp, torch.ones(64, device=DEV), torch.zeros(64, device=DEV), relu=False)
    X.assert_planes_bits(yb.t[0], yb.t[1], zv * 1.0 + 0.0, "bn_apply -> planes")
    # spatial mean backward at a power-of-two pixel count: g / 4 is exact
    g = _probe_matrix(3, 128)
    g = torch.where(g.abs() < 1e-30, torch.zeros_like(g), g)      # keep g / 4 away from fp32's own subnormal range
    dx = K.spatial_mean_bwd_pl(g.to(DEV), 4)
    X.assert_planes_bits(dx.t[0], dx.t[1], (g * 0.25)[:, None, :].expand(3, 4, 128).contiguous(), "spatial_mean_bwd_pl")
    add = X.int_tensor(3, 4, 128, amax=60, seed=2).float()
    gi = X.int_tensor(3, 128, amax=1000, seed=3).float()
    dx = K.spatial_mean_bwd_pl(gi.to(DEV), 4, add=add.to(DEV))
    X.assert_planes_bits(dx.t[0], dx.t[1], (gi * 0.25)[:, None, :] + add, "spatial_mean_bwd_pl + add")


# ================================================================================================ part 3: writers of inexact values
def _same_as_fp32_form(planes, y32, what):
    """the planes output of an entry point against canonical_planes of its own fp32 output, bit for bit"""
    assert isinstance(planes, K.Planes) and tuple(planes.shape) == tuple(y32.shape), what
    assert bool(torch.isfinite(y32).all()), what
    X.assert_planes_bits(planes.t[0], planes.t[1], y32.cpu(), what)


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale


@pytest.mark.parametrize("H", [768, 64])
def test_layernorm_writers(H):
    rows = 77
    x, r = _rnd(rows, H).to(DEV), _rnd(rows, H, seed=1).to(DEV)
    g, b = (1 + 0.1 * _rnd(H, seed=2)).to(DEV), (0.1 * _rnd(H, seed=3)).to(DEV)
    y32, xhat, rstd = K.residual_ln_fwd(x, r, g, b, 1e-12)
    yp, _, _ = K.residual_ln_fwd(x, r, g, b, 1e-12, out_planes=True)
    _same_as_fp32_form(yp, y32, "residual_ln_fwd")
    gy, add = _rnd(rows, H, seed=4).to(DEV), _rnd(rows, H, seed=5).to(DEV)
    dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    for extra in ({}, {"dx_add": add}):
        dx32 = K.residual_ln_bwd(gy, xhat, rstd, g, dg, db, **extra)
        dxp = K.residual_ln_bwd(gy, xhat, rstd, g, dg, db, out_planes=True, **extra)
        _same_as_fp32_form(dxp, dx32, f"residual_ln_bwd {sorted(extra)}")


def test_embed_ln_writer():
    V, H, L, B = 50, 64, 8, 3
    word, pos, typ = _rnd(V, H).to(DEV), _rnd(16, H, seed=1).to(DEV), _rnd(H, seed=2).to(DEV)
    g, b = (1 + 0.1 * _rnd(H, seed=3)).to(DEV), (0.1 * _rnd(H, seed=4)).to(DEV)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(5)).to(DEV)
    y32, _, _ = K.embed_ln_fwd(ids, word, pos, typ, g, b, 1e-12, L)
    yp, _, _ = K.embed_ln_fwd(ids, word, pos, typ, g, b, 1e-12, L, out_planes=True)
    _same_as_fp32_form(yp, y32, "embed_ln_fwd")


@pytest.mark.parametrize("L,ragged", [(32, True), (65, True)])      # the one-block kernels and (L > 64) the tiled ones
def test_attention_writers(L, ragged):
    B, nH, dH = 3, 4, 64
    qkv, mask, gc, _, _ = attention_reference(B, L, nH, dH, ragged)
    qd, md, gd = qkv.to(DEV), mask.to(DEV), gc.to(DEV)
    c32, probs = K.attn_fwd(qd, md, B, L, nH, dH)
    cp, _ = K.attn_fwd(qd, md, B, L, nH, dH, out_planes=True)
    _same_as_fp32_form(cp, c32, f"attn_fwd L={L}")
    d32 = K.attn_bwd(qd, probs, gd, B, L, nH, dH)
    dp = K.attn_bwd(qd, probs, gd, B, L, nH, dH, out_planes=True)
    _same_as_fp32_form(dp, d32, f"attn_bwd L={L}")


@pytest.mark.parametrize("rows,C", [(300, 136), (5, 8)])
def test_bn_train_dz_writer(rows, C):
    dy, z = _rnd(rows, C), _rnd(rows, C, seed=1) * 3 + 5
    A, B, Cc = (_rnd(C, seed=s).to(DEV) for s in (2, 3, 4))
    dyp, zp = K.split_planes(dy.to(DEV)), K.split_planes(z.to(DEV))
    dz32 = K.bn_train_dz(dyp.float(), zp.float(), A, B, Cc)          # the same values, in fp32 storage
    _same_as_fp32_form(K.bn_train_dz(dyp, zp, A, B, Cc), dz32, "bn_train_dz")


def _two_roundings_of_fp32_form(planes, y32, what):
    """the derived fallback (exact_ref.assert_two_roundings) for a writer whose two output forms are not one instruction sequence"""
    assert isinstance(planes, K.Planes) and tuple(planes.shape) == tuple(y32.shape) and bool(torch.isfinite(y32).all()), what
    X.assert_two_roundings(planes.t[0], planes.t[1], y32, what)


@pytest.mark.parametrize("shape", [(200, 192, 72), (200, 136, 72)])
def test_gelu_epilogue_writers(shape, precision, wide):
    M, N, Kd = shape
    xp, wp = K.split_planes(_rnd(M, Kd, scale=0.5).to(DEV)), K.split_planes(_rnd(N, Kd, seed=1, scale=0.5).to(DEV))
    b = _rnd(N, seed=2).to(DEV)
    y32 = K.linear_fwd_pl(xp, wp, bias=b, act=K.ACT_GELU)
    _same_as_fp32_form(K.linear_fwd_pl(xp, wp, bias=b, act=K.ACT_GELU, out_planes=True), y32, f"GELU epilogue {shape}")
    # GELU': the two forms are different instantiations of one source line (csrc/gemm_epilogue.h, `v[q] *= gelu_erf_grad(aux)`).
    # EPI_KINDS holds EF_OUTPL | EF_AUX_GELU (kind 4, flags compiled in) but no fp32-output twin, so the fp32 form runs the generic
    # feature set (flags read at run time).  The library is built with the compiler's default floating-point contraction, which
    # may fuse the multiplies and adds of gelu_parts() (cxrk_common.h) differently in the two instantiations: the fp32 values
    # then differ in the last place at a fraction of a percent of the elements, and so does the rounding of lo.  The bit-exact
    # comparison therefore does not apply to this writer; it gets the derived bound.
    dyp, pre = K.split_planes(_rnd(M, N, seed=3, scale=0.5).to(DEV)), _rnd(M, Kd, seed=4).to(DEV)
    d32 = K.linear_bwd_data_pl(dyp, wp, aux=pre, auxmode=K.AUX_GELU_GRAD)
    _two_roundings_of_fp32_form(K.linear_bwd_data_pl(dyp, wp, aux=pre, auxmode=K.AUX_GELU_GRAD, out_planes=True), d32, f"GELU' epilogue {shape}")
