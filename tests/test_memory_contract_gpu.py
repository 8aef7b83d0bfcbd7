"""The memory contract of every cxrk entry point (tests/memguard.py): each call runs three times -- through the ordinary session
workspace, and through a workspace of EXACTLY the bytes its `*_ws_bytes` query returns, between guard regions, pre-filled once with
NaN and once with +-1e30 -- into outputs that sit between 4 MiB guards and start as a sentinel bit pattern.  Required: the three
results bit-identical (nothing reads memory it did not write), guards / pitch padding intact (nothing stores outside its tensor or
workspace), every output element written, and the values within the operation's bound of tests/test_kernels_gpu.py against a float64
CPU reference computed from the values the kernel actually sees.  ReLU / mask decisions are inputs here, never recomputed: no
element is excluded from any comparison.  Shapes sit on the edges of each kernel's partition arithmetic (part caps, ragged tiles,
empty split-K slabs, chunk boundaries), not at typical sizes."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memguard as MG
from kernel_refs import ln_bwd_ref as _ln_bwd_ref, ln_case as _ln_case      # shared with tests/test_fallback_paths_gpu.py

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
BF, U8, I32 = torch.bfloat16, torch.uint8, torch.int32


def _split() -> bool:
    return _cxr_lib.get_precision() == "split_bf16"


def tl(t: float) -> float:
    """the bound tests/test_kernels_gpu.py's close() applies: `t` of the output scale, at least 3e-4 in split-bf16 mode"""
    return max(t, 3e-4) if _split() else t


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.contiguous().to(DEV)


def pl(t):
    """fp32 CPU tensor -> (Planes on the device, the float64 values the kernels see)"""
    p = K.split_planes(dev(t.float()))
    return p, p.float().cpu().double()


def pitched(t, ld):
    """device copy of a 2-D tensor with row pitch ld inside guards; returns (view, guard object to check afterwards)"""
    g = MG.Guarded(t.shape, t.dtype, ld=ld, device=DEV, name="pitched input").load(t)
    return g.t, g


def pitched_planes(t, ld):
    """Planes [rows, cols] with row pitch ld (both planes and the gap between them guarded) + the float64 values seen"""
    p = K.split_planes(dev(t.float()))
    g = MG.Guarded((2,) + tuple(t.shape), BF, ld=ld, gap=24, device=DEV, name="pitched planes input").load(p.t)
    return K.Planes(g.t), g, p.float().cpu().double()


def bits_of(dec):
    """bool [rows, C] -> packed ReLU decision bits [rows, C / 8] on the device"""
    return torch.from_numpy(np.packbits(dec.numpy(), axis=1, bitorder="little")).to(DEV)


def contract(call, outs, ref=None, tol=None):
    return MG.run_contract(call, outs, ref, tol, module=K, device=DEV)


def refusals(call, outs):
    """declared size 0 -> CXRK_ERR_WS; full size but 4 bytes off the 256-byte alignment the header states -> bad argument"""
    MG.refuses_short_workspace(call, outs, module=K, device=DEV)
    MG.refuses_misaligned_workspace(call, outs, module=K, device=DEV)


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_SHAPES = [(r, c) for r in (1, 511, 512, 513) for c in (6, 8, 136, 264)] + [(262145, 8), (262145, 264)]


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES)
def test_colsum_family(rows, cols):
    """cxrk_colsum / _pl / cxrk_colvar: 512 rows per part, at most 512 parts (262 145 rows: rows_per 513, the part count recomputed
    to 511), a second 256-column block above 256 columns, the scalar kernel at 6 columns; pitched input, alpha, accumulation.
    Bound 2e-5 of the output scale: the 262 145 x 264 float32 sum in the kernel's order is 4.4e-7 off float64 (a lost part: 2e-3)."""
    x = rnd(rows, cols)
    x64 = x.double()
    base = rnd(cols, seed=7)
    xd = dev(x)
    contract(lambda o: K.colsum(xd, o["out"]), {"out": Out((cols,))}, {"out": x64.sum(0)}, tl(2e-5))
    big = rows > 1000
    if not big:
        xp, g = pitched(x, cols + (8 if cols % 4 == 0 else 1))
        contract(lambda o: K.colsum(xp, o["out"], alpha=-0.5, accumulate=True), {"out": Out((cols,), init=base)},
                 {"out": base.double() - 0.5 * x64.sum(0)}, tl(2e-5))
        g.check()
    mean = dev((x64.mean(0) + 0.1).float())
    dv = x64 - mean.cpu().double()
    contract(lambda o: K.colvar(xd, mean, o["out"], alpha=0.25), {"out": Out((cols,))}, {"out": 0.25 * (dv * dv).sum(0)}, tl(2e-5))
    if cols % 8:
        return
    p, seen = pl(x)
    contract(lambda o: K.colsum(p, o["out"], alpha=2.0), {"out": Out((cols,))}, {"out": 2.0 * seen.sum(0)}, tl(2e-5))
    dv = seen - mean.cpu().double()
    contract(lambda o: K.colvar(p, mean, o["out"]), {"out": Out((cols,))}, {"out": (dv * dv).sum(0)}, tl(2e-5))
    if not big:
        pp, g, seen = pitched_planes(x, cols + 16)
        contract(lambda o: K.colsum(pp, o["out"], accumulate=True), {"out": Out((cols,), init=base)}, {"out": base.double() + seen.sum(0)},
                 tl(2e-5))
        g.check()
    if (rows, cols) == (513, 136):
        refusals(lambda o: K.colsum(xd, o["out"]), {"out": Out((cols,))})
        refusals(lambda o: K.colsum(p, o["out"]), {"out": Out((cols,))})
        refusals(lambda o: K.colvar(xd, mean, o["out"]), {"out": Out((cols,))})


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("rows,C", [(r, c) for r in (1, 2, 777, 70000) for c in (8, 264)])
def test_colstats_coldot(rows, C, planes):
    """cxrk_colstats (two partial regions in one workspace) and cxrk_coldot (with and without the shift), bounds as in
    test_train_mode_batchnorm_kernels: mean 1e-6, variances and dots 2e-5."""
    g = torch.Generator().manual_seed(rows + C)
    z = torch.randn(rows, C, generator=g) * torch.linspace(0.1, 3.0, C) + torch.linspace(-300.0, 300.0, C)
    a = torch.randn(rows, C, generator=g)
    if planes:
        (zd, z64), (ad, a64) = pl(z), pl(a)
    else:
        zd, z64, ad, a64 = dev(z), z.double(), dev(a), a.double()
    m64 = z64.mean(0)
    for unbiased in (False, True):
        if rows == 1 and unbiased:
            continue
        var = ((z64 - m64) ** 2).sum(0) / (max(1, rows - 1) if unbiased else rows)
        ref = {"mean": m64} if rows == 1 else {"mean": m64, "var": var}
        o = contract(lambda o: K.colstats(zd, unbiased=unbiased, out=(o["mean"], o["var"])), {"mean": Out((C,)), "var": Out((C,))}, ref,
                     {"mean": tl(1e-6), "var": tl(2e-5)})
        if rows == 1:
            assert float(o["var"].t.abs().max()) == 0.0
    shift = dev(m64.float())
    contract(lambda o: K.coldot(ad, zd, out=o["out"]), {"out": Out((C,))}, {"out": (a64 * z64).sum(0)}, tl(2e-5))
    contract(lambda o: K.coldot(ad, zd, shift, out=o["out"]), {"out": Out((C,))}, {"out": (a64 * (z64 - shift.cpu().double())).sum(0)},
             tl(2e-5))
    if (rows, C) == (777, 264):
        refusals(lambda o: K.colstats(zd, out=(o["mean"], o["var"])), {"mean": Out((C,)), "var": Out((C,))})
        refusals(lambda o: K.coldot(ad, zd, out=o["out"]), {"out": Out((C,))})


# ------------------------------------------------------------------------------------------------ split-K GEMM
@pytest.mark.parametrize("M,N,Kd", [(136, 72, 203), (64, 264, 1000), (200, 136, 72)])
@pytest.mark.parametrize("splitk", [2, 3, 7, 40])
def test_gemm_splitk_fp32(M, N, Kd, splitk):
    """dw[M, N] = alpha a[Kd, M]^T b[Kd, N] through split-K slabs in the workspace: ragged in every dimension, and more slabs than
    K-tiles (splitk 40 against 72 / 203 reduction rows): a slab with no work must be zero or left out, never stale.  Bound 5e-5
    (the weight-gradient bound of test_gemm_nn_tn / test_gemm_strided_rows_and_large_splitk)."""
    a, b = rnd(Kd, M), rnd(Kd, N, seed=1)
    ref = a.double().T @ b.double()
    ad, bd = dev(a), dev(b)
    base = rnd(M, N, seed=2)
    contract(lambda o: K.gemm(ad, bd, o["c"], M, N, Kd, True, False, splitk=splitk), {"c": Out((M, N))}, {"c": ref}, tl(5e-5))
    contract(lambda o: K.gemm(ad, bd, o["c"], M, N, Kd, True, False, splitk=splitk, alpha=-0.75, accumulate=True),
             {"c": Out((M, N), ld=N + 4, init=base)}, {"c": base.double() - 0.75 * ref}, tl(5e-5))
    if splitk == 3 and M == 136:
        refusals(lambda o: K.gemm(ad, bd, o["c"], M, N, Kd, True, False, splitk=splitk), {"c": Out((M, N))})


@pytest.mark.parametrize("M,N,Kd", [(136, 72, 200), (64, 264, 1000), (264, 520, 136)])
@pytest.mark.parametrize("splitk", [2, 3, 7, 40])
def test_gemm_splitk_planes(M, N, Kd, splitk, wide):
    """the same on planes operands (cxrk_gemm_pl, fp32 output); bound 2e-4 (test_planes_gemm_family)"""
    a, b = rnd(Kd, M, scale=0.5), rnd(Kd, N, seed=1, scale=0.5)
    (ap, a64), (bp, b64) = pl(a), pl(b)
    ref = a64.T @ b64
    base = rnd(M, N, seed=2)
    contract(lambda o: K.gemm_pl(ap, bp, M, N, Kd, True, False, out=o["c"], splitk=splitk), {"c": Out((M, N))}, {"c": ref}, tl(2e-4))
    contract(lambda o: K.gemm_pl(ap, bp, M, N, Kd, True, False, out=o["c"], splitk=splitk, alpha=0.5, accumulate=True),
             {"c": Out((M, N), init=base)}, {"c": base.double() + 0.5 * ref}, tl(2e-4))
    if splitk == 3 and M == 136:
        refusals(lambda o: K.gemm_pl(ap, bp, M, N, Kd, True, False, out=o["c"], splitk=splitk), {"c": Out((M, N))})


# ------------------------------------------------------------------------------------------------ planes GEMM, fused column sums
@pytest.mark.parametrize("N", [8, 136, 768])
@pytest.mark.parametrize("M", [1, 63, 65, 200, 1000, 4096])
def test_gemm_pl_fused_colsum(M, N, wide):
    """dx = dy w (+ mask bits) with the column sums of the stored dx from the same epilogue: one partial row per 64 output rows of the
    padded row tiling -- ragged last tiles, a single row, tiles of 64 / 128 / 256 rows.  Planes and fp32 output, pitched fp32 output
    (the CLS-row case), fresh and accumulated sums.  Bounds of test_planes_gemm_family: 2e-4 output, 4 x 2e-4 column sums."""
    Kd = 72
    dy, w = rnd(M, Kd, scale=0.5), rnd(Kd, N, seed=1, scale=0.5)
    (dyp, dy64), (wp, w64) = pl(dy), pl(w)
    ref = dy64 @ w64
    base = rnd(N, seed=3)
    contract(lambda o: K.linear_bwd_data_pl(dyp, wp, out=K.Planes(o["dx"]), colsum=o["cs"]), {"dx": Out((2, M, N), BF), "cs": Out((N,))},
             {"dx": ref, "cs": ref.sum(0)}, {"dx": tl(2e-4), "cs": tl(8e-4)})
    contract(lambda o: K.linear_bwd_data_pl(dyp, wp, out=o["dx"], colsum=o["cs"], colsum_accumulate=True),
             {"dx": Out((M, N), ld=N + 24), "cs": Out((N,), init=base)}, {"dx": ref, "cs": base.double() + ref.sum(0)},
             {"dx": tl(2e-4), "cs": tl(8e-4)})
    dec = rnd(M, N, seed=6) > 0
    mbits = bits_of(dec)
    refm = ref * dec
    contract(lambda o: K.linear_bwd_data_pl(dyp, wp, maskin=mbits, out=K.Planes(o["dx"]), colsum=o["cs"]),
             {"dx": Out((2, M, N), BF, gap=64), "cs": Out((N,))}, {"dx": refm, "cs": refm.sum(0)}, {"dx": tl(2e-4), "cs": tl(8e-4)})
    if (M, N) == (200, 136):
        refusals(lambda o: K.linear_bwd_data_pl(dyp, wp, out=o["dx"], colsum=o["cs"]), {"dx": Out((M, N)), "cs": Out((N,))})


# ------------------------------------------------------------------------------------------------ convolution gradients
def _filters(Ko, R, C, seed=1):
    return rnd(Ko, R, R, C, seed=seed, scale=1.0 / math.sqrt(C * R * R))


def _dgrad_ref(dy64, w64, N, H, W, C, R, stride, pad):
    """float64 data gradient, NHWC: dy [N, Ho, Wo, Ko], w [Ko, R, R, C]"""
    dx = torch.nn.grad.conv2d_input((N, C, H, W), w64.permute(0, 3, 1, 2), dy64.permute(0, 3, 1, 2), stride=stride, padding=pad)
    return dx.permute(0, 2, 3, 1).contiguous()


DGRADS = [  # N, H, W, C, Ko, R, stride, pad
    (2, 15, 15, 64, 128, 3, 2, 1), (3, 7, 9, 128, 64, 3, 2, 1), (2, 14, 14, 512, 64, 3, 2, 1),
    (2, 12, 12, 64, 64, 3, 1, 1), (3, 56, 56, 64, 64, 3, 1, 1), (5, 7, 58, 64, 64, 3, 1, 1), (2, 9, 59, 64, 64, 3, 1, 1), (1, 3, 5, 64, 64, 3, 1, 1),
    (2, 14, 14, 64, 256, 1, 1, 0), (3, 9, 9, 128, 128, 3, 1, 1), (2, 7, 7, 512, 64, 1, 1, 0), (2, 7, 9, 128, 64, 1, 1, 0),
    (12, 56, 56, 64, 64, 1, 1, 0),          # 37 632 pixels: 588 partial rows -> the two-stage finish (np > 512)
]


@pytest.mark.parametrize("cfg", DGRADS)
def test_conv_bwd_data_with_sums(cfg, wide):
    """cxrk_conv_bn_act_bwd_data / _pl / _pl_s2res with the fused column sums: the query is an upper bound over tile choices, the launch
    counts partial rows from the tile policy, the window-resident kernel and the parity classes, and finishes in one or two stages
    behind them.  With residual and mask (inputs), and plain.  Bounds: 5e-5 fp32 operands, 3e-4 planes (the conv tests)."""
    N, H, W, C, Ko, R, stride, pad = cfg
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    dy, w, add = rnd(N, Ho, Wo, Ko, seed=2), _filters(Ko, R, C), rnd(N, H, W, C, seed=3)
    dec = rnd(N * H * W, C, seed=4) > 0
    args = (N, H, W, C, Ko, R, R, stride, pad)
    # planes
    (dyp, dy64), (wp, w64), (addp, add64) = pl(dy), pl(w.reshape(Ko, -1)), pl(add)
    mbits = bits_of(dec)
    g64 = _dgrad_ref(dy64, w64.view(Ko, R, R, C), N, H, W, C, R, stride, pad)
    full = (g64 + add64) * dec.view(N, H, W, C)
    spec = {"dx": Out((2, N, H, W, C), BF), "sums": Out((C,))}
    tol = {"dx": tl(3e-4), "sums": tl(3e-4)}
    contract(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *args, sums=o["sums"]), spec,
             {"dx": full, "sums": full.reshape(-1, C).sum(0)}, tol)
    contract(lambda o: K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(o["dx"]), *args, sums=o["sums"]), spec,
             {"dx": g64, "sums": g64.reshape(-1, C).sum(0)}, tol)
    if stride == 1:
        comp, comp64 = pl(rnd(N, (H + 1) // 2, (W + 1) // 2, C, seed=5))
        scat = torch.zeros(N, H, W, C, dtype=torch.float64)
        scat[:, ::2, ::2] = comp64
        s2 = (g64 + scat) * dec.view(N, H, W, C)
        contract(lambda o: K.conv_bwd_data_pl(dyp, wp, comp, mbits, K.Planes(o["dx"]), *args, sums=o["sums"], residual_s2=True), spec,
                 {"dx": s2, "sums": s2.reshape(-1, C).sum(0)}, tol)
    if wide != "policy":          # fp32 operands never take the 256x256 kernel: once is enough
        return
    src = rnd(N, H, W, C, seed=6)
    dyd, wd, addd, srcd = dev(dy), dev(w), dev(add), dev(src)
    g64 = _dgrad_ref(dy.double(), w.double(), N, H, W, C, R, stride, pad)
    full = (g64 + add.double()) * (src > 0)
    spec = {"dx": Out((N, H, W, C)), "sums": Out((C,))}
    contract(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *args, sums=o["sums"]), spec,
             {"dx": full, "sums": full.reshape(-1, C).sum(0)}, tl(5e-5))
    if cfg == DGRADS[0]:
        refusals(lambda o: K.conv_bwd_data(dyd, wd, addd, srcd, o["dx"], *args, sums=o["sums"]), spec)
        refusals(lambda o: K.conv_bwd_data_pl(dyp, wp, addp, mbits, K.Planes(o["dx"]), *args, sums=o["sums"]),
                 {"dx": Out((2, N, H, W, C), BF), "sums": Out((C,))})
    if cfg == DGRADS[3]:
        refusals(lambda o: K.conv_bwd_data_pl(dyp, wp, comp, mbits, K.Planes(o["dx"]), *args, sums=o["sums"], residual_s2=True),
                 {"dx": Out((2, N, H, W, C), BF), "sums": Out((C,))})


WGRADS = [  # N, H, W, C (real), Cpad, Ko, R, stride, pad
    (2, 32, 32, 3, 4, 64, 7, 2, 3), (2, 14, 14, 64, 64, 256, 1, 1, 0), (3, 9, 9, 128, 128, 128, 3, 1, 1), (2, 15, 15, 64, 64, 128, 3, 2, 1),
    (2, 7, 7, 512, 512, 2048, 1, 1, 0), (2, 12, 12, 64, 64, 64, 3, 1, 1), (3, 13, 13, 128, 128, 256, 1, 2, 0),
]


@pytest.mark.parametrize("cfg", WGRADS)
def test_conv_bwd_params(cfg, wide):
    """cxrk_conv_bn_act_bwd_params / _pl: split-K slabs plus the dgamma dot partials behind them in one workspace sized for the
    larger of two split-K policies.  With and without dgamma, accumulated.  Bounds: weight gradient 5e-5 / 3e-4 (planes), dbeta
    the same; dgamma 2e-3 / 2e-2 (planes) on these zero-mean inputs, as in the conv tests."""
    N, H, W, C, Cpad, Ko, R, stride, pad = cfg
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    x = torch.zeros(N, H, W, Cpad)
    x[..., :C] = rnd(N, H, W, C)
    dy, w = rnd(N, Ho, Wo, Ko, seed=2), _filters(Ko, R, C)
    scale, rstd, rmean = 1 + 0.1 * rnd(Ko, seed=3), 0.5 + rnd(Ko, seed=4).abs(), 0.1 * rnd(Ko, seed=5)
    base_w, base_g, base_b = rnd(Ko, R, R, C, seed=6), rnd(Ko, seed=7), rnd(Ko, seed=8)
    sd, rd, md, wd = dev(scale), dev(rstd), dev(rmean), dev(w)

    def refs(x64, dy64):
        raw = torch.nn.grad.conv2d_weight(x64.permute(0, 3, 1, 2), (Ko, Cpad, R, R), dy64.permute(0, 3, 1, 2), stride=stride, padding=pad)
        raw = raw.permute(0, 2, 3, 1)[..., :C]
        sumdy = dy64.reshape(-1, Ko).sum(0)
        dgam = rstd.double() * ((w.double() * raw).sum((1, 2, 3)) - rmean.double() * sumdy)
        return scale.double()[:, None, None, None] * raw, dgam, sumdy

    def run(fn, xin, dyin, x64, dy64, tw, tg):
        dw64, dg64, sumdy64 = refs(x64, dy64)
        sumdy = dev(sumdy64.float())
        spec = {"dw": Out((Ko, R, R, C)), "dg": Out((Ko,)), "db": Out((Ko,))}
        contract(lambda o: fn(xin, dyin, wd, sd, rd, md, sumdy, o["dw"], o["dg"], o["db"], False), spec,
                 {"dw": dw64, "dg": dg64, "db": sumdy.cpu().double()}, {"dw": tw, "dg": tg, "db": tw})
        contract(lambda o: fn(xin, dyin, wd, sd, rd, md, sumdy, o["dw"], o["dg"], o["db"], True),
                 {"dw": Out((Ko, R, R, C), init=base_w), "dg": Out((Ko,), init=base_g), "db": Out((Ko,), init=base_b)},
                 {"dw": base_w.double() + dw64, "dg": base_g.double() + dg64, "db": base_b.double() + sumdy.cpu().double()},
                 {"dw": tw, "dg": tg, "db": tw})
        contract(lambda o: fn(xin, dyin, wd, sd, None, None, None, o["dw"], None, None, False), {"dw": Out((Ko, R, R, C))}, {"dw": dw64}, tw)
        return spec, sumdy

    xd, dyd = dev(x), dev(dy)
    tail = (N, H, W, C, Cpad, Ko, R, R, stride, pad)
    if wide == "policy":          # fp32 operands never take the 256x256 kernel: once is enough
        spec, sumdy = run(lambda a, b, *r: K.conv_bwd_params(a, b, *r, *tail), xd, dyd, x.double(), dy.double(), tl(5e-5), 2e-2 if _split() else 2e-3)
        if cfg == WGRADS[2]:
            refusals(lambda o: K.conv_bwd_params(xd, dyd, wd, sd, rd, md, sumdy, o["dw"], o["dg"], o["db"], False, *tail), spec)
    if Cpad != C:
        return
    (xp, x64), (dyp, dy64) = pl(x), pl(dy)
    tail = (N, H, W, C, Ko, R, R, stride, pad)
    spec, sumdy = run(lambda a, b, *r: K.conv_bwd_params_pl(a, b, *r, *tail), xp, dyp, x64, dy64, tl(3e-4), 2e-2)
    if cfg == WGRADS[2]:
        refusals(lambda o: K.conv_bwd_params_pl(xp, dyp, wd, sd, rd, md, sumdy, o["dw"], o["dg"], o["db"], False, *tail), spec)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("H", [64, 128, 768])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 77, 16400])
def test_residual_ln_bwd(rows, H):
    """cxrk_residual_ln_bwd: 16 rows per block up to 1024 blocks (16 400 rows: rows_per 17, block count recomputed), two or three
    partial regions per block.  dx fp32 / planes, dx_add, dxsum fresh / accumulated, dgamma / dbeta accumulated.  Bound 2e-5
    (test_layernorm_fwd_bwd)."""
    dy, xhat, rstd, gamma, add = _ln_case(rows, H)
    dx64, dg64, db64 = _ln_bwd_ref(dy.double(), xhat.double(), rstd.double(), gamma.double())
    dyd, xd, rd, gd, addd = dev(dy), dev(xhat), dev(rstd), dev(gamma), dev(add)
    base = rnd(H, seed=9)
    t = tl(2e-5)
    vec = {"dg": Out((H,)), "db": Out((H,))}
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], dx_add=addd, out=o["dx"]), dict(vec, dx=Out((rows, H))),
             {"dx": dx64 + add.double(), "dg": dg64, "db": db64}, t)
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], dx_add=addd, out=K.Planes(o["dx"]), dxsum=o["s"]),
             dict(vec, dx=Out((2, rows, H), BF), s=Out((H,))),
             {"dx": dx64 + add.double(), "dg": dg64, "db": db64, "s": (dx64 + add.double()).sum(0)}, t)
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], accumulate=True, out=o["dx"], dxsum=o["s"], dxsum_accumulate=True),
             {"dg": Out((H,), init=base), "db": Out((H,), init=base), "dx": Out((rows, H)), "s": Out((H,), init=base)},
             {"dx": dx64, "dg": base.double() + dg64, "db": base.double() + db64, "s": base.double() + dx64.sum(0)}, t)
    if (rows, H) == (77, 128):
        refusals(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], out=o["dx"]), dict(vec, dx=Out((rows, H))))


@pytest.mark.parametrize("rows_per_seq,rows,H", [(1, 1, 64), (16, 16 * 5, 128), (11, 11 * 7, 768), (16, 16400, 64)])
def test_residual_ln_bwd_drop(rows_per_seq, rows, H):
    """cxrk_residual_ln_bwd_drop, mode 1 (dx, dxm = keep s dx, column sums of dxm) and mode 2 (dy masked on load), against the keep
    mask cxrk_dropout_mask gives for the same descriptor (an input of the reference).  Bound 2e-5."""
    dy, xhat, rstd, gamma, _ = _ln_case(rows, H)
    dyd, xd, rd, gd = dev(dy), dev(xhat), dev(rstd), dev(gamma)
    drop = K.Drop(seed=0x1234567890, counter=5, layer=1, site=K.DROP_ATTN_OUT, row_offset=3, p=0.25)
    nseq = rows // rows_per_seq
    keep = K.dropout_mask(drop, nseq, rows_per_seq, H).view(rows, H).cpu().double() / (1 - 0.25)
    t = tl(2e-5)
    dx64, dg64, db64 = _ln_bwd_ref(dy.double(), xhat.double(), rstd.double(), gamma.double())
    base = rnd(H, seed=9)
    spec = {"dg": Out((H,)), "db": Out((H,)), "dx": Out((rows, H)), "dxm": Out((rows, H)), "s": Out((H,), init=base)}
    contract(lambda o: K.residual_ln_bwd_drop(dyd, xd, rd, gd, o["dg"], o["db"], drop, rows_per_seq, out=(o["dx"], o["dxm"]), dxsum=o["s"],
                                              dxsum_accumulate=True), spec,
             {"dx": dx64, "dxm": dx64 * keep, "dg": dg64, "db": db64, "s": base.double() + (dx64 * keep).sum(0)}, t)
    specp = {"dg": Out((H,)), "db": Out((H,)), "dx": Out((2, rows, H), BF), "dxm": Out((2, rows, H), BF), "s": Out((H,))}
    contract(lambda o: K.residual_ln_bwd_drop(dyd, xd, rd, gd, o["dg"], o["db"], drop, rows_per_seq, out=(K.Planes(o["dx"]), K.Planes(o["dxm"])),
                                              dxsum=o["s"]), specp,
             {"dx": dx64, "dxm": dx64 * keep, "dg": dg64, "db": db64, "s": (dx64 * keep).sum(0)}, t)
    dym = dy.double() * keep
    dx64, dg64, db64 = _ln_bwd_ref(dym, xhat.double(), rstd.double(), gamma.double())
    contract(lambda o: K.residual_ln_bwd_drop(dyd, xd, rd, gd, o["dg"], o["db"], drop, rows_per_seq, mask_dy=True, out=(o["dx"], None)),
             {"dg": Out((H,)), "db": Out((H,)), "dx": Out((rows, H))}, {"dx": dx64, "dg": dg64, "db": db64}, t)
    if rows == 80:
        refusals(lambda o: K.residual_ln_bwd_drop(dyd, xd, rd, gd, o["dg"], o["db"], drop, rows_per_seq, out=(o["dx"], o["dxm"])),
                 {"dg": Out((H,)), "db": Out((H,)), "dx": Out((rows, H)), "dxm": Out((rows, H))})


# ------------------------------------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("L,ragged", [(65, True), (100, False), (200, True), (512, True), (96, "empty"), (64, True)])
def test_attn_bwd(L, ragged):
    """cxrk_attn_bwd / _drop: the dS workspace of the tiled form (L > 64; L = 64 asks for none), ragged and padding-only masks as in
    test_attention_fwd_bwd.  The probabilities (and, with dropout, the keep mask) are inputs of the reference.  Bound 5e-5."""
    B, nH, dH = 3, 4, (64 if L != 100 else 32)
    qkv = rnd(B * L, 3 * nH * dH, scale=0.7)
    mask = torch.ones(B, L, dtype=torch.int64)
    if ragged:
        for i in range(B):
            mask[i, max(1, L - 3 * i - 2):] = 0
    if ragged == "empty":
        mask[1] = 0
    gc = rnd(B * L, nH * dH, seed=2)
    qd, gd = dev(qkv), dev(gc)
    _, probs = K.attn_fwd(qd, dev(mask), B, L, nH, dH)
    P = probs.cpu().double()
    q, k, v = qkv.double().view(B, L, 3, nH, dH).permute(2, 0, 3, 1, 4)
    dO = gc.double().view(B, L, nH, dH).permute(0, 2, 1, 3)

    def ref(keep):
        Pd = P * keep
        dV = Pd.transpose(-1, -2) @ dO
        dP = (dO @ v.transpose(-1, -2)) * keep
        dS = P * (dP - (dP * P).sum(-1, keepdim=True)) / math.sqrt(dH)
        return torch.stack([dS @ k, dS.transpose(-1, -2) @ q, dV]).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * nH * dH)

    W3 = 3 * nH * dH
    contract(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=o["dqkv"]), {"dqkv": Out((B * L, W3))}, {"dqkv": ref(1.0)}, tl(5e-5))
    drop = K.Drop(seed=77, counter=2, layer=0, site=K.DROP_ATTN_PROBS, row_offset=1, p=0.1)
    keep = K.dropout_mask(drop, B, L, L, nH=nH).cpu().double() / 0.9
    contract(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, drop=drop, out=K.Planes(o["dqkv"])), {"dqkv": Out((2, B * L, W3), BF)},
             {"dqkv": ref(keep)}, tl(5e-5))
    if L == 100:
        refusals(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=o["dqkv"]), {"dqkv": Out((B * L, W3))})
        refusals(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, drop=drop, out=o["dqkv"]), {"dqkv": Out((B * L, W3))})


# ------------------------------------------------------------------------------------------------ embedding scatter
@pytest.mark.parametrize("H", [64, 72])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 4099])
@pytest.mark.parametrize("ids_kind", ["one", "distinct", "mixed"])
def test_embed_bwd(T, H, ids_kind):
    """cxrk_embed_bwd: five regions and the radix sort's temporary storage carved out of one pointer; 32 sorted entries per chunk.
    All tokens one id (one run over every chunk), all ids distinct (every run interior or boundary of length one), a real mix;
    accumulation into a non-zero table.  Bound 2e-5 (test_embed_ln_and_scatter)."""
    V = T + 3
    g = torch.Generator().manual_seed(T + H)
    if ids_kind == "one":
        ids = torch.full((T,), 2, dtype=torch.int64)
    elif ids_kind == "distinct":
        ids = torch.randperm(V, generator=g)[:T]
    else:
        ids = torch.randint(0, V, (T,), generator=g)
        ids[torch.rand(T, generator=g) < 0.55] = 0
        ids[::32] = 1
        ids[-7:] = V - 1
    dx, base = rnd(T, H, seed=1), rnd(V, H, seed=2)
    idd, dxd = dev(ids), dev(dx)
    ref = base.double().index_add_(0, ids, dx.double())
    contract(lambda o: K.embed_bwd(idd, dxd, o["dword"]), {"dword": Out((V, H), init=base)}, {"dword": ref}, tl(2e-5))
    if (T, H, ids_kind) == (33, 72, "mixed"):
        refusals(lambda o: K.embed_bwd(idd, dxd, o["dword"]), {"dword": Out((V, H))})


# ------------------------------------------------------------------------------------------------ cosine heads, BCE, weight reset
COS = [(1, 1, 64), (7, 10, 100), (64, 32, 128), (65, 33, 128), (33000, 10, 64), (70, 100, 128), (9, 33, 512)]


@pytest.mark.parametrize("B,P,D", COS)
def test_pairwise_cosine_bwd(B, P, D):
    """cxrk_pairwise_cosine_bwd / _max_bwd: 64 rows per block up to 512 blocks (33 000 rows), the prompts walked in chunks of pc_max =
    16 KiB / (4 D) (32 at D = 128: P = 32, 33, 100 sit on and across the boundary; 8 at D = 512), every chunk's partials in the same
    workspace.  need_dx=False, accumulate_dy.  cos / norms / winners are the forward kernel's outputs (inputs here).  Bound 2e-5."""
    x, y, dcos = rnd(B, D), rnd(P, D, seed=1), rnd(B, P, seed=2)
    xd, yd, dcd = dev(x), dev(y), dev(dcos)
    cosv, xn, yn = K.pairwise_cosine_fwd(xd, yd)
    x64, y64 = x.double(), y.double()
    nx, ny = x64.norm(dim=1, keepdim=True), y64.norm(dim=1, keepdim=True)
    xh, yh = x64 / nx, y64 / ny
    c64 = xh @ yh.T

    def ref(d):
        return (d @ yh - (d * c64).sum(1, keepdim=True) * xh) / nx, (d.T @ xh - (d * c64).sum(0)[:, None] * yh) / ny

    t = tl(2e-5)
    dx64, dy64 = ref(dcos.double())
    base = rnd(P, D, seed=3)
    contract(lambda o: K.pairwise_cosine_bwd(xd, yd, cosv, dcd, xn, yn, out=(o["dx"], o["dy"])), {"dx": Out((B, D)), "dy": Out((P, D))},
             {"dx": dx64, "dy": dy64}, t)
    contract(lambda o: K.pairwise_cosine_bwd(xd, yd, cosv, dcd, xn, yn, need_dx=False, out=(None, o["dy"]), accumulate_dy=True),
             {"dy": Out((P, D), init=base)}, {"dy": base.double() + dy64}, t)
    for G in sorted({1, P} | ({5} if P % 5 == 0 else set())):
        Pg = P // G
        _, _, _, _, _, arg = K.pairwise_cosine_max_fwd(xd, yd, G)
        dmax = rnd(B, G, seed=4)
        d = torch.zeros(B, G, Pg, dtype=torch.float64)
        d.scatter_(2, arg.cpu().long().unsqueeze(-1), dmax.double().unsqueeze(-1))
        dx64, dy64 = ref(d.view(B, P))
        dmd = dev(dmax)
        contract(lambda o: K.pairwise_cosine_max_bwd(xd, yd, cosv, dmd, arg, xn, yn, out=(o["dx"], o["dy"])),
                 {"dx": Out((B, D)), "dy": Out((P, D))}, {"dx": dx64, "dy": dy64}, t)
    if (B, P) == (7, 10):
        refusals(lambda o: K.pairwise_cosine_bwd(xd, yd, cosv, dcd, xn, yn, out=(o["dx"], o["dy"])), {"dx": Out((B, D)), "dy": Out((P, D))})
        refusals(lambda o: K.pairwise_cosine_max_bwd(xd, yd, cosv, dmd, arg, xn, yn, out=(o["dx"], o["dy"])), {"dx": Out((B, D)), "dy": Out((P, D))})


@pytest.mark.parametrize("diff", [True, False])
@pytest.mark.parametrize("B,C", [(1, 1), (51, 5), (257, 1), (14000, 5)])
def test_bce_posneg(B, C, diff):
    """cxrk_bce_posneg_fwd_bwd: B C = 1, 255, 257, 70 000 (256 elements per block, at most 256 blocks), labels as a column view of a
    wider tensor.  logits / dcos: 2e-5.  The scalar loss: |loss - ref| < 1e-6 absolute as in test_pairwise_cosine_bce_eval up to 257
    elements; at 70 000 a sequential float32 mean is already 2.9e-6 off float64, so there 2e-5 relative (a lost block: 4e-3)."""
    g = torch.Generator().manual_seed(B + C)
    cosv = torch.tanh(torch.randn(B, 2 * C, generator=g))
    lab_wide = (torch.rand(B, C + 3, generator=g) > 0.5).float()
    labels = lab_wide[:, :C]
    c64 = cosv.double().requires_grad_(True)
    logits = c64[:, 0::2] - c64[:, 1::2] if diff else c64[:, 0::2]
    loss = F.binary_cross_entropy_with_logits(logits, labels.double())
    loss.backward()
    cd, ld = dev(cosv), dev(lab_wide)[:, :C]
    o = contract(lambda o: K.bce_posneg_fwd_bwd(cd, ld, diff=diff, out=(o["logits"], o["dcos"], o["loss"])),
                 {"logits": Out((B, C)), "dcos": Out((B, 2 * C)), "loss": Out(())},
                 {"logits": logits.detach(), "dcos": c64.grad, "loss": loss.detach()}, tl(2e-5))
    if B * C <= 257:
        assert abs(float(o["loss"].t) - float(loss.detach())) < 1e-6
    if (B, C, diff) == (51, 5, True):
        refusals(lambda o: K.bce_posneg_fwd_bwd(cd, ld, out=(o["logits"], o["dcos"], o["loss"])),
                 {"logits": Out((B, C)), "dcos": Out((B, 2 * C)), "loss": Out(())})


@pytest.mark.parametrize("n", [1, 255, 257, 65537, (1 << 20) + 3])
def test_weight_reset(n):
    """cxrk_weight_reset: per-block min / max partials (256 elements per block, at most 256 blocks) combined with fminf / fmaxf --
    which swallow a NaN, hence the +-1e30 poison.  In place on pnew; the counter accumulates over two calls.  Exact."""
    from oracle import ref_step
    new, old = rnd(n, seed=7), rnd(n, seed=8)
    if n > 4:
        new[:n // 3] = old[:n // 3] + 1e-4 * rnd(n // 3, seed=9)
    ref, cnt = ref_step.weight_reset(new, old, 0.3)
    oldd = dev(old)
    counts = []

    def call(o):
        K.weight_reset(o["p"], oldd, 0.3, o["cnt"])
        c1 = int(o["cnt"][0])
        K.weight_reset(o["p"], oldd, 0.3, o["cnt"])      # restored entries now have |diff| = 0 -> min 0, a threshold no larger than the
                                                         # first: exactly the same entries are counted again
        counts.append((c1, int(o["cnt"][0])))

    o = contract(call, {"p": Out((n,), init=new), "cnt": Out((2,), torch.int64, init=torch.tensor([5, 0]))})
    assert all(c == (5 + cnt, 5 + 2 * cnt) for c in counts), (counts, cnt)
    first = MG.Guarded((n,), device=DEV).load(new)
    K.weight_reset(first.t, oldd, 0.3, torch.zeros(2, dtype=torch.int64, device=DEV))
    first.check()
    assert torch.equal(first.t.cpu(), ref)
    if n == 257:
        refusals(lambda o: K.weight_reset(o["p"], oldd, 0.3, o["cnt"]), {"p": Out((n,)), "cnt": Out((2,), torch.int64)})


# ================================================================================================ guarded outputs, no workspace
# Entry points without scratch memory but with ragged-tail stores: sizes that are not multiples of the kernel's vector width / tile.
def guarded(call, outs, ref=None, tol=None):
    """two runs over the two byte sentinels (integer outputs: identical payloads = fully written); guards, padding, values"""
    return MG.run_contract(call, outs, ref, tol, module=K, device=DEV, runs=("session", "nan"))


def cabi(name, *args):
    """a direct C-ABI call on the current stream (wrappers that allocate their outputs themselves)"""
    _cxr_lib.check(getattr(_cxr_lib.load(), name)(*args, K._stream()), name)


def P(t):
    return None if t is None else (t.ptr() if isinstance(t, K.Planes) else t.data_ptr())


def _conv_ref(x64, w64, stride, pad):
    """NHWC float64 forward convolution, w [Ko, R, R, C]"""
    return F.conv2d(x64.permute(0, 3, 1, 2), w64.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("cfg", [(3, 9, 9, 128, 128, 3, 1, 1), (2, 15, 15, 64, 128, 3, 2, 1), (5, 7, 58, 64, 64, 3, 1, 1), (1, 3, 5, 64, 64, 3, 1, 1),
                                 (2, 14, 14, 64, 256, 1, 1, 0), (3, 13, 13, 128, 256, 1, 2, 0)])
def test_conv_fwd_outputs(cfg, wide):
    """conv + shift + residual + ReLU: planes output with the decision bits, and fp32.  relu is 1-Lipschitz, so the float64 reference
    needs no decisions; the bits must be those of the stored values.  Bounds 2e-4 planes / 2e-5 fp32 (the conv tests)."""
    N, H, W, C, Ko, R, stride, pad = cfg
    x, w, shift = rnd(N, H, W, C), _filters(Ko, R, C), rnd(Ko, seed=2)
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    res = rnd(N, Ho, Wo, Ko, seed=3)
    shd = dev(shift)
    tail = (N, H, W, C, Ko, R, R, stride, pad, True)
    (xp, x64), (wp, w64), (rp, r64) = pl(x), pl(w.reshape(Ko, -1)), pl(res)
    ref = torch.relu(_conv_ref(x64, w64.view(Ko, R, R, C), stride, pad) + shift.double() + r64)
    o = guarded(lambda o: K.conv_fwd_pl(xp, wp, shd, rp, K.Planes(o["y"]), o["mask"], *tail),
                {"y": Out((2, N, Ho, Wo, Ko), BF), "mask": Out((N * Ho * Wo, Ko // 8), U8)}, {"y": ref}, tl(2e-4))
    assert bool((K.unpack_mask(o["mask"].t, Ko) == (o["y"].value().view(-1, Ko) > 0)).all())
    if wide == "policy":
        xd, wd, rd = dev(x), dev(w), dev(res)
        ref = torch.relu(_conv_ref(x.double(), w.double(), stride, pad) + shift.double() + res.double())
        guarded(lambda o: K.conv_fwd(xd, wd, shd, rd, o["y"], *tail), {"y": Out((N, Ho, Wo, Ko))}, {"y": ref}, tl(2e-5))


def test_stem_conv_fwd_outputs():
    """the 7x7 / stride-2 stem: 3 real channels padded to 4, fp32 input, fp32 and planes output"""
    N, H, Ko = 2, 30, 64
    x = torch.zeros(N, H, H, 4)
    x[..., :3] = rnd(N, H, H, 3)
    w = torch.zeros(Ko, 7, 7, 4)
    w[..., :3] = _filters(Ko, 7, 3)
    shift = rnd(Ko, seed=2)
    xd, wd, shd = dev(x), dev(w), dev(shift)
    ref = torch.relu(_conv_ref(x.double(), w.double(), 2, 3) + shift.double())
    tail = (N, H, H, 4, Ko, 7, 7, 2, 3, True)
    guarded(lambda o: K.conv_fwd(xd, wd, shd, None, o["y"], *tail), {"y": Out((N, 15, 15, Ko))}, {"y": ref}, tl(2e-5))
    guarded(lambda o: K.conv_fwd_pl(xd, wd, shd, None, K.Planes(o["y"]), None, *tail), {"y": Out((2, N, 15, 15, Ko), BF)}, {"y": ref}, tl(2e-4))


@pytest.mark.parametrize("cfg", [(2, 14, 14, 256, 512, 1, 2, 0), (3, 13, 13, 128, 256, 1, 2, 0), (1, 3, 5, 64, 64, 3, 1, 1), (2, 15, 15, 64, 128, 3, 2, 1)])
def test_conv_bwd_data_outputs(cfg, wide):
    """data gradients without the fused sums, incl. the 1x1 / stride-2 form (three parity classes zero-filled, one computed) and its
    compact variant.  Bounds 3e-4 planes / 5e-5 fp32."""
    N, H, W, C, Ko, R, stride, pad = cfg
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    dy, w = rnd(N, Ho, Wo, Ko, seed=2), _filters(Ko, R, C)
    args = (N, H, W, C, Ko, R, R, stride, pad)
    (dyp, dy64), (wp, w64) = pl(dy), pl(w.reshape(Ko, -1))
    g64 = _dgrad_ref(dy64, w64.view(Ko, R, R, C), N, H, W, C, R, stride, pad)
    guarded(lambda o: K.conv_bwd_data_pl(dyp, wp, None, None, K.Planes(o["dx"]), *args), {"dx": Out((2, N, H, W, C), BF)}, {"dx": g64}, tl(3e-4))
    if R == 1 and stride == 2:
        guarded(lambda o: K.linear_bwd_data_pl(dyp.view(N * Ho * Wo, Ko), wp, out=K.Planes(o["dx"])), {"dx": Out((2, N * Ho * Wo, C), BF)},
                {"dx": g64[:, ::2, ::2].reshape(-1, C)}, tl(3e-4))
    if wide == "policy":
        dyd, wd = dev(dy), dev(w)
        g64 = _dgrad_ref(dy.double(), w.double(), N, H, W, C, R, stride, pad)
        guarded(lambda o: K.conv_bwd_data(dyd, wd, None, None, o["dx"], *args), {"dx": Out((N, H, W, C))}, {"dx": g64}, tl(5e-5))


@pytest.mark.parametrize("M,N", [(200, 192), (65, 64), (1000, 320)])
def test_linear_pl_side_outputs(M, N, wide):
    """planes linear layer with the ReLU decision bits (`maskout`) and with the pre-activation copy (`preact_out`); bound 2e-4"""
    Kd = 72
    x, w, b = rnd(M, Kd, scale=0.5), rnd(N, Kd, seed=1, scale=0.5), rnd(N, seed=2)
    (xp, x64), (wp, w64) = pl(x), pl(w)
    bd = dev(b)
    pre = x64 @ w64.T + b.double()
    o = guarded(lambda o: K.linear_fwd_pl(xp, wp, bias=bd, act=K.ACT_RELU, out=K.Planes(o["y"]), maskout=o["mask"]),
                {"y": Out((2, M, N), BF), "mask": Out((M, N // 8), U8)}, {"y": torch.relu(pre)}, tl(2e-4))
    assert bool((K.unpack_mask(o["mask"].t, N) == (o["y"].value() > 0)).all())
    guarded(lambda o: K.linear_fwd_pl(xp, wp, bias=bd, act=K.ACT_GELU, out=o["y"], preact_out=o["pre"]),
            {"y": Out((M, N), ld=N + 8), "pre": Out((M, N))}, {"y": F.gelu(pre), "pre": pre}, tl(2e-4))


def test_split_merge_planes_outputs():
    x = rnd(37, 8)
    xd = dev(x)
    o = guarded(lambda o: K.split_planes(xd, out=K.Planes(o["p"])), {"p": Out((2, 37, 8), BF, gap=8)}, {"p": x.double()}, 2e-5)
    assert torch.equal(o["p"].t[0].float().cpu(), x.bfloat16().float())
    p, seen = pl(x)
    guarded(lambda o: cabi("cxrk_merge_planes", p.ptr(), p.plane, p.numel(), P(o["x"])), {"x": Out((37, 8))}, {"x": seen}, 1e-7)


@pytest.mark.parametrize("planes", [False, True])
def test_bn_apply_and_dz_outputs(planes):
    """cxrk_bn_apply (+ residual, ReLU bits) and cxrk_bn_train_dz, 8 channels per thread over 77 x 72; bounds 3e-5 / 1e-4
    (test_train_mode_batchnorm_kernels)"""
    rows, C = 77, 72
    z, res, dy = rnd(rows, C), rnd(rows, C, seed=1), rnd(rows, C, seed=2)
    sc, sh, A, B, Cc = (dev(rnd(C, seed=s)) for s in range(3, 8))
    wrap = pl if planes else (lambda t: (dev(t), t.double()))
    (zd, z64), (rd, r64), (dyd, dy64) = wrap(z), wrap(res), wrap(dy)
    spec = (lambda: Out((2, rows, C), BF)) if planes else (lambda: Out((rows, C)))
    pln = (lambda t: K.Planes(t)) if planes else (lambda t: t)
    plane = rows * C if planes else 0
    ref = torch.relu(z64 * sc.cpu().double() + sh.cpu().double() + r64)
    o = guarded(lambda o: cabi("cxrk_bn_apply", P(zd), plane, P(sc), P(sh), P(rd), plane, P(pln(o["y"])), plane, P(o["mask"]), rows, C, 1),
                {"y": spec(), "mask": Out((rows, C // 8), U8)}, {"y": ref}, tl(3e-5))
    assert bool((K.unpack_mask(o["mask"].t, C) == (o["y"].value() > 0)).all())
    ref = A.cpu().double() * dy64 + B.cpu().double() + Cc.cpu().double() * z64
    guarded(lambda o: cabi("cxrk_bn_train_dz", P(dyd), plane, P(zd), plane, P(A), P(B), P(Cc), P(pln(o["dz"])), plane, rows, C), {"dz": spec()},
            {"dz": ref}, tl(1e-4))


def test_maxpool_outputs():
    """3x3 / stride-2 max-pool on 13 x 11 (ragged last window), forward values exact, winners shown written by the two-sentinel rule
    and used by the backward; fp32 (C = 12: three float4 per pixel) and planes (C = 24)"""
    N, H, W = 2, 13, 11
    Ho, Wo = 7, 6
    for planes, C in ((False, 12), (True, 24)):
        x = rnd(N, H, W, C)
        dy = rnd(N, Ho, Wo, C, seed=1)
        if planes:
            (xd, x64), (dyd, dy64) = pl(x), pl(dy)
        else:
            xd, x64, dyd, dy64 = dev(x), x.double(), dev(dy), dy.double()
        xa = x64.permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.max_pool2d(xa, 3, 2, 1)
        y.backward(dy64.permute(0, 3, 1, 2))
        yref, gref = y.detach().permute(0, 2, 3, 1), xa.grad.permute(0, 2, 3, 1)
        if planes:
            o = guarded(lambda o: cabi("cxrk_maxpool_fwd_pl", xd.ptr(), xd.plane, P(o["y"]), N * Ho * Wo * C, P(o["idx"]), N, H, W, C),
                        {"y": Out((2, N, Ho, Wo, C), BF), "idx": Out((N, Ho, Wo, C), U8)}, {"y": yref}, 1e-7)
            pooled, idx = K.Planes(o["y"].t), o["idx"].t
            guarded(lambda o: cabi("cxrk_maxpool_bwd_pl", dyd.ptr(), dyd.plane, P(idx), pooled.ptr(), P(o["dx"]), N, H, W, C), {"dx": Out((N, H, W, C))},
                    {"dx": gref * (x64 > 0)}, tl(2e-5))
        else:
            o = guarded(lambda o: cabi("cxrk_maxpool_fwd", P(xd), P(o["y"]), P(o["idx"]), N, H, W, C),
                        {"y": Out((N, Ho, Wo, C)), "idx": Out((N, Ho, Wo, C), U8)}, {"y": yref}, 1e-7)
            idx = o["idx"].t
            guarded(lambda o: cabi("cxrk_maxpool_bwd", P(dyd), P(idx), P(xd), P(o["dx"]), N, H, W, C, 0), {"dx": Out((N, H, W, C))}, {"dx": gref},
                    tl(2e-5))


def test_spatial_mean_and_layout_outputs():
    N, Pn, C = 3, 49, 136
    x, g, add = rnd(N, Pn, C), rnd(N, C, seed=1), rnd(N, Pn, C, seed=2)
    xd, gd, addd = dev(x), dev(g), dev(add)
    guarded(lambda o: cabi("cxrk_spatial_mean_fwd", P(xd), P(o["y"]), N, Pn, C), {"y": Out((N, C))}, {"y": x.double().mean(1)}, tl(2e-5))
    bref = (g.double() / Pn)[:, None, :].expand(N, Pn, C)
    guarded(lambda o: cabi("cxrk_spatial_mean_bwd", P(gd), P(o["dx"]), N, Pn, C), {"dx": Out((N, Pn, C))}, {"dx": bref}, tl(2e-5))
    guarded(lambda o: cabi("cxrk_spatial_mean_bwd_pl", P(gd), P(addd), P(o["dx"]), N * Pn * C, N, Pn, C), {"dx": Out((2, N, Pn, C), BF)},
            {"dx": bref + add.double()}, tl(2e-5))
    img = rnd(2, 3, 5, 7)
    imd = dev(img)
    ref = torch.zeros(2, 5, 7, 4, dtype=torch.float64)
    ref[..., :3] = img.double().permute(0, 2, 3, 1)
    guarded(lambda o: cabi("cxrk_nchw_to_nhwc", P(imd), P(o["y"]), 2, 3, 5, 7, 4), {"y": Out((2, 5, 7, 4))}, {"y": ref}, 1e-7)
    t = rnd(2, 5, 7, 12)
    td = dev(t)
    guarded(lambda o: cabi("cxrk_nhwc_to_nchw", P(td), P(o["y"]), 2, 12, 5, 7), {"y": Out((2, 12, 5, 7))}, {"y": t.double().permute(0, 3, 1, 2)}, 1e-7)


@pytest.mark.parametrize("H", [72, 768])
def test_layernorm_fwd_outputs(H):
    """embed_ln_fwd / residual_ln_fwd and their dropout forms (keep mask = dropout_ref's numpy restatement); bound 2e-5"""
    import dropout_ref as DR
    B, L, V = 3, 7, 50
    T = B * L
    word, pos, typ = rnd(V, H), rnd(16, H, seed=1), rnd(H, seed=2)
    gam, bet = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(5))
    e = word.double()[ids] + pos.double()[:L][None] + typ.double()
    mu, var = e.mean(-1, keepdim=True), e.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-12)
    xhat = (e - mu) * rstd
    y = xhat * gam.double() + bet.double()
    idd, wd, pd, td, gd, bd = dev(ids), dev(word), dev(pos), dev(typ), dev(gam), dev(bet)
    spec = {"y": Out((T, H)), "xhat": Out((T, H)), "rstd": Out((T,))}
    refs = {"y": y.view(T, H), "xhat": xhat.view(T, H), "rstd": rstd.view(T)}
    guarded(lambda o: cabi("cxrk_embed_ln_fwd", P(idd), P(wd), P(pd), P(td), P(gd), P(bd), 1e-12, T, L, H, P(o["y"]), 0, P(o["xhat"]), P(o["rstd"])),
            spec, refs, tl(2e-5))
    drop = K.Drop(seed=99, counter=3, layer=0, site=K.DROP_EMBED, row_offset=2, p=0.2)
    keep = DR.factors(DR.keep_mask(*drop[:5], 0.2, B, L, H), 0.2).double().view(T, H)
    specp = dict(spec, y=Out((2, T, H), BF))
    guarded(lambda o: cabi("cxrk_embed_ln_fwd_drop", P(idd), P(wd), P(pd), P(td), P(gd), P(bd), 1e-12, T, L, H, P(o["y"]), T * H, P(o["xhat"]),
                           P(o["rstd"]), *drop.args()), specp, dict(refs, y=y.view(T, H) * keep), tl(2e-5))
    # residual LayerNorm
    x, res = rnd(T, H, seed=6), rnd(T, H, seed=7)
    xd, rd = dev(x), dev(res)

    def ln(s):
        mu, var = s.mean(-1, keepdim=True), s.var(-1, unbiased=False, keepdim=True)
        r = 1 / torch.sqrt(var + 1e-12)
        return {"y": (s - mu) * r * gam.double() + bet.double(), "xhat": (s - mu) * r, "rstd": r.view(-1)}

    guarded(lambda o: cabi("cxrk_residual_ln_fwd", P(xd), P(rd), P(gd), P(bd), 1e-12, T, H, P(o["y"]), T * H, P(o["xhat"]), P(o["rstd"])), specp,
            ln(x.double() + res.double()), tl(2e-5))
    drop = K.Drop(seed=99, counter=3, layer=1, site=K.DROP_FFN_OUT, row_offset=0, p=0.2)
    keep = DR.factors(DR.keep_mask(*drop[:5], 0.2, B, L, H), 0.2).double().view(T, H)
    guarded(lambda o: cabi("cxrk_residual_ln_fwd_drop", P(xd), P(rd), 0, H, P(gd), P(bd), 1e-12, T, H, L, P(o["y"]), 0, P(o["xhat"]), P(o["rstd"]),
                           *drop.args()), spec, ln(x.double() * keep + res.double()), tl(2e-5))


@pytest.mark.parametrize("L", [17, 100])
def test_attn_fwd_and_dropout_mask_outputs(L):
    """attention forward (context + saved probabilities; with dropout the probabilities stay undropped) and the keep-mask generator at a
    column count that is not a multiple of its four columns per thread (L = 17); bound 2e-5"""
    import dropout_ref as DR
    B, nH, dH = 3, 4, 32
    qkv = rnd(B * L, 3 * nH * dH, scale=0.7)
    mask = torch.ones(B, L, dtype=torch.int64)
    for i in range(B):
        mask[i, max(1, L - 3 * i - 2):] = 0
    q, k, v = qkv.double().view(B, L, 3, nH, dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(dH) + (1.0 - mask[:, None, None, :].double()) * torch.finfo(torch.float32).min
    Pr = torch.softmax(s, -1)
    qd, md = dev(qkv), dev(mask)
    spec = {"ctx": Out((B * L, nH * dH)), "probs": Out((B, nH, L, L))}
    guarded(lambda o: cabi("cxrk_attn_fwd", P(qd), P(md), B, L, nH, dH, P(o["ctx"]), 0, P(o["probs"])), spec,
            {"ctx": (Pr @ v).transpose(1, 2).reshape(B * L, nH * dH), "probs": Pr}, tl(2e-5))
    drop = K.Drop(seed=5, counter=9, layer=2, site=K.DROP_ATTN_PROBS, row_offset=4, p=0.1)
    km = DR.keep_mask(*drop[:5], 0.1, B, L, L, nH)
    keep = DR.factors(km, 0.1).double()
    guarded(lambda o: cabi("cxrk_attn_fwd_drop", P(qd), P(md), B, L, nH, dH, P(o["ctx"]), B * L * nH * dH, P(o["probs"]), *drop.args()),
            dict(spec, ctx=Out((2, B * L, nH * dH), BF)), {"ctx": ((Pr * keep) @ v).transpose(1, 2).reshape(B * L, nH * dH), "probs": Pr}, tl(2e-5))
    o = guarded(lambda o: cabi("cxrk_dropout_mask", *drop.args(), B, L, nH, L, P(o["keep"])), {"keep": Out((B, nH, L, L), U8)})
    assert torch.equal(o["keep"].t.cpu().bool(), torch.from_numpy(km))


def test_rowwise_small_outputs():
    """planes_add_rows (row-strided destination), gelu_bwd (n not a multiple of anything), scale_mask with a device scalar"""
    rows, cols = 5, 72
    src, dst = rnd(rows, cols), rnd(rows, 3 * cols, seed=1)
    sp, seen = pl(src)
    ref = dst.double().clone()
    ref[:, :cols] += seen
    o = guarded(lambda o: K.planes_add_rows(sp, o["dst"][:, :cols]), {"dst": Out((rows, 3 * cols), init=dst)}, {"dst": ref}, tl(2e-5))
    n = 1027
    dy, pre = rnd(n), rnd(n, seed=1)
    a = pre.double().clone().requires_grad_(True)
    F.gelu(a).backward(dy.double())
    dyd, pred = dev(dy), dev(pre)
    guarded(lambda o: cabi("cxrk_gelu_bwd", P(dyd), P(pred), n, P(o["dx"])), {"dx": Out((n,))}, {"dx": a.grad}, tl(2e-5))
    msrc, alpha = rnd(n, seed=2), torch.tensor(-1.75)
    md, ad = dev(msrc), dev(alpha)
    guarded(lambda o: K.scale_mask(dyd, md, ad, 0.5, out=o["y"]), {"y": Out((n,))}, {"y": 0.5 * -1.75 * dy.double() * (msrc > 0)}, tl(2e-5))


def test_l2norm_infonce_outputs():
    """l2norm_fwd into one half of a [B, 2 D] send buffer (the other half must stay untouched), l2norm_bwd from it; row_lse with a
    diagonal offset on a pitched block with fewer rows than columns, the loss fresh and accumulated; grad_inplace on the same.  2e-5."""
    B, D = 7, 100
    x, d = rnd(B, D), rnd(B, D, seed=1)
    xd, dd = dev(x), dev(d)
    other = rnd(B, D, seed=2)
    x64 = x.double()
    nrm = x64.norm(dim=1, keepdim=True)
    for half in (0, 1):
        buf = torch.zeros(B, 2 * D)
        buf[:, (1 - half) * D:(2 - half) * D] = other
        ref = buf.double().clone()
        ref[:, half * D:(half + 1) * D] = x64 / nrm
        o = guarded(lambda o: cabi("cxrk_l2norm_fwd", P(xd), B, D, 1e-12, o["buf"][:, half * D:].data_ptr(), 2 * D, P(o["norm"])),
                    {"buf": Out((B, 2 * D), init=buf), "norm": Out((B,))}, {"buf": ref, "norm": nrm.view(-1)}, tl(2e-5))
        assert torch.equal(o["buf"].t[:, (1 - half) * D:(2 - half) * D].cpu(), other), "the other half of the send buffer was touched"
    xh = MG.Guarded((B, 2 * D), device=DEV).load(torch.cat([other, (x64 / nrm).float()], 1))
    xa = x64.clone().requires_grad_(True)
    F.normalize(xa, dim=1).backward(d.double())
    nd = dev(nrm.view(-1).float())
    guarded(lambda o: cabi("cxrk_l2norm_bwd", P(dd), xh.t[:, D:].data_ptr(), 2 * D, P(nd), B, D, P(o["dx"])), {"dx": Out((B, D))}, {"dx": xa.grad}, tl(2e-5))
    xh.check()
    rows, cols, off, ld = 5, 13, 6, 16
    S = rnd(rows, cols, scale=3.0)
    Sg = MG.Guarded((rows, cols), ld=ld, device=DEV).load(S)
    S64 = S.double()
    lse = torch.logsumexp(S64, 1)
    diag = S64[torch.arange(rows), off + torch.arange(rows)]
    lval = 0.25 * (lse - diag).sum()
    spec = {"lse": Out((rows,)), "diag": Out((rows,))}
    guarded(lambda o: cabi("cxrk_infonce_row_lse", P(Sg.t), ld, rows, cols, off, P(o["lse"]), P(o["diag"]), P(o["loss"]), 0.25, 0),
            dict(spec, loss=Out(())), {"lse": lse, "diag": diag, "loss": lval}, tl(2e-5))
    guarded(lambda o: cabi("cxrk_infonce_row_lse", P(Sg.t), ld, rows, cols, off, P(o["lse"]), P(o["diag"]), P(o["loss"]), 0.25, 1),
            dict(spec, loss=Out((), init=torch.tensor(2.5))), {"lse": lse, "diag": diag, "loss": 2.5 + lval}, tl(2e-5))
    Sg.check()
    lse_col = rnd(cols, seed=3).double() + 4
    lr, lc = dev(lse.float()), dev(lse_col.float())
    gref = torch.exp(S64 - lr.cpu().double()[:, None]) + torch.exp(S64 - lc.cpu().double()[None, :])
    gref[torch.arange(rows), off + torch.arange(rows)] -= 2
    guarded(lambda o: cabi("cxrk_infonce_grad_inplace", P(o["S"]), ld, rows, cols, off, P(lr), P(lc)), {"S": Out((rows, cols), ld=ld, init=S)},
            {"S": gref}, tl(2e-5))


def test_cosine_heads_outputs():
    """pairwise_cosine_fwd / _max_fwd (B not a multiple of the 4 rows per block; argmax int32 by the two-sentinel rule), patch_similarity,
    eval_score (both pred_diff), group_mean; bound 2e-5"""
    B, G, Pg, D = 7, 3, 5, 100
    Pn = G * Pg
    x, y = rnd(B, D), rnd(Pn, D, seed=1)
    xd, yd = dev(x), dev(y)
    x64, y64 = x.double(), y.double()
    nx, ny = x64.norm(dim=1), y64.norm(dim=1)
    c64 = (x64 / nx[:, None]) @ (y64 / ny[:, None]).T
    spec = {"cos": Out((B, Pn)), "xn": Out((B,)), "yn": Out((Pn,))}
    refs = {"cos": c64, "xn": nx, "yn": ny}
    guarded(lambda o: cabi("cxrk_pairwise_cosine_fwd", P(xd), P(yd), B, Pn, D, P(o["cos"]), P(o["xn"]), P(o["yn"])), spec, refs, tl(2e-5))
    grp = c64.view(B, G, Pg)
    o = guarded(lambda o: cabi("cxrk_pairwise_cosine_max_fwd", P(xd), P(yd), B, G, Pg, D, P(o["cos"]), P(o["xn"]), P(o["yn"]), P(o["max"]),
                               P(o["mean"]), P(o["arg"])), dict(spec, max=Out((B, G)), mean=Out((B, G)), arg=Out((B, G), I32)),
                dict(refs, max=grp.max(2).values, mean=grp.mean(2)), tl(2e-5))
    assert torch.equal(o["arg"].t.cpu().long(), grp.max(2).indices)
    R = 13
    pat, txt = rnd(R, D, seed=2), rnd(D, seed=3)
    pd, td = dev(pat), dev(txt)
    guarded(lambda o: cabi("cxrk_patch_similarity", P(pd), P(td), R, D, P(o["sim"])), {"sim": Out((R,))}, {"sim": pat.double() @ txt.double()}, tl(2e-5))
    C = 5
    cosv = torch.tanh(rnd(B, 2 * C, seed=4))
    cd = dev(cosv)
    c = cosv.double()
    for pred_diff in (0, 1):
        o = guarded(lambda o: cabi("cxrk_eval_score", P(cd), B, C, pred_diff, P(o["score"]), P(o["pred"])), {"score": Out((B, C)), "pred": Out((B, C))})
        sc, pr = K.eval_score(cd, bool(pred_diff))        # the wrapper's own (unguarded) result: same kernel, same bits
        assert torch.equal(o["score"].t, sc) and torch.equal(o["pred"].t, pr)
    sc, pr = K.eval_score(cd)
    assert MG.rel_err(sc, (c[:, 0::2] + 1) / 2) < tl(2e-5) and torch.equal(pr.cpu(), (cosv[:, 0::2] > cosv[:, 1::2]).float())
    e, gm = rnd(G * Pg, D, seed=5), rnd(G, D, seed=6)
    ed, gd = dev(e), dev(gm)
    guarded(lambda o: cabi("cxrk_group_mean_fwd", P(ed), G, Pg, D, P(o["out"])), {"out": Out((G, D))}, {"out": e.double().view(G, Pg, D).mean(1)}, tl(2e-5))
    guarded(lambda o: cabi("cxrk_group_mean_bwd", P(gd), G, Pg, D, P(o["din"])), {"din": Out((G * Pg, D))},
            {"din": (gm.double() / Pg)[:, None].expand(G, Pg, D).reshape(G * Pg, D)}, tl(2e-5))


@pytest.mark.parametrize("n", [1, 3, 1027])
def test_optimiser_outputs(n):
    """adam_fused (float4 body + scalar tail) and sgd with every tensor ending 4 bytes before its back guard, weight decay and gradient
    scale away from their defaults; bound 1e-6 (test_adam_sgd_weight_reset)"""
    p0, g, m0, v0 = rnd(n), rnd(n, seed=1), 0.1 * rnd(n, seed=2), 0.01 * rnd(n, seed=3).abs()
    gd = MG.Guarded((n,), device=DEV).load(g)
    # the hyper-parameters as the kernel sees them (float32 arguments): 1 - float32(0.999) is 1.3e-5 off 0.001
    lr, b1, b2, eps, wd, gs = (float(np.float32(t)) for t in (1e-2, 0.9, 0.999, 1e-8, 0.05, 0.5))
    step = 3
    g64 = gs * g.double() + wd * p0.double()
    m = b1 * m0.double() + (1 - b1) * g64
    v = b2 * v0.double() + (1 - b2) * g64 * g64
    pref = p0.double() - lr * (m / (1 - b1 ** step)) / (torch.sqrt(v / (1 - b2 ** step)) + eps)
    guarded(lambda o: K.adam_fused(o["p"], gd.t, o["m"], o["v"], lr, b1, b2, eps, wd, step, gs),
            {"p": Out((n,), init=p0), "m": Out((n,), init=m0), "v": Out((n,), init=v0)}, {"p": pref, "m": m, "v": v}, 1e-6)
    guarded(lambda o: K.sgd(o["p"], gd.t, 0.1, wd, gs), {"p": Out((n,), init=p0)}, {"p": p0.double() - 0.1 * g64}, 1e-6)
    gd.check()


# ================================================================================================ model-level stale-memory independence
JUNK_SIZES = [1 << 26] * 8 + [n for n in (1 << 10, 1 << 14, 1 << 18, 1 << 22) for _ in range(16)]


def _poison_free_blocks():
    """NaN-fill then free a spread of allocator blocks: the next torch.empty() of a matching size class returns NaNs"""
    junk = [torch.full((n,), float("nan"), device=DEV) for n in JUNK_SIZES]
    del junk


def _three_ways(run):
    """run() -> {name: tensor}: as is; after dropping the workspace and poisoning the allocator's free blocks; with a 512 MiB workspace
    pre-filled with 1e6 plus the same junk.  Bit-identical and finite, or something read memory that nothing wrote."""
    results = []
    for mode in ("as is", "fresh workspace + NaN free blocks", "512 MiB workspace of 1e6 + NaN free blocks"):
        if mode != "as is":
            torch.cuda.synchronize()
            K._ws.bufs.clear()
            if mode.startswith("512"):
                K.workspace(1 << 29, torch.device("cuda", torch.cuda.current_device())).fill_(1.0e6)
            _poison_free_blocks()
        out = run()
        torch.cuda.synchronize()
        results.append((mode, {k: v.detach().clone() for k, v in out.items()}))
    K._ws.bufs.clear()
    base = results[0][1]
    for k, v in base.items():
        assert bool(torch.isfinite(v.float()).all()), f"{k}: not finite"
    for mode, r in results[1:]:
        assert r.keys() == base.keys()
        bad = [k for k in base if not torch.equal(base[k], r[k])]
        assert not bad, f"{len(bad)} of {len(base)} tensors differ between 'as is' and '{mode}': {bad[:8]}"


@pytest.mark.parametrize("train_bn", [False, True])
def test_image_model_is_independent_of_stale_memory(train_bn):
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    model = get_biovil_resnet(None)
    syn.fill_module_(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV)
    x = syn.synthetic_images(2, 224, seed=27).to(DEV)
    probe = torch.randn(2, 128, generator=torch.Generator().manual_seed(3)).to(DEV)

    def run():
        model.load_state_dict(sd0)                      # train mode moves the running statistics: start every pass from the same ones
        model.train() if train_bn else model.eval()
        model.zero_grad(set_to_none=True)
        emb = model(x)
        (emb * probe).sum().backward()
        out = {"emb": emb}
        out.update({"grad " + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        out.update({"state " + k: v for k, v in model.state_dict().items() if "running_" in k})
        return out

    _three_ways(run)


@pytest.mark.parametrize("dropout", [False, True])
def test_text_model_is_independent_of_stale_memory(dropout):
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    cfg = CXRBertConfig(vocab_size=128, hidden_size=64, num_attention_heads=4, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=64, projection_size=128)
    model = CXRBertModel(cfg)
    syn.fill_module_(model)
    model.to(DEV)
    ids, mask = syn.synthetic_tokens(5, 17, vocab=128, seed=11, ragged=True)
    ids, mask = ids.to(DEV), mask.to(DEV)
    probe = torch.randn(5, 128, generator=torch.Generator().manual_seed(4)).to(DEV)

    def run():
        if dropout:
            model.train()
            model.enable_dropout_(seed=1234)
            model.dropout_state = (1234, 7)             # the same (seed, counter) in every pass
        else:
            model.eval()
        model.zero_grad(set_to_none=True)
        proj = model.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
        (proj * probe).sum().backward()
        out = {"proj": proj}
        out.update({"grad " + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        return out

    _three_ways(run)


def test_joint_step_is_independent_of_stale_memory():
    """test_joint_step_vs_cpu_oracle's configuration: loss, every gradient and the parameters after the fused Adam step"""
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    B, L = 4, 16
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=32)
    images = syn.synthetic_images(B, 64, seed=3).to(DEV)
    ids, mask = syn.synthetic_tokens(B, L, vocab=300, seed=4, ragged=True)
    ids, mask = ids.to(DEV), mask.to(DEV)

    def run():
        tm, im = CXRBertModel(cfg).eval(), get_biovil_resnet(None).eval()
        syn.fill_module_(tm)
        syn.fill_module_(im)
        tr = JointContrastiveTrainer(im.to(DEV), tm.to(DEV), lr=1e-4, temperature=0.07)
        tr.optimizer.zero_grad()
        loss = tr.forward_loss(images, ids, mask)
        loss.backward()
        out = {"loss": loss}
        out.update({"grad i." + n: p.grad.detach().clone() for n, p in im.named_parameters() if p.grad is not None})
        out.update({"grad t." + n: p.grad.detach().clone() for n, p in tm.named_parameters() if p.grad is not None})
        tr.optimizer.step()
        out["params"] = tr.optimizer.flat_p
        return out

    _three_ways(run)


def test_out_arguments_are_validated():
    """the optional `out=` arguments take what the wrapper would have allocated itself and nothing else"""
    f = dict(dtype=torch.float32, device=DEV)
    z = torch.zeros(16, 8, **f)
    with pytest.raises(ValueError):
        K.colstats(z, out=(torch.empty(8, **f), torch.empty(7, **f)))
    with pytest.raises(ValueError):
        K.coldot(z, z, out=torch.empty(8, device=DEV, dtype=torch.float64))
    qkv, probs, dctx = torch.zeros(2 * 8, 3 * 2 * 4, **f), torch.zeros(2, 2, 8, 8, **f), torch.zeros(2 * 8, 2 * 4, **f)
    with pytest.raises(ValueError):
        K.attn_bwd(qkv, probs, dctx, 2, 8, 2, 4, out=torch.empty(16, 23, **f))
    with pytest.raises(ValueError):
        K.attn_bwd(qkv, probs, dctx, 2, 8, 2, 4, out=torch.empty(16, 48, **f)[:, :24])       # strided columns
    dg, db = torch.empty(8, **f), torch.empty(8, **f)
    drop = K.Drop(seed=1, counter=0, layer=0, site=K.DROP_ATTN_OUT, row_offset=0, p=0.1)
    with pytest.raises(ValueError):                                                          # fp32 dx with planes dxm
        K.residual_ln_bwd_drop(z, z, torch.ones(16, **f), torch.ones(8, **f), dg, db, drop, 4, out=(torch.empty(16, 8, **f), K.Planes.empty(16, 8, device=DEV)))
    with pytest.raises(ValueError):                                                          # dxm given for the mask_dy form
        K.residual_ln_bwd_drop(z, z, torch.ones(16, **f), torch.ones(8, **f), dg, db, drop, 4, mask_dy=True, out=(torch.empty(16, 8, **f), torch.empty(16, 8, **f)))
    x, y = torch.ones(5, 8, **f), torch.ones(3, 8, **f)
    cosv, xn, yn = K.pairwise_cosine_fwd(x, y)
    with pytest.raises(ValueError):
        K.pairwise_cosine_bwd(x, y, cosv, cosv, xn, yn, out=(torch.empty(5, 8, **f), torch.empty(4, 8, **f)))
    with pytest.raises(ValueError):
        K.pairwise_cosine_bwd(x, y, cosv, cosv, xn, yn, need_dx=False, out=(torch.empty(5, 8, **f), torch.empty(3, 8, **f)))
    with pytest.raises(ValueError):
        K.bce_posneg_fwd_bwd(torch.zeros(4, 6, **f), torch.zeros(4, 3, **f), out=(torch.empty(4, 3, **f), torch.empty(4, 5, **f), torch.empty((), **f)))


# ================================================================================================ coverage table
# every `*_ws_bytes` query of include/cxrk.h -> the entry points it sizes -> the test that runs them on an exact-size guarded workspace
WS_TABLE = {
    "cxrk_gemm_splitk_ws_bytes": (("cxrk_gemm_f32", "cxrk_gemm_pl"), ("test_gemm_splitk_fp32", "test_gemm_splitk_planes")),
    "cxrk_gemm_pl_colsum_ws_bytes": (("cxrk_gemm_pl",), ("test_gemm_pl_fused_colsum",)),
    "cxrk_colsum_ws_bytes": (("cxrk_colsum", "cxrk_colsum_pl", "cxrk_colvar"), ("test_colsum_family",)),
    "cxrk_coldot_ws_bytes": (("cxrk_coldot", "cxrk_colstats"), ("test_colstats_coldot",)),
    "cxrk_conv_bwd_data_colsum_ws_bytes": (("cxrk_conv_bn_act_bwd_data", "cxrk_conv_bn_act_bwd_data_pl", "cxrk_conv_bn_act_bwd_data_pl_s2res"),
                                           ("test_conv_bwd_data_with_sums",)),
    "cxrk_conv_wgrad_ws_bytes": (("cxrk_conv_bn_act_bwd_params", "cxrk_conv_bn_act_bwd_params_pl"), ("test_conv_bwd_params",)),
    "cxrk_residual_ln_bwd_ws_bytes": (("cxrk_residual_ln_bwd", "cxrk_residual_ln_bwd_drop"), ("test_residual_ln_bwd", "test_residual_ln_bwd_drop")),
    "cxrk_attn_bwd_ws_bytes": (("cxrk_attn_bwd", "cxrk_attn_bwd_drop"), ("test_attn_bwd",)),
    "cxrk_embed_bwd_ws_bytes": (("cxrk_embed_bwd",), ("test_embed_bwd",)),
    "cxrk_pairwise_cosine_bwd_ws_bytes": (("cxrk_pairwise_cosine_bwd", "cxrk_pairwise_cosine_max_bwd"), ("test_pairwise_cosine_bwd",)),
    "cxrk_bce_posneg_ws_bytes": (("cxrk_bce_posneg_fwd_bwd",), ("test_bce_posneg",)),
    "cxrk_weight_reset_ws_bytes": (("cxrk_weight_reset",), ("test_weight_reset",)),
}


def test_every_workspace_query_has_a_contract_test():
    """a future entry point with a workspace cannot be added without a row here (the header is parsed as tests/test_cabi.py does)"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cxrk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(cxrk_[a-z0-9_]+)\s*\(", hdr))
    assert {n for n in names if n.endswith("_ws_bytes")} == set(WS_TABLE)
    takes_ws = set(re.findall(r"\b(cxrk_[a-z0-9_]+)\s*\([^;]*?\bfloat\*\s*ws\b", hdr))
    assert takes_ws == {e for entries, _ in WS_TABLE.values() for e in entries}
    for entries, tests in WS_TABLE.values():
        assert all(e in names for e in entries)
        for t in tests:
            assert callable(globals().get(t)), t
