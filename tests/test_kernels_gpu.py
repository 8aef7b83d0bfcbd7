"""Kernel-level parity: every cxrk entry point against plain PyTorch-CPU fp32 on the same seeded inputs.
Tolerance: the north star's 1e-3 relative fp32 bar; the kernels are fp32 end to end so they are checked much
tighter (2e-5 of the output scale) to catch layout / indexing mistakes."""
import math
import os

import numpy as np

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from oracle import ref_loss, ref_step  # noqa: E402
from kernel_refs import attention_reference  # noqa: E402

DEV = "cuda"
from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402


def _split() -> bool:
    return _cxr_lib.get_precision() == "split_bf16"


def close(a, b, tol=2e-5, what=""):
    if _split():      # CXRK_PRECISION=split_bf16: ~2^-16 per product -> allow 3e-4 of the output scale
        tol = max(tol, 3e-4)
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().clamp_min(1e-20)
    err = (a - b).abs().max() / scale
    assert torch.isfinite(a).all(), what
    assert err < tol, f"{what}: rel-to-max err {err:.3e} (tol {tol})"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,Kd", [(200, 136, 72), (128, 128, 32), (50, 300, 40), (300, 48, 132), (1024, 128, 768), (33, 64, 8)])
def test_gemm_nt_epilogues(M, N, Kd):
    x, w, b, r = rnd(M, Kd), rnd(N, Kd, seed=1), rnd(N, seed=2), rnd(M, N, seed=3)
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    close(K.linear_fwd(xd, wd), x @ w.T, what="plain")
    close(K.linear_fwd(xd, wd, bias=bd, act=K.ACT_RELU, residual=rd), F.relu(x @ w.T + b + r), what="bias+res+relu")
    pre = torch.empty(M, N, device=DEV)
    close(K.linear_fwd(xd, wd, bias=bd, act=K.ACT_GELU, preact_out=pre), F.gelu(x @ w.T + b), what="gelu")
    close(pre, x @ w.T + b, what="preact")


@pytest.mark.parametrize("M,N,Kd", [(200, 136, 72), (64, 256, 128), (512, 64, 260), (1000, 768, 128)])
def test_gemm_nn_tn(M, N, Kd):
    dy, w, x, aux = rnd(M, N), rnd(N, Kd, seed=1), rnd(M, Kd, seed=2), rnd(M, Kd, seed=3)
    dyd, wd, xd, auxd = dy.to(DEV), w.to(DEV), x.to(DEV), aux.to(DEV)
    close(K.linear_bwd_data(dyd, wd), dy @ w, what="dgrad")
    close(K.linear_bwd_data(dyd, wd, aux=auxd, auxmode=K.AUX_RELU_MASK), (dy @ w) * (aux > 0), what="dgrad relu mask")
    a = aux.clone().requires_grad_(True)
    F.gelu(a).backward(dy @ w)
    close(K.linear_bwd_data(dyd, wd, aux=auxd, auxmode=K.AUX_GELU_GRAD), a.grad, what="dgrad gelu'")
    dw = torch.zeros(N, Kd, device=DEV)
    close(K.linear_bwd_weight(dyd, xd, dw), dy.T @ x, what="wgrad")
    close(K.linear_bwd_weight(dyd, xd, dw, accumulate=True), 2 * (dy.T @ x), what="wgrad accumulate")
    out = torch.empty(N, Kd, device=DEV)
    close(K.gemm(dyd, xd, out, N, Kd, M, True, False, splitk=3), dy.T @ x, what="wgrad splitk=3")
    cs = torch.empty(N, device=DEV)
    close(K.colsum(dyd, cs), dy.sum(0), what="colsum")


def test_gemm_strided_rows_and_large_splitk():
    # CLS-row gather: A rows with stride L*H (modelling_cxrbert.py:98-99)
    h = rnd(16 * 32, 768)
    w = rnd(128, 768, seed=1)
    hd = h.to(DEV)
    cls = hd.view(16, 32 * 768)[:, :768]
    close(K.linear_fwd(cls, w.to(DEV)), h.view(16, 32, 768)[:, 0] @ w.T, what="strided A")
    dy, x = rnd(8192, 256), rnd(8192, 128, seed=4)
    dw = torch.empty(256, 128, device=DEV)
    close(K.linear_bwd_weight(dy.to(DEV), x.to(DEV), dw), dy.T @ x, tol=5e-5, what="wgrad auto split-K")


def test_gemm_rejects_cpu_and_bad_alignment():
    with pytest.raises(ValueError):
        K.linear_fwd(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError):
        K.linear_fwd(torch.zeros(4, 6, device=DEV), torch.zeros(4, 6, device=DEV))  # K % 4 != 0


# ------------------------------------------------------------------------------------------------ conv
CONVS = [  # N,H,W,C,Ko,R,stride,pad
    (2, 14, 14, 64, 64, 1, 1, 0), (2, 14, 14, 64, 256, 1, 1, 0), (3, 9, 9, 128, 128, 3, 1, 1),
    (2, 14, 14, 128, 128, 3, 2, 1), (2, 14, 14, 256, 512, 1, 2, 0), (2, 12, 12, 64, 64, 3, 1, 1),
    (2, 15, 15, 64, 128, 3, 2, 1),
    # real ResNet-50 shapes (batch 2)
    (2, 14, 14, 256, 1024, 1, 1, 0), (2, 14, 14, 1024, 256, 1, 1, 0), (2, 7, 7, 512, 2048, 1, 1, 0),
    (2, 14, 14, 256, 256, 3, 1, 1), (2, 28, 28, 512, 128, 1, 1, 0), (2, 56, 56, 256, 64, 1, 1, 0),
    (2, 28, 28, 64, 64, 3, 2, 1), (3, 13, 13, 128, 256, 1, 2, 0), (2, 14, 14, 512, 512, 3, 2, 1),
]


def _conv_case(N, H, W, C, Ko, R, stride, pad, seed=0, cin_real=None):
    cr = cin_real or C
    x = rnd(N, cr, H, W, seed=seed)
    w = rnd(Ko, cr, R, R, seed=seed + 1, scale=1.0 / math.sqrt(cr * R * R))
    gamma, beta = 1 + 0.1 * rnd(Ko, seed=seed + 2), 0.1 * rnd(Ko, seed=seed + 3)
    rm, rv = 0.1 * rnd(Ko, seed=seed + 4), 0.5 + rnd(Ko, seed=seed + 5).abs()
    return x, w, gamma, beta, rm, rv


@pytest.mark.parametrize("cfg", CONVS + [(2, 32, 32, 4, 64, 7, 2, 3)])
def test_conv_bn_relu_fwd_bwd(cfg):
    N, H, W, C, Ko, R, stride, pad = cfg
    cr = 3 if C == 4 else C
    x, w, gamma, beta, rm, rv = _conv_case(*cfg, cin_real=cr)
    for t in (x, w, gamma, beta):
        t.requires_grad_(True)
    z = F.conv2d(x, w, stride=stride, padding=pad)
    ybn = F.batch_norm(z, rm, rv, gamma, beta, training=False, eps=1e-5)
    res = rnd(*ybn.shape, seed=9)
    pre = ybn + res
    Ho, Wo = pre.shape[2], pre.shape[3]
    # device forward first: the reference backward is then taken under the device's ReLU decisions (a pre-activation
    # within rounding of zero may fall on either side; see oracle/ref_image.ReluPolicy)
    xd = K.nchw_to_nhwc(x.detach().to(DEV), C)
    w_cl = w.detach().permute(0, 2, 3, 1).contiguous().to(DEV)  # [Ko][R][S][C_real]
    ws = torch.empty(Ko, R, R, C, device=DEV)
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    g_, b_, rm_, rv_ = gamma.detach().to(DEV), beta.detach().to(DEV), rm.to(DEV), rv.to(DEV)
    K.bn_fold(w_cl, g_, b_, rm_, rv_, 1e-5, Ko, R * R, cr, C, ws, sc, sh, rstd)
    resd = res.permute(0, 2, 3, 1).contiguous().to(DEV)
    yd = torch.empty(N, Ho, Wo, Ko, device=DEV)
    K.conv_fwd(xd, ws, sh, resd, yd, N, H, W, C, Ko, R, R, stride, pad, True)
    mask = (K.nhwc_to_nchw(yd) > 0).cpu()
    flips = mask != (pre.detach() > 0)
    assert int(flips.sum()) <= 8 and (not flips.any() or float(pre.detach()[flips].abs().max() / pre.detach().abs().max()) < 2e-4)
    y = pre * mask
    gy = rnd(*y.shape, seed=10)
    y.backward(gy)
    close(K.nhwc_to_nchw(yd), y, what="conv fwd")
    # backward: mask by own relu (host-side here; fused into the producing dgrad in the model)
    gyd = gy.permute(0, 2, 3, 1).contiguous().to(DEV) * (yd > 0)
    sumdy = K.colsum(gyd.view(-1, Ko), torch.empty(Ko, device=DEV))
    dw = torch.empty(Ko, R, R, cr, device=DEV)
    dg, db = torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)
    K.conv_bwd_params(xd, gyd, w_cl, sc, rstd, rm_, sumdy, dw, dg, db, False, N, H, W, cr, C, Ko, R, R, stride, pad)
    close(dw.permute(0, 3, 1, 2), w.grad, tol=5e-5, what="conv wgrad")
    # dgamma = rstd * (<w, dW_raw> - mean * sum dy): exact algebra; on these zero-mean random gradients the sum cancels more than
    # on a real network (where it was measured at < 1e-6 against the direct form, scripts/exp_dgamma.py)
    close(dg, gamma.grad, tol=2e-2 if _split() else 2e-3, what="bn dgamma")
    close(db, beta.grad, tol=5e-5, what="bn dbeta")
    K.conv_bwd_params(xd, gyd, w_cl, sc, rstd, rm_, sumdy, dw, dg, db, True, N, H, W, cr, C, Ko, R, R, stride, pad)
    close(dw.permute(0, 3, 1, 2), 2 * w.grad, tol=5e-5, what="conv wgrad accumulate")
    close(db, 2 * beta.grad, tol=5e-5, what="bn dbeta accumulate")
    if C != 4:
        dxd = torch.empty(N, H, W, C, device=DEV)
        K.conv_bwd_data(gyd, ws, None, None, dxd, N, H, W, C, Ko, R, R, stride, pad)
        close(K.nhwc_to_nchw(dxd), x.grad, tol=5e-5, what="conv dgrad")
        add = rnd(N, H, W, C, seed=11).to(DEV)
        if R == 1 and stride == 2:  # three of the four output-parity classes receive no tap: plain form only
            with pytest.raises(ValueError):
                K.conv_bwd_data(gyd, ws, add, xd, dxd, N, H, W, C, Ko, R, R, stride, pad)
        else:
            K.conv_bwd_data(gyd, ws, add, xd, dxd, N, H, W, C, Ko, R, R, stride, pad)
            close(K.nhwc_to_nchw(dxd), (x.grad + K.nhwc_to_nchw(add).cpu()) * (x.detach() > 0), tol=5e-5, what="dgrad+res+mask")
            # same launch with the fused column sums (the BatchNorm beta gradient of the producing unit)
            sums, dx2 = torch.empty(C, device=DEV), torch.empty_like(dxd)
            K.conv_bwd_data(gyd, ws, add, xd, dx2, N, H, W, C, Ko, R, R, stride, pad, sums=sums)
            assert torch.equal(dx2, dxd)
            close(sums, dxd.double().view(-1, C).sum(0).float(), tol=5e-5, what="dgrad column sums")


@pytest.mark.parametrize("ratio", [0.0, 5.0, 50.0])
def test_bn_gamma_gradient_on_post_relu_input(ratio):
    """The BatchNorm gamma gradient taken from the weight gradient, dgamma = rstd * (<w, dW_raw> - mean * sum(dy)), at the network's
    own operating point: the unit's input is post-ReLU (all positive, like every unit of the trunk), the gradient sits behind the
    unit's own ReLU, and the running mean is `ratio` sigma away from the batch mean.  Against the direct sum dy * (z - mean) * rstd in
    fp64: the north star's 1e-3 (measured 2-4e-7 in fp32 mode, 2-5e-6 in split-bf16: scripts/exp_dgamma.py).  The 2e-3 / 2e-2
    allowances of the conv tests above are for their zero-mean random inputs, where the direct sum itself cancels."""
    N, H, C, Ko, R = 16, 28, 128, 128, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, H, generator=g).abs()
    w = torch.randn(Ko, C, R, R, generator=g) / math.sqrt(C * R * R)
    dy = torch.randn(N, Ko, H, H, generator=g) * (torch.rand(N, Ko, H, H, generator=g) > 0.5)
    z = F.conv2d(x.double(), w.double(), padding=1)
    sig = z.std(dim=(0, 2, 3))
    rm = (z.mean(dim=(0, 2, 3)) + ratio * sig).float()
    rv = (sig * sig).float()
    rstd64 = 1.0 / torch.sqrt(rv.double() + 1e-5)
    ref = (dy.double() * (z - rm.double()[None, :, None, None]) * rstd64[None, :, None, None]).sum(dim=(0, 2, 3))
    gamma, beta = torch.ones(Ko, device=DEV), torch.zeros(Ko, device=DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    w_cl = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    dw, dg, db = torch.empty(Ko, R, R, C, device=DEV), torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)
    if _split():
        wsp = K.Planes.empty(Ko, R * R * C, device=DEV)
        K.bn_fold_pl(w_cl, gamma, beta, rm.to(DEV), rv.to(DEV), 1e-5, Ko, R * R, C, C, wsp, sc, sh, rstd)
        xp, dyp = K.split_planes(xd.view(-1, C)), K.split_planes(dyd.view(-1, Ko))
        sumdy = K.colsum(dyp, torch.empty(Ko, device=DEV))
        K.conv_bwd_params_pl(xp, dyp, w_cl, sc, rstd, rm.to(DEV), sumdy, dw, dg, db, False, N, H, H, C, Ko, R, R, 1, 1)
    else:
        ws = torch.empty(Ko, R, R, C, device=DEV)
        K.bn_fold(w_cl, gamma, beta, rm.to(DEV), rv.to(DEV), 1e-5, Ko, R * R, C, C, ws, sc, sh, rstd)
        sumdy = K.colsum(dyd.view(-1, Ko), torch.empty(Ko, device=DEV))
        K.conv_bwd_params(xd, dyd, w_cl, sc, rstd, rm.to(DEV), sumdy, dw, dg, db, False, N, H, H, C, C, Ko, R, R, 1, 1)
    err = float((dg.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err < 1e-3, (ratio, err)
    assert err < (5e-5 if _split() else 5e-6), (ratio, err)      # where the kernels actually are


@pytest.mark.parametrize("gval", [0.0, 1e-30, 1e-6, 1e-3])
def test_bn_gamma_gradient_does_not_divide_by_gamma(gval):
    """dgamma used to be sum(dy*(y_bn - beta)) / gamma — inf / NaN / 1e-2 errors for zero-init-residual or pruned
    channels.  It is now taken from the weight gradient and must match PyTorch for any gamma."""
    N, H, C, Ko, R = 2, 10, 64, 64, 3
    x, w, gamma, beta, rm, rv = _conv_case(N, H, H, C, Ko, R, 1, 1)
    gamma = torch.full_like(gamma, gval)
    gamma[::2] = 1.0 + 0.1 * torch.arange(Ko // 2)
    for t in (x, w, gamma, beta):
        t.requires_grad_(True)
    y = F.batch_norm(F.conv2d(x, w, padding=1), rm, rv, gamma, beta, training=False, eps=1e-5)
    gy = rnd(*y.shape, seed=10)
    y.backward(gy)
    xd = K.nchw_to_nhwc(x.detach().to(DEV), C)
    w_cl = w.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    ws = torch.empty(Ko, R, R, C, device=DEV)
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    K.bn_fold(w_cl, gamma.detach().to(DEV), beta.detach().to(DEV), rm.to(DEV), rv.to(DEV), 1e-5, Ko, R * R, C, C, ws, sc, sh, rstd)
    gyd = gy.permute(0, 2, 3, 1).contiguous().to(DEV)
    sumdy = K.colsum(gyd.view(-1, Ko), torch.empty(Ko, device=DEV))
    dw, dg, db = torch.empty(Ko, R, R, C, device=DEV), torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)
    K.conv_bwd_params(xd, gyd, w_cl, sc, rstd, rm.to(DEV), sumdy, dw, dg, db, False, N, H, H, C, C, Ko, R, R, 1, 1)
    assert torch.isfinite(dg).all()
    close(dg, gamma.grad, tol=2e-3, what=f"dgamma at gamma={gval}")
    close(dw.permute(0, 3, 1, 2), w.grad, tol=5e-5, what="dw")


# ------------------------------------------------------------------------------------------------ planes (split-bf16) storage
def _pl(t):
    return K.split_planes(t.contiguous().to(DEV))


def test_planes_roundtrip_and_colsum():
    x = rnd(300, 136)
    p = _pl(x)
    assert p.t.dtype == torch.bfloat16 and tuple(p.shape) == (300, 136)
    close(p.float(), x, tol=2e-5, what="hi + lo ~ x (2^-17)")
    assert float((p.t[0].float().cpu() - x.bfloat16().float()).abs().max()) == 0.0     # hi plane = round-to-nearest bf16
    close(K.colsum(p, torch.empty(136, device=DEV)), x.sum(0), tol=2e-5, what="colsum planes")


@pytest.mark.parametrize("rows,C,planes", [(5000, 64, False), (5000, 64, True), (777, 264, True), (1, 8, False), (70000, 16, True)])
def test_train_mode_batchnorm_kernels(rows, C, planes):
    """csrc/bn_train.hip against torch.nn.functional.batch_norm(training=True) + autograd (float64 on the CPU): one-pass statistics
    with a LARGE common offset (the case a naive sum-of-squares loses), apply + ReLU decision bits, running-stat update, dgamma /
    dbeta / dz."""
    g = torch.Generator().manual_seed(rows + C)
    z = torch.randn(rows, C, generator=g) * torch.linspace(0.1, 3.0, C) + torch.linspace(-300.0, 300.0, C)
    res = torch.randn(rows, C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    wrap = _pl if planes else (lambda t: t.contiguous().to(DEV))
    zd = wrap(z)
    zq = zd.float().cpu() if planes else z                   # the values the kernels see (planes storage rounds to ~2^-17)
    if rows == 1:                                            # torch refuses one value per channel; mean = z, variance 0
        mean, var = K.colstats(zd)
        close(mean, zq[0], tol=1e-6, what="mean of one row")
        assert float(var.abs().max()) == 0.0
        return
    # reference in float64
    z64 = zq.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y64 = F.relu(F.batch_norm(z64, rm, rv, g64, b64, training=True, momentum=0.1, eps=1e-5) + res.double())
    # kernels
    mean, var = K.colstats(zd)
    close(mean, zq.double().mean(0).float(), tol=1e-6, what="mean")
    close(var, zq.double().var(0, unbiased=False).float(), tol=2e-5, what="biased var")
    close(K.colstats(zd, unbiased=True)[1], zq.double().var(0, unbiased=True).float(), tol=2e-5, what="unbiased var")
    rmd, rvd = rm0.to(DEV), rv0.to(DEV)
    scale, shift, rstd = K.bn_train_fwd_coeffs(mean, var, gamma.to(DEV), beta.to(DEV), 1e-5, rows, 0.1, rmd, rvd)
    y, mask = K.bn_apply(zd, scale, shift, residual=wrap(res), relu=True, want_mask=True)
    yf = y.float() if planes else y
    close(yf, y64.detach().float(), tol=3e-5, what="y")
    close(rmd, rm.float(), tol=2e-6, what="running_mean")
    close(rvd, rv.float(), tol=2e-5, what="running_var")
    bits = torch.from_numpy(np.unpackbits(mask.cpu().numpy(), axis=1, bitorder="little")[:, :C].astype(bool))
    agree = (bits == (y64.detach() > 0)).float().mean()
    assert agree > 0.9999, agree                              # decisions within rounding of zero may differ
    # backward: dy masked by the kernel's own decisions, as image_encoder._backward does
    dym = dy * bits
    dyd = wrap(dym)
    dyq = dyd.float().cpu() if planes else dym
    sumdy = K.colsum(dyd, torch.empty(C, device=DEV))
    close(K.coldot(dyd, zd), (dyq.double() * zq.double()).sum(0).float(), tol=2e-5, what="plain dot")
    dot = K.coldot(dyd, zd, mean)
    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    A, B, Cc = K.bn_train_bwd_coeffs(gamma.to(DEV), mean, rstd, sumdy, dot, rows, dgam, dbet, False)
    dz = K.bn_train_dz(dyd, zd, A, B, Cc)
    dzf = dz.float() if planes else dz
    # reference with the same decisions
    z64b = zq.double().requires_grad_(True)
    g64b, b64b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.batch_norm(z64b, None, None, g64b, b64b, training=True, eps=1e-5).backward(dyq.double())
    # the products are centred (z - mean) before they are summed: what is left of the +-300 offsets is the rounding of the fp32
    # mean itself (300 * 2^-24 against a spread of 0.1 .. 3), 1e-4 of dgamma at the narrow channels
    close(dbet, b64b.grad.float(), tol=2e-5, what="dbeta")
    close(dgam, g64b.grad.float(), tol=3e-4, what="dgamma")
    close(dzf, z64b.grad.float(), tol=1e-4, what="dz")


PL_GEMMS = [(200, 136, 72), (1024, 128, 768), (64, 256, 128), (512, 64, 264), (4096, 512, 512), (8192, 768, 256)]


@pytest.mark.parametrize("M,N,Kd", PL_GEMMS)
def test_planes_gemm_family(M, N, Kd, wide):
    """Every GEMM form of the BERT path on planes operands (128x128-class tiles and, from 1 GFLOP with both dimensions >= 256,
    the 256x256 LDS-DMA kernel) with every fused epilogue, against PyTorch-CPU fp32."""
    x, w, b, r = rnd(M, Kd, scale=0.5), rnd(N, Kd, seed=1, scale=0.5), rnd(N, seed=2), rnd(M, N, seed=3)
    xp, wp = _pl(x), _pl(w)
    ref = x @ w.T
    tol = 2e-4
    close(K.linear_fwd_pl(xp, wp), ref, tol=tol, what="plain -> fp32")
    close(K.linear_fwd_pl(xp, wp, out_planes=True).float(), ref, tol=tol, what="plain -> planes")
    close(K.linear_fwd_pl(xp, wp, bias=b.to(DEV), residual=_pl(r)), ref + b + r, tol=tol, what="bias + planes residual -> fp32")
    close(K.linear_fwd_pl(xp, wp, bias=b.to(DEV), residual=r.to(DEV)), ref + b + r, tol=tol, what="bias + fp32 residual -> fp32")
    pre = torch.empty(M, N, device=DEV)
    y = K.linear_fwd_pl(xp, wp, bias=b.to(DEV), act=K.ACT_GELU, preact_out=pre, out_planes=True)
    close(y.float(), F.gelu(ref + b), tol=tol, what="gelu -> planes")
    close(pre, ref + b, tol=tol, what="preact copy")
    mask = torch.empty(M, N // 8, dtype=torch.uint8, device=DEV) if N % 64 == 0 else None
    if mask is not None:
        y = K.linear_fwd_pl(xp, wp, bias=b.to(DEV), act=K.ACT_RELU, out_planes=True, maskout=mask)
        close(y.float(), F.relu(ref + b), tol=tol, what="relu -> planes")
        dec = K.unpack_mask(mask, N)
        assert bool((dec == (y.float().cpu() > 0)).all())
    # data gradient forms
    dy, aux = rnd(M, N, seed=4, scale=0.5), rnd(M, Kd, seed=5)
    dyp = _pl(dy)
    close(K.linear_bwd_data_pl(dyp, wp), dy @ w, tol=tol, what="dgrad -> fp32")
    close(K.linear_bwd_data_pl(dyp, wp, residual=_pl(aux)), dy @ w + aux, tol=tol, what="dgrad + planes residual")
    a = aux.clone().requires_grad_(True)
    F.gelu(a).backward(dy @ w)
    close(K.linear_bwd_data_pl(dyp, wp, aux=aux.to(DEV), auxmode=K.AUX_GELU_GRAD, out_planes=True).float(), a.grad, tol=tol, what="dgrad gelu'")
    dec = (rnd(M, Kd, seed=6) > 0)
    bits = torch.from_numpy(__import__("numpy").packbits(dec.numpy(), axis=1, bitorder="little")).to(DEV)
    close(K.linear_bwd_data_pl(dyp, wp, maskin=bits, out_planes=True).float(), (dy @ w) * dec, tol=tol, what="dgrad bit mask")
    out = torch.full((M, Kd), 1.0, device=DEV)
    close(K.linear_bwd_data_pl(dyp, wp, out=out, accumulate=True), dy @ w + 1.0, tol=tol, what="dgrad accumulate")
    if Kd % 8 == 0:   # column sums of the stored gradient from the same epilogue (generic feature set, and the compiled-in GELU' one)
        cs = torch.full((Kd,), 3.0, device=DEV)
        K.linear_bwd_data_pl(dyp, wp, out_planes=True, colsum=cs)
        close(cs, (dy @ w).sum(0), tol=tol * 4, what="dgrad fused column sums")
        pre = rnd(M, Kd, seed=12)
        gp = 0.5 * (1 + torch.erf(pre / math.sqrt(2))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2 * math.pi)
        dxg = K.linear_bwd_data_pl(dyp, wp, aux=pre.to(DEV), auxmode=K.AUX_GELU_GRAD, out_planes=True, colsum=cs, colsum_accumulate=True)
        close(dxg.float(), (dy @ w) * gp, tol=tol, what="dgrad through gelu'")
        close(cs, (dy @ w).sum(0) + ((dy @ w) * gp).sum(0), tol=tol * 4, what="fused column sums, accumulated")
    # weight gradient (split-K)
    dw = torch.zeros(N, Kd, device=DEV)
    close(K.linear_bwd_weight_pl(dyp, xp, dw), dy.T @ x, tol=tol, what="wgrad")
    close(K.linear_bwd_weight_pl(dyp, xp, dw, accumulate=True), 2 * (dy.T @ x), tol=tol, what="wgrad accumulate")


def test_planes_gemm_strided_rows(wide):
    h, w = rnd(16 * 32, 768), rnd(128, 768, seed=1)
    hp = _pl(h)
    cls = K.Planes(hp.t.view(2, 16, 32 * 768)[:, :, :768])        # CLS rows: row stride L*H
    close(K.linear_fwd_pl(cls, _pl(w)), h.view(16, 32, 768)[:, 0] @ w.T, tol=2e-4, what="strided planes A")
    dx = torch.zeros(16 * 32, 768, device=DEV)
    dy = rnd(16, 128, seed=2)
    K.linear_bwd_data_pl(_pl(dy), _pl(w), out=dx.view(16, 32 * 768)[:, :768], accumulate=True)
    ref = torch.zeros(16, 32, 768)
    ref[:, 0] = dy @ w
    close(dx.view(16, 32, 768), ref, tol=2e-4, what="strided fp32 output rows")
    K.planes_add_rows(_pl(dy @ w), dx.view(16, 32 * 768)[:, :768])
    close(dx.view(16, 32, 768), 2 * ref, tol=2e-4, what="planes_add_rows")


PL_CONVS = [  # N,H,W,C,Ko,R,stride,pad
    (2, 14, 14, 64, 64, 1, 1, 0), (2, 14, 14, 64, 256, 1, 1, 0), (3, 9, 9, 128, 128, 3, 1, 1), (2, 14, 14, 128, 128, 3, 2, 1),
    (2, 14, 14, 256, 512, 1, 2, 0), (2, 15, 15, 64, 128, 3, 2, 1), (2, 14, 14, 1024, 256, 1, 1, 0), (2, 7, 7, 512, 2048, 1, 1, 0),
    (2, 56, 56, 256, 64, 1, 1, 0),
    # >= 1 GFLOP: the 256x256 LDS-DMA kernel takes forward / data gradient / weight gradient where both tile dimensions fill
    (16, 28, 28, 128, 128, 3, 1, 1), (32, 28, 28, 256, 256, 3, 2, 1), (64, 14, 14, 256, 1024, 1, 1, 0), (64, 14, 14, 1024, 256, 1, 1, 0),
    (32, 28, 28, 512, 1024, 1, 2, 0),
    # 3x3 / stride 1 / 64 -> 64: the window-resident kernel (csrc/conv_halo.h): two tiles with a ragged end, the real 56-pixel rows
    # (36.75 tiles, windows crossing image boundaries), the widest row it takes (58) and the first it leaves to the implicit GEMM (59)
    (2, 12, 12, 64, 64, 3, 1, 1), (3, 56, 56, 64, 64, 3, 1, 1), (5, 7, 58, 64, 64, 3, 1, 1), (2, 9, 59, 64, 64, 3, 1, 1), (1, 3, 5, 64, 64, 3, 1, 1),
]


@pytest.mark.parametrize("cfg", PL_CONVS)
def test_planes_conv_bn_relu_fwd_bwd(cfg, wide):
    """conv + BN + identity + ReLU forward (planes in / out, ReLU bit mask), data gradient (bit mask, residual, fused column sums)
    and weight gradient (+ BN gradients) on planes operands against PyTorch-CPU fp32."""
    N, H, W, C, Ko, R, stride, pad = cfg
    x, w, gamma, beta, rm, rv = _conv_case(*cfg)
    for t in (x, w, gamma, beta):
        t.requires_grad_(True)
    z = F.conv2d(x, w, stride=stride, padding=pad)
    ybn = F.batch_norm(z, rm, rv, gamma, beta, training=False, eps=1e-5)
    res = rnd(*ybn.shape, seed=9)
    pre = ybn + res
    Ho, Wo = pre.shape[2], pre.shape[3]
    xd = _pl(x.detach().permute(0, 2, 3, 1))
    w_cl = w.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    ws = K.Planes.empty(Ko, R * R * C, device=DEV)
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    g_, b_, rm_, rv_ = gamma.detach().to(DEV), beta.detach().to(DEV), rm.to(DEV), rv.to(DEV)
    K.bn_fold_pl(w_cl, g_, b_, rm_, rv_, 1e-5, Ko, R * R, C, C, ws, sc, sh, rstd)
    resd = _pl(res.permute(0, 2, 3, 1))
    yd = K.Planes.empty(N, Ho, Wo, Ko, device=DEV)
    mask = torch.empty(N * Ho * Wo, Ko // 8, dtype=torch.uint8, device=DEV)
    K.conv_fwd_pl(xd, ws, sh, resd, yd, mask, N, H, W, C, Ko, R, R, stride, pad, True)
    yf = yd.float()
    dec = K.unpack_mask(mask, Ko).view(N, Ho, Wo, Ko)
    assert bool((dec == (yf.cpu() > 0)).all())
    dec_nchw = dec.permute(0, 3, 1, 2)
    flips = dec_nchw != (pre.detach() > 0)
    assert int(flips.sum()) <= max(8, flips.numel() // 20000) and (not flips.any() or float(pre.detach()[flips].abs().max() / pre.detach().abs().max()) < 2e-3)
    y = pre * dec_nchw
    gy = rnd(*y.shape, seed=10)
    y.backward(gy)
    close(K.nhwc_to_nchw(yf), y, tol=2e-4, what="planes conv fwd")
    gyd = _pl((gy * dec_nchw).permute(0, 2, 3, 1))
    sumdy = K.colsum(gyd.view(N * Ho * Wo, Ko), torch.empty(Ko, device=DEV))
    dw, dg, db = torch.empty(Ko, R, R, C, device=DEV), torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)
    K.conv_bwd_params_pl(xd, gyd, w_cl, sc, rstd, rm_, sumdy, dw, dg, db, False, N, H, W, C, Ko, R, R, stride, pad)
    close(dw.permute(0, 3, 1, 2), w.grad, tol=3e-4, what="planes conv wgrad")
    close(dg, gamma.grad, tol=2e-2, what="planes bn dgamma")
    close(db, beta.grad, tol=3e-4, what="planes bn dbeta")
    dxd = K.Planes.empty(N, H, W, C, device=DEV)
    K.conv_bwd_data_pl(gyd, ws, None, None, dxd, N, H, W, C, Ko, R, R, stride, pad)
    close(K.nhwc_to_nchw(dxd.float()), x.grad, tol=3e-4, what="planes conv dgrad")
    if not (R == 1 and stride == 2):
        add = rnd(N, H, W, C, seed=11)
        xdec = (rnd(N, H, W, C, seed=12) > 0)
        bits = torch.from_numpy(__import__("numpy").packbits(xdec.view(-1, C).numpy(), axis=1, bitorder="little")).to(DEV)
        sums = torch.empty(C, device=DEV)
        K.conv_bwd_data_pl(gyd, ws, _pl(add), bits, dxd, N, H, W, C, Ko, R, R, stride, pad, sums=sums)
        ref = (x.grad.permute(0, 2, 3, 1) + add) * xdec
        close(dxd.float(), ref, tol=3e-4, what="planes dgrad + residual + bit mask")
        close(sums, ref.double().reshape(-1, C).sum(0).float(), tol=3e-4, what="planes dgrad column sums")


@pytest.mark.parametrize("N,H,W,C,Ko,R", [(3, 8, 8, 256, 64, 1), (2, 7, 9, 128, 64, 1), (2, 12, 12, 64, 64, 3), (4, 28, 28, 512, 128, 1)])
def test_planes_dgrad_compact_stride2_residual(N, H, W, C, Ko, R, wide):
    """The data gradient with the identity-branch gradient of a stride-2 projection given COMPACT ([N, H/2, W/2, C], even pixels only)
    equals, bit for bit, the one with the same values scattered into a full-resolution residual (zeros elsewhere): output, column
    sums — and the compact gradient itself equals the even pixels of the dense 1x1 / stride-2 data gradient."""
    g = torch.Generator().manual_seed(N * H + C)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    # (1) the projection's data gradient: dense form vs compact form
    Kd = 2 * C
    gd = _pl(torch.randn(N, Ho, Wo, Kd, generator=g))
    wd = _pl(torch.randn(Kd, C, generator=g) * 0.05)
    dense = K.Planes.empty(N, H, W, C, device=DEV)
    K.conv_bwd_data_pl(gd, wd, None, None, dense, N, H, W, C, Kd, 1, 1, 2, 0)
    comp = K.conv1x1_s2_bwd_data_compact_pl(gd, wd, N, H, W, C, Kd)
    assert tuple(comp.shape) == (N, Ho, Wo, C)
    df = dense.float()
    assert torch.equal(df[:, ::2, ::2], comp.float())
    mask_odd = torch.ones(H, W, dtype=torch.bool); mask_odd[::2, ::2] = False
    assert float(df[:, mask_odd.to(DEV)].abs().max()) == 0.0
    # (2) conv1's data gradient with either residual
    dy = _pl(torch.randn(N, H, W, Ko, generator=g))
    w1 = _pl(torch.randn(Ko, R * R * C, generator=g) * 0.05)
    maskin = torch.randint(0, 256, (N * H * W, C // 8), dtype=torch.uint8, generator=g).to(DEV)
    outs = []
    for res, s2 in ((dense, False), (comp, True)):
        dx = K.Planes.empty(N, H, W, C, device=DEV)
        sums = torch.empty(C, device=DEV)
        K.conv_bwd_data_pl(dy, w1, res, maskin, dx, N, H, W, C, Ko, R, R, 1, R // 2, sums, residual_s2=s2)
        outs.append((dx.t.clone(), sums.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    # and the residual really arrived: without it the result differs at the even pixels
    dx0 = K.Planes.empty(N, H, W, C, device=DEV)
    K.conv_bwd_data_pl(dy, w1, None, maskin, dx0, N, H, W, C, Ko, R, R, 1, R // 2)
    diff = (dx0.float() - K.Planes(outs[1][0]).float()).abs()
    assert float(diff[:, ::2, ::2].max()) > 0.0 and float(diff[:, mask_odd.to(DEV)].max()) == 0.0
    with pytest.raises(ValueError):
        K.conv_bwd_data_pl(dy, w1, dense, maskin, dx0, N, H, W, C, Ko, R, R, 1, R // 2, residual_s2=True)     # wrong residual shape


def test_planes_stem_maxpool_and_mean():
    """stem (fp32 image -> planes), max-pool on planes (+ backward masked by the sign of the pooled value), mean backward."""
    N, H, C, Ko = 2, 32, 4, 64
    x, w, gamma, beta, rm, rv = _conv_case(N, H, H, C, Ko, 7, 2, 3, cin_real=3)
    ybn = F.batch_norm(F.conv2d(x, w, stride=2, padding=3), rm, rv, gamma, beta, training=False, eps=1e-5)
    xd = K.nchw_to_nhwc(x.to(DEV), 4)
    w_cl = w.permute(0, 2, 3, 1).contiguous().to(DEV)
    ws = torch.empty(Ko, 7, 7, 4, device=DEV)
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    K.bn_fold(w_cl, gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), 1e-5, Ko, 49, 3, 4, ws, sc, sh, rstd)
    yd = K.Planes.empty(N, 16, 16, Ko, device=DEV)
    K.conv_fwd_pl(xd, ws, sh, None, yd, None, N, H, H, 4, Ko, 7, 7, 2, 3, True)
    close(K.nhwc_to_nchw(yd.float()), F.relu(ybn), tol=2e-4, what="stem -> planes")
    stem = yd.float().permute(0, 3, 1, 2).cpu().requires_grad_(True)       # continue from the device's own values
    pooled_ref = F.max_pool2d(stem, 3, 2, 1)
    gp = rnd(*pooled_ref.shape, seed=3)
    pooled_ref.backward(gp)
    pd, idx = K.maxpool_fwd_pl(yd)
    assert float((K.nhwc_to_nchw(pd.float()).cpu() - pooled_ref.detach()).abs().max()) == 0.0
    ds = K.maxpool_bwd_pl(_pl(gp.permute(0, 2, 3, 1)), idx, pd, 16, 16)
    close(K.nhwc_to_nchw(ds), stem.grad * (stem.detach() > 0), tol=2e-5, what="maxpool bwd (+ stem ReLU)")
    g, add = rnd(3, 128, seed=1), rnd(3, 49, 128, seed=2)
    close(K.spatial_mean_bwd_pl(g.to(DEV), 49, add=add.to(DEV)).float(), (g / 49)[:, None, :] + add, tol=2e-5, what="spatial mean bwd -> planes")


def test_maxpool_spatial_mean():
    x = F.relu(rnd(2, 8, 13, 13)).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    gy = rnd(*y.shape, seed=3)
    y.backward(gy)
    xd = K.nchw_to_nhwc(x.detach().to(DEV), 8)
    yd, idx = K.maxpool_fwd(xd)
    close(K.nhwc_to_nchw(yd), y, what="maxpool fwd")
    dx = K.maxpool_bwd(gy.permute(0, 2, 3, 1).contiguous().to(DEV), idx, xd, False)
    close(K.nhwc_to_nchw(dx), x.grad, what="maxpool bwd")
    p = rnd(3, 49, 128)
    close(K.spatial_mean_fwd(p.to(DEV)), p.mean(1), what="spatial mean")
    g = rnd(3, 128, seed=1)
    close(K.spatial_mean_bwd(g.to(DEV), 49), (g / 49)[:, None, :].expand(3, 49, 128), what="spatial mean bwd")


# ------------------------------------------------------------------------------------------------ BERT pieces
@pytest.mark.parametrize("H", [768, 128, 64])
def test_layernorm_fwd_bwd(H):
    rows = 77
    x, r = rnd(rows, H), rnd(rows, H, seed=1)
    g, b = (1 + 0.1 * rnd(H, seed=2)).requires_grad_(True), (0.1 * rnd(H, seed=3)).requires_grad_(True)
    s = (x + r).requires_grad_(True)
    y = F.layer_norm(s, (H,), g, b, 1e-12)
    gy = rnd(rows, H, seed=4)
    y.backward(gy)
    yd, xhat, rstd = K.residual_ln_fwd(x.to(DEV), r.to(DEV), g.detach().to(DEV), b.detach().to(DEV), 1e-12)
    close(yd, y, what="ln fwd")
    dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    add = rnd(rows, H, seed=5)
    dx = K.residual_ln_bwd(gy.to(DEV), xhat, rstd, g.detach().to(DEV), dg, db, dx_add=add.to(DEV))
    close(dx, s.grad + add, what="ln dx")
    close(dg, g.grad, what="ln dgamma")
    close(db, b.grad, what="ln dbeta")
    if H % 8 == 0:   # planes outputs (what the next GEMM reads in split-bf16 mode)
        yp, _, _ = K.residual_ln_fwd(x.to(DEV), r.to(DEV), g.detach().to(DEV), b.detach().to(DEV), 1e-12, out_planes=True)
        close(yp.float(), y, what="ln fwd -> planes")
        dxp = K.residual_ln_bwd(gy.to(DEV), xhat, rstd, g.detach().to(DEV), dg, db, out_planes=True)
        close(dxp.float(), s.grad, what="ln dx -> planes")
        # fused column sums of the result (bias gradient of the dense layer in front of the LayerNorm), fresh and accumulated
        bsum = torch.full((H,), 7.0, device=DEV)
        K.residual_ln_bwd(gy.to(DEV), xhat, rstd, g.detach().to(DEV), dg, db, dx_add=add.to(DEV), out_planes=True, dxsum=bsum)
        close(bsum, (s.grad + add).sum(0), what="ln fused column sums")
        K.residual_ln_bwd(gy.to(DEV), xhat, rstd, g.detach().to(DEV), dg, db, dx_add=add.to(DEV), dxsum=bsum, dxsum_accumulate=True)
        close(bsum, 2 * (s.grad + add).sum(0), what="ln fused column sums, accumulated")
        close(dg, g.grad, what="ln dgamma beside the fused sums")


def test_embed_ln_and_scatter():
    V, H, L, B = 50, 64, 8, 3
    word, pos, typ = rnd(V, H), rnd(16, H, seed=1), rnd(2, H, seed=2)
    g, b = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(5))
    ref = F.layer_norm(word[ids] + pos[:L][None] + typ[0], (H,), g, b, 1e-12)
    y, xhat, rstd = K.embed_ln_fwd(ids.to(DEV), word.to(DEV), pos.to(DEV), typ[0].contiguous().to(DEV), g.to(DEV), b.to(DEV), 1e-12, L)
    close(y.view(B, L, H), ref, what="embed ln")
    yp, _, _ = K.embed_ln_fwd(ids.to(DEV), word.to(DEV), pos.to(DEV), typ[0].contiguous().to(DEV), g.to(DEV), b.to(DEV), 1e-12, L, out_planes=True)
    close(yp.float().view(B, L, H), ref, what="embed ln -> planes")
    dx = rnd(B * L, H, seed=6)
    dword = torch.zeros(V, H, device=DEV)
    K.embed_bwd(ids.to(DEV).view(-1), dx.to(DEV), dword)
    refw = torch.zeros(V, H).index_add_(0, ids.view(-1), dx)
    close(dword, refw, what="embed scatter-add")
    # token-id statistics of a real batch: a few ids ([PAD], [CLS], [SEP]) own long runs that span many 32-entry chunks of the sorted
    # list, most ids occur once or twice; T not a multiple of the chunk; accumulation into a non-zero buffer; two runs bit-identical
    g = torch.Generator().manual_seed(11)
    T, V2, H2 = 4099, 300, 72
    ids2 = torch.randint(0, V2, (T,), generator=g)
    ids2[torch.rand(T, generator=g) < 0.55] = 0          # "[PAD]"
    ids2[::32] = 101 % V2                                 # "[CLS]" at a fixed stride
    ids2[-7:] = V2 - 1                                    # a run that ends the sorted list
    dx2 = rnd(T, H2, seed=12)
    base = rnd(V2, H2, seed=13)
    out1, out2 = base.clone().to(DEV), base.clone().to(DEV)
    K.embed_bwd(ids2.to(DEV), dx2.to(DEV), out1)
    K.embed_bwd(ids2.to(DEV), dx2.to(DEV), out2)
    ref2 = base.double().index_add_(0, ids2, dx2.double()).float()
    close(out1, ref2, what="embed scatter-add, long runs")
    assert torch.equal(out1, out2), "the scatter must be deterministic (no atomics)"


@pytest.mark.parametrize("L,ragged", [(32, False), (32, True), (17, True), (64, False), (16, "empty"),
                                      (65, True), (100, False), (200, True), (512, True), (96, "empty")])   # > 64: the tiled kernels
def test_attention_fwd_bwd(L, ragged):
    B, nH, dH = 3, 4, (64 if L != 100 else 32)
    qkv, mask, gc, ctx, dqkv = attention_reference(B, L, nH, dH, ragged)      # PyTorch-CPU fp32 (tests/kernel_refs.py)
    qd = qkv.to(DEV)
    cd, probs = K.attn_fwd(qd, mask.to(DEV), B, L, nH, dH)
    close(cd, ctx, what="attn fwd")
    dq = K.attn_bwd(qd, probs, gc.to(DEV), B, L, nH, dH)
    close(dq, dqkv, tol=5e-5, what="attn bwd")
    cp, _ = K.attn_fwd(qd, mask.to(DEV), B, L, nH, dH, out_planes=True)
    close(cp.float(), ctx, what="attn fwd -> planes")
    close(K.attn_bwd(qd, probs, gc.to(DEV), B, L, nH, dH, out_planes=True).float(), dqkv, tol=5e-5, what="attn bwd -> planes")


# ------------------------------------------------------------------------------------------------ heads
def test_l2norm_infonce_pieces(golden_dir):
    import numpy as np
    g = np.load(f"{golden_dir}/g4_infonce.npz")
    I, T = torch.from_numpy(g["I"]), torch.from_numpy(g["T"])
    ih, inorm = K.l2norm_fwd(I.to(DEV))
    close(ih, F.normalize(I, dim=1), what="l2norm")
    d = rnd(32, 128, seed=3)
    x = I.clone().requires_grad_(True)
    F.normalize(x, dim=1).backward(d)
    close(K.l2norm_bwd(d.to(DEV), ih, inorm), x.grad, what="l2norm bwd")
    S = torch.from_numpy(g["S_tau0.07"])
    lse, diag = K.infonce_row_lse(S.to(DEV), 0)
    close(lse, torch.logsumexp(S, 1), what="row lse")
    close(diag, S.diag(), what="diag")


def test_epilogue_lane_maps_standalone():
    """csrc/epilogue_check: every compiled-in fp32 feature set of the GEMM epilogue on small / ragged / strided shapes with
    guard regions around all buffers (a store outside its tensor is reported, not a fault) against a CPU fp64 reference."""
    import subprocess
    exe = os.path.join(os.path.dirname(_cxr_lib.__file__), "csrc", "epilogue_check")
    if not os.path.exists(exe):   # normally built by __graft_entry__.build() with the library; the box has hipcc too
        subprocess.run(["make", "-C", os.path.dirname(exe), "epilogue_check"], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    bad = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert r.returncode == 0 and not bad and "0 failing cases" in r.stdout, "\n".join(bad[:10]) + r.stderr[-500:]


def test_pairwise_cosine_max_and_patch_similarity_vs_fixture(golden_dir):
    """MAX_EMB head (`Trainer.py:1691-1693`) and the patch-wise similarity GEMV (`vlp/inference_engine.py:104`) against the
    committed G6 vectors (similarity map: outputs of the reference's own static methods; cosine: restatement, parity unpinned)."""
    g = np.load(os.path.join(golden_dir, "g6_simmap_maxemb.npz"))
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    cosv, xn, yn, mx, mean, arg = K.pairwise_cosine_max_fwd(x, y, 10)
    close(mx, torch.from_numpy(g["max"]), what="max over prompts")
    close(mean, torch.from_numpy(g["mean"]), what="mean over prompts")
    assert torch.equal(arg.cpu(), torch.from_numpy(g["argmax"])), "winner index (first on ties)"
    assert int(arg[0, 1]) in (0, 1, 2, 3) and not bool((arg[:, 1] == 1).any()), "rows 4 and 5 of y are equal: index 0 must win over 1"
    dx, dy = K.pairwise_cosine_max_bwd(x, y, cosv, torch.from_numpy(g["dmax"]).to(DEV), arg, xn, yn)
    close(dx, torch.from_numpy(g["dx"]), what="max-cosine dx")
    close(dy, torch.from_numpy(g["dy"]), what="max-cosine dy")
    # autograd surface + ragged sizes (B not a multiple of the 4 rows per block, one prompt per group = plain cosine)
    xs, ys = rnd(7, 128, seed=3).to(DEV).requires_grad_(True), rnd(3, 128, seed=4).to(DEV).requires_grad_(True)
    m1, a1, _ = Fh.pairwise_cosine_max(xs, ys, 3)
    close(m1, ref_loss.pairwise_cosine_similarity(xs.detach().cpu(), ys.detach().cpu()), what="Pg = 1 is the plain cosine")
    close(a1, m1.detach(), what="mean of one")
    m1.sum().backward()
    xr, yr = xs.detach().cpu().requires_grad_(True), ys.detach().cpu().requires_grad_(True)
    ref_loss.pairwise_cosine_max(xr, yr, 3)[0].sum().backward()
    close(xs.grad, xr.grad, what="dx via autograd"); close(ys.grad, yr.grad, what="dy via autograd")
    # similarity map: HIP GEMV + host gaussian == the reference's _get_similarity_map_from_embeddings output, then its resize
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.vlp import ImageTextInferenceEngine as E
    pat, txt = torch.from_numpy(g["patches"]).to(DEV), torch.from_numpy(g["text"]).to(DEV)
    raw = K.patch_similarity(pat.reshape(-1, 128), txt[0])
    close(raw, (torch.from_numpy(g["patches"]).reshape(-1, 128) @ torch.from_numpy(g["text"]).T).reshape(-1), what="patch . text")
    sim = E._get_similarity_map_from_embeddings(pat, txt)
    assert sim.shape == (15, 15) and float((sim - torch.from_numpy(g["sim"])).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        K.patch_similarity(pat.reshape(-1, 128), txt[0, :64])


def test_pairwise_cosine_bce_eval(golden_dir):
    B, D, C = 70, 128, 5
    x, y = rnd(B, D).requires_grad_(True), rnd(2 * C, D, seed=1).requires_grad_(True)
    labels = (rnd(B, C, seed=2) > 0.5).float()
    cos = ref_loss.pairwise_cosine_similarity(x, y)
    logits = cos[:, 0::2] - cos[:, 1::2]
    loss = F.binary_cross_entropy_with_logits(logits, labels)
    loss.backward()
    cd, xn, yn = K.pairwise_cosine_fwd(x.detach().to(DEV), y.detach().to(DEV))
    close(cd, cos, what="cosine fwd")
    lg, dcos, ls = K.bce_posneg_fwd_bwd(cd, labels.to(DEV))
    close(lg, logits, what="logits")
    assert abs(ls.item() - loss.item()) < 1e-6
    dx, dy = K.pairwise_cosine_bwd(x.detach().to(DEV), y.detach().to(DEV), cd, dcos, xn, yn)
    close(dx, x.grad, what="cosine dx")
    close(dy, y.grad, what="cosine dy")
    # class-incremental column subset (Trainer.py:701-714): labels[:, :3] is a strided view
    lg3, _, ls3 = K.bce_posneg_fwd_bwd(cd[:, :6].contiguous(), labels.to(DEV)[:, :3])
    assert abs(ls3.item() - F.binary_cross_entropy_with_logits(logits[:, :3], labels[:, :3]).item()) < 1e-6
    sc, pr = K.eval_score(cd)
    close(sc, (cos[:, 0::2] + 1) / 2, what="score")
    assert torch.equal(pr.cpu(), (cos[:, 0::2] > cos[:, 1::2]).float())
    e = rnd(10 * 4, D, seed=5)
    close(K.group_mean_fwd(e.to(DEV), 10, 4), e.view(10, 4, D).mean(1), what="group mean")
    gm = rnd(10, D, seed=6)
    close(K.group_mean_bwd(gm.to(DEV), 10, 4), (gm / 4)[:, None].expand(10, 4, D).reshape(40, D), what="group mean bwd")


# ------------------------------------------------------------------------------------------------ optimiser
def test_adam_sgd_weight_reset():
    n = 65920 + 3
    p0, gs = rnd(n), [rnd(n, seed=s) for s in range(1, 4)]
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3)
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step, g in enumerate(gs, 1):
        p.grad = g.clone()
        opt.step()
        K.adam_fused(pd, g.to(DEV), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, step)
        close(pd, p, tol=1e-6, what=f"adam step {step}")
    q = p0.clone().requires_grad_(True)
    so = torch.optim.SGD([q], lr=0.1)
    q.grad = gs[0].clone()
    so.step()
    qd = p0.to(DEV)
    K.sgd(qd, gs[0].to(DEV), 0.1)
    close(qd, q, tol=1e-6, what="sgd")
    new, old = rnd(5000, seed=7), rnd(5000, seed=8)
    ref, cnt = ref_step.weight_reset(new, old, 0.3)
    nd = new.to(DEV)
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    K.weight_reset(nd, old.to(DEV), 0.3, counters)
    assert torch.equal(nd.cpu(), ref)
    assert counters[0].item() == cnt


# ------------------------------------------------------------------------------------------------ 256x256 tile
def test_wide_kernel_policy_at_step_shapes():
    """The library's own policy (`cxrk_gemm_wide_tile`) sends the big BERT shapes to the 256x256 LDS-DMA kernel and keeps small /
    narrow ones on the 128x128-class tiles (both kernels are checked on every test shape through the `wide` fixture)."""
    lib = _cxr_lib.load()
    assert lib.cxrk_gemm_wide_tile(32768, 3072, 768, 1, 3) == 1 and lib.cxrk_gemm_wide_tile(32768, 768, 3072, 1, 0) == 1
    assert lib.cxrk_gemm_wide_tile(1024, 128, 768, 1, 0) == 0 and lib.cxrk_gemm_wide_tile(200, 136, 72, 1, 0) == 0
    sk = lib.cxrk_gemm_wgrad_splitk(768, 3072, 32768, 1)
    assert sk > 1 and lib.cxrk_gemm_wide_tile(768, 3072, 32768, sk, 0) == 1
    assert lib.cxrk_gemm_wgrad_splitk(768, 3072, 32768, 0) >= 1
