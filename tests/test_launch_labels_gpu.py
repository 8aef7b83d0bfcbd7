"""What the library says it launched (`cxrk_last_launch_label` / `_count` / `_split_bf16`, csrc/gemm_dispatch.h) against literals
read off the tile ladders the call sites carried before the policy existed once: one library call at a tiny shape per case.
Kernel instantiations are written as scripts/pmc_summary_key.py abbreviates rocprofv3's names.  The process-wide tile mode is
the default (CXRK_WIDE=1) except where a case sets mode 2 itself."""
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"


def _f32(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(DEV)


def _pl(*shape):
    return K.split_planes(_f32(*shape))


def _pw(cfg, la, lb):
    return f"gemm_pw_kernel<{cfg},{la},{lb}>"


def _said(label, count=1, split=1):
    lib = _lib.load()
    got = (lib.cxrk_last_launch_label().decode(), lib.cxrk_last_launch_count(), lib.cxrk_last_launch_split_bf16())
    assert got == (label, count, split), got


@pytest.fixture(autouse=True)
def _policy_mode():
    lib = _lib.load()
    old = lib.cxrk_set_wide_mode(1)
    try:
        yield
    finally:
        lib.cxrk_set_wide_mode(old)


# ---- dense on planes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,cfg", [(128, 128, "Pw128"), (128, 64, "Pw256x64"), (64, 128, "Pw64x256"),
                                     (64, 64, "Pw256x64")])   # the N <= 64 rule fires before the M <= 64 rule
def test_dense_planes_nt(M, N, cfg):
    K.linear_fwd_pl(_pl(M, 64), _pl(N, 64))
    _said(_pw(cfg, "DmaDenseKC", "DmaDenseKC"))


def test_dense_planes_nn():
    K.linear_bwd_data_pl(_pl(128, 64), _pl(64, 128))
    _said(_pw("Pw128", "DmaDenseKC", "DmaDenseMC"))


def test_dense_planes_tn():
    K.linear_bwd_weight_pl(_pl(64, 128), _pl(64, 128), torch.empty(128, 128, device=DEV))
    _said(_pw("Pw128", "DmaDenseMC", "DmaDenseMC"))


def test_dense_planes_nt_wide_mode_2():
    lib = _lib.load()
    old = lib.cxrk_set_wide_mode(2)
    try:
        K.linear_fwd_pl(_pl(128, 64), _pl(128, 64))
        _said(_pw("Pw256", "DmaDenseKC", "DmaDenseKC"))
    finally:
        lib.cxrk_set_wide_mode(old)


# ---- dense on fp32 (under 1 GFLOP: the exact-fp32 mainloop in either precision mode) -----------------------------------------------
@pytest.mark.parametrize("M,N,tile", [(128, 128, "2,2"), (128, 64, "4,1"), (64, 128, "1,4")])
def test_dense_f32_nt(M, N, tile):
    K.gemm(_f32(M, 64), _f32(N, 64), torch.empty(M, N, device=DEV), M, N, 64, False, True)
    _said(f"gemm_f32_kernel<DenseKC,DenseKC,{tile}>", split=0)


# ---- convolution forward -----------------------------------------------------------------------------------------------------
def _fwd(x, w, N, H, W, C, Ko, R, stride, pad):
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    K.conv_fwd_pl(x, w, torch.zeros(Ko, device=DEV), None, K.Planes.empty(N, Ho, Wo, Ko, device=DEV), None, N, H, W, C, Ko, R, R, stride, pad,
                  False)


@pytest.mark.parametrize("HW,C,Ko,R,label", [
    (8, 64, 128, 1, _pw("Pw128", "DmaConvIm2colKC", "DmaDenseKC")),
    (4, 64, 128, 1, _pw("Pw128", "DmaConvIm2colKC", "DmaDenseKC")),      # 16 rows: the forward never takes 64x256
    (8, 128, 64, 1, _pw("Pw256x64", "DmaConvIm2colKC", "DmaDenseKC")),
    (8, 64, 64, 3, "conv3x3_halo_kernel<fwd>"),
])
def test_conv_fwd(HW, C, Ko, R, label):
    _fwd(_pl(1, HW, HW, C), _pl(Ko, R * R * C), 1, HW, HW, C, Ko, R, 1, R // 2)
    _said(label)


def test_conv_fwd_stem():
    _fwd(_f32(1, 16, 16, 4), _f32(64, 7, 7, 4), 1, 16, 16, 4, 64, 7, 2, 3)
    _said("gemm_f32_kernel<ConvIm2colKC,DenseKC,4,1>", split=0)


# ---- convolution data gradient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Ko,R,stride,label,count", [
    (128, 128, 1, 1, _pw("Pw128", "DmaConvDgradKC", "DmaConvFilterMC"), 1),
    (64, 128, 1, 1, _pw("Pw256x64", "DmaConvDgradKC", "DmaConvFilterMC"), 1),
    (64, 64, 3, 1, "conv3x3_halo_kernel<dgrad>", 1),
    (128, 128, 3, 2, _pw("Pw128", "DmaConvDgradS2KC", "DmaConvFilterS2MC"), 4),     # one launch per output-parity class
    (128, 128, 1, 2, _pw("Pw128", "DmaConvDgradS2KC", "DmaConvFilterS2MC"), 1),     # only the even / even class has a tap
])
def test_conv_dgrad(C, Ko, R, stride, label, count):
    H = W = 8
    pad = R // 2
    Ho = (H + 2 * pad - R) // stride + 1
    K.conv_bwd_data_pl(_pl(1, Ho, Ho, Ko), _pl(Ko, R * R * C), None, None, K.Planes.empty(1, H, W, C, device=DEV), 1, H, W, C, Ko, R, R,
                       stride, pad)
    _said(label, count)


# ---- convolution weight gradient ---------------------------------------------------------------------------------------------
def _wgrad(C, Ko, R):
    H = W = 8
    vec = [torch.ones(Ko, device=DEV) for _ in range(4)]
    out = [torch.empty(Ko, R, R, C, device=DEV), torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)]
    K.conv_bwd_params_pl(_pl(1, H, W, C), _pl(1, H, W, Ko), _f32(Ko, R, R, C), *vec, *out, False, 1, H, W, C, Ko, R, R, 1, R // 2)


@pytest.mark.parametrize("C,Ko,R,label", [
    (128, 128, 1, _pw("Pw128", "DmaDenseMC", "DmaConvIm2colMC")),
    (128, 64, 1, _pw("Pw64x256", "DmaDenseMC", "DmaConvIm2colMC")),
    (64, 128, 1, _pw("Pw128", "DmaDenseMC", "DmaConvIm2colMC")),        # 64 columns: the weight gradient never takes 256x64
    (64, 64, 3, "conv3x3_wgrad_window_kernel"),
])
def test_conv_wgrad(C, Ko, R, label):
    _wgrad(C, Ko, R)
    _said(label)


def test_conv_wgrad_window_switched_off():
    old = os.environ.get("CXRK_HALO_WGRAD")
    os.environ["CXRK_HALO_WGRAD"] = "0"      # read by the library on every call
    try:
        _wgrad(64, 64, 3)
        _said(_pw("Pw64x256", "DmaDenseMC", "DmaConvIm2colMC"))
    finally:
        if old is None:
            del os.environ["CXRK_HALO_WGRAD"]
        else:
            os.environ["CXRK_HALO_WGRAD"] = old
