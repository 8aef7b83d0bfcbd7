"""The window-resident weight gradient of the 3x3 / stride 1 / 64 -> 64 convolutions on planes operands (csrc/conv_halo_wgrad.h)
against an fp64 CPU conv2d backward: shapes that exercise every ring / range / border case, the tap masks in isolation, both
dispatch paths in one process (bit-identical), and the workspace contract.  Tolerances: those of test_planes_conv_bn_relu_fwd_bwd (3e-4 / 2e-2 /
3e-4 of the tensor maximum)."""
import ctypes
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
C = KO = 64
EPS = 1e-5
SWITCH = "CXRK_HALO_WGRAD"
# (N, H, W): a single pixel (only the centre tap is live); 15 pixels, less than one K-tile; rows longer than a K-tile with
# M % 32 != 0; 294 K-tiles in 33 slabs, the last one shorter, rings crossing image boundaries; the widest row taken;
# every pixel a border pixel and every K-tile spanning eight images
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 5, 33), (3, 56, 56), (5, 7, 58), (40, 2, 2)]
TOL_DW, TOL_DG, TOL_DB = 3e-4, 2e-2, 3e-4


def _rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def _case(N, H, W):
    """Inputs (fp32, CPU) and the fp64 reference of one shape, computed once and shared by the tests; never modified."""
    seed = 7919 * N + 101 * H + W
    x, dy = _rnd(N, C, H, W, seed=seed), _rnd(N, KO, H, W, seed=seed + 1)
    w = _rnd(KO, C, 3, 3, seed=seed + 2) / math.sqrt(9 * C)
    gamma, rm = 1 + 0.1 * _rnd(KO, seed=seed + 3), 0.1 * _rnd(KO, seed=seed + 4)
    rv = 0.5 + _rnd(KO, seed=seed + 5).abs()
    rstd = 1.0 / torch.sqrt(rv + EPS)
    sc = gamma * rstd
    x64, dy64, w64 = x.double(), dy.double(), w.double()
    dw_raw = torch.nn.grad.conv2d_weight(x64, w.shape, dy64, padding=1)                 # [Ko, C, 3, 3]
    z = F.conv2d(x64, w64, padding=1)
    ref = {
        "dw": (sc.double().view(-1, 1, 1, 1) * dw_raw).permute(0, 2, 3, 1).contiguous(),   # [Ko, 3, 3, C]
        "dg": (dy64 * (z - rm.double().view(1, -1, 1, 1)) * rstd.double().view(1, -1, 1, 1)).sum((0, 2, 3)),
        "db": dy64.sum((0, 2, 3)),
    }
    return {"x": x, "dy": dy, "w_cl": w.permute(0, 2, 3, 1).contiguous(), "sc": sc, "rstd": rstd, "rm": rm, "ref": ref}


def _device_inputs(N, H, W):
    c = _case(N, H, W)
    xp = K.split_planes(c["x"].permute(0, 2, 3, 1).contiguous().to(DEV))
    dyp = K.split_planes(c["dy"].permute(0, 2, 3, 1).contiguous().to(DEV))
    sumdy = K.colsum(dyp.view(N * H * W, KO), torch.empty(KO, device=DEV))
    return c, xp, dyp, sumdy, [c[k].to(DEV) for k in ("w_cl", "sc", "rstd", "rm")]


def _run(N, H, W, dw=None, accumulate=False):
    c, xp, dyp, sumdy, (w_cl, sc, rstd, rm) = _device_inputs(N, H, W)
    if dw is None:
        dw = torch.empty(KO, 3, 3, C, device=DEV)
    dg, db = (torch.zeros(KO, device=DEV) for _ in range(2))
    K.conv_bwd_params_pl(xp, dyp, w_cl, sc, rstd, rm, sumdy, dw, dg, db, accumulate, N, H, W, C, KO, 3, 3, 1, 1)
    return dw, dg, db


def _err(a, b):
    a, b = a.detach().double().cpu(), b.double()
    assert a.shape == b.shape and bool(torch.isfinite(a).all())
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _check(out, ref, what):
    dw, dg, db = out
    errs = (_err(dw, ref["dw"]), _err(dg, ref["dg"]), _err(db, ref["db"]))
    print(f"{what}: rel-to-max err dW {errs[0]:.3e} dgamma {errs[1]:.3e} dbeta {errs[2]:.3e}")
    assert errs[0] < TOL_DW and errs[1] < TOL_DG and errs[2] < TOL_DB, (what, errs)


@pytest.fixture
def switch():
    """Sets CXRK_HALO_WGRAD for the library (which reads it on every call) and restores it."""
    old = os.environ.get(SWITCH)

    def set_(v):
        if v is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = v
    yield set_
    set_(old)


# ---- 1. shapes and values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_values_accumulate_and_determinism(shape, switch):
    switch(None)
    ref = _case(*shape)["ref"]
    first = _run(*shape)
    _check(first, ref, f"window wgrad {shape}")
    second = _run(*shape)
    for a, b in zip(first, second):
        assert torch.equal(a, b), f"{shape}: a second call is not bit-identical"
    base = _rnd(KO, 3, 3, C, seed=5).to(DEV)
    dw, dg, db = _run(*shape, dw=base.clone(), accumulate=True)
    exp = {"dw": base.double().cpu() + ref["dw"], "dg": ref["dg"], "db": ref["db"]}
    _check((dw, dg, db), exp, f"window wgrad {shape} accumulate")


# ---- 2. tap masks in isolation ----------------------------------------------------------------------------------------------
def _onehot_pixels(N, H, W):
    """Corner, edge and interior pixels, the first / last pixel of an image in the middle of the batch, and the pixels on either
    side of K-tile boundaries (multiples of 32 in the flattened index): at most 64, one per filter."""
    pts = {(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (N - 1, H - 1, W - 1), (0, 0, W // 2), (0, H // 2, 0), (0, H // 2, W - 1),
           (N - 1, H - 1, W // 2), (N // 2, H // 2, W // 2), (N // 2, 0, 0), (N // 2, H - 1, W - 1)}
    M = N * H * W
    for m in (31, 32, 63, 64, M // 2 // 32 * 32 - 1, M // 2 // 32 * 32, (M - 1) // 32 * 32 - 1, (M - 1) // 32 * 32, M - 1):
        if 0 <= m < M:
            pts.add((m // (H * W), (m // W) % H, m % W))
    return sorted(pts)[:KO]


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 33), (3, 56, 56), (40, 2, 2)])
def test_tap_masks_exact(shape, switch):
    """x = 1 everywhere, dy a one-hot (pixel i in filter i): dW[i][r][s][:] is exactly 1 where the neighbour exists, exactly 0
    where it does not — exact in split-bf16 too."""
    switch(None)
    N, H, W = shape
    pts = _onehot_pixels(N, H, W)
    dy = torch.zeros(N, H, W, KO)
    exp = torch.zeros(KO, 3, 3, C)
    for i, (n, h, w) in enumerate(pts):
        dy[n, h, w, i] = 1.0
        for r in range(3):
            for s in range(3):
                if 0 <= h + r - 1 < H and 0 <= w + s - 1 < W:
                    exp[i, r, s, :] = 1.0
    xp = K.split_planes(torch.ones(N, H, W, C, device=DEV))
    dyp = K.split_planes(dy.to(DEV))
    ones, zeros = torch.ones(KO, device=DEV), torch.zeros(KO, device=DEV)
    sumdy = K.colsum(dyp.view(N * H * W, KO), torch.empty(KO, device=DEV))
    dw, dg, db = torch.empty(KO, 3, 3, C, device=DEV), torch.empty(KO, device=DEV), torch.empty(KO, device=DEV)
    K.conv_bwd_params_pl(xp, dyp, torch.zeros(KO, 3, 3, C, device=DEV), ones, ones, zeros, sumdy, dw, dg, db, False, N, H, W, C, KO, 3, 3, 1, 1)
    assert torch.equal(dw.cpu(), exp), f"{shape}: tap masks differ at {(dw.cpu() != exp).nonzero()[:8].tolist()}"


# ---- 3. both paths in one process -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 56, 56), (2, 5, 33), (40, 2, 2)])
def test_both_paths_one_process(shape, switch):
    ref = _case(*shape)["ref"]
    label = _lib.load().cxrk_last_launch_label
    switch("0")
    gemm = _run(*shape)
    assert label() == b"gemm_pw_kernel<Pw64x256,DmaDenseMC,DmaConvIm2colMC>"   # the paths are bit-identical: only this tells them apart
    _check(gemm, ref, "implicit GEMM (CXRK_HALO_WGRAD=0)")
    switch("1")
    window = _run(*shape)
    assert label() == b"conv3x3_wgrad_window_kernel"
    _check(window, ref, "window kernel (CXRK_HALO_WGRAD=1)")
    # the window kernel writes the implicit GEMM's split-K slabs with every element's products added in the same order, and
    # the slab reduction is shared: more than "equal up to summation order", the two paths agree bit for bit
    for a, b, what in zip(window, gemm, ("dW", "dgamma", "dbeta")):
        assert torch.equal(a, b), f"{shape}: {what} of the two paths differs"


def test_more_slabs_than_cus_bit_identical(switch):
    """(26, 56, 56): 81 536 pixels are 284 split-K slabs, more than the 256 CUs: the slabs beyond one per CU are computed by three
    blocks each (one filter row per block).  No CPU reference at this size: the implicit GEMM, checked above and in
    test_kernels_gpu.py, is the reference, and the result must equal it bit for bit."""
    N, H, W = 26, 56, 56
    assert _lib.load().cxrk_gemm_wgrad_splitk(KO, 9 * C, N * H * W, 1) > torch.cuda.get_device_properties(0).multi_processor_count
    xp = K.split_planes(_rnd(N, H, W, C, seed=11).to(DEV))
    dyp = K.split_planes(_rnd(N, H, W, KO, seed=12).to(DEV))
    sumdy = K.colsum(dyp.view(N * H * W, KO), torch.empty(KO, device=DEV))
    w_cl = (_rnd(KO, 3, 3, C, seed=13) / 24).to(DEV)
    sc, rstd, rm = (1 + 0.1 * _rnd(KO, seed=14)).to(DEV), (1 + 0.1 * _rnd(KO, seed=15)).abs().to(DEV), (0.1 * _rnd(KO, seed=16)).to(DEV)
    outs = {}
    for path in ("0", "1"):
        switch(path)
        dw, dg, db = torch.empty(KO, 3, 3, C, device=DEV), torch.empty(KO, device=DEV), torch.empty(KO, device=DEV)
        K.conv_bwd_params_pl(xp, dyp, w_cl, sc, rstd, rm, sumdy, dw, dg, db, False, N, H, W, C, KO, 3, 3, 1, 1)
        outs[path] = (dw, dg, db)
    for a, b, what in zip(outs["1"], outs["0"], ("dW", "dgamma", "dbeta")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{what} of the two paths differs"


# ---- 4. workspace query -----------------------------------------------------------------------------------------------------
def _window_need_bytes(N, H, W):
    M = N * H * W
    sk = _lib.load().cxrk_gemm_wgrad_splitk(KO, 9 * C, M, 1)         # the kernel writes the split-K slabs of the implicit GEMM
    if sk > 1:
        kchunk = -(-(-(-M // sk)) // 32) * 32
        sk = -(-M // kchunk)
    return (max(sk, 1) * KO * 9 * C + KO * ((9 * C + 63) // 64)) * 4


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_query_covers_the_window_kernel(shape, switch):
    """The query covers both paths; the entry point runs on exactly the queried bytes (pre-filled with NaN) and refuses a
    misaligned workspace with -1."""
    switch(None)
    N, H, W = shape
    lib = _lib.load()
    nbytes = lib.cxrk_conv_wgrad_ws_bytes(N, H, W, C, KO, 3, 3, 1, 1)
    assert nbytes >= _window_need_bytes(N, H, W)
    c, xp, dyp, sumdy, (w_cl, sc, rstd, rm) = _device_inputs(N, H, W)
    ws = torch.full((nbytes // 4 + 64,), float("nan"), device=DEV)
    assert ws.data_ptr() % 256 == 0
    dw, dg, db = torch.empty(KO, 3, 3, C, device=DEV), torch.empty(KO, device=DEV), torch.empty(KO, device=DEV)

    def call(ws_ptr, ws_bytes):
        return lib.cxrk_conv_bn_act_bwd_params_pl(xp.ptr(), xp.plane, dyp.ptr(), dyp.plane, w_cl.data_ptr(), sc.data_ptr(), rstd.data_ptr(),
                                                  rm.data_ptr(), sumdy.data_ptr(), dw.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, N, H, W, C, KO,
                                                  3, 3, 1, 1, ctypes.c_void_p(ws_ptr), ws_bytes, K._stream())
    for path in ("0", "1"):
        switch(path)
        assert call(ws.data_ptr() + 4, nbytes) == -1, "a misaligned workspace must be refused"
        assert call(ws.data_ptr(), nbytes) == 0
        _check((dw, dg, db), c["ref"], f"{shape} on exactly the queried workspace, {SWITCH}={path}")
        ws.fill_(float("nan"))
