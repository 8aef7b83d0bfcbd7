"""The device code the host dispatch selects only for odd widths, unaligned operands and small heads, which no other module launches:

  * the per-column branch of `gemm_epilogue64_f32` (csrc/gemm_core.h, `ep.vec == false`): N % 4 != 0, a row stride of C / R / aux / C2
    that is no multiple of 4, or C / R / aux / C2 / bias not 16-byte aligned;
  * `ln_fwd_kernel<false>` / `<true>` (csrc/bert.hip): H % 8 != 0 or an operand not 16-byte aligned;
  * `ln_bwd_kernel`: H % 4 != 0 or an operand not 16-byte aligned;
  * attention at head sizes other than 32 and 64 (LDS rows of dH + 4 floats), one head, one sequence.

Every reference is float64 on the CPU from the same seeded float32 inputs; the measure is that of tests/test_kernels_gpu.py's close()
(max |err| / max |ref|) with its bounds: 2e-5 fp32 GEMM / LayerNorm / attention forward, 5e-5 attention backward, at least 3e-4 in
split-bf16 mode.  Each test first asserts, on its own inputs, the condition the dispatch reads, so a later change of shapes cannot
move it back onto the vector path unnoticed.  Pitched and offset outputs sit between tests/memguard.py guards."""
import math

import pytest
import torch
import torch.nn.functional as F

import memguard as MG
from kernel_refs import attention_reference, ln_bwd_ref, ln_case, ln_fwd_ref, rnd

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
BF = torch.bfloat16


def _split() -> bool:
    return _cxr_lib.get_precision() == "split_bf16"


def tl(t: float) -> float:
    """the bound close() of tests/test_kernels_gpu.py applies: `t` of the output scale, at least 3e-4 in split-bf16 mode"""
    return max(t, 3e-4) if _split() else t


def close(got, ref, tol=2e-5, what=""):
    err = MG.rel_err(got.detach().float(), ref)
    bound = tl(tol)
    assert err < bound, f"{what}: rel-to-max err {err:.3e} (tol {bound})"


def dev(t):
    return t.contiguous().to(DEV)


def offset_by_one(t):
    """device copy of `t` that starts one float into its storage (4 bytes off the allocator's alignment)"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def pitched(t, ld):
    """device copy of a 2-D tensor with row pitch ld inside guards; returns (view, guard object to check afterwards)"""
    g = MG.Guarded(t.shape, t.dtype, ld=ld, device=DEV, name="pitched input").load(t)
    return g.t, g


def guarded(call, outs, ref, tol):
    """one run into sentinel-filled outputs between guards: guards / padding intact, every element written, values"""
    return MG.run_contract(call, outs, ref, tol, module=K, device=DEV, runs=("session",))


def contract(call, outs, ref, tol):
    """session workspace, then an exact-size workspace poisoned with NaN and with +-1e30: bit-identical, guards intact, values"""
    return MG.run_contract(call, outs, ref, tol, module=K, device=DEV)


def aligned16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def gelu_grad64(a):
    return 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------------------------------------ GEMM, scalar epilogue
NT_ODD = [(33, 5, 8),          # a single column block, cut inside the first float4
          (1, 1, 4),           # one row, one column
          (200, 130, 72),      # ragged in both tile dimensions, two column tiles of the 128-class tile
          (70, 63, 40),        # the column below a 64-wide wave sub-tile ...
          (70, 65, 40),        # ... and the one above it
          (300, 7, 132)]       # a ragged M tile (256-row tile of the N <= 64 dispatch) with odd N


@pytest.mark.parametrize("M,N,Kd", NT_ODD)
def test_gemm_nt_odd_width(M, N, Kd):
    """y = act(alpha x w^T + bias + residual) at N % 4 != 0: every feature the per-column branch re-implements (bias, residual,
    pre-activation copy, ReLU, GELU, accumulate = residual aliasing the output, alpha).  Bound 2e-5 (test_gemm_nt_epilogues)."""
    assert N % 4 != 0 and Kd % 4 == 0                      # prep_epilogue: vec = (N % 4 == 0) && ...
    x, w, b, r = rnd(M, Kd), rnd(N, Kd, seed=1), rnd(N, seed=2), rnd(M, N, seed=3)
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(r)
    lin = x.double() @ w.double().T
    pre = lin + b.double()
    t = tl(2e-5)
    guarded(lambda o: K.linear_fwd(xd, wd, out=o["y"]), {"y": Out((M, N))}, {"y": lin}, t)
    guarded(lambda o: K.linear_fwd(xd, wd, bias=bd, act=K.ACT_RELU, residual=rd, out=o["y"]), {"y": Out((M, N))},
            {"y": torch.relu(pre + r.double())}, t)
    guarded(lambda o: K.linear_fwd(xd, wd, bias=bd, act=K.ACT_GELU, preact_out=o["pre"], out=o["y"]), {"y": Out((M, N)), "pre": Out((M, N))},
            {"y": F.gelu(pre), "pre": pre}, t)
    guarded(lambda o: K.gemm(xd, wd, o["y"], M, N, Kd, False, True, accumulate=True), {"y": Out((M, N), init=r)},
            {"y": r.double() + lin}, t)
    guarded(lambda o: K.gemm(xd, wd, o["y"], M, N, Kd, False, True, bias=bd, alpha=-0.75), {"y": Out((M, N))},
            {"y": -0.75 * lin + b.double()}, t)


GM, GN, GK = 200, 136, 72        # NT: y[GM, GN] = x[GM, GK] w[GN, GK]^T;  NN: dx[GM, GK] = dy[GM, GN] w[GN, GK]


def test_gemm_nt_aligned_width_one_operand_off():
    """N = 136 (a multiple of 4): `vec` is cleared by exactly one operand at a time -- the output's row stride, the residual's address,
    the pre-activation copy's row stride, the bias address.  Every output has a pitch, so its padding columns are checked.  2e-5."""
    M, N, Kd = GM, GN, GK
    assert N % 4 == 0
    x, w, b, r = rnd(M, Kd), rnd(N, Kd, seed=1), rnd(N, seed=2), rnd(M, N, seed=3)
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(r)
    lin = x.double() @ w.double().T
    pre = lin + b.double()
    t = tl(2e-5)

    def odd_out(o):                                          # output rows N + 1 floats apart
        assert o["y"].stride(0) % 4 != 0 and aligned16(o["y"], bd, rd)
        K.linear_fwd(xd, wd, bias=bd, act=K.ACT_RELU, residual=rd, out=o["y"])
    guarded(odd_out, {"y": Out((M, N), ld=N + 1)}, {"y": torch.relu(pre + r.double())}, t)

    def odd_out_acc(o):                                      # the same with the output as its own residual
        assert o["y"].stride(0) % 4 != 0 and aligned16(o["y"])
        K.gemm(xd, wd, o["y"], M, N, Kd, False, True, accumulate=True, alpha=0.5)
    guarded(odd_out_acc, {"y": Out((M, N), ld=N + 1, init=r)}, {"y": r.double() + 0.5 * lin}, t)

    r1 = offset_by_one(r)                                    # residual one float into its buffer

    def off_res(o):
        assert o["y"].stride(0) % 4 == 0 and aligned16(o["y"], bd) and r1.data_ptr() % 16 != 0 and r1.stride(0) % 4 == 0
        K.linear_fwd(xd, wd, bias=bd, residual=r1, out=o["y"])
    guarded(off_res, {"y": Out((M, N), ld=N + 4)}, {"y": pre + r.double()}, t)

    def odd_pre(o):                                          # pre-activation copy with an odd row stride
        assert o["pre"].stride(0) % 4 != 0 and o["y"].stride(0) % 4 == 0 and aligned16(o["y"], o["pre"], bd)
        K.linear_fwd(xd, wd, bias=bd, act=K.ACT_GELU, preact_out=o["pre"], out=o["y"])
    guarded(odd_pre, {"y": Out((M, N), ld=N + 4), "pre": Out((M, N), ld=N + 1)}, {"y": F.gelu(pre), "pre": pre}, t)

    b1 = offset_by_one(b)                                    # bias one float into its buffer

    def off_bias(o):
        assert o["y"].stride(0) % 4 == 0 and aligned16(o["y"]) and b1.data_ptr() % 16 != 0
        K.linear_fwd(xd, wd, bias=b1, act=K.ACT_RELU, out=o["y"])
    guarded(off_bias, {"y": Out((M, N), ld=N + 4)}, {"y": torch.relu(pre)}, t)


def test_gemm_nn_aligned_width_one_operand_off():
    """The data-gradient form at Kd = 72 output columns: output row stride Kd + 1; residual one float in; the ReLU-mask and the GELU'
    source with row stride Kd + 3.  2e-5 (test_gemm_nn_tn)."""
    M, N, Kd = GM, GN, GK
    assert Kd % 4 == 0 and N % 4 == 0
    dy, w, aux, r = rnd(M, N), rnd(N, Kd, seed=1), rnd(M, Kd, seed=3), rnd(M, Kd, seed=4)
    dyd, wd, auxd = dev(dy), dev(w), dev(aux)
    g64 = dy.double() @ w.double()
    t = tl(2e-5)

    def odd_out(o):
        assert o["dx"].stride(0) % 4 != 0 and aligned16(o["dx"], auxd) and auxd.stride(0) % 4 == 0
        K.linear_bwd_data(dyd, wd, aux=auxd, auxmode=K.AUX_RELU_MASK, out=o["dx"])
    guarded(odd_out, {"dx": Out((M, Kd), ld=Kd + 1)}, {"dx": g64 * (aux > 0)}, t)

    r1 = offset_by_one(r)

    def off_res(o):
        assert o["dx"].stride(0) % 4 == 0 and aligned16(o["dx"]) and r1.data_ptr() % 16 != 0
        K.linear_bwd_data(dyd, wd, residual=r1, out=o["dx"])
    guarded(off_res, {"dx": Out((M, Kd), ld=Kd + 4)}, {"dx": g64 + r.double()}, t)

    auxp, g = pitched(aux, Kd + 3)
    for mode, ref in ((K.AUX_RELU_MASK, g64 * (aux > 0)), (K.AUX_GELU_GRAD, g64 * gelu_grad64(aux.double()))):
        def odd_aux(o):
            assert auxp.stride(0) % 4 != 0 and aligned16(o["dx"], auxp) and o["dx"].stride(0) % 4 == 0
            K.linear_bwd_data(dyd, wd, aux=auxp, auxmode=mode, out=o["dx"])
        guarded(odd_aux, {"dx": Out((M, Kd), ld=Kd + 4)}, {"dx": ref}, t)
    g.check()


@pytest.mark.parametrize("epilogue", ["plain", "bias_relu"])
def test_gemm_nt_odd_width_one_gflop(epilogue):
    """2 M N K = 1.077e9 >= 2^30: in split-bf16 mode `launch_gemm` sends fp32 operands to `gemm_x3_kernel`, which ends in the same
    per-column branch at N = 1027.  2e-5 in fp32 mode, 3e-4 in split-bf16 mode."""
    M, N, Kd = 4096, 1027, 128
    assert N % 4 != 0 and 2.0 * M * N * Kd >= 2 ** 30
    x, w, b = rnd(M, Kd), rnd(N, Kd, seed=1), rnd(N, seed=2)
    xd, wd, bd = dev(x), dev(w), dev(b)
    lin = x.double() @ w.double().T
    if epilogue == "plain":
        guarded(lambda o: K.linear_fwd(xd, wd, out=o["y"]), {"y": Out((M, N))}, {"y": lin}, tl(2e-5))
    else:
        guarded(lambda o: K.linear_fwd(xd, wd, bias=bd, act=K.ACT_RELU, out=o["y"]), {"y": Out((M, N))}, {"y": torch.relu(lin + b.double())},
                tl(2e-5))


def test_conv_bwd_data_sums_need_aligned_operands():
    """The fused column sums of the data gradient exist in the 16-byte epilogue only.  cxrk_conv_bn_act_bwd_data used to accept `sums`
    with a dx / residual / relu_src that is 4 bytes off: the per-column branch then stored dx correctly and left every sum ZERO.
    Now such a call is a bad argument and writes nothing; without `sums` the same operands run the per-column branch (5e-5, the
    convolution data-gradient bound of test_conv_bn_relu_fwd_bwd)."""
    N, H, W, C, Ko, R, stride, pad = 2, 12, 12, 64, 64, 3, 1, 1
    args = (N, H, W, C, Ko, R, R, stride, pad)
    dy, w = rnd(N, H, W, Ko, seed=2), rnd(Ko, R, R, C, seed=1, scale=1.0 / math.sqrt(C * R * R))
    add, src = rnd(N, H, W, C, seed=3), rnd(N, H, W, C, seed=6)
    dyd, wd, addd, srcd = dev(dy), dev(w), dev(add), dev(src)
    g64 = torch.nn.grad.conv2d_input((N, C, H, W), w.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2), stride=stride,
                                     padding=pad).permute(0, 2, 3, 1)
    full = (g64 + add.double()) * (src > 0)
    nan = torch.full((N, H, W, C), float("nan"))
    for which in ("dx", "residual", "relu_src"):
        dx = offset_by_one(nan) if which == "dx" else dev(nan)
        res = offset_by_one(add) if which == "residual" else addd
        rs = offset_by_one(src) if which == "relu_src" else srcd
        assert sum(t.data_ptr() % 16 != 0 for t in (dx, res, rs)) == 1
        sums = torch.full((C,), float("nan"), device=DEV)
        with pytest.raises(ValueError, match="cxrk code -1"):
            K.conv_bwd_data(dyd, wd, res, rs, dx, *args, sums=sums)
        assert bool(torch.isnan(dx).all()) and bool(torch.isnan(sums).all()), f"{which} off by 4 bytes: written although refused"
        K.conv_bwd_data(dyd, wd, res, rs, dx, *args)            # no sums: the per-column branch serves it
        close(dx, full, tol=5e-5, what=f"dgrad, {which} off by 4 bytes")
    sums = torch.empty(C, device=DEV)                           # all aligned: served, and the sums are those of dx
    dx = torch.empty(N, H, W, C, device=DEV)
    K.conv_bwd_data(dyd, wd, addd, srcd, dx, *args, sums=sums)
    close(sums, full.reshape(-1, C).sum(0), tol=5e-5, what="fused column sums")


# ------------------------------------------------------------------------------------------------ LayerNorm forward, scalar
def _ln_inputs(rows, H):
    return rnd(rows, H), rnd(rows, H, seed=1), 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)


def _check_ln_fwd(got, ref, tol=2e-5, what=""):
    for name, g, r in zip(("y", "xhat", "rstd"), got, ref):
        if g is not None:
            close(g, r, tol=tol, what=f"{what} {name}")


@pytest.mark.parametrize("rows", [1, 5, 77])             # 5: a last block with one of its 4 waves at work
@pytest.mark.parametrize("H", [4, 60, 100, 1020, 1023])
def test_ln_fwd_scalar(rows, H):
    """`ln_fwd_kernel<false>`: y, xhat and rstd of LayerNorm(x [+ res]) with eps = 1e-12, with and without the saved statistics.  2e-5
    (test_layernorm_fwd_bwd)."""
    assert H % 8 != 0                                       # ln_vec8_ok
    x, r, g, b = _ln_inputs(rows, H)
    xd, rd, gd, bd = dev(x), dev(r), dev(g), dev(b)
    for res in (r, None):
        s = x.double() + (res.double() if res is not None else 0.0)
        ref = ln_fwd_ref(s, g.double(), b.double(), 1e-12)
        for save in (True, False):
            y, xhat, rstd = K.residual_ln_fwd(xd, rd if res is not None else None, gd, bd, 1e-12, save=save)
            assert (xhat is None) == (not save) and (rstd is None) == (not save)
            _check_ln_fwd((y, xhat, rstd), ref, what=f"res={res is not None} save={save}")


@pytest.mark.parametrize("H", [100, 60])
def test_embed_ln_fwd_scalar(H):
    """`ln_fwd_kernel<true>`: word[ids] + pos[token % L] + type, repeated ids, L smaller than the position table.  2e-5."""
    assert H % 8 != 0
    V, L, B, NPOS = 50, 7, 3, 16
    word, pos, typ = rnd(V, H), rnd(NPOS, H, seed=1), rnd(2, H, seed=2)
    g, b = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(5))
    ids[1] = ids[0]                                         # a repeated sequence
    ids[2, 1:4] = ids[2, 0]                                 # a repeated id inside one
    assert L < NPOS
    s = word[ids].double().view(B * L, H) + pos[:L].double().repeat(B, 1) + typ[0].double()
    ref = ln_fwd_ref(s, g.double(), b.double(), 1e-12)
    got = K.embed_ln_fwd(dev(ids), dev(word), dev(pos), dev(typ[0]), dev(g), dev(b), 1e-12, L)
    _check_ln_fwd(got, ref, what="embed ln")
    with pytest.raises(ValueError):                         # planes output needs the 8-column kernel
        K.embed_ln_fwd(dev(ids), dev(word), dev(pos), dev(typ[0]), dev(g), dev(b), 1e-12, L, out_planes=True)


def test_ln_fwd_width_limits():
    """H = 1024 is the widest row (16 columns per lane, vector kernel); H = 1025 is refused."""
    rows = 5
    x, r, g, b = _ln_inputs(rows, 1024)
    got = K.residual_ln_fwd(dev(x), dev(r), dev(g), dev(b), 1e-12)
    _check_ln_fwd(got, ln_fwd_ref(x.double() + r.double(), g.double(), b.double(), 1e-12), what="H=1024")
    x, r, g, b = _ln_inputs(rows, 1025)
    with pytest.raises(ValueError):
        K.residual_ln_fwd(dev(x), dev(r), dev(g), dev(b), 1e-12)
    dy, xhat, rstd, gamma, _ = ln_case(rows, 1025)
    with pytest.raises(ValueError):
        K.residual_ln_bwd(dev(dy), dev(xhat), dev(rstd), dev(gamma), torch.empty(1025, device=DEV), torch.empty(1025, device=DEV))


@pytest.mark.parametrize("which", ["x", "gamma"])
def test_ln_fwd_scalar_at_aligned_width(which):
    """H = 128 through the scalar kernel: x, or gamma, starts one float into its storage.  2e-5."""
    rows, H = 77, 128
    x, r, g, b = _ln_inputs(rows, H)
    xd = offset_by_one(x) if which == "x" else dev(x)
    gd = offset_by_one(g) if which == "gamma" else dev(g)
    rd, bd = dev(r), dev(b)
    assert H % 8 == 0 and sum(t.data_ptr() % 16 != 0 for t in (xd, rd, gd, bd)) == 1
    got = K.residual_ln_fwd(xd, rd, gd, bd, 1e-12)
    _check_ln_fwd(got, ln_fwd_ref(x.double() + r.double(), g.double(), b.double(), 1e-12), what=f"{which} off by 4 bytes")


def test_ln_fwd_planes_refused_at_odd_width():
    """Planes output exists in the 8-column kernel only: at H = 100 the call is a bad argument and writes nothing."""
    rows, H = 4, 100
    assert H % 8 != 0 and (rows * H) % 8 == 0               # the plane stride is fine: the width alone refuses
    x, r, g, b = _ln_inputs(rows, H)
    xd, rd, gd, bd = dev(x), dev(r), dev(g), dev(b)
    with pytest.raises(ValueError):
        K.residual_ln_fwd(xd, rd, gd, bd, 1e-12, out_planes=True)
    y = K.Planes(torch.full((2, rows, H), float("nan"), dtype=BF, device=DEV))
    xhat, rstd = torch.full((rows, H), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
    rc = _cxr_lib.load().cxrk_residual_ln_fwd(xd.data_ptr(), rd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-12, rows, H, y.ptr(), y.plane,
                                              xhat.data_ptr(), rstd.data_ptr(), K._stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t.float()).all()) and bool(torch.isnan(xhat).all()) and bool(torch.isnan(rstd).all())


# float32 PyTorch-CPU F.layer_norm on the rows of test_ln_fwd_large_common_offset against the float64 reference (max |err| / max |ref|)
LN_OFFSET_TORCH_F32_ERR = {100: 1.41e-4, 128: 1.88e-4}


@pytest.mark.parametrize("H", [100, 128])                  # the scalar and the vector kernel
def test_ln_fwd_large_common_offset(H):
    """Rows with a large common offset, x = 300 + 0.1 randn: the case a one-pass variance (E[x^2] - mean^2: 9e4 - 9e4 in float32) loses;
    mirrors test_train_mode_batchnorm_kernels.  The float64 reference uses the float32 inputs as given.  Here 2e-5 is below what
    float32 can give: the mean of 100 values near 300 is known to ~1e-5, a tenth of a thousandth of the spread 0.1.  float32
    PyTorch-CPU F.layer_norm on these rows is 1.41e-4 (H = 100) / 1.88e-4 (H = 128) off the float64 reference; the bound for y and xhat
    is 4 times that.  rstd does not see the shift of the mean (it enters the variance squared) and keeps 2e-5."""
    rows = 77
    gen = torch.Generator().manual_seed(H)
    x = 300 + 0.1 * torch.randn(rows, H, generator=gen)
    g, b = 1 + 0.1 * torch.randn(H, generator=gen), 0.1 * torch.randn(H, generator=gen)
    assert (H % 8 != 0) == (H == 100)
    ref = ln_fwd_ref(x.double(), g.double(), b.double(), 1e-12)
    y, xhat, rstd = K.residual_ln_fwd(dev(x), None, dev(g), dev(b), 1e-12)
    tol = 4 * LN_OFFSET_TORCH_F32_ERR[H]
    close(y, ref[0], tol=tol, what="y")
    close(xhat, ref[1], tol=tol, what="xhat")
    close(rstd, ref[2], what="rstd")


# ------------------------------------------------------------------------------------------------ LayerNorm backward, scalar
def _ln_bwd_contracts(rows, H, dyd, dy, xhat, rstd, gamma, add):
    dx64, dg64, db64 = ln_bwd_ref(dy.double(), xhat.double(), rstd.double(), gamma.double())
    xd, rd, gd, addd = dev(xhat), dev(rstd), dev(gamma), dev(add)
    base = rnd(H, seed=9)
    t = tl(2e-5)
    vec = {"dg": Out((H,)), "db": Out((H,))}
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], out=o["dx"]), dict(vec, dx=Out((rows, H))),
             {"dx": dx64, "dg": dg64, "db": db64}, t)
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], dx_add=addd, out=o["dx"]), dict(vec, dx=Out((rows, H))),
             {"dx": dx64 + add.double(), "dg": dg64, "db": db64}, t)
    contract(lambda o: K.residual_ln_bwd(dyd, xd, rd, gd, o["dg"], o["db"], accumulate=True, out=o["dx"]),
             {"dg": Out((H,), init=base), "db": Out((H,), init=-2 * base), "dx": Out((rows, H))},
             {"dx": dx64, "dg": base.double() + dg64, "db": -2 * base.double() + db64}, t)


@pytest.mark.parametrize("H", [6, 63, 101, 1022])
@pytest.mark.parametrize("rows", [1, 15, 17, 77, 16400])   # 16 400: rows_per becomes 17 and the block count is recomputed
def test_ln_bwd_scalar(rows, H):
    """`ln_bwd_kernel` under the memory contract of test_residual_ln_bwd (exact, poisoned workspace; guarded outputs): plain, with
    dx_add, and accumulated into non-zero dgamma / dbeta.  2e-5."""
    assert H % 4 != 0                                       # ln_bwd_vec_ok
    dy, xhat, rstd, gamma, add = ln_case(rows, H)
    _ln_bwd_contracts(rows, H, dev(dy), dy, xhat, rstd, gamma, add)


def test_ln_bwd_scalar_at_aligned_width():
    """H = 128 through the scalar kernel: dy starts one float into its storage."""
    rows, H = 77, 128
    dy, xhat, rstd, gamma, add = ln_case(rows, H)
    dyd = offset_by_one(dy)
    assert H % 4 == 0 and dyd.data_ptr() % 16 != 0
    _ln_bwd_contracts(rows, H, dyd, dy, xhat, rstd, gamma, add)


def test_ln_bwd_refusals_at_odd_width():
    """The fused column sums and the planes output exist in the vector kernel only: bad argument at H = 63, nothing written."""
    rows, H = 4, 63
    assert H % 4 != 0 and (rows * H) % 4 == 0
    dy, xhat, rstd, gamma, _ = ln_case(rows, H)
    dyd, xd, rd, gd = dev(dy), dev(xhat), dev(rstd), dev(gamma)

    def nans(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)

    dg, db, dx, s = nans(H), nans(H), nans(rows, H), nans(H)
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.residual_ln_bwd(dyd, xd, rd, gd, dg, db, out=dx, dxsum=s)
    dxp = K.Planes(nans(2, rows, H, dtype=BF))
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.residual_ln_bwd(dyd, xd, rd, gd, dg, db, out=dxp)
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.residual_ln_bwd(dyd, xd, rd, gd, dg, db, out_planes=True)
    torch.cuda.synchronize()
    for name, v in (("dgamma", dg), ("dbeta", db), ("dx", dx), ("dxsum", s), ("dx planes", dxp.t.float())):
        assert bool(torch.isnan(v).all()), f"{name}: written although refused"


# ------------------------------------------------------------------------------------------------ attention, small heads
ATTN = [(dH, L, 2, 3) for dH in (4, 12, 60) for L in (1, 17, 64, 65, 130)]         # short form up to L = 64, tiled above
ATTN += [(dH, L, 1, 1) for dH in (4, 12, 60) for L in (17, 65)]                    # one sequence, one head


@pytest.mark.parametrize("dH,L,B,nH", ATTN)
def test_attention_small_heads(dH, L, B, nH):
    """Forward and backward at head sizes whose LDS rows (dH + 4 floats) and float4 loop bounds differ from those of 32 / 64, ragged
    key mask of test_attention_fwd_bwd, fp32 and planes outputs; the backward into guarded outputs through the exact, poisoned dS
    workspace of the tiled form.  Forward 2e-5, backward 5e-5 against float64 autograd."""
    assert dH not in (32, 64) and dH % 4 == 0 and 4 <= dH <= 64 and 1 <= L <= 512
    qkv, mask, gc, ctx, dqkv = attention_reference(B, L, nH, dH, True, dtype=torch.float64)
    qd, md, gd = dev(qkv), dev(mask), dev(gc)
    cd, probs = K.attn_fwd(qd, md, B, L, nH, dH)
    close(cd, ctx, what="attn fwd")
    close(probs.sum(-1), torch.ones(B, nH, L, dtype=torch.float64), what="rows of probs sum to 1")
    cp, _ = K.attn_fwd(qd, md, B, L, nH, dH, save_probs=False, out_planes=True)
    close(cp.float(), ctx, what="attn fwd -> planes")
    W3 = 3 * nH * dH
    contract(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=o["dqkv"]), {"dqkv": Out((B * L, W3))}, {"dqkv": dqkv}, tl(5e-5))
    contract(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=K.Planes(o["dqkv"])), {"dqkv": Out((2, B * L, W3), BF)}, {"dqkv": dqkv},
             tl(5e-5))


@pytest.mark.parametrize("dH,L", [(6, 17), (68, 17), (64, 513)])
def test_attention_refuses_unsupported_shapes(dH, L):
    """dH % 4 != 0, dH > 64 and L > 512 raise before anything is launched."""
    B, nH = 1, 2
    qd = dev(rnd(B * L, 3 * nH * dH))
    md = torch.ones(B, L, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="cxrk code -4"):
        K.attn_fwd(qd, md, B, L, nH, dH)
    with pytest.raises(ValueError, match="cxrk code -4"):
        K.attn_fwd(qd, md, B, L, nH, dH, out_planes=True)
    probs = torch.zeros(B, nH, L, L, device=DEV)
    gd = dev(rnd(B * L, nH * dH, seed=2))
    out = torch.full((B * L, 3 * nH * dH), float("nan"), device=DEV)
    with pytest.raises(ValueError, match="cxrk code -4"):
        K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "written although refused"
