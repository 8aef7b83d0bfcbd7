"""The stem fused with its max-pool (csrc/stem_pool.hip; include/cxrk.h, cxrk_stem_pool_fwd / cxrk_stem_pool_bwd_sums).

Forward: pooled planes and winner bytes of the one-kernel form against `conv_fwd_pl(relu=True)` + `maxpool_fwd_pl`, as bit patterns.
Backward: the BatchNorm sums taken in pooled space against a float64 sum of the gradient tensor `maxpool_bwd_pl` writes.
Both entry points under guards and poison, the launch labels, and the image encoder with the switch CXRK_STEM_POOL on against off.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import image_encoder as IE  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet  # noqa: E402
import memguard as MG  # noqa: E402
from nonfinite_ref import inject  # noqa: E402

DEV = "cuda"
C, KO, R, STRIDE, PAD = 4, 64, 7, 2, 3
# (N, H, W): the existing stem test's size; stem 15 x 15 (last window row / column clipped); non-square, stem 19 x 13; pooled
# 24 x 20 = four 7-row and three 8-column tiles with ragged edges in both directions
SHAPES = [(2, 32, 32), (3, 30, 30), (1, 38, 26), (3, 96, 80)]
# 2 * 50176 * 64 * 196 = 1.26 GFLOP: from 1 GFLOP on the split-bf16 mode runs the bf16 mainloop (the smaller shapes take the
# exact-fp32 one in either mode), so this is the size at which the fused kernel takes its other path; 8 x 7 full tiles per image
BIG = (4, 224, 224)
# the column-sum tolerance of tests/test_kernels_gpu.py (`close(K.colsum(...), ...)`, max |diff| / max |ref|, fp32 accumulation)
COLSUM_TOL = 2e-5


def _hw(H, W):
    Hs, Ws = (H + 2 * PAD - R) // STRIDE + 1, (W + 2 * PAD - R) // STRIDE + 1
    return Hs, Ws, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1


def _inputs(N, H, W, kind="uniform", seed=0):
    g = torch.Generator().manual_seed(seed + 7 * N + H + 3 * W)
    x = torch.rand(N, H, W, C, generator=g)
    x[..., 3] = 0                                # the zero-padded fourth channel
    w = torch.randn(KO, R, R, C, generator=g) * 0.1
    w[..., 3] = 0
    shift = torch.randn(KO, generator=g) * 0.1
    if kind == "zero_block":                     # whole windows tie: at 0 where the channel's shift is negative, at the shift elsewhere
        x[:, H // 8: H - H // 8, W // 8: W - W // 8] = 0
    elif kind == "all_zero":                     # a shift so negative that every output is 0: every window ties, the first valid tap wins
        shift = torch.full((KO,), -1e3)
    return x, w, shift


def _unfused(x, w, shift):
    N, H, W, _ = x.shape
    Hs, Ws, _, _ = _hw(H, W)
    y = K.Planes.empty(N, Hs, Ws, KO, device=DEV)
    K.conv_fwd_pl(x, w, shift, None, y, None, N, H, W, C, KO, R, R, STRIDE, PAD, True)
    split = _lib.load().cxrk_last_launch_split_bf16()
    return K.maxpool_fwd_pl(y) + (split,)


def _fused(x, w, shift, want_idx=True):
    N, H, W, _ = x.shape
    out = K.stem_pool_fwd_pl(x, w, shift, N, H, W, C, KO, R, R, STRIDE, PAD, want_idx)
    assert out is not None
    return out + (_lib.load().cxrk_last_launch_split_bf16(),)


def _bits(p: K.Planes):
    return p.t.view(torch.int16)


def _assert_same(x, w, shift, what):
    x, w, shift = x.to(DEV), w.to(DEV), shift.to(DEV)
    ry, ri, rsplit = _unfused(x, w, shift)
    y, idx, split = _fused(x, w, shift)
    assert split == rsplit, (what, "the fused kernel must run the mainloop the unfused stem runs", split, rsplit)
    assert tuple(y.shape) == tuple(ry.shape) and tuple(idx.shape) == tuple(ri.shape)
    nhi = int((_bits(y)[0] != _bits(ry)[0]).sum()); nlo = int((_bits(y)[1] != _bits(ry)[1]).sum()); ni = int((idx != ri).sum())
    print(f"{what}: differing hi {nhi} lo {nlo} idx {ni} of {idx.numel()}")
    assert (nhi, nlo, ni) == (0, 0, 0), what
    y2, none, _ = _fused(x, w, shift, want_idx=False)          # the no-grad form: idx = null
    assert none is None and torch.equal(_bits(y2), _bits(ry)), what
    return ry, ri


@pytest.mark.usefixtures("precision")
@pytest.mark.parametrize("shape,kind", [(s, k) for s in SHAPES for k in ("uniform", "zero_block", "all_zero")] + [(BIG, "uniform")])
def test_forward_is_bit_identical_to_conv_then_pool(shape, kind):
    ry, ri = _assert_same(*_inputs(*shape, kind=kind), what=f"{shape} {kind}")
    if kind == "all_zero":
        assert float(ry.float().abs().max()) == 0.0
        # first valid tap: (0,0) inside, (0,1) in the first column, (1,0) in the first row, (1,1) in the corner
        assert int(ri[0, 0, 0, 0]) == 4 and int(ri[0, 0, 1, 0]) == 3 and int(ri[0, 1, 0, 0]) == 1 and int(ri[0, 1, 1, 0]) == 0
    if kind == "zero_block":
        assert int((ri == 0).sum()) > ri.numel() // 8       # many windows tie, and their first tap wins


def test_forward_precision_mode_of_the_large_shape(precision):
    """split-bf16 mode runs the bf16 mainloop at the large shape only; fp32 mode never"""
    lib = _lib.load()
    for shape, want in ((SHAPES[0], 0), (BIG, int(precision == "split_bf16"))):
        x, w, shift = (t.to(DEV) for t in _inputs(*shape))
        assert _fused(x, w, shift)[2] == want, (shape, precision)
        assert lib.cxrk_last_launch_count() == 1


@pytest.mark.usefixtures("precision")
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", ["pixel", "tap"])
def test_forward_nonfinite_matches_the_unfused_pair(where, value):
    """a NaN / +Inf / -Inf in one image pixel (it reaches the 4 x 4 stem pixels around it, and through the pool their windows) or in
    one filter tap (a whole channel): the same bits as convolution + pool, which tests/nonfinite_ref.py pins against torch"""
    x, w, shift = _inputs(2, 32, 32, seed=3)
    if where == "pixel":
        x = inject(inject(x, (0, 9, 11, 1), value), (1, 31, 0, 2), value)
    else:
        w = inject(w, (5, 3, 2, 0), value)
    ry, _ = _assert_same(x, w, shift, what=f"{where} {value}")
    v = ry.float()
    assert not bool(torch.isfinite(v).all()) or value == float("-inf")     # -Inf pixels may be cut off by the ReLU
    assert bool(torch.isfinite(v[..., 6]).any())                            # and the rest of the tensor stays finite


@pytest.mark.usefixtures("precision")
@pytest.mark.parametrize("shape", SHAPES)
def test_bwd_sums_match_the_sum_of_the_pool_gradient(shape):
    """sums = column sums of the tensor maxpool_bwd_pl writes for the same (g, idx, pooled), summed in float64; pooled has about half
    its entries <= 0 (their windows are masked by the stem ReLU)"""
    N, H, W = shape
    Hs, Ws, Hp, Wp = _hw(H, W)
    x, w, shift = (t.to(DEV) for t in _inputs(*shape))
    _, idx, _ = _fused(x, w, shift)                                          # valid winners for this geometry
    gen = torch.Generator().manual_seed(11 + H)
    g = K.split_planes(torch.randn(N, Hp, Wp, KO, generator=gen).to(DEV))
    pooled_f = torch.randn(N, Hp, Wp, KO, generator=gen)
    pooled_f[0, 0, 0, :8] = 0.0
    pooled = K.split_planes(pooled_f.to(DEV))
    assert 0.4 < float((pooled_f <= 0).float().mean()) < 0.6
    dstem = K.maxpool_bwd_pl(g, idx, pooled, Hs, Ws)
    ref = dstem.double().sum(dim=(0, 1, 2)).cpu()
    s1 = K.stem_pool_bwd_sums(g, pooled)
    s2 = K.stem_pool_bwd_sums(g, pooled)
    err = float((s1.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{shape}: pooled-space sums against float64 sum of dstem: {err:.3e}")
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert err < COLSUM_TOL, err


# ------------------------------------------------------------------------------------------------ memory contract
def test_memory_contract_forward(precision):
    N, H, W = 3, 30, 30
    _, _, Hp, Wp = _hw(H, W)
    x, w, shift = (t.to(DEV) for t in _inputs(N, H, W))
    lib = _lib.load()
    ry, ri, _ = _unfused(x, w, shift)

    def call(o, with_idx=True):
        y = o["y"]
        rc = lib.cxrk_stem_pool_fwd(x.data_ptr(), w.data_ptr(), shift.data_ptr(), y.data_ptr(), y.stride(0), o["idx"].data_ptr() if with_idx else None,
                                    N, H, W, C, KO, R, R, STRIDE, PAD, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cxrk_stem_pool_fwd")

    outs = {"y": MG.Out((2, N, Hp, Wp, KO), torch.bfloat16, gap=64), "idx": MG.Out((N, Hp, Wp, KO), torch.uint8)}
    got = MG.run_contract(call, outs, device=DEV, runs=("session", "nan"))
    assert torch.equal(got["y"].bits(), _bits(ry)) and torch.equal(got["idx"].bits(), ri)
    # idx = null: the winners are not touched
    outs = {"y": MG.Out((2, N, Hp, Wp, KO), torch.bfloat16), "idx": MG.Out((N, Hp, Wp, KO), torch.uint8, written=False)}
    y = outs["y"].make("y", DEV, None, MG.BYTE_SENTINELS[0]); i = outs["idx"].make("idx", DEV, None, MG.BYTE_SENTINELS[0])
    before = i.backing.clone()
    call({"y": y.t, "idx": i.t}, with_idx=False)
    y.check()
    assert torch.equal(i.backing, before) and torch.equal(y.bits(), _bits(ry))
    # another geometry is refused, nothing launched
    before = y.backing.clone()
    rc = lib.cxrk_stem_pool_fwd(x.data_ptr(), w.data_ptr(), shift.data_ptr(), y.t.data_ptr(), y.t.stride(0), None, N, H, W, C, KO, 5, 5, STRIDE, 2,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -4 and torch.equal(y.backing, before) and lib.cxrk_last_launch_count() == 0


def test_memory_contract_bwd_sums(precision):
    N, Hp, Wp = 3, 24, 20
    rows = N * Hp * Wp
    gen = torch.Generator().manual_seed(5)
    g = K.split_planes(torch.randn(N, Hp, Wp, KO, generator=gen).to(DEV))
    pooled = K.split_planes(torch.randn(N, Hp, Wp, KO, generator=gen).to(DEV))
    lib = _lib.load()
    need = lib.cxrk_colsum_ws_bytes(rows, KO)
    assert need == lib.cxrk_colsum_ws_bytes(rows, KO) == ((rows + 511) // 512) * KO * 4     # the query is pure

    def call(o, short_by=0):
        ws = K.workspace(need, g.device)
        rc = lib.cxrk_stem_pool_bwd_sums(g.ptr(), g.plane, pooled.ptr(), o["sums"].data_ptr(), N, Hp, Wp, KO, ws.data_ptr(), (need - short_by) if short_by else ws.numel() * 4,
                                         torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "cxrk_stem_pool_bwd_sums")

    ref = (g.float().double() * (pooled.t[0].float() > 0)).sum(dim=(0, 1, 2)).cpu()
    outs = {"sums": MG.Out((KO,))}
    MG.run_contract(call, outs, reference={"sums": ref}, tol=COLSUM_TOL, device=DEV)
    MG.refuses_short_workspace(call, outs, device=DEV)
    MG.refuses_misaligned_workspace(call, outs, device=DEV)
    # one byte short of the exact size: refused, nothing written
    s = outs["sums"].make("sums", DEV, None, MG.BYTE_SENTINELS[0])
    before = s.backing.clone()
    with pytest.raises(RuntimeError, match="cxrk code -2"):
        call({"sums": s.t}, short_by=1)
    torch.cuda.synchronize()
    assert torch.equal(s.backing, before) and lib.cxrk_last_launch_count() == 0


def test_launch_labels(precision):
    """the labels are the kernels' rocprofv3 names as scripts/pmc_summary_key.py abbreviates them"""
    lib = _lib.load()
    x, w, shift = (t.to(DEV) for t in _inputs(*SHAPES[0]))
    y, idx, _ = _fused(x, w, shift)
    assert lib.cxrk_last_launch_label() == b"stem_pool_fwd_kernel<false>" and lib.cxrk_last_launch_count() == 1
    K.stem_pool_bwd_sums(y, y)
    assert lib.cxrk_last_launch_label() == b"stem_pool_sums_partial_kernel" and lib.cxrk_last_launch_count() == 1
    if precision == "split_bf16":
        x, w, shift = (t.to(DEV) for t in _inputs(*BIG))
        _fused(x, w, shift)
        assert lib.cxrk_last_launch_label() == b"stem_pool_fwd_kernel<true>"


# ------------------------------------------------------------------------------------------------ model level
def test_image_model_switch_on_against_off(monkeypatch):
    """ImageModel forward + backward, 2 images of 64 px, split-bf16: CXRK_STEM_POOL on against off.  Embeddings and every gradient
    are bit-identical (the stem's weight gradient included: it still reads the max-pool gradient in the unfused pixel order), except the
    stem's BatchNorm gamma / beta, whose sum over the pixels is taken in another order.  For those two, against a float64 reference
    built from the device's own max-pool gradient (beta: its sum; gamma: its sum against the normalised float64 convolution), the
    fused path's norm-relative error stays within twice the unfused path's and both under the suite's 1e-3.
    Measured (MI355X): gamma 1.031e-07 fused / 1.037e-07 unfused, beta 1.093e-07 / 5.962e-08."""
    model = get_biovil_resnet(None).eval()
    syn.fill_module_(model)
    model.to(DEV)
    x = syn.synthetic_images(2, 64, seed=33).to(DEV)
    cot = torch.randn(2, 128, generator=torch.Generator().manual_seed(6)).to(DEV)
    named = [(n, p) for n, p in model.named_parameters() if not n.startswith("encoder.encoder.fc.")]
    bufs = dict(model.named_buffers())

    def run(switch):
        monkeypatch.setenv("CXRK_STEM_POOL", switch)
        for _, p in named:
            p.grad = None
        dbg = {}
        monkeypatch.setattr(IE, "_debug", dbg)
        e = model(x)
        dec = IE.device_decisions(e.grad_fn.state)
        (e * cot).sum().backward()
        monkeypatch.setattr(IE, "_debug", None)
        with IE.capture_relu_decisions() as cap:
            model(x)
        return e.detach().clone(), {n: p.grad.detach().clone() for n, p in named}, dec, cap[0], dbg["ds"].double().cpu()

    old = _lib.get_precision()
    _lib.set_precision("split_bf16")
    try:
        e1, g1, d1, c1, ds1 = run("1")
        e0, g0, d0, c0, ds0 = run("0")
    finally:
        _lib.set_precision(old)
        for _, p in named:
            p.grad = None
    assert torch.equal(e1.view(torch.int32), e0.view(torch.int32))
    assert torch.equal(ds1, ds0)
    assert IE.count_decision_differences(d1, d0)["relu"] == 0 and IE.count_decision_differences(d1, d0)["pool_taps"] == 0
    assert torch.equal(d1["stem_pos"], d0["stem_pos"]) and torch.equal(d1["pool_taps"], d0["pool_taps"])
    assert len(c1) == len(c0) and all(torch.equal(a, b) for a, b in zip(c1, c0)) and torch.equal(c1.pool_taps, c0.pool_taps)
    bn = ("encoder.encoder.bn1.weight", "encoder.encoder.bn1.bias")
    diff = [n for n, _ in named if n not in bn and not torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32))]
    assert not diff, diff
    # float64 reference of the stem's BatchNorm gradients from the device's own max-pool gradient
    w64 = dict(named)["encoder.encoder.conv1.weight"].detach().double().cpu()
    z = F.conv2d(x.double().cpu(), w64, stride=STRIDE, padding=PAD)
    rm, rv = bufs["encoder.encoder.bn1.running_mean"].double().cpu(), bufs["encoder.encoder.bn1.running_var"].double().cpu()
    xhat = (z - rm[None, :, None, None]) / torch.sqrt(rv[None, :, None, None] + IE.BN_EPS)
    ds = ds1.permute(0, 3, 1, 2)
    ref = {bn[0]: (ds * xhat).sum(dim=(0, 2, 3)), bn[1]: ds.sum(dim=(0, 2, 3))}
    for n in bn:
        err1 = float((g1[n].double().cpu() - ref[n]).norm() / ref[n].norm())
        err0 = float((g0[n].double().cpu() - ref[n]).norm() / ref[n].norm())
        print(f"{n}: norm-relative error fused {err1:.3e} unfused {err0:.3e}")
        assert err1 < 1e-3 and err0 < 1e-3, (n, err1, err0)
        assert err1 <= 2 * err0, (n, err1, err0)
