"""The on-device image augmentation (csrc/augment.hip; include/cxrk.h, "augment") on the GPU: the two kernels against
the numpy restatement (tests/augment_ref.py) with bounds derived from the roundings they perform, the bit-exact equalities the
contract states, non-finite propagation, the refusals, and the model / trainer / data-parallel wiring."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

import augment_ref as AR
from memguard import Guarded
from incremental_multimodal_medical_learning_ii_amd import functional as Fh
from incremental_multimodal_medical_learning_ii_amd import kernels as K
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
from incremental_multimodal_medical_learning_ii_amd.augment import AugmentCall, AugmentSpec
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EPS = 2.0 ** -24              # unit roundoff of fp32: one correctly rounded operation has relative error <= EPS
FN_ULP = 2.0                  # HIP's documented maximum error of sinf / cosf / expf / logf is 1 or 2 ulp; 1 ulp <= 2 EPS relative
DIV_ULP = 2.5                 # fp32 division (2.5 ulp without the correctly-rounded option)
SPEC = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, contrast=0.2)
SEED = 0xC0FFEE_1234_5678


def _images(N, C, Hs, Ws, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, Hs, Ws, generator=g, dtype=torch.float32)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. parameter rows
def _param_bounds(spec, x64: np.ndarray, Ho: int, Wo: int) -> np.ndarray:
    """Bound [N, 8] on |device row - float64 row|, first order in EPS, from the operations csrc/augment.hip performs (written out in
    DESIGN.md 5.4): every fp32 operation contributes EPS relative, a library function 2 FN_ULP EPS relative, a division
    2 DIV_ULP EPS.  Nothing in here comes from an observed error."""
    N, C, Hs, Ws = x64.shape
    fn, dv = 2 * FN_ULP, 2 * DIV_ULP
    phimax = math.radians(spec.rotate_deg)
    trig = 3 * phimax + fn                                # |d cos|, |d sin| / EPS: phi carries 3 roundings (pi/180, two products)
    Lmax = max(abs(math.log(spec.zoom[0])), abs(math.log(spec.zoom[1])))
    r_z = 17 * Lmax + fn + dv                             # relative error of 1 / z / EPS: two logf, difference, product, sum, expf, division
    kmax = max(Ws / Wo, Hs / Ho) / spec.zoom[0]
    r_k = r_z + dv + 1                                    # (Ws / Wo) * (1 / z)
    e_a = kmax * (r_k + trig + 2)                         # the four matrix entries: k * cos * f
    D = max(Ho, Wo)
    e_o = (3 * spec.translate + 0.5) * D                  # ox, oy = (1/2 - Wo/2) - tx
    O = (0.5 + spec.translate) * D
    e_t = 2 * e_a * O + 2 * kmax * e_o + 6 * kmax * O + 0.5 * max(Hs, Ws)    # a02, a12: two products, two sums
    br, ct = spec.brightness, spec.contrast
    e_gain = (1 + ct) * (1 + 2 * br) + (1 + br) * (1 + 2 * ct) + (1 + br) * (1 + ct)
    # the mean: 256 threads sum E / 256 terms each in sequence, 6 shuffle levels, 4 wave sums, one division
    E = C * Hs * Ws
    absmean = np.abs(x64).mean(axis=(1, 2, 3))
    m = np.abs(x64.mean(axis=(1, 2, 3)))
    e_m = (math.ceil(E / 256) + 11) * absmean + m
    Mb = (1 + br) * m
    e_bias = Mb * (1 + 3 * ct) + ct * (1 + br) * e_m + ct * m * (1 + 2 * br) + 2 * ct * Mb
    out = np.empty((N, 8))
    out[:, [0, 1, 3, 4]] = e_a
    out[:, [2, 5]] = e_t
    out[:, 6] = e_gain
    out[:, 7] = e_bias
    return out * EPS * 1.01                               # 1.01: the second-order terms


@pytest.mark.parametrize("C", [1, 3])
def test_augment_params_match_numpy(C, capsys):
    N, Hs, Ws, off, counter = 5, 19, 23, 3, 11
    spec = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, contrast=0.2, out_size=(16, 12))
    x = _images(N, C, Hs, Ws, seed=C)
    g = Guarded((N, 8), device=DEV, name="params")
    K.augment_params(x.to(DEV), spec, SEED, counter, off, out=g.t)
    torch.cuda.synchronize()
    g.check()
    got = g.value().numpy()
    x64 = x.double().numpy()
    ref = AR.param_rows(spec, SEED, counter, off, N, Hs, Ws, x64.mean(axis=(1, 2, 3)))
    flips = AR.draws(spec, SEED, counter, np.arange(N) + off, 16, 12)["flip"]
    assert flips.any() and not flips.all()                                   # the case covers both signs
    # the uniform-derived decision: det of the linear part is negative iff the image is flipped
    assert np.array_equal((got[:, 0] * got[:, 4] - got[:, 1] * got[:, 3]) < 0, flips)
    bound = _param_bounds(spec, x64, 16, 12)
    err = np.abs(got - ref)
    with capsys.disabled():
        print(f"\n[augment_params C={C}] max err / bound per column: {np.round((err / bound).max(axis=0), 4).tolist()}; max abs err {err.max():.3e}")
    assert np.all(err <= bound), (err / bound).max()


def test_augment_params_identity_and_contrast_free_rows():
    N, Hs, Ws = 4, 19, 23
    x = _images(N, 3, Hs, Ws).to(DEV)
    rows = K.augment_params(x, AugmentSpec(), 1, 2, 3).cpu().numpy()
    assert np.array_equal(np.abs(rows), np.tile(np.array([1, 0, 0.5, 0, 1, 0.5, 1, 0], dtype=np.float32), (N, 1)))
    # contrast == 0: the source is not read (a poisoned source gives the same rows), and the bias is exactly 0
    spec = AugmentSpec(rotate_deg=20.0, brightness=0.3)
    a = K.augment_params(x, spec, 1, 2, 3)
    b = K.augment_params(torch.full_like(x, float("nan")), spec, 1, 2, 3)
    assert torch.equal(_bits(a), _bits(b)) and not bool(a[:, 7].any())


# ------------------------------------------------------------------------------------------------ 2. the sampler
def _sample_bound(x64: np.ndarray, rows: np.ndarray, Ho: int, Wo: int) -> np.ndarray:
    """Bound [N] on |device output - float64 sampler| with the SAME (device) parameter rows.  The device forms each coordinate with
    two fmaf and one subtraction: three roundings, of magnitudes |a01| yo + |a02|, |xs| and |xs - 1/2| (only coordinates within
    [-2, size + 2] reach a tap).  The zero-extended bilinear interpolant moves by at most (largest neighbour difference) per unit of
    coordinate.  The blend: four weights of three roundings each and four fmaf; then one fmaf for gain and bias."""
    N, C, Hs, Ws = x64.shape
    pad = np.pad(x64, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dx = np.abs(np.diff(pad, axis=3)).max(axis=(1, 2, 3))
    dy = np.abs(np.diff(pad, axis=2)).max(axis=(1, 2, 3))
    vmax = np.abs(x64).max(axis=(1, 2, 3))
    r = np.abs(rows.astype(np.float64))
    cx = EPS * (r[:, 1] * (Ho - 1) + r[:, 2] + 2 * (Ws + 2))
    cy = EPS * (r[:, 4] * (Ho - 1) + r[:, 5] + 2 * (Hs + 2))
    # (the inner fmaf of ys is a11 yo + a12; the outer adds a10 xo: its magnitude is the coordinate itself)
    blend = 16 * EPS * vmax
    return (r[:, 6] * (cx * dx + cy * dy + blend) + EPS * (r[:, 6] * vmax + r[:, 7])) * 1.01


@pytest.mark.parametrize("clamp01", [False, True])
@pytest.mark.parametrize("shape", [(1, 19, 23, 16, 12), (3, 19, 23, 16, 12), (3, 40, 40, 32, 32), (1, 40, 40, 32, 32)],
                         ids=["c1-19x23-16x12", "c3-19x23-16x12", "c3-40x40-32x32", "c1-40x40-32x32"])
def test_augment_nhwc_matches_float64_sampler(shape, clamp01, capsys):
    C, Hs, Ws, Ho, Wo = shape
    N = 5
    spec = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, contrast=0.2, out_size=(Ho, Wo),
                       clamp01=clamp01)
    x = _images(N, C, Hs, Ws, seed=7) * 0.5 + 0.5            # values on both sides of the clamp
    xd = x.to(DEV)
    rows = K.augment_params(xd, spec, SEED, 5, 2)
    g = Guarded((N, Ho, Wo, 4), device=DEV, name="augmented")
    K.augment_nhwc(xd, 4, rows, (Ho, Wo), clamp01, out=g.t)
    torch.cuda.synchronize()
    g.check()                                                 # guards intact, every element written (no sentinel left)
    got = g.value().numpy()
    assert not got[..., 3].any() and np.array_equal(np.signbit(got[..., 3]), np.zeros_like(got[..., 3], dtype=bool))
    rows_np = rows.cpu().double().numpy()
    x64 = x.double().numpy()
    ref = AR.sample(x64, rows_np, Ho, Wo, clamp01)
    bound = _sample_bound(x64, rows_np, Ho, Wo)[:, None, None, None]
    err = np.abs(got - ref)
    with capsys.disabled():
        print(f"\n[augment_nhwc {shape} clamp={clamp01}] max err {err.max():.3e}, max err / bound {(err / bound).max():.4f}")
    assert np.all(err <= bound)
    if C == 1:
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    if clamp01:
        assert got.min() == 0.0 and got.max() == 1.0
    inside = (AR.taps(rows_np, Hs, Ws, Ho, Wo)[2] > 0).any(axis=0)
    assert inside.mean() > 0.5                                # the maps look at the image, not past it


def test_cpad_8_pads_with_zeros():
    x = _images(2, 3, 9, 11).to(DEV)
    rows = K.augment_params(x, SPEC, SEED, 0)
    g = Guarded((2, 9, 11, 8), device=DEV, name="augmented")
    K.augment_nhwc(x, 8, rows, out=g.t)
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(_bits(g.t[..., :4]), _bits(K.augment_nhwc(x, 4, rows))) and not bool(g.t[..., 3:].any())


# ------------------------------------------------------------------------------------------------ 3. bit-exact equalities
@pytest.mark.parametrize("shape", [(3, 19, 23), (2, 64, 64), (1, 7, 130)])
def test_identity_spec_is_the_layout_transform(shape):
    N, Hs, Ws = shape
    x = _images(N, 3, Hs, Ws, seed=3).to(DEV)
    want = K.nchw_to_nhwc(x, 4)
    got = Fh.augment_images(x, AugmentSpec(), SEED, 4, row_offset=9)
    assert torch.equal(_bits(got), _bits(want))
    x1 = x[:, :1].contiguous()
    got1 = Fh.augment_images(x1, AugmentSpec(), SEED, 4)
    assert torch.equal(_bits(got1), _bits(K.nchw_to_nhwc(x1.expand(-1, 3, -1, -1).contiguous(), 4)))
    # with any spec one channel equals the replicated image (the mean of the replicated image is the same sum in another order,
    # so the contrast term is left out of this equality)
    spec = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2)
    a = Fh.augment_images(x1, spec, SEED, 4)
    b = Fh.augment_images(x1.expand(-1, 3, -1, -1).contiguous(), spec, SEED, 4)
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 4. shard independence
def test_shards_and_counters():
    x = _images(5, 3, 19, 23, seed=4).to(DEV)
    spec = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, contrast=0.2, out_size=(16, 12))
    full = Fh.augment_images(x, spec, SEED, 6)
    part = Fh.augment_images(x[2:].contiguous(), spec, SEED, 6, row_offset=2)
    assert torch.equal(_bits(full[2:]), _bits(part))
    assert not torch.equal(_bits(Fh.augment_images(x[2:].contiguous(), spec, SEED, 6, row_offset=0)), _bits(part))
    other = Fh.augment_images(x, spec, SEED, 7)
    assert not torch.equal(_bits(other), _bits(full))
    assert not torch.equal(_bits(Fh.augment_images(x, spec, SEED + 1, 6)), _bits(full))
    assert torch.equal(_bits(Fh.augment_images(x, spec, SEED, 6)), _bits(full))              # the state repeats it
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                               # the stream does not enter
        again = Fh.augment_images(x, spec, SEED, 6)
    s.synchronize()
    assert torch.equal(_bits(again), _bits(full))


# ------------------------------------------------------------------------------------------------ 5. non-finite values
@pytest.mark.parametrize("clamp01", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_one_nonfinite_pixel_stays_inside_its_footprint(bad, clamp01):
    N, Hs, Ws, Ho, Wo = 3, 19, 23, 16, 12
    spec = AugmentSpec(rotate_deg=30.0, translate=0.05, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, out_size=(Ho, Wo), clamp01=clamp01)
    x = _images(N, 3, Hs, Ws, seed=5)
    n, c, yy, xx = 1, 2, 9, 11
    x[n, c, yy, xx] = bad
    xd = x.to(DEV)
    rows = K.augment_params(xd, spec, SEED, 1)                 # contrast 0: the source does not enter the rows
    got = K.augment_nhwc(xd, 4, rows, (Ho, Wo), clamp01).cpu().numpy()
    w = AR.tap_weight_of(rows.cpu().double().numpy(), Hs, Ws, Ho, Wo, n, yy, xx)
    # the footprint comes from the float64 sampler.  A weight below 1e-4 may round to zero on the device (coordinates of magnitude
    # ~20 carry ~1e-5 of fp32 rounding): those outputs may be either; there are few of them.
    must, free = w > 1e-4, (w > 0) & (w <= 1e-4)
    assert must.sum() >= 1 and free.sum() <= 2
    nonfinite = ~np.isfinite(got)
    if not (clamp01 and bad == float("inf")):                  # the clamp turns +Inf into 1, as torch.clamp does
        assert nonfinite[n, :, :, c][must].all()
    allowed = np.zeros_like(nonfinite)
    allowed[n, :, :, c] = must | free
    assert not (nonfinite & ~allowed).any()                    # other images, channels, pixels and the padding stay finite
    if bad != bad:
        assert np.isnan(got[n, :, :, c][must]).all()           # with clamp01 too: the NaN survives


def test_zero_weight_taps_do_not_leak():
    """identity map: three of the four taps of every output have weight exactly zero, and they sit on real pixels"""
    x = _images(2, 3, 9, 11, seed=6)
    x[0, 1, 4, 5] = float("nan")
    x[1, 0, 0, 0] = float("inf")
    got = Fh.augment_images(x.to(DEV), AugmentSpec(), SEED, 0).cpu()
    bad = ~torch.isfinite(got)
    assert int(bad.sum()) == 2 and bool(bad[0, 4, 5, 1]) and bool(bad[1, 0, 0, 0])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    x = _images(2, 3, 9, 11).to(DEV)
    rows = K.augment_params(x, SPEC, SEED, 0)
    with pytest.raises(ValueError):
        K.augment_params(x.cpu(), SPEC, SEED, 0)
    with pytest.raises(ValueError):
        K.augment_nhwc(x.cpu(), 4, rows)
    with pytest.raises(ValueError):
        Fh.augment_images(x[:, :2].contiguous(), SPEC, SEED, 0)
    with pytest.raises(ValueError):
        Fh.augment_images(x.clone().requires_grad_(True), SPEC, SEED, 0)
    with pytest.raises(ValueError):
        K.augment_nhwc(x, 4, rows[:1].contiguous())
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.augment_nhwc(x, 3, rows)                                       # Cpad = 3
    buf = torch.zeros(2 * 9 * 11 * 4 + 4, dtype=torch.float32, device=DEV)
    off = buf[1:-3].view(2, 9, 11, 4)                                     # 4 bytes off the 16-byte alignment
    assert off.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.augment_nhwc(x, 4, rows, out=off)
    torch.cuda.synchronize()
    assert not bool(buf.any())                                           # refused before any launch
    pbuf = torch.zeros(2 * 8 + 1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="cxrk code -1"):
        K.augment_params(x, SPEC, SEED, 0, out=pbuf[1:].view(2, 8))
    lib = K._lib.load()
    y = torch.zeros(2, 9, 11, 4, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.cxrk_augment_nhwc(x.data_ptr(), rows.data_ptr(), y.data_ptr(), 2, 2, 9, 11, 9, 11, 4, 0, st) == -4    # 2 channels
    assert lib.cxrk_augment_params(None, 2, 3, 9, 11, 9, 11, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.2, 1, 0, 0, rows.data_ptr(), st) == -1   # contrast without a source
    assert lib.cxrk_augment_params(x.data_ptr(), 2, 3, 9, 11, 9, 11, 0.0, 0.0, 1.2, 0.8, 0.0, 0.0, 0.0, 1, 0, 0, rows.data_ptr(), st) == -1  # lo > hi
    torch.cuda.synchronize()
    assert not bool(y.any())


# ------------------------------------------------------------------------------------------------ 7. model level
def _image_model():
    im = get_biovil_resnet(None).eval()
    syn.fill_module_(im)
    return im.to(DEV)


def _emb_and_grads(im, x):
    for p in im.parameters():
        p.grad = None
    emb = im(x)
    w = torch.linspace(-1.0, 1.0, emb.numel(), device=emb.device).view_as(emb)
    (emb * w).sum().backward()
    torch.cuda.synchronize()
    return emb.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in im.parameters()]


@pytest.mark.usefixtures("precision")
@pytest.mark.parametrize("src,out_size,C", [((64, 64), None, 3), ((80, 72), (64, 64), 3), ((80, 72), (64, 64), 1)],
                         ids=["64x64", "80x72-to-64x64", "80x72-to-64x64-gray"])
def test_image_model_augments_exactly_as_the_preaugmented_images(src, out_size, C):
    spec = AugmentSpec(rotate_deg=10.0, translate=0.05, zoom=(0.9, 1.1), flip_p=0.5, brightness=0.2, contrast=0.2, out_size=out_size)
    x = torch.rand(2, C, *src, generator=torch.Generator().manual_seed(8)).to(DEV)
    im = _image_model()
    call = AugmentCall(spec, SEED, 3, 5)
    pre = K.nhwc_to_nchw(Fh.augment_images(x, spec, call.seed, call.counter, call.row_offset))[:, :3].contiguous()
    assert pre.shape == (2, 3, 64, 64)
    e_ref, g_ref = _emb_and_grads(im, pre)
    im.augment_call = call
    try:
        e_aug, g_aug = _emb_and_grads(im, x)
        with torch.no_grad():                                  # a no-grad forward never augments
            if C == 3 and out_size is None:
                e_nograd = im(x)
            else:
                e_nograd = None
                if C == 1:
                    with pytest.raises(ValueError):
                        im(x)
        with pytest.raises(ValueError):
            im(x.clone().requires_grad_(True))
    finally:
        im.augment_call = None
    assert bool(torch.isfinite(e_ref).all())
    assert torch.equal(_bits(e_aug), _bits(e_ref))
    assert sum(g is not None for g in g_ref) > 100
    for a, b in zip(g_aug, g_ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(_bits(a), _bits(b))
    if e_nograd is not None:
        with torch.no_grad():
            e_plain = im(x)
        assert torch.equal(_bits(e_nograd), _bits(e_plain)) and not torch.equal(_bits(e_plain), _bits(e_ref))
    if C == 1:
        with pytest.raises(ValueError):                        # one channel only while an augmentation expands it
            im(x)


# ------------------------------------------------------------------------------------------------ 8. trainer
def _joint_models():
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=32)
    tm, im = CXRBertModel(cfg).eval(), get_biovil_resnet(None).eval()
    syn.fill_module_(tm)
    syn.fill_module_(im)
    return im.to(DEV), tm.to(DEV)


def _batch(B=8, L=16):
    images = syn.synthetic_images(B, 64, seed=3)
    ids, mask = syn.synthetic_tokens(B, L, vocab=300, seed=4, ragged=True)
    return images, ids, mask


TRAIN_SPEC = AugmentSpec(rotate_deg=10.0, translate=0.05, zoom=(0.9, 1.1), flip_p=0.0, brightness=0.2, contrast=0.2)


def test_trainer_without_augment_is_the_trainer_it_was():
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    images, ids, mask = (t.to(DEV) for t in _batch())
    runs = []
    for kwargs in ({}, {"augment": None}):
        tr = JointContrastiveTrainer(*_joint_models(), lr=1e-4, temperature=0.07, **kwargs)
        assert tr.augment is None and tr.augment_state is None
        loss = tr.step(images, ids, mask)
        torch.cuda.synchronize()
        runs.append((loss.clone(), tr.optimizer.flat_p.detach().clone()))
        with pytest.raises(RuntimeError):
            tr.augment_state = (1, 0)
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    with pytest.raises(ValueError):
        JointContrastiveTrainer(*_joint_models(), augment=None, augment_seed=3)


def test_trainer_augment_state_and_cleanup():
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    images, ids, mask = (t.to(DEV) for t in _batch())
    im, tm = _joint_models()
    tr = JointContrastiveTrainer(im, tm, lr=0.0, temperature=0.07, augment=TRAIN_SPEC, augment_seed=77)   # lr 0: the weights stay
    assert tr.augment_state == (77, 0)
    plain = JointContrastiveTrainer(*_joint_models(), lr=0.0, temperature=0.07).step(images, ids, mask)
    l1 = tr.step(images, ids, mask).clone()
    assert tr.augment_state == (77, 1) and im.augment_call is None
    l2 = tr.step(images, ids, mask).clone()
    assert tr.augment_state == (77, 2)
    tr.augment_state = (77, 0)
    l3 = tr.step(images, ids, mask).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(l1)) and not torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(l1), _bits(l3))
    assert not torch.equal(_bits(l1), _bits(plain))
    gray = tr.step(images[:, :1].contiguous(), ids, mask)      # one channel is expanded by the augmenting transform
    assert bool(torch.isfinite(gray))
    with pytest.raises(ValueError):
        tr.step(images.clone().requires_grad_(True), ids, mask)
    assert im.augment_call is None                             # cleared although the step raised
    # the default seed comes from torch's CPU generator
    torch.manual_seed(5)
    a = JointContrastiveTrainer(*_joint_models(), augment=TRAIN_SPEC).augment_state
    torch.manual_seed(5)
    b = JointContrastiveTrainer(*_joint_models(), augment={"rotate_deg": 5.0}).augment_state
    assert a == b and a[1] == 0


# ------------------------------------------------------------------------------------------------ 9. two ranks over gloo
B_GLOBAL = 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_build(seed):
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    im, tm = _joint_models()
    tr = JointContrastiveTrainer(im, tm, lr=1e-4, temperature=0.07, augment=TRAIN_SPEC, augment_seed=seed)
    return (tr,) + _batch(B_GLOBAL)


def _probe(tr):
    p = tr.optimizer.flat_p
    return p[:: max(1, p.numel() // 4096)].detach().cpu().numpy()


def _dp_worker(rank, world, port, out_dir, precision):
    sys.path.insert(0, ROOT)
    from incremental_multimodal_medical_learning_ii_amd import _lib as lib
    lib.set_precision(precision)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    tr, images, ids, mask = _dp_build(seed=4321 if rank == 0 else 1)     # seeded differently: rank 0's seed must win
    assert tr.augment_state == (4321, 0)
    B = B_GLOBAL // world
    sl = slice(rank * B, (rank + 1) * B)
    loss = tr.step(images[sl].to(DEV), ids[sl].to(DEV), mask[sl].to(DEV))
    torch.cuda.synchronize()
    assert tr.augment_state == (4321, 1) and tr.image_model.augment_call is None
    tr.augment_state = (1000 + rank, 5)                                  # assigned per rank: the next sync takes rank 0's again
    tr.sync_augment_state()
    states = [None] * world
    dist.all_gather_object(states, tr.augment_state)
    assert states[0] == states[1] == (1000, 5), states
    tr.sync_augment_state()                                              # nothing changed since: no further broadcast
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=float(loss.item()), sample=_probe(tr))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_augmented_step_matches_single_process_global_batch(tmp_path, precision):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path), precision), nprocs=world, join=True)
    tr, images, ids, mask = _dp_build(seed=4321)
    loss = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    torch.cuda.synchronize()
    sample = _probe(tr)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    for k in range(world):        # the bounds of tests/test_dropout_gpu.py for the same comparison
        assert abs(float(r[k]["loss"]) - loss.item()) / abs(loss.item()) < 1e-5, (k, float(r[k]["loss"]), loss.item())
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    tr0, _, _, _ = _dp_build(seed=4321)
    before = _probe(tr0)
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert agree > 0.99, agree
    # another seed gives another step: the augmentation matters
    tr2, _, _, _ = _dp_build(seed=4322)
    loss2 = tr2.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    assert abs(float(loss2.item()) - loss.item()) > 1e-6 * abs(loss.item())
