"""Host-side checks of the image augmentation contract (include/cxrk.h, "augment"): the numpy restatement
(tests/augment_ref.py) against its own stated properties and against torch's affine_grid + grid_sample, and `AugmentSpec`'s
argument checks.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as AR
from incremental_multimodal_medical_learning_ii_amd.augment import AugmentCall, AugmentSpec, DEFAULT_SPEC_ARGS, spec_from

SPEC = AugmentSpec(rotate_deg=30.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, brightness=0.2, contrast=0.2)


def test_uniforms_are_exact_fp32_values_inside_the_open_unit_interval():
    u = AR.uniforms(0x1234_5678_9ABC_DEF0, 7, np.arange(4096))
    assert u.shape == (4096, 8)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # 24 significant bits
    assert u.min() > 0.0 and u.max() < 1.0
    s = 2 * u - 1                                                               # the symmetric form the draws use: exact as well
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    assert abs(u.mean() - 0.5) < 4 * math.sqrt(1 / 12 / u.size)


def test_the_counter_word_cannot_be_a_dropout_word():
    # dropout: low byte = layer << 2 | site with site 0 (embeddings) at layer 0 only; 0xF0 is (layer 60, site 0)
    assert AR.SITE_BYTE == 0xF0 and (AR.SITE_BYTE & 3) == 0 and (AR.SITE_BYTE >> 2) != 0


def test_identity_spec_gives_the_identity_map_and_unit_gain():
    rows = AR.param_rows(AugmentSpec(), 99, 3, 5, 7, 19, 23, means=np.linspace(-1, 1, 7))
    want = np.tile(np.array([1, 0, 0.5, 0, 1, 0.5, 1, 0], dtype=np.float64), (7, 1))   # xs = xo + 1/2: pixel centres
    assert np.array_equal(np.abs(rows), want)                                            # (abs: -0 == 0)
    x = np.random.default_rng(0).standard_normal((7, 3, 19, 23))
    y = AR.sample(x, rows, 19, 23)
    assert np.array_equal(y[..., :3], x.transpose(0, 2, 3, 1)) and not y[..., 3].any()


def test_drawn_quantities_lie_in_their_ranges():
    rng = np.random.default_rng(1)
    flips = []
    for seed in rng.integers(0, 2 ** 63, size=16):
        d = AR.draws(SPEC, int(seed), int(seed) % 1000, np.arange(256), 224, 200)
        assert np.all(np.abs(d["phi"]) < math.radians(30.0))
        assert np.all(np.abs(d["tx"]) < 0.1 * 200 * (1 + 1e-7)) and np.all(np.abs(d["ty"]) < 0.1 * 224 * (1 + 1e-7))
        assert np.all(d["z"] > 0.8 * (1 - 1e-7)) and np.all(d["z"] < 1.25 * (1 + 1e-7))
        assert np.all(np.abs(d["b"] - 1) < 0.2 * (1 + 1e-7)) and np.all(np.abs(d["c"] - 1) < 0.2 * (1 + 1e-7))
        flips.append(d["flip"])
    flips = np.concatenate(flips)                          # 4096 draws
    for p in (0.5, 0.1):
        spec = AugmentSpec(flip_p=p)
        fl = np.concatenate([AR.draws(spec, s, 0, np.arange(1024), 8, 8)["flip"] for s in (11, 12, 13, 14)])
        assert abs(fl.mean() - p) < 4 * math.sqrt(p * (1 - p) / fl.size)
    assert abs(flips.mean() - 0.5) < 4 * math.sqrt(0.25 / flips.size)
    assert not AR.draws(AugmentSpec(flip_p=0.0), 5, 0, np.arange(4096), 8, 8)["flip"].any()
    assert AR.draws(AugmentSpec(flip_p=1.0), 5, 0, np.arange(4096), 8, 8)["flip"].all()


def test_rows_depend_on_seed_counter_and_global_index_only():
    N, Hs, Ws = 9, 19, 23
    means = np.random.default_rng(2).standard_normal(N)
    full = AR.param_rows(SPEC, 42, 5, 0, N, Hs, Ws, means)
    for cut in range(1, N):
        a = AR.param_rows(SPEC, 42, 5, 0, cut, Hs, Ws, means[:cut])
        b = AR.param_rows(SPEC, 42, 5, cut, N - cut, Hs, Ws, means[cut:])
        assert np.array_equal(np.concatenate([a, b]), full)
    assert not np.array_equal(AR.param_rows(SPEC, 42, 6, 0, N, Hs, Ws, means), full)          # another call
    assert not np.array_equal(AR.param_rows(SPEC, 43, 5, 0, N, Hs, Ws, means), full)          # another seed
    assert np.array_equal(AR.param_rows(SPEC, 42, 5 + 2 ** 24, 0, N, Hs, Ws, means), full)    # 24 counter bits are keyed
    assert len({tuple(r) for r in full[:, :6]}) == N                                          # every image its own map


@pytest.mark.parametrize("spec", [
    AugmentSpec(rotate_deg=30.0), AugmentSpec(zoom=(0.7, 1.4)), AugmentSpec(translate=0.2), AugmentSpec(flip_p=1.0),
    AugmentSpec(out_size=(16, 12)), AugmentSpec(rotate_deg=25.0, translate=0.1, zoom=(0.8, 1.25), flip_p=0.5, out_size=(20, 28)),
], ids=["rotate", "zoom", "translate", "flip", "resize", "all"])
def test_sampler_agrees_with_torch_affine_grid_and_grid_sample(spec):
    """An independent implementation of the same semantics: grid_sample(bilinear, zeros, align_corners=False) in float64."""
    N, Hs, Ws = 6, 19, 23
    Ho, Wo = spec.size_for(Hs, Ws)
    x = np.random.default_rng(3).standard_normal((N, 3, Hs, Ws))
    rows = AR.param_rows(spec, 2024, 1, 4, N, Hs, Ws)
    if spec.flip_p == 1.0:
        assert np.all(rows[:, 0] < 0)
    got = AR.sample(x, rows, Ho, Wo)[..., :3]
    theta = torch.from_numpy(AR.theta_for_affine_grid(rows, Hs, Ws, Ho, Wo))
    grid = F.affine_grid(theta, (N, 3, Ho, Wo), align_corners=False)
    ref = F.grid_sample(torch.from_numpy(x), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    ref = ref.permute(0, 2, 3, 1).numpy()
    # both are float64; they differ by the rounding of coordinates of magnitude <= 32: |d coord| ~ 1e-14, times the tap differences
    assert np.abs(got - ref).max() < 1e-11 * np.abs(x).max()
    assert np.abs(ref).max() > 0.1


def test_photometric_terms():
    N, Hs, Ws = 4, 8, 8
    rng = np.random.default_rng(4)
    x = rng.random((N, 1, Hs, Ws))
    spec = AugmentSpec(brightness=0.3, contrast=0.4)
    means = x.mean(axis=(1, 2, 3))
    rows = AR.param_rows(spec, 1, 0, 0, N, Hs, Ws, means)
    d = AR.draws(spec, 1, 0, np.arange(N), Hs, Ws)
    y = AR.sample(x, rows, Hs, Ws)
    want = d["b"][:, None, None] * ((x[:, 0] - means[:, None, None]) * d["c"][:, None, None] + means[:, None, None])
    for c in range(3):                                               # one channel replicated to three
        assert np.allclose(y[..., c], want, rtol=0, atol=1e-14)
    assert not y[..., 3].any()
    yc = AR.sample(x * 3 - 1, rows, Hs, Ws, clamp01=True)
    assert yc.min() == 0.0 and yc.max() == 1.0
    xn = x.copy()
    xn[0, 0, 2, 3] = np.nan
    assert np.isnan(AR.sample(xn, rows, Hs, Ws, clamp01=True)[0, 2, 3, :3]).all()        # the clamp keeps a NaN


@pytest.mark.parametrize("kwargs", [
    {"rotate_deg": float("nan")}, {"rotate_deg": float("inf")}, {"rotate_deg": -1.0}, {"translate": float("inf")}, {"translate": -0.1},
    {"zoom": (0.0, 1.0)}, {"zoom": (-1.0, 1.0)}, {"zoom": (1.2, 0.8)}, {"zoom": (1.0, float("inf"))}, {"zoom": 1.0}, {"zoom": (1.0,)},
    {"flip_p": -0.1}, {"flip_p": 1.5}, {"flip_p": float("nan")}, {"brightness": 1.0}, {"brightness": -0.1}, {"brightness": float("nan")},
    {"contrast": 1.0}, {"contrast": 2.0}, {"contrast": float("-inf")}, {"out_size": (0, 8)}, {"out_size": (8, -1)}, {"out_size": 8},
    {"out_size": (8.5, 8)}, {"rotate_deg": "10"},
])
def test_spec_refuses_invalid_arguments(kwargs):
    with pytest.raises(ValueError):
        AugmentSpec(**kwargs)


def test_spec_defaults_and_conversions():
    s = AugmentSpec()
    assert s.is_identity and s.size_for(5, 7) == (5, 7) and AugmentSpec(out_size=(3, 4)).size_for(5, 7) == (3, 4)
    with pytest.raises(Exception):
        s.rotate_deg = 1.0                                            # frozen
    assert spec_from(None) is None and spec_from(False) is None and spec_from(s) is s
    d = spec_from(True)
    assert d == AugmentSpec(**DEFAULT_SPEC_ARGS) and d.flip_p == 0.0 and d.rotate_deg == 10.0 and d.zoom == (0.9, 1.1)
    assert spec_from({"zoom": [0.9, 1.1], "out_size": [8, 8]}) == AugmentSpec(zoom=(0.9, 1.1), out_size=(8, 8))
    with pytest.raises(TypeError):
        spec_from("yes")
    assert AugmentCall(s, 1, 2).row_offset == 0


def test_driver_flags():
    from incremental_multimodal_medical_learning_ii_amd import drivers
    ap = drivers.make_parser()
    base = ["class-inc"]
    assert drivers.augment_from_args(ap.parse_args(base + ["--joint"])) is None
    d = drivers.augment_from_args(ap.parse_args(base + ["--joint", "--augment"]))
    assert AugmentSpec(**d) == AugmentSpec(**DEFAULT_SPEC_ARGS)
    d = drivers.augment_from_args(ap.parse_args(base + ["--joint", "--augment", "--aug-rotate", "5", "--aug-zoom", "0.8", "1.2", "--aug-flip", "0.5"]))
    assert AugmentSpec(**d) == AugmentSpec(rotate_deg=5.0, translate=0.05, zoom=(0.8, 1.2), flip_p=0.5, brightness=0.2, contrast=0.2)
    with pytest.raises(SystemExit):
        drivers.augment_from_args(ap.parse_args(base + ["--joint", "--aug-rotate", "5"]))
    with pytest.raises(SystemExit):
        drivers.main(base + ["--augment"])                             # needs --joint
