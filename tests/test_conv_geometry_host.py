"""Convolution geometry beyond ResNet's own grid: the tables of tests/test_conv_geometry_gpu.py, the float64 references it compares
the kernels with, and (here, on the CPU) the proof that those references are right where they are rarely used.

The references are `F.conv2d`, `torch.nn.grad.conv2d_input` and `torch.nn.grad.conv2d_weight` in float64.  This file checks each of
them against the definition written out as nested loops, at every geometry of the tables (with two channels, so the loops stay
cheap): pad above and below "same", R != S, stride 2 with a left-over row or column, images of one pixel.

Tuples are (N, H, W, C, Ko, R, S, stride, pad); tensors are NHWC, filters [Ko, R, S, C], as include/cxrk.h lays them out."""
import pytest
import torch
import torch.nn.functional as F

# ---- geometries that compute -------------------------------------------------------------------------------------------------
PAD_OFF_SAME = [
    (2, 7, 9, 64, 32, 3, 3, 1, 0), (2, 7, 9, 64, 32, 3, 3, 1, 2),
    (2, 7, 9, 32, 64, 1, 1, 1, 1),            # 1x1 with pad 1: the border outputs are shift plus residual only
    (2, 8, 5, 32, 32, 3, 3, 2, 2), (2, 9, 6, 32, 64, 2, 2, 2, 0), (3, 7, 8, 32, 32, 2, 2, 1, 1), (2, 6, 7, 32, 32, 5, 5, 1, 2),
]
# stride 2, a 3-wide filter extent, pad 0: the data gradient's tap lists carry an offset of -1 (csrc/conv_dgrad.hip, s2_classes)
S2_PAD0 = [
    (2, 8, 5, 64, 32, 3, 3, 2, 0), (2, 7, 9, 64, 32, 3, 3, 2, 0), (3, 3, 3, 32, 32, 3, 3, 2, 0), (2, 7, 9, 32, 32, 1, 3, 2, 0),
    (2, 7, 9, 32, 32, 3, 1, 2, 0),
]
R_NE_S = [(2, 7, 9, 32, 32, 1, 3, 1, 1), (2, 7, 9, 32, 32, 3, 1, 1, 1), (2, 8, 7, 32, 32, 3, 1, 2, 1), (2, 8, 7, 32, 32, 3, 2, 2, 1)]
# stride 2 with a left-over row or column in either direction, and 1x1 / stride 2 on a rectangle
S2_LEFTOVER = [(2, 13, 8, 64, 64, 3, 3, 2, 1), (2, 8, 13, 64, 64, 3, 3, 2, 1), (2, 13, 8, 64, 128, 1, 1, 2, 0)]
# tiny images: a 256-row tile spans up to 256 of them; at H = 1 or W = 1 with stride 2 some output-parity classes are empty
TINY = [
    (300, 1, 1, 32, 32, 3, 3, 1, 1), (300, 1, 1, 32, 32, 1, 1, 1, 0), (70, 1, 1, 32, 32, 3, 3, 2, 1), (40, 2, 3, 32, 32, 3, 3, 2, 1),
    (33, 1, 6, 32, 32, 3, 3, 1, 1), (5, 1, 6, 32, 32, 1, 3, 2, 0),
]
# Ko = 64 twins: the planes forward writes its ReLU decision bits 64 output channels at a time (include/cxrk.h), so the rows above
# with Ko = 32 run that forward without them; these bring the bits to a stride-2 / pad-0, an R != S and two tiny-image geometries
KO64 = [(2, 8, 5, 64, 64, 3, 3, 2, 0), (2, 8, 7, 32, 64, 3, 2, 2, 1), (70, 1, 1, 32, 64, 3, 3, 2, 1), (300, 1, 1, 32, 64, 3, 3, 1, 1)]
COMPUTES = PAD_OFF_SAME + S2_PAD0 + R_NE_S + S2_LEFTOVER + TINY + KO64

# channel edges of the fp32 forward and weight gradient, (N, H, W, C, Cpad, Ko, R, S, stride, pad): K tails of 72, 144 and 432 on the
# per-lane-tap gather, a 32-multiple channel count sent down that path by R*S > 32, and padded input channels (as at the stem)
CHANNEL_EDGES = [
    (2, 7, 9, 8, 8, 32, 3, 3, 1, 1), (2, 7, 9, 16, 16, 32, 3, 3, 1, 1), (2, 7, 9, 48, 48, 32, 3, 3, 1, 1), (2, 9, 11, 32, 32, 32, 7, 7, 2, 3),
    (2, 7, 9, 5, 8, 32, 3, 3, 1, 1),
]

# the (R, S, stride, pad) rows of the seeded sweep's convolution family (tests/sweep_conv_cases.py GEOMS_LANE) that no table above
# holds, on the 7 x 9 image (9 x 11 where the 7 x 7 and 9 x 1 filters want room): the loop check below covers their references too
SWEEP_GEOMETRIES = [(2, 7, 9, 32, 32, 1, 1, 1, 0), (2, 7, 9, 32, 32, 1, 1, 2, 0), (2, 7, 9, 32, 32, 3, 3, 1, 1), (2, 7, 9, 32, 32, 3, 3, 2, 1),
                    (2, 7, 9, 32, 32, 3, 1, 2, 1), (2, 7, 9, 32, 32, 3, 2, 2, 1), (2, 7, 9, 32, 32, 2, 2, 2, 0), (2, 7, 9, 32, 32, 2, 2, 1, 1),
                    (2, 7, 9, 32, 32, 5, 5, 1, 2), (2, 9, 11, 32, 32, 7, 7, 2, 3), (2, 9, 11, 32, 32, 9, 1, 1, 4)]

# the data gradient with a COMPACT stride-2 residual (tests/test_kernels_gpu.py::test_planes_dgrad_compact_stride2_residual): N, H, W, C, Ko, R
COMPACT_RESIDUAL = [(3, 13, 8, 64, 64, 3), (2, 8, 13, 128, 64, 1)]

# ---- geometries that are refused ---------------------------------------------------------------------------------------------
# (what, entry points, code, tuple); entry points: "fdw" = forward, data gradient and weight gradient, "d" = data gradient, each in both
# storage forms; "f_pl" = the planes forward only.  code: the one include/cxrk.h states, -1 CXRK_ERR_ARG, -4 CXRK_ERR_UNSUPPORTED
REFUSED = [
    ("Ho <= 0", "fdw", -1, (2, 1, 6, 32, 32, 3, 3, 1, 0)),
    ("Ho, Wo <= 0 at stride 2", "fdw", -1, (2, 2, 2, 32, 32, 5, 5, 2, 0)),
    ("extent -1 at stride 2 (truncating division gives 1)", "fdw", -1, (2, 2, 2, 32, 32, 3, 3, 2, 0)),
    ("pad -1", "fdw", -1, (2, 7, 9, 32, 32, 3, 3, 1, -1)),
    ("stride-2 data gradient, R = 5", "d", -1, (2, 8, 8, 32, 32, 5, 5, 2, 2)),
    ("data gradient, R*S > 32", "d", -4, (2, 9, 9, 32, 32, 7, 7, 1, 3)),
    ("data gradient, Ko % 32 != 0", "d", -4, (2, 7, 9, 32, 48, 3, 3, 1, 1)),
    ("planes forward, C % 32 != 0", "f_pl", -4, (2, 7, 9, 16, 32, 3, 3, 1, 1)),
    ("planes forward, 7x7", "f_pl", -4, (2, 9, 9, 32, 32, 7, 7, 2, 3)),
    ("stride 3", "fdw", -1, (2, 9, 9, 32, 32, 3, 3, 3, 1)),
]


def conv_out(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def dgrad_side_ok(H, W, R, S, stride, pad):
    """The data gradient takes a residual / mask unless it runs by output-parity classes (stride 2) and some class that has pixels
    is reached by no filter tap (its pixels are exactly zero: plain form only, include/cxrk.h)."""
    if stride == 1:
        return True
    rows = all(any((ph + pad - r) % 2 == 0 for r in range(R)) for ph in range(min(2, H)))
    cols = all(any((pw + pad - s) % 2 == 0 for s in range(S)) for pw in range(min(2, W)))
    return rows and cols


def dgrad_sums_ok(H, W, R, S, stride, pad):
    return dgrad_side_ok(H, W, R, S, stride, pad) and not (R == 1 and stride == 2)


# ---- the float64 references of the GPU file ------------------------------------------------------------------------------------
def fwd_ref(x64, w64, stride, pad):
    """z [N, Ho, Wo, Ko] = conv(x [N, H, W, C], w [Ko, R, S, C])"""
    return F.conv2d(x64.permute(0, 3, 1, 2), w64.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def dgrad_ref(dy64, w64, H, W, stride, pad):
    """dx [N, H, W, C] from dy [N, Ho, Wo, Ko], w [Ko, R, S, C]"""
    N, C = dy64.shape[0], w64.shape[3]
    dx = torch.nn.grad.conv2d_input((N, C, H, W), w64.permute(0, 3, 1, 2), dy64.permute(0, 3, 1, 2), stride=stride, padding=pad)
    return dx.permute(0, 2, 3, 1).contiguous()


def wgrad_ref(x64, dy64, R, S, stride, pad):
    """dw [Ko, R, S, C] from x [N, H, W, C], dy [N, Ho, Wo, Ko]"""
    Ko, C = dy64.shape[3], x64.shape[3]
    dw = torch.nn.grad.conv2d_weight(x64.permute(0, 3, 1, 2), (Ko, C, R, S), dy64.permute(0, 3, 1, 2), stride=stride, padding=pad)
    return dw.permute(0, 2, 3, 1).contiguous()


# ---- the definition, as loops ----------------------------------------------------------------------------------------------------
def loops(x, w, dy, stride, pad):
    """y[n, ho, wo, ko] = sum_{r, s, c} x[n, ho*stride - pad + r, wo*stride - pad + s, c] * w[ko, r, s, c] over the taps inside the image,
    and the two gradients of sum(y * dy): one pass over (ho, wo, r, s), the batch and channel sums as small matrix products"""
    N, H, W, C = x.shape
    Ko, R, S, _ = w.shape
    _, Ho, Wo, _ = dy.shape
    y, dx, dw = torch.zeros_like(dy), torch.zeros_like(x), torch.zeros_like(w)
    for ho in range(Ho):
        for wo in range(Wo):
            for r in range(R):
                for s in range(S):
                    hi, wi = ho * stride - pad + r, wo * stride - pad + s
                    if 0 <= hi < H and 0 <= wi < W:
                        y[:, ho, wo] += x[:, hi, wi] @ w[:, r, s].T
                        dx[:, hi, wi] += dy[:, ho, wo] @ w[:, r, s]
                        dw[:, r, s] += dy[:, ho, wo].T @ x[:, hi, wi]
    return y, dx, dw


def _small(cfg):
    """the table's geometry with two channels"""
    if len(cfg) == 10:
        N, H, W, _, _, _, R, S, stride, pad = cfg
    else:
        N, H, W, _, _, R, S, stride, pad = cfg
    return N, H, W, 2, 2, R, S, stride, pad


def _all_geometries():
    seen = []
    for cfg in COMPUTES + CHANNEL_EDGES + SWEEP_GEOMETRIES + [(N, H, W, C, Ko, R, R, 1, R // 2) for N, H, W, C, Ko, R in COMPACT_RESIDUAL] + \
            [(N, H, W, 2 * C, C, 1, 1, 2, 0) for N, H, W, C, Ko, R in COMPACT_RESIDUAL]:
        s = _small(cfg)
        if s not in seen:
            seen.append(s)
    return seen


@pytest.mark.parametrize("cfg", _all_geometries())
def test_references_match_the_definition(cfg):
    N, H, W, C, Ko, R, S, stride, pad = cfg
    Ho, Wo = conv_out(H, W, R, S, stride, pad)
    assert Ho > 0 and Wo > 0
    g = torch.Generator().manual_seed(H * 100 + W * 10 + R + S + stride + pad)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(Ko, R, S, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, Ho, Wo, Ko, generator=g, dtype=torch.float64)
    y, dx, dw = loops(x, w, dy, stride, pad)
    for name, got, ref in (("forward", fwd_ref(x, w, stride, pad), y), ("data gradient", dgrad_ref(dy, w, H, W, stride, pad), dx),
                           ("weight gradient", wgrad_ref(x, dy, R, S, stride, pad), dw)):
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = float((got - ref).abs().max())
        assert err < 1e-12 * max(1.0, float(ref.abs().max())), f"{name}: {err:.3e}"


def test_tables_are_what_they_claim():
    """every computing geometry has an output, every refused one is refused for the stated reason, and the stride-2 / pad-0 rows
    really produce the negative tap offset"""
    for cfg in COMPUTES:
        N, H, W, C, Ko, R, S, stride, pad = cfg
        Ho, Wo = conv_out(H, W, R, S, stride, pad)
        assert Ho > 0 and Wo > 0 and stride in (1, 2) and pad >= 0, cfg
        assert C % 32 == 0 and Ko % 32 == 0 and R * S <= 32 and (stride == 1 or max(R, S) <= 3), cfg
    for cfg in S2_PAD0:
        N, H, W, C, Ko, R, S, stride, pad = cfg
        offs = [(p + pad - t) // 2 for ext in (R, S) for p in (0, 1) for t in range(ext) if (p + pad - t) % 2 == 0]
        assert stride == 2 and pad == 0 and min(offs) == -1, cfg
    for what, eps, code, cfg in REFUSED:
        N, H, W, C, Ko, R, S, stride, pad = cfg
        Ho, Wo = conv_out(H, W, R, S, stride, pad)
        bad_geom = Ho <= 0 or Wo <= 0 or pad < 0 or stride not in (1, 2)
        bad_dgrad = Ko % 32 != 0 or R * S > 32 or (stride == 2 and max(R, S) > 3)
        bad_fwd_pl = C % 32 != 0 or R * S > 32
        assert bad_geom or (eps == "d" and bad_dgrad) or (eps == "f_pl" and bad_fwd_pl), (what, cfg)
        assert code == (-1 if bad_geom or (eps == "d" and stride == 2 and max(R, S) > 3) else -4), (what, code)
    # a parity class without a tap: 1-wide extents at stride 2; with a single row the odd class has no pixels and nothing is lost
    assert not dgrad_side_ok(7, 9, 1, 3, 2, 0) and dgrad_side_ok(1, 6, 1, 3, 2, 0) and not dgrad_sums_ok(1, 6, 1, 3, 2, 0)
    assert dgrad_side_ok(9, 6, 2, 2, 2, 0) and dgrad_side_ok(8, 5, 3, 3, 2, 0) and not dgrad_side_ok(13, 8, 1, 1, 2, 0)
