"""Test-only restatement of the on-device image augmentation (include/cxrk.h, "augment") in numpy, float64: the Philox draws,
the parameter rows and the bilinear sampler with zero fill.  Nothing here shares code with csrc/augment.hip."""
from __future__ import annotations

import math

import numpy as np

from dropout_ref import philox4x32_10

SITE_BYTE = 0xF0


def uniforms(seed: int, counter: int, n) -> np.ndarray:
    """float64 [len(n), 8]: u_k = ((w_k >> 9) + 0.5) 2^-23 of the image's two Philox blocks (global image indices n)"""
    n = np.asarray(n, dtype=np.uint64).reshape(-1)
    c3 = np.uint64(((counter & 0xFFFFFF) << 8) | SITE_BYTE)
    words = []
    for b in (0, 1):
        words += philox4x32_10(np.full_like(n, b), n, np.zeros_like(n), np.full_like(n, c3), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = np.stack(words, axis=1).astype(np.uint64)
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def draws(spec, seed: int, counter: int, n, Ho: int, Wo: int) -> dict:
    """the drawn quantities of the images with global indices n (float64 arrays; flip is bool)"""
    u = uniforms(seed, counter, n)
    f32 = lambda v: float(np.float32(v))     # the spec crosses the C ABI as fp32
    lo, hi = f32(spec.zoom[0]), f32(spec.zoom[1])
    return {
        "phi": (2 * u[:, 0] - 1) * f32(spec.rotate_deg) * math.pi / 180.0,
        "tx": (2 * u[:, 1] - 1) * f32(spec.translate) * Wo,
        "ty": (2 * u[:, 2] - 1) * f32(spec.translate) * Ho,
        "z": np.exp(math.log(lo) + u[:, 3] * (math.log(hi) - math.log(lo))),
        "flip": u[:, 4] < f32(spec.flip_p),
        "b": 1 + (2 * u[:, 5] - 1) * f32(spec.brightness),
        "c": 1 + (2 * u[:, 6] - 1) * f32(spec.contrast),
    }


def param_rows(spec, seed: int, counter: int, row_offset: int, N: int, Hs: int, Ws: int, means=None) -> np.ndarray:
    """float64 [N, 8]: a00 a01 a02 a10 a11 a12 gain bias of images row_offset .. row_offset + N - 1; `means` [N] = the image means
    (needed when spec.contrast != 0)"""
    Ho, Wo = (Hs, Ws) if spec.out_size is None else spec.out_size
    d = draws(spec, seed, counter, np.arange(N) + row_offset, Ho, Wo)
    f = np.where(d["flip"], -1.0, 1.0)
    cs, sn = np.cos(d["phi"]), np.sin(d["phi"])
    kx, ky = (Ws / Wo) / d["z"], (Hs / Ho) / d["z"]
    a00, a01, a10, a11 = kx * cs * f, -kx * sn, ky * sn * f, ky * cs
    ox, oy = 0.5 - Wo / 2 - d["tx"], 0.5 - Ho / 2 - d["ty"]
    m = np.zeros(N) if means is None else np.asarray(means, dtype=np.float64)
    return np.stack([a00, a01, Ws / 2 + a00 * ox + a01 * oy, a10, a11, Hs / 2 + a10 * ox + a11 * oy,
                     d["b"] * d["c"], d["b"] * m * (1 - d["c"])], axis=1)


def taps(rows: np.ndarray, Hs: int, Ws: int, Ho: int, Wo: int):
    """per output pixel the four taps of the bilinear sample: integer coordinates (ys, xs) [4, N, Ho, Wo], weights [4, N, Ho, Wo]
    (0 for a tap outside the source) in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1)"""
    rows = np.asarray(rows, dtype=np.float64)
    xo = np.arange(Wo, dtype=np.float64)[None, None, :]
    yo = np.arange(Ho, dtype=np.float64)[None, :, None]
    r = rows[:, :, None, None]
    fx = r[:, 0] * xo + r[:, 1] * yo + r[:, 2] - 0.5
    fy = r[:, 3] * xo + r[:, 4] * yo + r[:, 5] - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    wx1, wy1 = fx - x0, fy - y0
    ys = np.stack([y0, y0, y0 + 1, y0 + 1]).astype(np.int64)
    xs = np.stack([x0, x0 + 1, x0, x0 + 1]).astype(np.int64)
    w = np.stack([(1 - wy1) * (1 - wx1), (1 - wy1) * wx1, wy1 * (1 - wx1), wy1 * wx1])
    inside = (ys >= 0) & (ys < Hs) & (xs >= 0) & (xs < Ws)
    return ys, xs, np.where(inside, w, 0.0)


def sample(src: np.ndarray, rows: np.ndarray, Ho: int, Wo: int, clamp01: bool = False, cpad: int = 4) -> np.ndarray:
    """src [N, C, Hs, Ws] (C = 3 or 1) sampled through `rows` [N, 8] -> float64 [N, Ho, Wo, cpad]: bilinear, zero fill, then
    gain v + bias (fill included), then the optional clamp; one source channel is replicated to three; padded channels are 0.
    A tap of weight zero does not contribute (its value may be non-finite)."""
    src = np.asarray(src, dtype=np.float64)
    N, C, Hs, Ws = src.shape
    ys, xs, w = taps(rows, Hs, Ws, Ho, Wo)
    yc, xc = np.clip(ys, 0, Hs - 1), np.clip(xs, 0, Ws - 1)
    ni = np.arange(N)[None, :, None, None]
    out = np.zeros((N, Ho, Wo, cpad))
    rows = np.asarray(rows, dtype=np.float64)
    for c in range(3):
        v = src[ni, min(c, C - 1), yc, xc]                                  # [4, N, Ho, Wo]
        acc = np.where(w != 0, w * np.where(w != 0, v, 0.0), 0.0).sum(axis=0)
        acc = rows[:, 6, None, None] * acc + rows[:, 7, None, None]
        if clamp01:
            acc = np.where(acc < 0, 0.0, np.where(acc > 1, 1.0, acc))        # comparisons: a NaN stays
        out[..., c] = acc
    return out


def tap_weight_of(rows: np.ndarray, Hs: int, Ws: int, Ho: int, Wo: int, n: int, y: int, x: int) -> np.ndarray:
    """[Ho, Wo]: the total bilinear weight output pixels of image n give to source pixel (y, x)"""
    ys, xs, w = taps(rows[n:n + 1], Hs, Ws, Ho, Wo)
    return np.where((ys == y) & (xs == x), w, 0.0).sum(axis=0)[0]


def theta_for_affine_grid(rows: np.ndarray, Hs: int, Ws: int, Ho: int, Wo: int) -> np.ndarray:
    """The same maps as torch `affine_grid(theta, align_corners=False)` wants them: [N, 2, 3] from normalised output coordinates
    (xn = (2 xo + 1) / Wo - 1) to normalised source coordinates (xs = (xn_s + 1) Ws / 2)."""
    r = np.asarray(rows, dtype=np.float64)
    a00, a01, a02, a10, a11, a12 = (r[:, k] for k in range(6))
    # xo = (xn + 1) Wo / 2 - 1/2, and xn_s = 2 xs / Ws - 1
    t = np.empty((r.shape[0], 2, 3))
    t[:, 0, 0] = a00 * Wo / Ws
    t[:, 0, 1] = a01 * Ho / Ws
    t[:, 0, 2] = (2 / Ws) * (a00 * (Wo / 2 - 0.5) + a01 * (Ho / 2 - 0.5) + a02) - 1
    t[:, 1, 0] = a10 * Wo / Hs
    t[:, 1, 1] = a11 * Ho / Hs
    t[:, 1, 2] = (2 / Hs) * (a10 * (Wo / 2 - 0.5) + a11 * (Ho / 2 - 0.5) + a12) - 1
    return t
