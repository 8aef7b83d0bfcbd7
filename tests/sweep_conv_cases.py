"""Family H of the differential sweep (tests/sweep_cases.py registers it): the convolutions, one operation per case -- forward,
data gradient or weight gradient -- on fp32 operands ("H32": K.conv_fwd, K.conv_fwd_pl on fp32 inputs as the stem calls it,
K.conv_bwd_data, K.conv_bwd_params) and on planes operands ("HPL": K.conv_fwd_pl, K.conv_bwd_data_pl with the dense or the compact
stride-2 residual, K.conv_bwd_params_pl).

  gen(i, schedule)         the frozen ConvCase of (SEED, family, index)
  legal(case)              the rules of include/cxrk.h for the entry point of the case, and the two caps of the family
  build(case)              CPU inputs (float32; decision bits uint8)
  evaluate(case, inp, dt)  F.conv2d / conv2d_input / conv2d_weight (the functions tests/test_conv_geometry_host.py checks against nested
                           loops) in float64 on the values the kernel sees, then the epilogue of include/cxrk.h in `dt`.  float32: the
                           float64 contraction rounded ONCE, then the epilogue in float32 -- never the host's float32 convolution, whose
                           blocking differs between processors (family G's finding)
  check(case, ref, got)    every output through BOTH comparators (below); exact outputs bit for bit
  predict(case, wide)      the dispatch of csrc/conv_fwd.hip, conv_dgrad.hip, conv_wgrad.hip, gemm_dispatch.h and wgrad_splitk_policy
                           restated: launches, label, tile, split-K, slabs, reducer grouping, epilogue branch

Sampling.  The stratum of the GEMM rows (forward N Ho Wo, data gradient N H W) or of the reduction length (weight gradient N Ho Wo),
the filter geometry (R, S, stride, pad), the epilogue and the value profile are independent covering dimensions.  Channels, image
sizes and the image count depend on them through the caps (every tensor <= 8 MiB as fp32; 2 M N K < 2^30 per launch, which keeps
fp32 operands on the exact-fp32 mainloop in both precision modes and the tile policy off the 256x256 tile unless it is forced):
each list that a cap or a fitting filter narrows has a covering sequence of its own (`Schedule`).  The last seven cases of every HPL
operation are the window-resident trio's: 3x3 / stride 1 / pad 1, C = Ko = 64, W <= 58 (the first of them W = 58), the last one W = 59,
which must take the implicit GEMM.  Every eighth case draws H and W from (1, 2, 3): tiles that span dozens of images.

Values.  "randn"; "chan_scaled": a factor 2^e, e in -10 .. 4, per channel of x (forward, weight gradient) or dy (data gradient) and,
independently, per channel of the filter's other side (forward: its output channels, data gradient: its input channels) or of dy
(weight gradient), so that output channels / filters of one tensor lie up to 2^14 apart; "relu_like": x >= 0 and dy each with about
half their elements exactly zero, what the network feeds.  C < Cpad (H32 forward and weight gradient, Cpad 4 with 3 and 8 with 5 real
channels): the padded channels of x and of the scaled filter are zero, the raw filter and its gradient have the real count.

Bounds.  (1) elementwise, forward_bound: |got - ref| <= c mag, mag the same contraction on absolute values plus |shift|, |residual|,
|dw0|, and c = (K + 8) 2^-24 (fp32 operands) or (3 K + 8) 2^-24 on the magnitudes of the three plane terms hi hi + hi lo + lo hi
(planes operands; the reference is the sum of those terms, as gemm_acc forms it); K = R S C, R S Ko or N Ho Wo is the whole
contraction, so any summation order and any split-K is covered.  A planes output adds 2^-16 |ref|; `sums` takes c + (rows + 8) 2^-24
on the summed magnitudes; dgamma (c + (R S Cpad + 8) 2^-24) |rstd| (sum |w| mag_raw + |mean sumdy|) (+ |dgamma0|); dbeta is bit for
bit sumdy, or fl(dbeta0 + sumdy).  (2) the level: forward and data gradient per output channel (col_scaled), dw per filter
(row_scaled), sums and dgamma per element, against max(floor, 8 e32) with the floors of floor_of (2e-5 forward, 5e-5 gradients, 3e-4
planes / split mode; dgamma 2e-3 fp32, 2e-2 planes / split mode, today's).

No GPU and no library import here."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import sweep_cases as SC
import test_conv_geometry_host as G

COUNTS = (("fwd", 40), ("dgrad", 40), ("wgrad", 40))
OPS = tuple(op for op, _ in COUNTS)
MAX_ELEMS = (8 << 20) // 4            # every tensor <= 8 MiB as fp32
MAX_FLOPS = 1 << 30                   # 2 M N K per launch stays below: exact-fp32 mainloop, no 256x256 tile by policy
GEOMS = ((1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 1, 1),
         (3, 3, 1, 1), (3, 3, 2, 1), (3, 3, 1, 0), (3, 3, 1, 2), (3, 3, 2, 0),
         (1, 3, 1, 1), (3, 1, 2, 1), (3, 2, 2, 1),
         (2, 2, 2, 0), (2, 2, 1, 1), (5, 5, 1, 2))
GEOMS_LANE = GEOMS + ((7, 7, 2, 3), (9, 1, 1, 4))     # the per-lane-tap gather: R S > 32, R > 8 (H32 forward and weight gradient)
HW = (1, 2, 3, 7, 8, 13, 28, 56, 58, 59)              # 58, 59: either side of HALO_MAXW
ROWS = (("<64", 1, 63), ("64..255", 64, 255), ("257..511", 257, 511), (">=1024", 1024, 4096))
RED = (("<32", 1, 31), ("32..255", 32, 255), ("256..2047", 256, 2047), ("2048..16383", 2048, 16383), (">=16384", 16384, 20000))
C_STRATA = {("H32", "fwd"): (4, 8, 12, 16, 32, 48, 64, 72, 128, 264), ("H32", "dgrad"): (4, 8, 12, 16, 32, 48, 64, 72, 128, 264),
            ("H32", "wgrad"): (4, 8, 12, 16, 32, 48, 64, 72, 128, 264),
            ("HPL", "fwd"): (32, 64, 96, 128, 288), ("HPL", "dgrad"): (8, 24, 32, 64, 72, 128, 136, 264),
            ("HPL", "wgrad"): (8, 24, 32, 64, 72, 136)}
KO_STRATA = {("H32", "fwd"): (1, 3, 6, 8, 30, 32, 64, 72, 136, 264), ("HPL", "fwd"): (8, 24, 32, 64, 72, 128, 136, 264),
             ("H32", "dgrad"): (32, 64, 96, 128, 288), ("HPL", "dgrad"): (32, 64, 96, 128, 288),
             ("H32", "wgrad"): (4, 12, 32, 64, 72, 136, 264), ("HPL", "wgrad"): (8, 24, 32, 64, 72, 136, 264)}
REAL_C = {4: 3, 8: 5}                 # H32 forward and weight gradient: Cpad -> real channels
FWD_EPI = tuple(range(8))             # bit 0 shift, bit 1 residual, bit 2 relu
DGRAD_EPI = ("plain", "residual", "mask", "residual+mask", "plain+sums", "residual+sums", "mask+sums", "residual+mask+sums")
DGRAD_EPI_COMPACT = ("compact", "compact+mask+sums")      # HPL at stride 1
WGRAD_BN = ("full", "none", "noscale")                    # none: dgamma = dbeta = NULL; noscale: scale = NULL
PROFILES = ("randn", "chan_scaled", "relu_like")
TRIO = 7                              # the last cases of every HPL operation
HALO_MAXW, HALO_CH = 58, 64           # csrc/conv_halo.h
BK = 32                               # the K-tile of every mainloop (csrc/gemm_common.h)


@dataclass(frozen=True)
class ConvCase:
    index: int
    family: str          # "H32" / "HPL"
    op: str              # "fwd", "dgrad", "wgrad"
    N: int
    H: int
    W: int
    C: int               # real input channels
    Cpad: int            # stored input channels
    Ko: int
    R: int
    S: int
    stride: int
    pad: int
    rows: str            # the stratum of the GEMM rows / the reduction length
    form: str            # "f32", "stem" (K.conv_fwd_pl on fp32 operands: planes output) or "pl"
    shift: bool = False
    residual: str = "none"       # "none", "dense", "compact"
    relu: bool = False
    bits: bool = False           # forward: the ReLU decision bits are requested
    mask: bool = False
    sums: bool = False
    accumulate: bool = False
    bn: str = "full"
    profile: str = "randn"

    @property
    def geom(self):
        return self.R, self.S, self.stride, self.pad

    @property
    def out_hw(self):
        return G.conv_out(self.H, self.W, self.R, self.S, self.stride, self.pad)

    @property
    def planes_out(self) -> bool:
        return self.op != "wgrad" and self.form != "f32"


# ---------------------------------------------------------------------------------------------------------------- generator
def _n_range(op, geom, Cp, Ko, H, W, lo, hi) -> Optional[Tuple[int, int]]:
    """the image counts that put the rows / the reduction length in [lo, hi] under both caps"""
    R, S, stride, pad = geom
    if H + 2 * pad - R < 0 or W + 2 * pad - S < 0:
        return None
    Ho, Wo = G.conv_out(H, W, R, S, stride, pad)
    per = H * W if op == "dgrad" else Ho * Wo
    work = 2 * per * Ko * R * S * Cp          # per image: 2 M N K of all three operations (the stride-2 classes share it out)
    if Ko * R * S * Cp > MAX_ELEMS:
        return None
    nlo = -(-lo // per)
    nhi = min(hi // per, MAX_ELEMS // (H * W * Cp), MAX_ELEMS // (Ho * Wo * Ko), (MAX_FLOPS - 1) // work)
    return (nlo, nhi) if 1 <= nlo <= nhi else None


def _sizes(op, geom, Cp, Ko, lo, hi, hs=HW, ws=HW):
    return [(H, W) for H in hs for W in ws if _n_range(op, geom, Cp, Ko, H, W, lo, hi)]


def gen(i: int, sched) -> ConvCase:
    fam = sched.family
    op, k = SC._op_of(COUNTS, i)
    S = lambda dim, strata: sched(op + "." + dim, strata)      # noqa: E731
    r = SC._rng(fam, i)
    trio = fam == "HPL" and k >= 40 - TRIO
    tiny = k % 8 == 3 and not trio
    strata = RED if op == "wgrad" else ROWS
    hs = ws = tuple(v for v in HW if v <= 3) if tiny else HW
    if trio:      # the rows strata that the fixed width leaves: a covering sequence of their own
        geom, Cp, Ko = (3, 3, 1, 1), 64, 64
        ws = (58,) if k == 40 - TRIO else (59,) if k == 39 else tuple(v for v in HW if v <= HALO_MAXW)
        label, lo, hi = S("rows", [s for s in strata if _sizes(op, geom, Cp, Ko, s[1], s[2], hs, ws)])
    else:
        label, lo, hi = S("rows", strata)
        lane = fam == "H32" and op != "dgrad"
        geom = S("geom", GEOMS_LANE if lane else GEOMS)
        cs, ks = C_STRATA[fam, op], KO_STRATA[fam, op]
        Cp = S("C", [c for c in cs if any(_sizes(op, geom, c, ko, lo, hi, hs, ws) for ko in ks)])
        Ko = S("Ko", [ko for ko in ks if _sizes(op, geom, Cp, ko, lo, hi, hs, ws)])
    f: Dict[str, object] = {}
    epi = None
    if op == "dgrad" and geom[2] == 1:      # at stride 1 every form exists; the compact residual wants an odd extent
        epi = S("epi", DGRAD_EPI + (DGRAD_EPI_COMPACT if fam == "HPL" else ()))
        if epi.startswith("compact"):
            odd = [(H, W) for H, W in _sizes(op, geom, Cp, Ko, lo, hi, hs, ws) if H % 2 or W % 2]
            hs = tuple(sorted({H for H, W in odd if H % 2})) or hs
    ok = _sizes(op, geom, Cp, Ko, lo, hi, hs, ws)
    H = S("H", sorted({h for h, _ in ok}))
    W = S("W", sorted({w for h, w in ok if h == H}))
    nlo, nhi = _n_range(op, geom, Cp, Ko, H, W, lo, hi)
    N = r.randint(nlo, min(nhi, max(2 * nlo, nlo + 3)))
    R, Sf, stride, pad = geom
    C = REAL_C.get(Cp, Cp) if fam == "H32" and op != "dgrad" else Cp
    form = "pl" if fam == "HPL" else "f32"
    if op == "fwd":
        e = S("epi", FWD_EPI)
        if fam == "H32":
            form = S("form", ("f32", "stem") if Ko % 8 == 0 else ("f32",))
        f.update(shift=bool(e & 1), residual="dense" if e & 2 else "none", relu=bool(e & 4))
        f["bits"] = form != "f32" and f["relu"] and Ko % 64 == 0
    elif op == "dgrad":
        if epi is None:      # stride 2: a class that no tap reaches leaves the plain form only, a 1-wide filter row no sums
            forms = [e for e in DGRAD_EPI if (e == "plain" or G.dgrad_side_ok(H, W, R, Sf, stride, pad))
                     and ("sums" not in e or G.dgrad_sums_ok(H, W, R, Sf, stride, pad))]
            epi = S("epi", forms)
        f.update(residual="compact" if "compact" in epi else "dense" if "residual" in epi else "none", mask="mask" in epi, sums="sums" in epi)
    else:
        f.update(accumulate=S("accumulate", (False, True)), bn=S("bn", WGRAD_BN))
    return ConvCase(i, fam, op, N, H, W, C, Cp, Ko, R, Sf, stride, pad, label, form, profile=S("profile", PROFILES), **f)


def contraction_length(c: ConvCase) -> int:
    Ho, Wo = c.out_hw
    return c.R * c.S * c.Cpad if c.op == "fwd" else c.R * c.S * c.Ko if c.op == "dgrad" else c.N * Ho * Wo


def gemm_rows(c: ConvCase) -> int:
    Ho, Wo = c.out_hw
    return c.N * c.H * c.W if c.op == "dgrad" else c.N * Ho * Wo


def _tile_span_ok(rows_per_image: int, image_elems: int) -> bool:      # csrc/conv_common.h
    return (256 // max(rows_per_image, 1) + 2) * image_elems * 4 < (1 << 31)


def legal(c: ConvCase) -> bool:
    N, H, W, C, Cp, Ko, R, S, stride, pad = c.N, c.H, c.W, c.C, c.Cpad, c.Ko, c.R, c.S, c.stride, c.pad
    pl = c.family == "HPL"
    q = 8 if pl else 4
    ok = N > 0 and H > 0 and W > 0 and R > 0 and S > 0 and pad >= 0 and stride in (1, 2)              # conv_geom_ok
    ok &= H + 2 * pad - R >= 0 and W + 2 * pad - S >= 0
    Ho, Wo = c.out_hw
    ok &= gemm_rows(c) < (1 << 31) and 1 <= C <= Cp
    if c.op == "fwd":
        ok &= Cp % q == 0 and (C == Cp or (not pl and C == REAL_C.get(Cp)))                              # conv_fwd.hip:16
        ok &= _tile_span_ok(Ho * Wo, H * W * Cp)
        if c.form != "f32":
            ok &= Ko % 8 == 0 and (not c.bits or (c.relu and Ko % 64 == 0))                              # conv_fwd.hip:55, prep_epilogue
        else:
            ok &= not c.bits
        if pl:
            ok &= Cp % BK == 0 and R * S <= 32 and R <= 8                                                # conv_fwd.hip:28
        ok &= c.residual in ("none", "dense") and not c.mask and not c.sums
    elif c.op == "dgrad":
        ok &= C == Cp and Cp % q == 0 and Ko % q == 0                                                    # conv_dgrad.hip:81,206
        ok &= Ko % BK == 0 and R * S <= 32 and R <= 8                                                    # conv_dgrad.hip:83
        ok &= _tile_span_ok((H // stride) * (W // stride), Ho * Wo * Ko)
        side = c.residual != "none" or c.mask
        if stride == 2:
            ok &= R <= 3 and S <= 3                                                                      # conv_dgrad.hip:100
            ok &= not side or G.dgrad_side_ok(H, W, R, S, stride, pad)                                   # conv_dgrad.hip:106
            ok &= not c.sums or G.dgrad_sums_ok(H, W, R, S, stride, pad)                                 # conv_dgrad.hip:166,214
        if c.residual == "compact":
            ok &= pl and stride == 1 and N * ((H + 1) // 2) * ((W + 1) // 2) * C * 2 < (1 << 31)         # conv_dgrad.hip:197,199
    else:
        ok &= Cp % q == 0 and Ko % q == 0 and (C == Cp or (not pl and C == REAL_C.get(Cp)))              # conv_wgrad.hip:108,110
        ok &= H * W * Cp * 12 < (1 << 31)                                                                # conv_wgrad.hip:115
        ok &= c.bn in WGRAD_BN
    # the caps of the family
    sizes = [N * H * W * Cp, N * Ho * Wo * Ko, Ko * R * S * Cp]
    assert max(sizes) <= MAX_ELEMS, c
    assert 2 * gemm_rows(c) * (Cp if c.op == "dgrad" else Ko) * contraction_length(c) < MAX_FLOPS if c.op != "wgrad" else \
        2 * Ko * R * S * Cp * contraction_length(c) < MAX_FLOPS, c
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _chan_scale(g, n: int) -> torch.Tensor:
    return 2.0 ** torch.randint(-10, 5, (n,), generator=g).double().float()


def _half_zero(g, t: torch.Tensor) -> torch.Tensor:
    return t * (torch.rand(t.shape, generator=g) < 0.5)


def build(c: ConvCase) -> Dict[str, torch.Tensor]:
    g = SC._gen(c.family, c.index)
    N, H, W, C, Cp, Ko, R, S = c.N, c.H, c.W, c.C, c.Cpad, c.Ko, c.R, c.S
    Ho, Wo = c.out_hw
    sc_c, sc_k = torch.ones(Cp), torch.ones(Ko)
    if c.profile == "chan_scaled":
        sc_c, sc_k = _chan_scale(g, Cp), _chan_scale(g, Ko)
    live = (torch.arange(Cp) < C).float()
    inp: Dict[str, torch.Tensor] = {}
    w = SC._randn(g, Ko, R, S, Cp) / math.sqrt(R * S * C) * live
    rms = float((sc_c[:C] ** 2).mean().sqrt())
    if c.op in ("fwd", "wgrad"):
        x = SC._randn(g, N, H, W, Cp)
        if c.profile == "relu_like":
            x = torch.relu(x)
        inp["x"] = x * sc_c * live
    if c.op in ("dgrad", "wgrad"):
        dy = SC._randn(g, N, Ho, Wo, Ko)
        if c.profile == "relu_like":
            dy = _half_zero(g, dy)
        inp["dy"] = dy * (sc_k if c.op != "fwd" else 1.0)
    if c.op == "fwd":
        inp["w"] = w * sc_k[:, None, None, None]
        if c.shift:
            inp["shift"] = 0.3 * SC._randn(g, Ko) * sc_k * rms
        if c.residual != "none":
            inp["residual"] = SC._randn(g, N, Ho, Wo, Ko) * sc_k * rms
    elif c.op == "dgrad":
        inp["w"] = w * sc_c       # the side of the filter that becomes the output's channels
        out_rms = float((sc_k ** 2).mean().sqrt())
        if c.residual == "dense":
            inp["residual"] = SC._randn(g, N, H, W, Cp) * sc_c * out_rms
        elif c.residual == "compact":
            inp["residual"] = SC._randn(g, N, (H + 1) // 2, (W + 1) // 2, Cp) * sc_c * out_rms
        if c.mask:
            src = SC._randn(g, N, H, W, Cp)
            if c.family == "H32":      # relu_src with exact zeros of either sign: neither passes (relu_src > 0)
                u = torch.rand(src.shape, generator=g)
                src = torch.where(u < 0.1, torch.zeros_like(src), torch.where(u < 0.2, -torch.zeros_like(src), src))
                inp["relu_src"] = src
            else:
                inp["maskin"] = SC.pack_bits((src > 0).view(-1, Cp))
    else:
        inp["w"] = (SC._randn(g, Ko, R, S, Cp) / math.sqrt(R * S * C))[..., :C].contiguous()      # the raw filter, real channels
        inp["scale"], inp["rstd"] = 1 + 0.1 * SC._randn(g, Ko), 0.5 + SC._randn(g, Ko).abs()
        inp["rmean"] = 0.1 * SC._randn(g, Ko)
        dy_seen = SC._seen(None, inp["dy"], c.family == "HPL", torch.float64)
        inp["sumdy"] = dy_seen.reshape(-1, Ko).sum(0).float()
        if c.accumulate:
            k = math.sqrt(contraction_length(c)) * rms
            inp["dw0"] = SC._randn(g, Ko, R, S, C) * sc_k[:, None, None, None] * sc_c[:C] * k
            inp["dgamma0"], inp["dbeta0"] = SC._randn(g, Ko) * sc_k * k, SC._randn(g, Ko) * sc_k * k
    return inp


# ---------------------------------------------------------------------------------------------------------------- reference
def _bilinear(c: ConvCase, a, b):
    """the contraction of the operation in float64: a is x (forward, weight gradient) or dy (data gradient), b the filter or dy"""
    if c.op == "fwd":
        return G.fwd_ref(a, b, c.stride, c.pad)
    if c.op == "dgrad":
        return G.dgrad_ref(a, b, c.H, c.W, c.stride, c.pad)
    return G.wgrad_ref(a, b, c.R, c.S, c.stride, c.pad)


def operands(c: ConvCase, inp):
    return (inp["dy"], inp["w"]) if c.op == "dgrad" else (inp["x"], inp["dy"]) if c.op == "wgrad" else (inp["x"], inp["w"])


def contraction(c: ConvCase, inp, drop_lo_hi: bool = False):
    """(contraction, its magnitude sum) in float64; planes operands: the three plane terms hi hi + hi lo + lo hi (the first two as one
    call, their sum is exact in float64 operands), magnitudes term by term"""
    a, b = operands(c, inp)
    if c.family == "H32":
        a, b = a.double(), b.double()
        return _bilinear(c, a, b), _bilinear(c, a.abs(), b.abs())
    (ah, al), (bh, bl) = ((t.double() for t in SC.canonical_planes(v.contiguous())) for v in (a, b))
    acc = _bilinear(c, ah, bh + bl)
    if not drop_lo_hi:
        acc = acc + _bilinear(c, al, bh)
    return acc, _bilinear(c, ah.abs(), bh.abs() + bl.abs()) + _bilinear(c, al.abs(), bh.abs())


def _cached_contraction(c: ConvCase, inp):
    if "aux:acc" not in inp:
        inp["aux:acc"], inp["aux:mag"] = contraction(c, inp)
    return inp["aux:acc"], inp["aux:mag"]


def scatter_compact(c: ConvCase, comp: torch.Tensor, He=None, We=None) -> torch.Tensor:
    """the compact residual [N, (H + 1) / 2, (W + 1) / 2, C] at the pixels with even (h, w); He, We: the extents a (wrong) kernel indexes with"""
    He, We = He or (c.H + 1) // 2, We or (c.W + 1) // 2
    flat = comp.reshape(-1, c.Cpad)
    n, h, w = torch.arange(c.N)[:, None, None], torch.arange(0, c.H, 2)[None, :, None], torch.arange(0, c.W, 2)[None, None, :]
    j = ((n * He + h // 2) * We + w // 2).clamp(max=flat.shape[0] - 1)
    out = torch.zeros(c.N, c.H, c.W, c.Cpad, dtype=comp.dtype)
    out[:, ::2, ::2] = flat[j]
    return out


def dgrad_mask(c: ConvCase, inp) -> Optional[torch.Tensor]:
    if not c.mask:
        return None
    if "relu_src" in inp:
        return inp["relu_src"] > 0
    return SC.unpack_bits(inp["maskin"], c.Cpad).view(c.N, c.H, c.W, c.Cpad)


def epilogue(c: ConvCase, inp, acc, mag, dt, **wrong):
    """the epilogue of include/cxrk.h in `dt` on a contraction (float64; float32 rounds it once first).  `wrong`: the fakes of
    tests/test_sweep_host.py"""
    acc, mag = acc.to(dt), mag.to(dt)
    pl = c.family == "HPL"
    if c.op == "fwd":
        pre, m = acc, mag
        if c.shift:
            pre, m = pre + inp["shift"].to(dt), m + inp["shift"].to(dt).abs()
        if c.residual != "none":
            res = SC._seen(None, inp["residual"], c.form != "f32", dt)
            pre, m = pre + res, m + res.abs()
        return {"y": torch.relu(pre) if c.relu else pre, "mag:y": m}
    if c.op == "dgrad":
        v, m = acc, mag
        if c.residual != "none":
            res = SC._seen(None, inp["residual"], pl, dt)
            if c.residual == "compact":
                res = scatter_compact(c, res, wrong.get("He"), wrong.get("We"))
            v, m = v + res, m + res.abs()
        keep = dgrad_mask(c, inp)
        if keep is not None:
            v, m = v * keep, m * keep
        out = {"dx": v, "mag:dx": m}
        if c.sums:
            out["sums"], out["mag:sums"] = v.reshape(-1, c.Cpad).sum(0), m.reshape(-1, c.Cpad).sum(0)
        return out
    raw, mraw = acc[..., :c.C], mag[..., :c.C]
    scale = inp["scale"].to(dt) if c.bn != "noscale" else torch.ones(c.Ko, dtype=dt)
    dw, mdw = scale[:, None, None, None] * raw, scale.abs()[:, None, None, None] * mraw
    if c.accumulate:
        dw, mdw = inp["dw0"].to(dt) + dw, mdw + inp["dw0"].to(dt).abs()
    out = {"dw": dw, "mag:dw": mdw}
    if c.bn != "none":
        w, rstd, mean, sumdy = (inp[k].to(dt) for k in ("w", "rstd", "rmean", "sumdy"))
        if wrong.get("dgamma") == "scaled_filter":
            w = w * scale[:, None, None, None]
        dot = (w * raw).sum((1, 2, 3)) - (0.0 if wrong.get("dgamma") == "no_mean" else mean * sumdy)
        dg, mdg = rstd * dot, rstd.abs() * ((w.abs() * mraw).sum((1, 2, 3)) + (mean * sumdy).abs())
        db = inp["sumdy"]
        if c.accumulate:
            dg, mdg = inp["dgamma0"].to(dt) + dg, mdg + inp["dgamma0"].to(dt).abs()
            db = inp["dbeta0"] + inp["sumdy"]          # float32, rounded once: what the kernel's one addition gives
        out.update({"dgamma": dg, "mag:dgamma": mdg, "dbeta": db})
    return out


def evaluate(c: ConvCase, inp, dt) -> Dict[str, torch.Tensor]:
    acc, mag = _cached_contraction(c, inp)
    return epilogue(c, inp, acc, mag, dt)


# ---------------------------------------------------------------------------------------------------------------- comparators
E32_OUTPUTS = ("y", "dx", "sums", "dw", "dgamma")


def level(c: ConvCase, name: str, got, ref) -> Tuple[float, tuple]:
    """the comparator of the precision level: dw per filter, everything else per output channel (a vector: per element)"""
    if name == "dw":
        return SC.row_scaled(got.reshape(c.Ko, -1), ref.reshape(c.Ko, -1))
    return SC.col_scaled(got.reshape(ref.shape), ref)


def floor(c: ConvCase, name: str, split: bool) -> float:
    low = split or c.family == "HPL" or c.planes_out
    if name == "dgamma":
        return 2e-2 if low else 2e-3
    f = 2e-5 if c.op == "fwd" else 5e-5
    return max(f, 3e-4) if low else f


def mainloop_c(c: ConvCase) -> float:
    return ((3 if c.family == "HPL" else 1) * contraction_length(c) + 8) * SC.U24


def check(c: ConvCase, ref, got, split: bool = False) -> List[Tuple[str, float, tuple]]:
    """[(output, error / elementwise bound, index), (output + "/level", error / max(floor, 8 e32), index)]; dbeta bit for bit"""
    cc = mainloop_c(c)
    res = []
    for name in E32_OUTPUTS:
        if name not in got:
            continue
        g, rf, mag = got[name].reshape(ref[name].shape), ref[name], ref["mag:" + name]
        extra = None
        if name == "dgamma":
            k = cc + (c.R * c.S * c.Cpad + 8) * SC.U24 + (2 * SC.U24 if c.accumulate else 0.0)
        elif name == "sums":
            k = cc + (gemm_rows(c) + 8) * SC.U24
            extra = (SC.PLANES_TOL * ref["dx"].abs()).reshape(-1, c.Cpad).sum(0) if c.planes_out else None
        else:
            k = cc
            extra = SC.PLANES_TOL * rf.abs() if c.planes_out else None
        res.append((name,) + SC.forward_bound(g, rf, mag, k, extra))
        ratio, idx = level(c, name, g, rf)
        res.append((name + "/level", ratio / max(floor(c, name, split), 8.0 * SC.E32[SC.group(c, name)]), idx))
    if "dbeta" in got:
        res.append(("dbeta",) + SC.exact_equal(got["dbeta"].float(), ref["dbeta"].float()))
    return res


# ---------------------------------------------------------------------------------------------------------------- dispatch, restated
def use_wide256(M: int, N: int, K: int, splitk: int, planes: bool, mode: int, min_k: int = 512) -> bool:      # csrc/gemm_core.h
    if not planes:
        return False
    if mode == 2:
        return True
    if 2.0 * M * N * K < 1073741824.0 or mode == 0 or M < 256 or N < 256:
        return False
    if (K // splitk if splitk > 1 else K) < min_k:
        return False
    tiles = -(-M // 256) * -(-N // 256) * max(splitk, 1)
    return tiles * 100 >= -(-tiles // 256) * 256 * 60


def pick_tile(kind: str, M: int, N: int, K: int, splitk: int, planes: bool, mode: int) -> str:      # csrc/gemm_dispatch.h
    if use_wide256(M, N, K, splitk, planes, mode, 64 if kind == "dgrad" else 512):
        return "256x256"
    if kind != "wgrad" and N <= 64:
        return "256x64"
    if kind == "wgrad" and M <= 64:
        return "64x256"
    return "128x128"


def wgrad_splitk_policy(M: int, N: int, K: int, planes: bool, mode: int) -> int:      # csrc/gemm_misc.hip
    maxk = max(K // (8 * BK), 1)
    if planes and mode != 0 and M >= 256 and N >= 256:
        sk = min(max(min(256 // (-(-M // 256) * -(-N // 256)), maxk), 1), 512)
        if use_wide256(M, N, K, sk, True, mode):
            return sk
    tiles = -(-M // 128) * -(-N // 128)
    return max(min((1536 + tiles - 1) // tiles, K // 256, 512), 1)


def slabs_written(K: int, splitk: int) -> int:      # launch_gemm / launch_gemm_pw / launch_conv3x3_wgrad_window
    if splitk <= 1:
        return 1
    kchunk = -(-(-(-K // splitk)) // BK) * BK
    return -(-K // kchunk)


def s2_classes(c: ConvCase):
    """csrc/conv_dgrad.hip s2_classes: [(ph, pw, Hs, Ws, row taps [(r, offset)], column taps)] of the classes that have pixels"""
    out = []
    for ph in range(2):
        for pw in range(2):
            Hs, Ws = (c.H - ph + 1) // 2, (c.W - pw + 1) // 2
            if Hs <= 0 or Ws <= 0:
                continue
            tr = [(r, (ph + c.pad - r) // 2) for r in range(c.R) if (ph + c.pad - r) % 2 == 0]
            ts = [(s, (pw + c.pad - s) // 2) for s in range(c.S) if (pw + c.pad - s) % 2 == 0]
            out.append((ph, pw, Hs, Ws, tr, ts))
    return out


def halo_applies(H, W, C, Ko, R, S, stride, pad) -> bool:      # csrc/conv_halo.h
    return (R, S, stride, pad) == (3, 3, 1, 1) and C == HALO_CH and Ko == 64 and W <= HALO_MAXW and H >= 1


_PW = {"256x256": "Pw256", "256x64": "Pw256x64", "64x256": "Pw64x256", "128x128": "Pw128"}
_WAVES = {"256x64": "4,1", "64x256": "1,4", "128x128": "2,2"}


def _label(planes: bool, tile: str, la: str, lb: str) -> str:
    if planes:
        return f"gemm_pw_kernel<{_PW[tile]},Dma{la},Dma{lb}>"
    return f"gemm_f32_kernel<{la},{lb},{_WAVES[tile]}>"


def predict(c: ConvCase, wide: bool = False, window_wgrad: bool = True) -> Dict[str, object]:
    """what the library launches for the case: `count` MFMA launches, `label` (the grammar of tests/test_launch_labels_gpu.py), `tile`,
    `path` ("gemm", "halo", "window"), `gather` ("tap", "lane"), `split_bf16`; weight gradient: `splitk` (the policy's answer),
    `slabs`, `sg_log2`; data gradient at stride 2: `classes` = [(M, K, negative tap offset)] of the launched ones, `zero_class`;
    `epi`: the branch of prep_epilogue ("fast", "vec", "scalar") and `kind_m1` (an fp32 output with N % 64 != 0)"""
    mode = 2 if wide else 1
    pl = c.family == "HPL"
    N, H, W, Cp, Ko, R, S, stride, pad = c.N, c.H, c.W, c.Cpad, c.Ko, c.R, c.S, c.stride, c.pad
    Ho, Wo = c.out_hw
    p: Dict[str, object] = {"count": 1, "split_bf16": int(pl), "path": "gemm"}
    if c.op == "fwd":
        M, Nn, Kd = N * Ho * Wo, Ko, R * S * Cp
        p["gather"] = "tap" if Cp % BK == 0 and R * S <= 32 and R <= 8 else "lane"
        tile = pick_tile("fwd", M, Nn, Kd, 1, pl, mode)
        if pl and halo_applies(H, W, Cp, Ko, R, S, stride, pad) and tile != "256x256":
            p.update(path="halo", label="conv3x3_halo_kernel<fwd>")
        else:
            p["label"] = _label(pl, tile, "ConvIm2colKC", "DenseKC")
    elif c.op == "dgrad":
        M, Nn, Kd = N * H * W, Cp, R * S * Ko
        if stride == 1:
            tile = pick_tile("dgrad", M, Nn, Kd, 1, pl, mode)
            if pl and halo_applies(H, W, Ko, Cp, R, S, stride, pad) and tile != "256x256":
                p.update(path="halo", label="conv3x3_halo_kernel<dgrad>")
            else:
                p["label"] = _label(pl, tile, "ConvDgradKC", "ConvFilterMC")
        else:
            cls = s2_classes(c)
            live = [(N * Hs * Ws, len(tr) * len(ts) * Ko, min(o for _, o in tr + ts) < 0) for _, _, Hs, Ws, tr, ts in cls if tr and ts]
            p.update(count=len(live), classes=live, zero_class=len(live) < len(cls))
            Ms, Ks, _ = max(live, key=lambda t: t[0] * t[1])
            tile = pick_tile("dgrad", Ms, Nn, Ks, 1, pl, mode)
            p["label"] = _label(pl, tile, "ConvDgradS2KC", "ConvFilterS2MC")
    else:
        M, Nn, Kd = Ko, R * S * Cp, N * Ho * Wo
        sk = wgrad_splitk_policy(M, Nn, Kd, pl, mode)
        tile = pick_tile("wgrad", M, Nn, Kd, sk, pl, mode)
        slabs = slabs_written(Kd, sk)
        p.update(splitk=sk, slabs=slabs, sg_log2=4 if slabs >= 64 else 2 if slabs >= 8 else 0)
        if pl and window_wgrad and halo_applies(H, W, Cp, Ko, R, S, stride, pad):
            p.update(path="window", label="conv3x3_wgrad_window_kernel", count=1 if slabs <= 256 else 2)
        else:
            p["label"] = _label(pl, tile, "DenseMC", "ConvIm2colMC")
    p["tile"] = tile if p["path"] == "gemm" else None
    # prep_epilogue (csrc/gemm_core.h): vec = 16-byte accesses (N % 4 == 0), fast adds N % 8 == 0 (all a planes operand is served by);
    # an fp32-output feature set with N % 64 != 0 leaves the specialised 4 + 4 lane map (kind = -1)
    p["epi"] = "fast" if Nn % 8 == 0 else "vec" if Nn % 4 == 0 else "scalar"
    p["kind_m1"] = (c.op == "wgrad" or c.form == "f32") and Nn % 64 != 0
    p["mnk"] = (M, Nn, Kd)
    return p
