"""Seeded, stratified case generators, float64 references, comparators and bounds of the differential sweep
(tests/test_sweep_host.py on the CPU, tests/test_sweep_gpu.py on the GPU).

  cases(family)            the frozen-dataclass cases of family "A" (attention), "B32" / "BPL" (dense GEMM on fp32 / planes operands),
                           "C" (column reductions), "D" (row-wise heads), "E" (BERT row kernels: LayerNorm, embedding, gelu',
                           planes_add_rows), "F" (image-side non-GEMM kernels: max-pool, layout, spatial mean, BatchNorm folding, the
                           train-mode BatchNorm chain), "G" (masked-language-modelling kernels: token masking, gather / scatter of
                           the selected rows, one chunked vocabulary sweep of the cross-entropy kernels, the whole head at
                           H = 768), "H32" / "HPL" (the convolutions on fp32 / planes operands, one of forward, data gradient and
                           weight gradient per case: generators, references and bounds in tests/sweep_conv_cases.py, registered
                           here); a pure function of (SEED, family, index)
  legal(case)              the rules the entry points check (include/cxrk.h), restated; every generated case satisfies them
  build(case)              CPU inputs (float32; masks int64, decision bits uint8, winners int32)
  evaluate(case, inp, dt)  the operation's defining formula in torch on the CPU in dtype `dt`
  reference(case, inp)     evaluate(..., float64)
  check(case, ref, got)    [(output name, error / bound, worst index)] through the family's comparator and bound

Sampling: every dimension of a family has a list of strata.  Case i takes, per dimension, the stratum `perm[i % n]` of a
permutation that is redrawn for every block of n consecutive cases (a covering schedule: each aligned block of n cases hits all n
strata, so the first max(n) cases of a family hit every stratum of every dimension), then random values inside the stratum.  Where
one dimension's draw narrows another's legal strata (an interior key tile needs L > 128, decision bits N % 64 == 0, ...), the
narrowed list has a covering sequence of its own (`Schedule`).

Bounds.  GEMM: elementwise |got - ref| <= c * mag with mag the float64 sum of magnitudes |alpha| |A| |B| + |bias| + |R| and
c = (K + 8) 2^-24 (fp32 mainloop: gamma_K of a sum of K products in any order, plus the epilogue's own operations) or
(3 K + 8) 2^-24 on the magnitudes of the three plane terms (planes mainloop; the reference is the sum of those terms, exact_ref.py).
A GELU / gelu' epilogue adds 2^-16 mag (the erf tolerance of test_gelu_epilogue_writers, on the magnitude the factor multiplies), a
planes output 2^-16 |ref| (exact_ref.assert_two_roundings, statement 1).  Attention, column reductions, heads: the project's
floors (2e-5 forward, 5e-5 backward, 1e-6 column means, 3e-4 planes / split mode) per row or per column, or 8 e32 where that is
larger: e32 is the same comparator on evaluate(..., float32) -- torch on the CPU, never a kernel -- maximised over the family's
cases of one (output group, profile); the table E32 below is pinned from both sides by tests/test_sweep_host.py.
E and F: copies, maxima and winning taps bit for bit; sums of a few terms elementwise against a derived multiple of 2^-24 on the
magnitudes of their terms (max-pool backward 3: at most four terms; embedding gradient count + 2; planes_add_rows 2; spatial mean P + 2,
its backward 3: fl(1 / P), the product, the optional addition); gelu' as in the GEMM epilogue; everything else per row or per column
against max(floor, 8 e32) as above.
G: the mask, gather, scatter, `hit` and `correct` (decisions and copies) bit for bit, as are the zeros behind the kept rows and in the
tail chunk's overlap columns; lse, row loss and loss per row against max(2e-6, 8 e32) (2e-6: test_cross_entropy_kernels); the logits
gradient elementwise against 8 e32 2^-24 |f| (p + [column == target]) (1 + |S| + |bias| + |x| + |lse|) + |f| 2^-126, from the float32
rounding of the reference's log-sum-exp (the kernel is judged from given saved values, as attn_backward), with e32 measured on
(exp(x - lse) - [target]) f in float32; the head's outputs per row (a vector is one row) against max(floor, 8 e32).

No GPU and no library import here."""
from __future__ import annotations

import math
import random
import zlib
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

SEED = 20261020
NCASES = {"A": 105, "B32": 96, "BPL": 96, "C": 104, "D": 112, "E": 111, "F": 102, "G": 108, "H32": 120, "HPL": 120}
FLOOR_REL = 1e-3     # a row / column below 1e-3 of its tensor's scale is judged as if it were at 1e-3 (today's metric judges it at 1)
U24 = 2.0 ** -24
ERF_TOL = 2.0 ** -16      # test_gelu_epilogue_writers (exact_ref.assert_two_roundings): what the library promises around erf
PLANES_TOL = 2.0 ** -16   # |hi + lo - y| <= 2^-16 |y|
PADS = (0, 8, 24, 64)
ALPHAS = (1.0, -0.5, 14.285)


# ---------------------------------------------------------------------------------------------------------------- sampling
def _rng(family: str, index: int, salt: str = "") -> random.Random:
    return random.Random(f"{SEED}/{family}/{index}/{salt}")


def _gen(family: str, index: int, salt: str = "") -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(f"{SEED}/{family}/{index}/{salt}".encode()))


def stratum(family: str, dim: str, strata, i: int):
    """covering schedule: the strata in a fresh random order for every block of len(strata) consecutive draws"""
    n = len(strata)
    perm = list(range(n))
    random.Random(f"{SEED}/{family}/{dim}/{n}/{i // n}").shuffle(perm)
    return strata[perm[i % n]]


class Schedule:
    """the draws of one family, case after case.  A dimension whose legal strata depend on another dimension's draw has one
    covering sequence per strata list (its own counter), so each list is covered by the cases that draw from it."""

    def __init__(self, family: str):
        self.family, self.count = family, {}

    def __call__(self, dim: str, strata):
        strata = tuple(strata)
        k = self.count.get((dim, strata), 0)
        self.count[(dim, strata)] = k + 1
        return stratum(self.family, dim, strata, k)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---------------------------------------------------------------------------------------------------------------- comparators
def _finite(got):
    return bool(torch.isfinite(got).all())


def row_scaled(got: torch.Tensor, ref: torch.Tensor, floor_rel: float = FLOOR_REL) -> Tuple[float, tuple]:
    """per output row (last dimension): max |got - ref| / max(max |ref_row|, floor), floor = floor_rel max |ref|.
    -> (worst ratio, index of the worst element); a non-finite or missing element counts as infinitely wrong"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0, ()
    if ref.dim() == 0:
        got, ref = got.reshape(1, 1), ref.reshape(1, 1)
    if not _finite(got):
        return math.inf, tuple((~torch.isfinite(got)).nonzero()[0].tolist())
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    floor = max(floor_rel * float(r2.abs().max()), 1e-30)
    ratio = (g2 - r2).abs() / r2.abs().max(1, keepdim=True).values.clamp_min(floor)
    k = int(ratio.argmax())
    return float(ratio.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), got.shape))


def col_scaled(got: torch.Tensor, ref: torch.Tensor, floor_rel: float = FLOOR_REL) -> Tuple[float, tuple]:
    """the same per column of a [..., C] tensor (a [C] vector: per element)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not _finite(got):
        return math.inf, tuple((~torch.isfinite(got)).nonzero()[0].tolist())
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    floor = max(floor_rel * float(r2.abs().max()), 1e-30)
    ratio = (g2 - r2).abs() / r2.abs().max(0, keepdim=True).values.clamp_min(floor)
    k = int(ratio.argmax())
    return float(ratio.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), got.shape))


def forward_bound(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, c: float, extra=None) -> Tuple[float, tuple]:
    """elementwise |got - ref| <= c mag (+ extra): -> (worst |got - ref| / bound, its index)"""
    got, ref, mag = got.detach().double().cpu(), ref.detach().double().cpu(), mag.detach().double().cpu()
    assert got.shape == ref.shape == mag.shape, (tuple(got.shape), tuple(ref.shape), tuple(mag.shape))
    if not _finite(got):
        return math.inf, tuple((~torch.isfinite(got)).nonzero()[0].tolist())
    bound = c * mag + (extra if extra is not None else 0.0)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    k = int(ratio.argmax())
    return float(ratio.reshape(-1)[k]), tuple(int(v) for v in torch.unravel_index(torch.tensor(k), got.shape))


def tensor_wide(got: torch.Tensor, ref: torch.Tensor) -> float:
    """today's metric (close() of tests/test_kernels_gpu.py): max |got - ref| / max |ref|"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not _finite(got):
        return math.inf
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


# ================================================================================================================ family A
A_L = (1, 2, 7, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 255, 256, 257, 511, 512)
A_DH = (4, 8, 12, 28, 32, 36, 60, 64)
A_NH = (1, 2, 3)
A_B = (1, 2, 5)
A_MASKS = ("ones", "suffix", "prefix", "holes", "tile", "single", "empty")
A_PROFILES = ("base", "std8", "std30_outlier", "flat")


@dataclass(frozen=True)
class AttnCase:
    index: int
    B: int
    L: int
    nH: int
    dH: int
    mask: str       # the pattern of every sequence of the case, parameters redrawn per sequence ("empty": one sequence has no key)
    profile: str


def _gen_a(i: int, S: Schedule) -> AttnCase:
    L, dH, nH = S("L", A_L), S("dH", A_DH), S("nH", A_NH)
    # an interior 64-key tile exists from three tiles on; the empty sequence stands next to a non-empty one
    mask = S("mask", A_MASKS if L > 128 else [m for m in A_MASKS if m != "tile"])
    B = S("B", A_B if mask != "empty" else [v for v in A_B if v > 1])
    return AttnCase(i, B, L, nH, dH, mask, S("profile", A_PROFILES))


def attention_mask(c: AttnCase) -> torch.Tensor:
    """int64 {0, 1} key mask [B, L]; L = 1 leaves only "ones" and "empty" distinguishable"""
    r = _rng("A", c.index, "mask")
    m = torch.ones(c.B, c.L, dtype=torch.int64)
    L = c.L
    empty_at = r.randrange(c.B) if c.mask == "empty" else -1
    for b in range(c.B):
        kind = c.mask
        if b == empty_at:
            m[b] = 0
            continue
        if kind == "empty":
            kind = r.choice(("ones", "suffix", "prefix", "holes", "single"))
        if L == 1 or kind == "ones":
            continue
        if kind == "suffix":
            m[b, L - r.randint(1, L - 1):] = 0
        elif kind == "prefix":
            m[b, :r.randint(1, L - 1)] = 0
        elif kind == "holes":
            bits = torch.tensor([r.random() < 0.5 for _ in range(L)])
            if not bool(bits.any()):
                bits[r.randrange(L)] = True
            m[b] = bits.long()
        elif kind == "tile":
            t = r.randint(1, (L - 1) // 64 - 1)     # neither the first nor the last tile
            m[b, 64 * t:64 * t + 64] = 0
        elif kind == "single":
            m[b] = 0
            m[b, r.randrange(L)] = 1
    return m


def _build_a(c: AttnCase):
    g = _gen("A", c.index)
    W = c.nH * c.dH
    qkv = (_randn(g, c.B * c.L, 3 * W) * 0.7).view(c.B, c.L, 3, W)
    mask = attention_mask(c)
    if c.profile == "std8":
        qkv[:, :, :2] *= 4.0
    elif c.profile == "std30_outlier":
        qkv[:, :, :2] *= 8.0
        r = _rng("A", c.index, "outlier")
        t0 = 64 * ((c.L - 1) // 64)
        for b in range(c.B):
            live = mask[b].nonzero().flatten().tolist()
            if not live:
                continue
            last = [j for j in live if j >= t0]
            j = r.choice(last) if last else live[-1]      # the last key tile; the last live key where that tile has none
            qkv[b, j, 1] *= 6.0
    elif c.profile == "flat":
        qkv[:, :, 0] = 0.0
    return {"qkv": qkv.reshape(c.B * c.L, 3 * W).contiguous(), "mask": mask, "dctx": _randn(g, c.B * c.L, W)}


def _attn_scores(c: AttnCase, x, mask):
    q, k, v = x.view(c.B, c.L, 3, c.nH, c.dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(c.dH)
    live = mask.bool()
    empty = ~live.any(1)
    # live keys only; the padding-only sequence is uniform over all L keys (HF's additive finfo.min absorbs every score) and its
    # gradient is that of a softmax at equal scores, which s - s.detach() states exactly
    s = torch.where(empty[:, None, None, None], s - s.detach(), s.masked_fill(~live[:, None, None, :], -math.inf))
    return s, v


def _eval_a(c: AttnCase, inp, dt):
    x = inp["qkv"].to(dt).clone().requires_grad_(True)
    s, v = _attn_scores(c, x, inp["mask"])
    p = torch.softmax(s, -1)
    ctx = (p @ v).transpose(1, 2).reshape(c.B * c.L, c.nH * c.dH)
    ctx.backward(inp["dctx"].to(dt))
    return {"probs": p.detach(), "ctx": ctx.detach(), "dqkv": x.grad}


def attn_backward(c: AttnCase, inp, probs, dt=torch.float64):
    """d qkv from GIVEN probabilities (those the kernel's forward wrote): dV = P^T dO, dS = P o (dP - rowsum(P o dP)) / sqrt(d)"""
    x = inp["qkv"].to(dt)
    q, k, v = x.view(c.B, c.L, 3, c.nH, c.dH).permute(2, 0, 3, 1, 4)
    do = inp["dctx"].to(dt).view(c.B, c.L, c.nH, c.dH).permute(0, 2, 1, 3)
    p = probs.to(dt)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) / math.sqrt(c.dH)
    d = torch.stack([ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do])      # [3, B, nH, L, dH]
    return d.permute(1, 3, 0, 2, 4).reshape(c.B * c.L, 3 * c.nH * c.dH)


# ================================================================================================================ family B
B_MN = (8, 16, 56, 64, 72, 120, 128, 136, 248, 256, 264, 520)
B_K = (8, 16, 24, 32, 40, 64, 72, 264, 520)
B_FORMS = {"B32": ("NT", "NN", "TN", "TT"), "BPL": ("NT", "NN", "TN")}
B_EPI = {"B32": ("plain", "splitk2", "splitk3", "splitk7", "bias_act", "residual", "aux", "accumulate", "mixed"),
         "BPL": ("plain", "splitk2", "splitk3", "splitk7", "bias_act", "residual", "aux", "accumulate", "mixed", "maskout", "colsum")}
B_PROFILES = ("randn", "scaled")
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


@dataclass(frozen=True)
class GemmCase:
    index: int
    family: str        # "B32": K.gemm on fp32 operands, "BPL": K.gemm_pl on planes operands
    M: int
    N: int
    K: int
    form: str          # N / T per operand: transA, transB
    epi: str           # the stratum the epilogue was drawn from
    pad_a: int
    pad_b: int
    pad_c: int
    pad_r: int
    pad_aux: int
    pad_c2: int
    gap_a: int         # planes only: extra elements between the hi and the lo plane
    gap_b: int
    gap_c: int
    gap_r: int
    bias: bool
    residual: str      # "none", "f32", "pl"
    preact: bool
    act: int
    auxmode: int       # 0 none, 1 (aux > 0), 2 gelu'(aux), 3 decision bits (planes)
    alpha: float
    accumulate: bool
    maskout: bool
    colsum: str        # "none", "fresh", "acc"
    splitk: int
    out_planes: bool
    profile: str

    @property
    def ta(self):
        return self.form[0] == "T"

    @property
    def tb(self):
        return self.form[1] == "T"


def _gen_b(i: int, S: Schedule) -> GemmCase:
    fam = S.family
    r = _rng(fam, i)
    pl = fam == "BPL"
    M, N, Kd = S("M", B_MN), S("N", B_MN), S("K", B_K)
    form, epi = S("form", B_FORMS[fam]), S("epi", B_EPI[fam])
    pads = {k: S(k, PADS) for k in ("pad_a", "pad_b", "pad_c", "pad_r", "pad_aux", "pad_c2")}
    gaps = {k: (S(k, PADS) if pl else 0) for k in ("gap_a", "gap_b", "gap_c", "gap_r")}
    alpha, profile = S("alpha", ALPHAS), S("profile", B_PROFILES)
    f = dict(bias=False, residual="none", preact=False, act=ACT_NONE, auxmode=0, accumulate=False, maskout=False, colsum="none", splitk=1,
             out_planes=False)
    res_kinds = ("f32", "pl") if pl else ("f32",)
    coin = lambda: r.random() < 0.5      # noqa: E731
    if epi.startswith("splitk"):         # plain epilogue, fp32 output (gemm_f32.hip:23, gemm_pl.hip:58)
        f.update(splitk=int(epi[6:]), accumulate=coin())
    elif epi == "bias_act":
        f.update(bias=True, act=r.choice((ACT_RELU, ACT_GELU)), preact=coin(), residual=r.choice(("none",) + res_kinds), out_planes=pl and coin())
    elif epi == "residual":
        f.update(residual=r.choice(res_kinds), bias=coin(), out_planes=pl and coin())
    elif epi == "aux":
        f.update(auxmode=r.choice((2, 3) if pl else (1, 2)), residual=r.choice(("none",) + res_kinds), out_planes=pl and coin())
    elif epi == "accumulate":            # C += result: no residual (gemm_f32.hip:27, gemm_pl.hip:62), fp32 output
        f.update(accumulate=True, bias=coin())
    elif epi == "mixed":
        f.update(bias=coin(), residual=r.choice(("none",) + res_kinds), preact=coin(), act=r.choice((ACT_NONE, ACT_RELU, ACT_GELU)),
                 auxmode=r.choice((0, 2, 3) if pl else (0, 1, 2)), out_planes=pl and coin())
    elif epi == "maskout":               # ReLU, with the decision bits of this launch where the width allows them (below)
        f.update(act=ACT_RELU, bias=coin(), residual=r.choice(("none",) + res_kinds), out_planes=coin())
    elif epi == "colsum":                # fused column sums of the stored output: splitk == 1 (gemm_pl.hip:54)
        f.update(colsum=r.choice(("fresh", "acc")), auxmode=r.choice((0, 2)), out_planes=coin(), residual=r.choice(("none",) + res_kinds))
    if f["auxmode"] and f["act"]:        # one factor per launch in the sweep: an activation or an aux multiplier
        f["act"] = ACT_NONE
    # every planes launch with a ReLU also writes its decision bits where they exist: N % 64 == 0 (gemm_core.h prep_epilogue)
    f["maskout"] = pl and f["act"] == ACT_RELU and N % 64 == 0
    return GemmCase(index=i, family=fam, M=M, N=N, K=Kd, form=form, epi=epi, alpha=alpha, profile=profile, **pads, **gaps, **f)


def gemm_lds(c: GemmCase) -> Dict[str, int]:
    """leading dimensions in elements"""
    a_cols, b_cols = (c.M if c.ta else c.K), (c.K if c.tb else c.N)
    return {"lda": a_cols + c.pad_a, "ldb": b_cols + c.pad_b, "ldc": c.N + c.pad_c, "ldr": c.N + c.pad_r, "ldaux": c.N + c.pad_aux,
            "ldc2": c.N + c.pad_c2}


def _legal_b(c: GemmCase) -> bool:
    pl = c.family == "BPL"
    ld = gemm_lds(c)
    a_rows, b_rows = (c.K if c.ta else c.M), (c.N if c.tb else c.K)
    q = 8 if pl else 4
    ok = c.M > 0 and c.N > 0 and c.K > 0                                               # gemm_f32.hip:11 / gemm_pl.hip:42
    ok &= ld["lda"] % q == 0 and ld["ldb"] % q == 0                                    # gemm_f32.hip:12 / gemm_pl.hip:43
    if pl:
        ok &= (a_rows * ld["lda"] + c.gap_a) % 8 == 0 and (b_rows * ld["ldb"] + c.gap_b) % 8 == 0      # aplane, bplane: gemm_pl.hip:43
        ok &= not (c.ta and c.tb)                                                      # gemm_pl.hip:46
        ok &= c.auxmode in (0, 2, 3)                                                   # gemm_pl.hip:47
    else:
        ok &= c.auxmode in (0, 1, 2)                                                   # gemm_f32.hip:15
        ok &= not c.maskout and c.colsum == "none" and not c.out_planes and c.residual != "pl" and c.auxmode != 3
    ok &= (c.M % q == 0) if c.ta else (c.K % q == 0)                                   # gemm_f32.hip:13 / gemm_pl.hip:44
    ok &= (c.K % q == 0) if c.tb else (c.N % q == 0)                                   # gemm_f32.hip:14 / gemm_pl.hip:45
    ok &= ld["lda"] < (1 << 20) and ld["ldb"] < (1 << 20)                              # gemm_f32.hip:17 / gemm_pl.hip:48
    plain = not c.bias and c.residual == "none" and c.auxmode == 0 and not c.maskout and not c.preact and c.act == ACT_NONE
    if c.splitk > 1:
        ok &= plain and c.N % 4 == 0 and not c.out_planes                              # gemm_f32.hip:23 / gemm_pl.hip:58
    if c.colsum != "none":
        ok &= c.splitk == 1 and c.N % 8 == 0                                           # gemm_pl.hip:54
    if c.accumulate:
        ok &= c.residual == "none" and not c.out_planes                                # gemm_f32.hip:27 / gemm_pl.hip:62
        ok &= c.act == ACT_NONE and c.auxmode == 0     # "C += result" (cxrk.h:47) is stated for the linear epilogue only
    if pl:      # the planes path serves the 16-byte epilogue only (gemm_pw.h:644 with gemm_core.h prep_epilogue)
        ok &= c.N % 8 == 0 and all(ld[k] % 4 == 0 for k in ("ldc", "ldr", "ldaux", "ldc2"))
        if c.out_planes:
            ok &= ld["ldc"] % 8 == 0 and (c.M * ld["ldc"] + c.gap_c) % 8 == 0
        if c.residual == "pl":
            ok &= ld["ldr"] % 8 == 0 and (c.M * ld["ldr"] + c.gap_r) % 8 == 0
        if c.maskout:
            ok &= c.act == ACT_RELU and c.N % 64 == 0                                  # prep_epilogue: maskout needs ReLU, N % 64
    return bool(ok)


def canonical_planes(y32: torch.Tensor):
    """exact_ref.canonical_planes: hi = bf16(y), lo = bf16(y - hi)"""
    hi = y32.bfloat16()
    return hi, (y32 - hi.float()).bfloat16()


def _build_b(c: GemmCase):
    g = _gen(c.family, c.index)
    M, N, Kd = c.M, c.N, c.K
    rs, cs = torch.ones(M), torch.ones(N)
    if c.profile == "scaled":
        rs, cs = 10.0 ** (torch.rand(M, generator=g) * 6 - 3), 10.0 ** (torch.rand(N, generator=g) * 6 - 3)
    a = _randn(g, M, Kd) * rs[:, None]          # op(A)[M, K]
    b = _randn(g, Kd, N) * cs[None, :]          # op(B)[K, N]
    out_scale = rs[:, None] * cs[None, :] * math.sqrt(Kd)
    inp = {"a": (a.T if c.ta else a).contiguous(), "b": (b.T if c.tb else b).contiguous()}
    if c.bias:
        inp["bias"] = _randn(g, N) * cs
    if c.residual != "none":
        inp["residual"] = _randn(g, M, N) * out_scale
    if c.accumulate:
        inp["c0"] = _randn(g, M, N) * out_scale
    if c.auxmode in (1, 2):
        inp["aux"] = _randn(g, M, N)
    if c.auxmode == 3:
        inp["maskin"] = pack_bits(torch.rand(M, N, generator=g) < 0.5)
    if c.colsum == "acc":
        inp["colsum0"] = _randn(g, N) * cs * math.sqrt(Kd * M)
    return inp


def pack_bits(dec: torch.Tensor) -> torch.Tensor:
    """bool [rows, C] (C % 8 == 0) -> uint8 [rows, C / 8], bit q of byte j = column 8 j + q"""
    w = (2 ** torch.arange(8)).to(torch.int64)
    return (dec.view(dec.shape[0], -1, 8).to(torch.int64) * w).sum(-1).to(torch.uint8)


def unpack_bits(b: torch.Tensor, C: int) -> torch.Tensor:
    return ((b.to(torch.int64)[:, :, None] >> torch.arange(8)) & 1).bool().reshape(b.shape[0], -1)[:, :C]


def _phi(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def _gelu(x):
    return x * _phi(x)


def _gelu_grad(x):
    return _phi(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _seen(c: GemmCase, t32: torch.Tensor, planes: bool, dt):
    """the value a kernel reads from a tensor stored as planes (hi + lo) or fp32"""
    if not planes:
        return t32.to(dt)
    hi, lo = canonical_planes(t32)
    return hi.to(dt) + lo.to(dt)


def gemm_acc(c: GemmCase, inp, dt, k_used=None):
    """(contraction, its magnitude sum) [M, N]: op(A) op(B), or the three plane terms of it (without a_lo b_lo)"""
    a, b = inp["a"], inp["b"]
    a = (a.T if c.ta else a)[:, :k_used]
    b = (b.T if c.tb else b)[:k_used]
    if c.family == "B32":
        a, b = a.to(dt), b.to(dt)
        return a @ b, a.abs() @ b.abs()
    (ah, al), (bh, bl) = canonical_planes(a.contiguous()), canonical_planes(b.contiguous())
    ah, al, bh, bl = (t.to(dt) for t in (ah, al, bh, bl))
    acc = ah @ bh + ah @ bl + al @ bh
    return acc, ah.abs() @ bh.abs() + ah.abs() @ bl.abs() + al.abs() @ bh.abs()


def _eval_b(c: GemmCase, inp, dt, k_used=None):
    acc, mag = gemm_acc(c, inp, dt, k_used)
    pre, mpre = c.alpha * acc, abs(c.alpha) * mag
    if c.bias:
        pre, mpre = pre + inp["bias"].to(dt), mpre + inp["bias"].to(dt).abs()
    radd = None
    if c.residual != "none":
        radd = _seen(c, inp["residual"], c.residual == "pl", dt)
    if c.accumulate:
        radd = inp["c0"].to(dt)
    if radd is not None:
        pre, mpre = pre + radd, mpre + radd.abs()
    y = torch.relu(pre) if c.act == ACT_RELU else _gelu(pre) if c.act == ACT_GELU else pre
    mult = None
    if c.auxmode == 1:
        mult = (inp["aux"] > 0).to(dt)
    elif c.auxmode == 2:
        mult = _gelu_grad(inp["aux"].to(dt))
    elif c.auxmode == 3:
        mult = unpack_bits(inp["maskin"], c.N).to(dt)
    out, mout = (y, mpre) if mult is None else (y * mult, mpre * mult.abs())
    res = {"out": out, "mag:out": mout, "mag:pre": mpre}
    if c.preact:
        res["preact"] = pre
    if c.colsum != "none":
        res["colsum"] = out.sum(0) + (inp["colsum0"].to(dt) if c.colsum == "acc" else 0.0)
        res["mag:colsum"] = mout.sum(0) + (inp["colsum0"].to(dt).abs() if c.colsum == "acc" else 0.0)
    return res


def gemm_c(c: GemmCase) -> float:
    return ((3 if c.family == "BPL" else 1) * c.K + 8) * U24


def _check_b(c: GemmCase, ref, got):
    cc = gemm_c(c)
    erf = ERF_TOL * ref["mag:pre"] if (c.act == ACT_GELU or c.auxmode == 2) else torch.zeros_like(ref["mag:pre"])
    out = []
    if "out" in got:
        extra = erf + (PLANES_TOL * ref["out"].abs() if c.out_planes else 0.0)
        out.append(("out",) + forward_bound(got["out"], ref["out"], ref["mag:out"], cc, extra))
    if "preact" in got:
        out.append(("preact",) + forward_bound(got["preact"], ref["preact"], ref["mag:pre"], cc))
    if "colsum" in got:      # the M stored elements, each within its own bound, summed in fp32 in some order
        extra = (erf + (PLANES_TOL * ref["out"].abs() if c.out_planes else 0.0)).sum(0)
        out.append(("colsum",) + forward_bound(got["colsum"], ref["colsum"], ref["mag:colsum"], cc + (c.M + 8) * U24, extra))
    return out


# ================================================================================================================ family C
C_ROWS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 70001)
C_COLS = (8, 16, 24, 136, 264, 1024, 2048)
C_OPS = ("colsum", "colvar", "colstats_biased", "colstats_unbiased", "coldot", "coldot_shift")
C_PROFILES = ("offset", "randn")
C_MAX_BYTES = 48 << 20


@dataclass(frozen=True)
class ColCase:
    index: int
    op: str
    planes: bool
    rows: int
    C: int
    pad: int           # ldx - C (colsum, colvar; the statistics take contiguous tensors)
    gap: int
    alpha: float       # colsum, colvar
    accumulate: bool   # colsum
    profile: str


def _gen_c(i: int, S: Schedule) -> ColCase:
    rows = S("rows", C_ROWS)
    C = S("C", [v for v in C_COLS if rows * (v + 64) * 4 <= C_MAX_BYTES])      # every tensor of a case stays under 64 MiB
    op, planes, profile = S("op", C_OPS), S("planes", (False, True)), S("profile", C_PROFILES)
    pad, gap, alpha, acc = S("pad", PADS), S("gap", PADS), S("alpha", ALPHAS), S("accumulate", (False, True))
    strided = op in ("colsum", "colvar")
    return ColCase(i, op, planes, rows, C, pad if strided else 0, gap if planes and strided else 0, alpha if strided else 1.0,
                   acc and op == "colsum", profile)


def _legal_c(c: ColCase) -> bool:
    ok = c.rows > 0 and c.C > 0                                              # gemm_misc.hip:227,245,263; bn_train.hip:273,306
    if c.planes or c.op.startswith(("colstats", "coldot")):
        ok &= c.C % 8 == 0                                                   # gemm_misc.hip:227; bn_train.hip:273,306
    if c.planes:
        ok &= (c.C + c.pad) % 8 == 0 and (c.rows * (c.C + c.pad) + c.gap) % 8 == 0       # ldx, plane: gemm_misc.hip:227
    return bool(ok) and c.rows * (c.C + c.pad) * 4 < (64 << 20)


def _build_c(c: ColCase):
    g = _gen("C", c.index)
    x = _randn(g, c.rows, c.C)
    if c.profile == "offset":
        x = x * 10.0 ** (torch.rand(c.C, generator=g) * 1.5 - 1.0) + (torch.rand(c.C, generator=g) * 600.0 - 300.0)
    inp = {"x": x}
    seen = _seen(None, x, c.planes, torch.float64)
    if c.op == "colsum" and c.accumulate:
        inp["out0"] = _randn(g, c.C) * math.sqrt(c.rows)
    if c.op == "colvar":
        inp["mean"] = seen.mean(0).float()
    if c.op.startswith("coldot"):
        inp["a"] = _randn(g, c.rows, c.C)
        if c.op == "coldot_shift":
            inp["bshift"] = seen.mean(0).float()
    return inp


def _eval_c(c: ColCase, inp, dt, rows_used=None):
    x = _seen(None, inp["x"], c.planes, dt)[:rows_used]
    n = c.rows
    if c.op == "colsum":
        s = c.alpha * x.sum(0)
        return {"out": s + inp["out0"].to(dt) if c.accumulate else s}
    if c.op == "colvar":
        d = x - inp["mean"].to(dt)
        return {"out": c.alpha * (d * d).sum(0)}
    if c.op.startswith("colstats"):
        mean = x.sum(0) / n
        d = x - mean
        scale = 1.0 / max(1, n - 1) if c.op == "colstats_unbiased" else 1.0 / n
        return {"mean": mean, "var": (d * d).sum(0) * scale}
    a = _seen(None, inp["a"], c.planes, dt)[:rows_used]
    b = x - inp["bshift"].to(dt) if c.op == "coldot_shift" else x
    return {"out": (a * b).sum(0)}


# ================================================================================================================ family D
D_L2_D, D_L2_ROWS = (1, 63, 64, 65, 128, 448, 511, 512), (1, 3, 4, 5, 257)
D_NCE_ROWS, D_NCE_COLS = (1, 4, 8, 33), (1, 3, 255, 256, 257, 1025)
D_COS_B, D_COS_D, D_COS_P = (1, 3, 4, 5, 63, 64, 65, 257), (4, 63, 64, 65, 128, 512), (1, 2, 8, 9, 33, 100)
D_BCE_N = (1, 255, 257, 65537)
D_GM_G, D_GM_N, D_GM_D = (1, 10), (1, 4, 10), (1, 128, 130)
D_COUNTS = (("l2norm", 20), ("infonce", 24), ("cosine", 40), ("bce", 16), ("group_mean", 12))


@dataclass(frozen=True)
class HeadCase:
    index: int
    op: str            # l2norm, infonce, cosine, bce (with eval_score), group_mean
    rows: int          # l2norm rows / infonce rows / cosine B / bce B / group_mean G
    cols: int          # l2norm D / infonce cols / cosine D / bce C / group_mean D
    n: int = 1         # cosine P / group_mean n
    groups: int = 0    # cosine: 0 plain, > 0 the maximum over groups of P / groups prompts
    pad: int = 0       # l2norm: ldxhat - D; infonce: ld - cols; bce: ldlab - C
    diag_off: int = 0
    flag_a: bool = False    # infonce loss_accumulate / cosine accumulate_dy / bce diff
    flag_b: bool = False    # cosine need_dx / eval_score pred_diff
    profile: str = "base"


def cosine_chunks(c: HeadCase) -> int:
    """prompt chunks of the cosine backward (csrc/loss.hip cosine_bwd: at most 64 KiB / (4 waves x D x 4 B) prompts per launch)"""
    return -(-c.n // max(1, 4096 // c.cols))


def _gen_d(i: int, sched: Schedule) -> HeadCase:
    k = i
    for op, cnt in D_COUNTS:
        if k < cnt:
            break
        k -= cnt
    r = _rng("D." + op, k)
    S = lambda dim, strata: sched(op + "." + dim, strata)      # noqa: E731
    if op == "l2norm":
        D = S("D", D_L2_D)
        return HeadCase(i, op, S("rows", D_L2_ROWS), D, pad=S("ld2", (0, D)))
    if op == "infonce":
        cols = S("cols", D_NCE_COLS)
        rows = S("rows", [v for v in D_NCE_ROWS if v <= cols])        # diag_off + rows <= cols (loss.hip:580)
        off = {"zero": 0, "middle": (cols - rows) // 2, "end": cols - rows}[S("diag_off", ("zero", "middle", "end"))]
        return HeadCase(i, op, rows, cols, pad=S("pad", PADS), diag_off=off, flag_a=S("acc", (False, True)), profile=S("profile", ("base", "sharp")))
    if op == "cosine":
        P = S("P", D_COS_P)
        mx = S("max", (False, True))
        groups = r.choice([g for g in range(1, P + 1) if P % g == 0]) if mx else 0
        return HeadCase(i, op, S("B", D_COS_B), S("D", D_COS_D), n=P, groups=groups, flag_a=S("accumulate_dy", (False, True)),
                        flag_b=S("need_dx", (True, False)))
    if op == "bce":
        n = S("n", D_BCE_N)
        C = r.choice([v for v in range(1, min(n, 64) + 1) if n % v == 0])
        return HeadCase(i, op, n // C, C, pad=S("pad", (1, 3, 8)), flag_a=S("diff", (True, False)), flag_b=S("pred_diff", (False, True)))
    return HeadCase(i, op, S("G", D_GM_G), S("D", D_GM_D), n=S("n", D_GM_N))


def _legal_d(c: HeadCase) -> bool:
    if c.op == "l2norm":
        return c.rows > 0 and 0 < c.cols <= 512 and c.pad >= 0                  # loss.hip:565,572 (D <= 64 NV, ldxhat >= D)
    if c.op == "infonce":
        return c.rows > 0 and c.cols > 0 and c.diag_off >= 0 and c.diag_off + c.rows <= c.cols       # loss.hip:580
    if c.op == "cosine":
        ok = c.rows > 0 and c.n > 0 and 0 < c.cols <= 512                       # loss.hip:749,765,778
        return ok and (c.groups == 0 or c.n % c.groups == 0) and 4096 // c.cols >= 1      # loss.hip:782,810
    if c.op == "bce":
        return c.rows > 0 and c.cols > 0 and c.pad >= 0                         # loss.hip:819,830 (ldlab >= C)
    return c.rows > 0 and c.n > 0 and c.cols > 0                                # loss.hip:838,844


def _unit(t):
    return t / t.norm(dim=1, keepdim=True)


def _build_d(c: HeadCase):
    g = _gen("D", c.index)
    if c.op == "l2norm":
        x = _randn(g, c.rows, c.cols)
        n64 = x.double().norm(dim=1).clamp_min(1e-12)
        return {"x": x, "dxhat": _randn(g, c.rows, c.cols), "xhat": (x.double() / n64[:, None]).float(), "norm": n64.float()}
    if c.op == "infonce":
        cos = _unit(_randn(g, c.rows, 32)) @ _unit(_randn(g, c.cols, 32)).T
        if c.profile == "sharp":          # cosines x 100 (the upper log-scale bound), one dominant column per row
            cos[torch.arange(c.rows), torch.randint(0, c.cols, (c.rows,), generator=g)] = 1.0
            S = cos * 100.0
        else:
            S = cos / 0.07
        S64 = S.double()
        return {"S": S, "lse_row": torch.logsumexp(S64, 1).float(), "lse_col": torch.logsumexp(S64, 0).float(), "loss0": _randn(g, 1)[0]}
    if c.op == "cosine":
        x, y = _randn(g, c.rows, c.cols), _randn(g, c.n, c.cols)
        x64, y64 = x.double(), y.double()
        cos = _unit(x64) @ _unit(y64).T
        inp = {"x": x, "y": y, "cos": cos.float(), "xn": x64.norm(dim=1).float(), "yn": y64.norm(dim=1).float(), "dy0": _randn(g, c.n, c.cols)}
        if c.groups:
            inp["dcos"] = _randn(g, c.rows, c.groups)
            inp["arg"] = inp["cos"].view(c.rows, c.groups, -1).max(2).indices.to(torch.int32)
        else:
            inp["dcos"] = _randn(g, c.rows, c.n)
        return inp
    if c.op == "bce":
        lab = (torch.rand(c.rows, c.cols + c.pad, generator=g) < 0.5).float()
        return {"cos": torch.tanh(_randn(g, c.rows, 2 * c.cols)), "labels": lab}
    return {"x": _randn(g, c.rows * c.n, c.cols), "dout": _randn(g, c.rows, c.cols)}


def _cos_dc(c: HeadCase, inp, dt):
    """the gradient that reaches cos [B, P]: dcos itself, or dmax routed to each group's winner"""
    if not c.groups:
        return inp["dcos"].to(dt)
    Pg = c.n // c.groups
    hit = torch.arange(Pg)[None, None, :] == inp["arg"].long()[:, :, None]
    return (hit.to(dt) * inp["dcos"].to(dt)[:, :, None]).reshape(c.rows, c.n)


def cosine_backward(c: HeadCase, inp, dt, p_lo=0, p_hi=None):
    """(dx, dy) from the saved cos / norms the kernel reads, prompts [p_lo, p_hi): dx_i = sum_p dc (yh_p - cos xh_i) / |x_i|,
    dy_p = sum_i dc (xh_i - cos yh_p) / |y_p|"""
    sl = slice(p_lo, p_hi)
    xh, yh = inp["x"].to(dt) / inp["xn"].to(dt)[:, None], (inp["y"].to(dt) / inp["yn"].to(dt)[:, None])[sl]
    dc, cs = _cos_dc(c, inp, dt)[:, sl], inp["cos"].to(dt)[:, sl]
    dx = (dc @ yh - (dc * cs).sum(1, keepdim=True) * xh) / inp["xn"].to(dt)[:, None]
    dy = (dc.T @ xh - (dc * cs).sum(0)[:, None] * yh) / inp["yn"].to(dt)[sl, None]
    return dx, dy


def _eval_d(c: HeadCase, inp, dt):
    if c.op == "l2norm":
        x = inp["x"].to(dt)
        n = x.norm(dim=1).clamp_min(1e-12)
        g, h = inp["dxhat"].to(dt), inp["xhat"].to(dt)
        return {"xhat": x / n[:, None], "norm": n[:, None], "dx": (g - h * (g * h).sum(1, keepdim=True)) / inp["norm"].to(dt)[:, None]}
    if c.op == "infonce":
        S = inp["S"].to(dt)
        ar = torch.arange(c.rows)
        lse, diag = torch.logsumexp(S, 1), S[ar, c.diag_off + ar]
        loss = (lse - diag).sum() * (0.5 / c.rows) + (inp["loss0"].to(dt) if c.flag_a else 0.0)
        grad = torch.exp(S - inp["lse_row"].to(dt)[:, None]) + torch.exp(S - inp["lse_col"].to(dt)[None, :])
        grad[ar, c.diag_off + ar] -= 2.0
        return {"lse": lse[:, None], "diag": diag[:, None], "loss": loss.reshape(1, 1), "grad": grad}
    if c.op == "cosine":
        x, y = inp["x"].to(dt), inp["y"].to(dt)
        xn, yn = x.norm(dim=1), y.norm(dim=1)
        cos = (x @ y.T / xn[:, None]) / yn[None, :]
        res = {"cos": cos, "xn": xn[:, None], "yn": yn[:, None]}
        if c.groups:
            grp = cos.view(c.rows, c.groups, -1)
            res.update(max=grp.max(2).values, mean=grp.mean(2))
        dx, dy = cosine_backward(c, inp, dt)
        if c.flag_b:
            res["dx"] = dx
        res["dy"] = dy + inp["dy0"].to(dt) if c.flag_a else dy
        return res
    if c.op == "bce":
        cos, lab = inp["cos"].to(dt), inp["labels"][:, :c.cols].to(dt)
        cp, cn = cos[:, 0::2], cos[:, 1::2]
        z = cp - cn if c.flag_a else cp
        loss = (z.clamp_min(0) - z * lab + torch.log1p(torch.exp(-z.abs()))).mean()
        dz = (torch.sigmoid(z) - lab) / z.numel()
        dcos = torch.stack([dz, -dz if c.flag_a else torch.zeros_like(dz)], 2).reshape(c.rows, 2 * c.cols)
        return {"logits": z, "dcos": dcos, "loss": loss.reshape(1, 1), "score": (cp - cn + 2) / 4 if c.flag_b else (cp + 1) / 2}
    x = inp["x"].to(dt)
    return {"out": x.view(c.rows, c.n, c.cols).mean(1),
            "din": (inp["dout"].to(dt) / c.n)[:, None].expand(c.rows, c.n, c.cols).reshape(c.rows * c.n, c.cols)}


# ================================================================================================================ family E
E_LN_H = (4, 8, 60, 64, 72, 100, 128, 256, 504, 512, 520, 768, 1016, 1023, 1024)
E_LNF_ROWS = (1, 3, 4, 5, 17, 257, 4099)
E_LNB_ROWS = (1, 15, 16, 17, 255, 16383, 16385, 16400)      # from 16383 on with H <= 128 only
E_EPS = (1e-12, 1e-5)
E_LN_PROFILES = ("randn", "row_offset", "row_scale", "outlier", "near_constant")
E_EMB_L, E_EMB_H = (1, 7, 32, 512), (8, 100, 768)
E_EB_T, E_EB_H = (1, 31, 32, 33, 63, 64, 65, 1025, 4099), (1, 8, 72, 257, 768)
E_EB_PATTERNS = ("one", "distinct", "zipf", "chunk_aligned", "long_then_split")
E_GELU_N = (1, 255, 256, 257, 65537)
E_ADD_ROWS, E_ADD_COLS, E_ADD_PAD = (1, 5, 8200), (8, 136, 512), (0, 4, 520)
E_COUNTS = (("ln_fwd", 30), ("ln_bwd", 32), ("embed_ln_fwd", 8), ("embed_bwd", 27), ("gelu_bwd", 5), ("planes_add_rows", 9))
EMBED_CH = 32              # sorted entries per chunk of the embedding gradient (csrc/embed.hip)
ADD_ROWS_CAP = 2048        # blocks of 256 threads, 8 columns each (csrc/bert.hip cxrk_planes_add_rows)


@dataclass(frozen=True)
class RowCase:
    index: int
    op: str                 # ln_fwd, ln_bwd, embed_ln_fwd, embed_bwd, gelu_bwd, planes_add_rows
    rows: int = 1           # LayerNorm rows / tokens T / gelu n / add_rows rows
    H: int = 8              # LayerNorm and embedding width / add_rows cols
    eps: float = 1e-12
    res: bool = False       # ln_fwd: a residual; ln_bwd: dx_add
    accumulate: bool = False
    dxsum: str = "none"     # ln_bwd: "none", "fresh", "acc"
    planes: bool = False    # ln_bwd: dx written as planes (the forward writes both forms wherever the planes form is legal)
    L: int = 1              # embed_ln_fwd: positions
    V: int = 1              # embedding rows
    pattern: str = ""       # embed_bwd
    pad: int = 0            # planes_add_rows: ld - cols
    profile: str = "base"


def _op_of(counts, i: int):
    for op, cnt in counts:
        if i < cnt:
            return op, i
        i -= cnt
    raise IndexError(i)


def _gen_e(i: int, sched: Schedule) -> RowCase:
    op, k = _op_of(E_COUNTS, i)
    S = lambda dim, strata: sched(op + "." + dim, strata)      # noqa: E731
    if op == "ln_fwd":
        return RowCase(i, op, rows=S("rows", E_LNF_ROWS), H=S("H", E_LN_H), eps=S("eps", E_EPS), res=S("res", (True, False)),
                       profile=S("profile", E_LN_PROFILES))
    if op == "ln_bwd":
        rows = S("rows", E_LNB_ROWS)
        H = S("H", E_LN_H if rows < 16383 else [h for h in E_LN_H if h <= 128])
        vec = H % 4 == 0                                          # bert.hip ln_bwd_vec_ok: planes and dxsum need the float4 kernel
        return RowCase(i, op, rows=rows, H=H, res=S("dx_add", (False, True)), accumulate=S("accumulate", (True, False)),
                       dxsum=S("dxsum", ("none", "fresh", "acc")) if vec else "none", planes=S("planes", (False, True)) if vec else False,
                       profile=S("profile", E_LN_PROFILES))
    if op == "embed_ln_fwd":
        L, H = S("L", E_EMB_L), S("H", E_EMB_H)
        whole = S("whole", (True, False))
        r = _rng("E." + op, k)
        T = L * r.randint(1, max(1, 600 // L)) + (0 if whole else r.randint(1, max(1, L - 1)))
        if L == 7 and whole:
            T = 14                                                # a last block of two rows: two idle waves
        return RowCase(i, op, rows=T, H=H, L=L, V=r.randint(2, 300))
    if op == "embed_bwd":
        T = S("T", E_EB_T)
        pattern = S("pattern", E_EB_PATTERNS if T > 100 else E_EB_PATTERNS[:4])      # >= 3 chunks and a split chunk need T > 96
        return RowCase(i, op, rows=T, H=S("H", E_EB_H), V=T + 7, pattern=pattern)
    if op == "gelu_bwd":
        return RowCase(i, op, rows=S("n", E_GELU_N))
    return RowCase(i, op, rows=E_ADD_ROWS[k % 3], H=E_ADD_COLS[k // 3], pad=S("pad", E_ADD_PAD))      # every rows x cols pair


def _legal_e(c: RowCase) -> bool:
    if c.op in ("ln_fwd", "embed_ln_fwd"):       # bert.hip:872,881 (planes output: the vec8 kernel, H % 8 == 0)
        return c.rows > 0 and 0 < c.H <= 1024 and c.L > 0 and c.V > 0
    if c.op == "ln_bwd":                         # bert.hip:928,931
        ok = c.rows > 0 and 0 < c.H <= 1024 and c.dxsum in ("none", "fresh", "acc")
        return ok and (c.H % 4 == 0 or (not c.planes and c.dxsum == "none")) and (c.rows < 16383 or c.H <= 128)
    if c.op == "embed_bwd":                      # embed.hip:100
        return 0 < c.rows < (1 << 31) and c.H > 0 and c.V > 0
    if c.op == "gelu_bwd":                       # bert.hip:838
        return c.rows > 0
    return c.rows > 0 and c.H > 0 and c.H % 8 == 0 and (c.H + c.pad) % 4 == 0 and (c.rows * c.H) % 8 == 0      # bert.hip:829


def ln_bwd_launch(rows: int) -> Tuple[int, int, int]:
    """(blocks asked for, rows per block, blocks launched) of the LayerNorm backward (csrc/bert.hip ln_bwd_blocks, launch_ln_bwd)"""
    nb0 = max(1, min(1024, (rows + 15) // 16))
    rows_per = -(-rows // nb0)
    return nb0, rows_per, -(-rows // rows_per)


def _ln_values(c: RowCase, g) -> torch.Tensor:
    x = _randn(g, c.rows, c.H)
    if c.profile == "row_offset":
        sign = torch.where(torch.rand(c.rows, generator=g) < 0.5, -1.0, 1.0)
        x = x + (sign * 10.0 ** (1.0 + 2.0 * torch.rand(c.rows, generator=g)))[:, None]
    elif c.profile == "row_scale":
        x = x * (10.0 ** (torch.rand(c.rows, generator=g) * 8.0 - 4.0))[:, None]
    elif c.profile == "outlier":
        x[torch.arange(c.rows), torch.randint(0, c.H, (c.rows,), generator=g)] *= 1e4
    elif c.profile == "near_constant":
        x = 1.0 + 1e-3 * x
    return x


def _ln_stats(x, eps: float):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd


def embed_ids(c: RowCase) -> torch.Tensor:
    """int64 ids [T] of an embed_bwd case; the runs of the list sorted by (id, position) are what the patterns shape"""
    r = _rng("E.ids", c.index)
    T, V = c.rows, c.V
    if c.pattern == "one":
        return torch.full((T,), r.randrange(V), dtype=torch.int64)
    if c.pattern == "distinct":
        return torch.tensor(r.sample(range(V), T), dtype=torch.int64)
    if c.pattern == "zipf":
        ids = [min(V - 1, int(r.paretovariate(1.1)) - 1) for _ in range(T)]
        ids[r.randrange(T)] = 0
        if T > 1:
            ids[r.randrange(T)] = V - 1
        return torch.tensor(ids, dtype=torch.int64)
    if c.pattern == "chunk_aligned":
        runs, left = [], T
        while left > 0:
            n = min(left, EMBED_CH * r.randint(1, 3))
            runs.append(n)
            left -= n
    else:      # long_then_split: a run over chunks 0, 1, 2 that ends inside chunk 2, whose rest is one second run; then the same
        runs, left = [], T      # motif again behind a short run, then short runs
        for n in (70 + r.randint(0, 20), 40, 3, 2 * EMBED_CH + r.randint(5, 25), 60):
            if left >= n:
                runs.append(n)
                left -= n
        while left > 0:
            n = min(left, r.randint(1, 40))
            runs.append(n)
            left -= n
    vals = sorted(r.sample(range(V), len(runs)))
    pos = list(range(T))
    r.shuffle(pos)
    ids = torch.empty(T, dtype=torch.int64)
    at = 0
    for v, n in zip(vals, runs):      # ascending ids over ascending runs: the sorted list has exactly these runs, in this order
        ids[torch.tensor(pos[at:at + n])] = v
        at += n
    return ids


def embed_chunks(ids: torch.Tensor):
    """(runs per chunk of the sorted list, chunks the longest boundary-finished run covers): the host view of csrc/embed.hip"""
    s = sorted(ids.tolist())
    chunks = [s[i:i + EMBED_CH] for i in range(0, len(s), EMBED_CH)]
    nruns = [len(set(ch)) for ch in chunks]
    span = {}
    for k, ch in enumerate(chunks):
        for v in set(ch):
            span.setdefault(v, set()).add(k)
    return nruns, max(len(v) for v in span.values())


def _build_e(c: RowCase):
    g = _gen("E", c.index)
    if c.op == "ln_fwd":
        inp = {"x": _ln_values(c, g), "gamma": 1.0 + 0.5 * _randn(g, c.H), "beta": _randn(g, c.H)}
        if c.res:      # the two summands cancel to the profile's values: the sum the kernel forms is what is normalised
            inp["res"] = _randn(g, c.rows, c.H) * inp["x"].abs().amax(1, keepdim=True).clamp_min(1e-30) * 0.5
            inp["x"] = inp["x"] - inp["res"]
        return inp
    if c.op == "ln_bwd":
        xhat, rstd = _ln_stats(_ln_values(c, g).double(), c.eps)
        inp = {"dy": _randn(g, c.rows, c.H), "xhat": xhat.float(), "rstd": rstd.float().reshape(-1), "gamma": 1.0 + 0.5 * _randn(g, c.H)}
        if c.res:
            inp["dx_add"] = _randn(g, c.rows, c.H) * inp["rstd"][:, None]
        if c.accumulate:
            inp["dgamma0"], inp["dbeta0"] = _randn(g, c.H) * math.sqrt(c.rows), _randn(g, c.H) * math.sqrt(c.rows)
        if c.dxsum == "acc":
            inp["dxsum0"] = _randn(g, c.H) * float(inp["rstd"].max()) * math.sqrt(c.rows)
        return inp
    if c.op == "embed_ln_fwd":
        ids = torch.randint(0, c.V, (c.rows,), generator=g)
        ids[0], ids[-1] = 0, c.V - 1
        if c.rows == 1:
            ids[0] = c.V - 1
        return {"ids": ids, "word": _randn(g, c.V, c.H), "pos": _randn(g, c.L, c.H), "type": _randn(g, c.H), "gamma": 1.0 + 0.5 * _randn(g, c.H),
                "beta": _randn(g, c.H)}
    if c.op == "embed_bwd":
        return {"ids": embed_ids(c), "dx": _randn(g, c.rows, c.H), "dword0": _randn(g, c.V, c.H)}
    if c.op == "gelu_bwd":
        pre = torch.linspace(-12.0, 12.0, c.rows)[torch.randperm(c.rows, generator=g)] + 0.01 * _randn(g, c.rows)
        return {"pre": pre if c.rows > 1 else torch.tensor([0.7]), "dy": _randn(g, c.rows)}
    return {"src": _randn(g, c.rows, c.H), "dst0": _randn(g, c.rows, c.H) * 3.0}


def _eval_e(c: RowCase, inp, dt, rows_used=None):
    if c.op in ("ln_fwd", "embed_ln_fwd"):
        if c.op == "ln_fwd":
            x = inp["x"].to(dt) + (inp["res"].to(dt) if c.res else 0.0)
        else:
            x = inp["word"].to(dt)[inp["ids"]] + inp["pos"].to(dt)[torch.arange(c.rows) % c.L] + inp["type"].to(dt)
        xhat, rstd = _ln_stats(x, c.eps)
        return {"y": xhat * inp["gamma"].to(dt) + inp["beta"].to(dt), "xhat": xhat, "rstd": rstd}
    if c.op == "ln_bwd":
        dy, xhat, rstd = inp["dy"].to(dt), inp["xhat"].to(dt), inp["rstd"].to(dt)[:, None]
        gy = dy * inp["gamma"].to(dt)
        dx = rstd * (gy - gy.mean(1, keepdim=True) - xhat * (gy * xhat).mean(1, keepdim=True))
        if c.res:
            dx = dx + inp["dx_add"].to(dt)
        u = slice(0, rows_used)
        out = {"dx": dx, "dgamma": (dy * xhat)[u].sum(0), "dbeta": dy[u].sum(0)}
        if c.accumulate:
            out["dgamma"], out["dbeta"] = out["dgamma"] + inp["dgamma0"].to(dt), out["dbeta"] + inp["dbeta0"].to(dt)
        if c.dxsum != "none":
            out["dxsum"] = dx[u].sum(0) + (inp["dxsum0"].to(dt) if c.dxsum == "acc" else 0.0)
        return out
    if c.op == "embed_bwd":
        base, dx, ids = inp["dword0"].to(dt), inp["dx"].to(dt), inp["ids"]
        count = torch.zeros(c.V, dtype=torch.float64).index_add_(0, ids, torch.ones(c.rows, dtype=torch.float64))
        mag = base.abs().double().index_add(0, ids, dx.abs().double())
        return {"dword": base.index_add(0, ids, dx), "mag:dword": (count[:, None] + 2.0) * U24 * mag}
    if c.op == "gelu_bwd":
        dy = inp["dy"].to(dt)
        ref = dy * _gelu_grad(inp["pre"].to(dt))
        return {"dx": ref, "mag:dx": ERF_TOL * dy.abs().double() + 2.0 * U24 * ref.abs().double()}
    src, dst = _seen(None, inp["src"], True, dt), inp["dst0"].to(dt)
    return {"dst": dst + src, "mag:dst": 2.0 * U24 * (dst.abs() + src.abs()).double()}


# ================================================================================================================ family F
F_POOL_HW, F_POOL_N, F_POOL_C = (1, 2, 3, 4, 7, 8, 13, 16, 17), (1, 2), (4, 8, 24, 64, 136)
F_POOL_PROFILES = ("randn", "relu", "constant", "negative")
F_LAY_C, F_LAY_PAD = (1, 3, 4, 5), ("C", "4", "8")
F_LAY_PAIRS = tuple((C, Cp) for C in F_LAY_C for Cp in sorted({C, 4, 8}) if Cp >= C)      # every (C, Cpad) there is: ten
F_SM_P, F_SM_C = (1, 2, 49, 50, 256, 1025), (1, 8, 130, 136, 2048)
F_FOLD_TAPS, F_FOLD_C, F_FOLD_KO = (1, 9, 49), ((3, 4), (3, 8), (64, 64), (60, 64)), (1, 5, 64)
F_BN_ROWS, F_BN_C = (1, 2, 3, 16, 257, 4097), (8, 24, 136, 1024)
F_BN_RES, F_BN_RELU, F_BN_MOM, F_BN_RATIO = ("none", "f32", "pl"), ("none", "relu", "mask"), (0.0, 0.1), (0, 30, 300, 3000)
F_COUNTS = (("maxpool", 36), ("layout", len(F_LAY_PAIRS)), ("spatial_mean", 12), ("bn_fold", 8), ("bn_train", 36))
BN_EPS = 1e-5
BN_GRID_CAP = 16384        # blocks of 256 threads, 8 columns each, of bn_apply and bn_train_dz (csrc/bn_train.hip grid_for)


@dataclass(frozen=True)
class ImgCase:
    index: int
    op: str                 # maxpool (forward and backward, fp32 and planes), layout (both transforms), spatial_mean, bn_fold, bn_train
    N: int = 1
    H: int = 1
    W: int = 1
    C: int = 8
    Cpad: int = 0           # layout, bn_fold
    relu: str = "none"      # maxpool: "mask" = relu_mask of the fp32 backward; bn_train: "none", "relu", "mask" (ReLU with decision bits)
    P: int = 1              # spatial_mean pixels
    add: bool = False       # spatial_mean_bwd_pl
    taps: int = 1           # bn_fold
    Ko: int = 1
    rows: int = 1           # bn_train
    planes: bool = False    # bn_train: z, dy, y, dz in planes storage
    residual: str = "none"  # bn_train: "none", "f32", "pl"
    momentum: float = 0.0
    running: bool = False
    accumulate: bool = False
    profile: str = "base"   # maxpool profile; bn_train: "offset<|mean| / std>"


def _gen_f(i: int, sched: Schedule) -> ImgCase:
    op, k = _op_of(F_COUNTS, i)
    S = lambda dim, strata: sched(op + "." + dim, strata)      # noqa: E731
    r = _rng("F." + op, k)
    if op == "maxpool":
        return ImgCase(i, op, N=S("N", F_POOL_N), H=S("H", F_POOL_HW), W=S("W", F_POOL_HW), C=S("C", F_POOL_C),
                       relu=S("relu_mask", ("mask", "none")), profile=S("profile", F_POOL_PROFILES))
    if op == "layout":
        C, Cpad = F_LAY_PAIRS[k]
        H = r.randint(1, 19)
        return ImgCase(i, op, N=r.randint(1, 3), H=H, W=r.choice([w for w in range(1, 300) if w != H]), C=C, Cpad=Cpad)
    if op == "spatial_mean":
        P, C = S("P", F_SM_P), S("C", F_SM_C)
        return ImgCase(i, op, N=min(r.randint(1, 3), max(1, C_MAX_BYTES // (9 * P * C))), P=P, C=C, add=S("add", (True, False)))      # x and add
    if op == "bn_fold":
        C, Cpad = S("C", F_FOLD_C)
        return ImgCase(i, op, C=C, Cpad=Cpad, taps=S("taps", F_FOLD_TAPS), Ko=S("Ko", F_FOLD_KO))
    planes, rows = S("planes", (False, True)), S("rows", F_BN_ROWS)
    C = S("C", [v for v in F_BN_C if 13 * rows * v <= C_MAX_BYTES])      # z, dy and the residual, 4 bytes each, and the vectors
    return ImgCase(i, op, rows=rows, C=C, planes=planes, residual=S("residual", F_BN_RES), relu=S("relu", F_BN_RELU),
                   momentum=S("momentum", F_BN_MOM), running=S("running", (True, False)), accumulate=S("accumulate", (False, True)),
                   profile=f"offset{S('ratio', F_BN_RATIO)}")


def _legal_f(c: ImgCase) -> bool:
    if c.op == "maxpool":                        # conv_misc.hip:293,302 (fp32: C % 4; the planes kernels, :312,323, run where C % 8 == 0)
        return c.N > 0 and c.H > 0 and c.W > 0 and c.C % 4 == 0
    if c.op == "layout":                         # conv_misc.hip:280,286
        return c.N > 0 and c.C > 0 and c.Cpad >= c.C
    if c.op == "spatial_mean":                   # conv_misc.hip:333,339 (the planes backward, :346, runs where C % 8 == 0)
        return c.N > 0 and c.P > 0 and c.C > 0
    if c.op == "bn_fold":                        # conv_misc.hip:261 (the planes form, :271, runs where Cpad % 8 == 0)
        return c.Ko > 0 and c.taps > 0 and c.C > 0 and c.Cpad >= c.C
    ok = c.rows > 0 and c.C > 0 and c.C % 8 == 0                                  # bn_train.hip:264,312
    return ok and c.relu in F_BN_RELU and c.residual in F_BN_RES                  # :265: decision bits only with the ReLU


def pool_out(n: int) -> int:
    return (n - 1) // 2 + 1


def _planes_exact(t32: torch.Tensor) -> torch.Tensor:
    """the values rounded to what planes storage holds (hi + lo, exact in float32): one tensor serves the fp32 and the planes kernels"""
    hi, lo = canonical_planes(t32.contiguous())
    return hi.float() + lo.float()


def pool_winners(x32: torch.Tensor):
    """torch's own 3x3 / stride 2 / pad 1 max-pool of float32 NHWC values: (flat NCHW indices [N, C, Ho, Wo], winning taps r * 3 + s as uint8
    NHWC): the first maximum in scan order under ties"""
    N, H, W, C = x32.shape
    _, ind = torch.nn.functional.max_pool2d(x32.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    ho, wo = torch.arange(ind.shape[2])[:, None], torch.arange(ind.shape[3])[None, :]
    tap = (ind // W - (2 * ho - 1)) * 3 + (ind % W - (2 * wo - 1))
    return ind, tap.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def pool_backward(c: ImgCase, ind, dy, dt, mask_out=None, mask_in=None):
    """(dx, the magnitude sum of its terms) NHWC from flat NCHW winners; mask_out [N, Ho, Wo, C] masks the windows, mask_in the pixels"""
    dy = dy.to(dt) * (mask_out.to(dt) if mask_out is not None else 1.0)
    dyn = dy.permute(0, 3, 1, 2).reshape(c.N, c.C, -1)
    res = []
    for t in (dyn, dyn.abs()):
        d = torch.zeros(c.N, c.C, c.H * c.W, dtype=dt).scatter_add_(2, ind.reshape(c.N, c.C, -1), t)
        d = d.view(c.N, c.C, c.H, c.W).permute(0, 2, 3, 1)
        res.append(d * mask_in.to(dt) if mask_in is not None else d)
    return res[0], res[1]


def bn_signs(rows: int, C: int, g) -> torch.Tensor:
    """+-1 alternating down every column from a random start: the two-cluster columns of the bn_train profile"""
    phase = torch.randint(0, 2, (C,), generator=g)
    return 1.0 - 2.0 * ((torch.arange(rows)[:, None] + phase[None, :]) % 2).float()


def _build_f(c: ImgCase):
    g = _gen("F", c.index)
    if c.op == "maxpool":
        x = _randn(g, c.N, c.H, c.W, c.C)
        if c.profile == "relu":
            x = torch.relu(x)
        elif c.profile == "constant":
            x = torch.full_like(x, _rng("F.const", c.index).choice((0.75, 0.0, -2.0)))
        elif c.profile == "negative":
            x = -x.abs() - 0.1
        return {"x": _planes_exact(x), "dy": _planes_exact(_randn(g, c.N, pool_out(c.H), pool_out(c.W), c.C))}
    if c.op == "layout":
        return {"x": _randn(g, c.N, c.C, c.H, c.W), "x2": _randn(g, c.N, c.H, c.W, c.C)}
    if c.op == "spatial_mean":
        inp = {"x": _randn(g, c.N, c.P, c.C) + 0.5, "dy": _randn(g, c.N, c.C)}
        if c.add:
            inp["add"] = _randn(g, c.N, c.P, c.C)
        return inp
    if c.op == "bn_fold":
        gamma = 1.0 + 0.5 * _randn(g, c.Ko)
        gamma[torch.rand(c.Ko, generator=g) < 0.3] = 0.0
        gamma[_rng("F.fold", c.index).randrange(c.Ko)] = 0.0
        rvar = torch.tensor([1e-10, 1.0, 1e4])[torch.randint(0, 3, (c.Ko,), generator=g)]
        return {"w": _randn(g, c.Ko, c.taps, c.C), "gamma": gamma, "beta": _randn(g, c.Ko), "rmean": _randn(g, c.Ko) * rvar.sqrt(), "rvar": rvar}
    # bn_train.  Every column holds two clusters, offset +- std (1 + N(0, 1) / 4), and beta and the residual are small against gamma:
    # y stays away from zero (the ReLU decision is unambiguous on all but a sliver, test_decision_bits_cap) while half of it is negative
    ratio = float(c.profile[6:])
    std = 10.0 ** (torch.rand(c.C, generator=g) * 1.5 - 1.0)
    sign = torch.where(torch.rand(c.C, generator=g) < 0.5, -1.0, 1.0)
    z = std * (sign * ratio + bn_signs(c.rows, c.C, g) * (1.0 + 0.25 * _randn(g, c.rows, c.C)))
    gamma = (0.5 + torch.rand(c.C, generator=g)) * torch.where(torch.rand(c.C, generator=g) < 0.5, -1.0, 1.0)
    beta = gamma * (0.15 + 0.1 * torch.rand(c.C, generator=g)) * torch.where(torch.rand(c.C, generator=g) < 0.5, -1.0, 1.0)
    inp = {"z": z, "gamma": gamma, "beta": beta, "dy": _randn(g, c.rows, c.C)}
    if c.residual != "none":
        inp["res"] = 0.05 * gamma.abs() * _randn(g, c.rows, c.C)
    if c.running:
        inp["rmean0"], inp["rvar0"] = _randn(g, c.C) * std, (0.5 + torch.rand(c.C, generator=g)) * std * std
    if c.accumulate:
        inp["dgamma0"], inp["dbeta0"] = _randn(g, c.C) * math.sqrt(c.rows), _randn(g, c.C) * math.sqrt(c.rows)
    return inp


def bn_forward(c: ImgCase, inp, dt):
    z, n = _seen(None, inp["z"], c.planes, dt), c.rows
    gamma, beta = inp["gamma"].to(dt), inp["beta"].to(dt)
    mean = z.sum(0) / n
    d = z - mean
    var = (d * d).sum(0) / n
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    out = {"mean": mean, "var": var, "scale": gamma * rstd, "shift": beta - mean * gamma * rstd, "rstd": rstd}
    if c.running:
        out["rmean"] = (1.0 - c.momentum) * inp["rmean0"].to(dt) + c.momentum * mean
        out["rvar"] = (1.0 - c.momentum) * inp["rvar0"].to(dt) + c.momentum * var * (n / (n - 1.0) if n > 1 else 1.0)
    if n == 1:      # torch refuses one value per channel: the normalised value is 0 / 0 in the limit; only the statistics are defined
        return out
    pre = d * rstd * gamma + beta
    if c.residual != "none":
        pre = pre + _seen(None, inp["res"], c.residual == "pl", dt)
    out["aux:pre"] = pre
    out["y"] = torch.relu(pre) if c.relu != "none" else pre
    return out


def bn_backward(c: ImgCase, inp, dt, fwd, bits=None):
    """the backward of the chain from the forward's (mean, rstd) in `dt` and GIVEN ReLU decisions (bool [rows, C]; None: no ReLU)"""
    z, n = _seen(None, inp["z"], c.planes, dt), c.rows
    dym = inp["dy"] * bits.float() if bits is not None else inp["dy"]          # exact in float32; then stored as dy is
    dy = _seen(None, dym, c.planes, dt)
    mean, rstd, gamma = fwd["mean"].to(dt), fwd["rstd"].to(dt), inp["gamma"].to(dt)
    sumdy, dot = dy.sum(0), (dy * (z - mean)).sum(0)
    dg, a = rstd * dot, gamma * rstd
    cc = -a * rstd * dg / n
    out = {"sumdy": sumdy, "dot": dot, "A": a, "B": -a * sumdy / n - cc * mean, "Cc": cc, "dgamma": dg, "dbeta": sumdy,
           "dz": a * (dy - sumdy / n - (z - mean) * rstd * dg / n)}
    if c.accumulate:
        out["dgamma"], out["dbeta"] = dg + inp["dgamma0"].to(dt), sumdy + inp["dbeta0"].to(dt)
    if n == 2:
        # two values per channel: xhat = +-1 up to eps, and dz vanishes identically (what is left is eps / var of its terms): a
        # column has no scale of its own to be judged by, and the value is what the rounding of B against Cc z leaves.  What
        # bn_train_dz computes is still well defined: A dy + (Cc z + B) of the coefficients it is GIVEN.  The evaluation returns that
        # form (equal to the line above in exact arithmetic), and check() judges a dz against the same form of the coefficients
        # that came with it (kind "form"), each of which is judged per column on its own
        out["dz"] = a * dy + (cc * z + out["B"])
        out["aux:dy"], out["aux:z"] = dy.double(), z.double()
    return out


def _eval_f(c: ImgCase, inp, dt):
    if c.op == "maxpool":
        x32 = inp["x"]
        ind, tap = pool_winners(x32)
        y = x32.permute(0, 3, 1, 2).reshape(c.N, c.C, -1).gather(2, ind.reshape(c.N, c.C, -1)).view(ind.shape).permute(0, 2, 3, 1).to(dt)
        dx, m = pool_backward(c, ind, inp["dy"], dt, mask_in=(x32 > 0) if c.relu == "mask" else None)
        dxp, mp = pool_backward(c, ind, inp["dy"], dt, mask_out=y > 0)
        return {"y": y, "idx": tap, "dx": dx, "mag:dx": 3.0 * U24 * m.double(), "dx_pl": dxp, "mag:dx_pl": 3.0 * U24 * mp.double()}
    if c.op == "layout":
        y = torch.zeros(c.N, c.H, c.W, c.Cpad, dtype=dt)
        y[..., :c.C] = inp["x"].to(dt).permute(0, 2, 3, 1)
        return {"nhwc": y, "nchw": inp["x2"].to(dt).permute(0, 3, 1, 2).contiguous()}
    if c.op == "spatial_mean":
        x, dy, add = inp["x"].to(dt), inp["dy"].to(dt), (inp["add"].to(dt) if c.add else None)
        dx = (dy / c.P)[:, None, :].expand(c.N, c.P, c.C)
        dxp = dx + add if c.add else dx
        # backward: dy * fl(1 / P) (+ add): two roundings, three with the addition; the planes form adds its storage tolerance (check)
        return {"y": x.mean(1), "mag:y": (c.P + 2) * U24 * x.abs().double().mean(1), "dx": dx.contiguous(), "mag:dx": 3.0 * U24 * dx.abs().double(),
                "dx_pl": dxp.contiguous(), "mag:dx_pl": 3.0 * U24 * (dx.abs() + (add.abs() if c.add else 0.0)).double()}
    if c.op == "bn_fold":
        rstd = 1.0 / torch.sqrt(inp["rvar"].to(dt) + BN_EPS)
        scale = inp["gamma"].to(dt) * rstd
        ws = torch.zeros(c.Ko, c.taps, c.Cpad, dtype=dt)
        ws[..., :c.C] = inp["w"].to(dt) * scale[:, None, None]
        return {"w_scaled": ws.view(c.Ko, -1), "scale": scale, "shift": inp["beta"].to(dt) - inp["rmean"].to(dt) * scale, "rstd": rstd}
    out = bn_forward(c, inp, dt)
    if c.rows > 1:
        out.update(bn_backward(c, inp, dt, out, (out["y"] > 0) if c.relu != "none" else None))
    return out


# how an output of E / F is judged: "row" / "col": row_scaled / col_scaled against max(floor, 8 e32); "exact": bit for bit;
# "sum": elementwise against the derived bound the evaluation returns as "mag:<name>"
_KIND = {"ln_fwd": {"y": "row", "xhat": "row", "rstd": "row"}, "embed_ln_fwd": {"y": "row", "xhat": "row", "rstd": "row"},
         "ln_bwd": {"dx": "row", "dgamma": "col", "dbeta": "col", "dxsum": "col"}, "embed_bwd": {"dword": "sum"}, "gelu_bwd": {"dx": "sum"},
         "planes_add_rows": {"dst": "sum"}, "maxpool": {"y": "exact", "idx": "exact", "dx": "sum", "dx_pl": "sum"},
         "layout": {"nhwc": "exact", "nchw": "exact"}, "spatial_mean": {"y": "sum", "dx": "sum", "dx_pl": "sum"},
         "bn_fold": {"w_scaled": "row", "scale": "col", "shift": "col", "rstd": "col"},
         "bn_train": {k: "col" for k in ("mean", "var", "scale", "shift", "rstd", "rmean", "rvar", "y", "sumdy", "dot", "A", "B", "Cc", "dgamma",
                                         "dbeta", "dz")},
         "mask_tokens": {k: "exact" for k in ("ids", "sel", "tgt", "stats", "count", "blocks")}, "gather": {"out": "exact"},
         "scatter": {"dlast": "exact"},
         "xent": {"lse": "col", "rowloss": "col", "loss": "row", "hit": "hit", "correct": "range", "grad": "grad", "grad_skip": "exact"},
         "head": {"loss": "row", "correct": "range", "dlast": "row", "dwd": "row", "dbd": "row", "dgamma": "row", "dbeta": "row", "dwdec": "row",
                  "dbdec": "row"}}


def kind_of(case, name: str) -> str:
    if case.op == "bn_train" and name == "dz" and case.rows == 2:
        return "form"     # bn_backward
    return _KIND[case.op][name]


def exact_equal(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, tuple]:
    """0 where the values and the signs of their zeros are those of the reference, else infinitely wrong at the first difference"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    got, ref = got.double(), ref.double()
    bad = (got != ref) | (torch.signbit(got) != torch.signbit(ref))
    return (math.inf, tuple(bad.nonzero()[0].tolist())) if bool(bad.any()) else (0.0, ())


def _check_ef(case, ref, got, split, planes_out):
    res = []
    for name, g in got.items():
        kind, r = kind_of(case, name), ref[name]
        if kind == "exact":
            res.append((name,) + exact_equal(g, r))
        elif kind == "form":      # fma(A, dy, fma(Cc, z, B)) rounds twice: 3 * 2^-24 on the three magnitudes, as test_grid_stride_wrap
            t = [got["A"].double().cpu() * ref["aux:dy"], got["Cc"].double().cpu() * ref["aux:z"], got["B"].double().cpu().expand_as(r)]
            extra = PLANES_TOL * (t[0] + t[1] + t[2]).abs() if name in planes_out else None
            res.append((name,) + forward_bound(g, t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs(), 3.0 * U24, extra))
        elif kind == "sum":
            extra = PLANES_TOL * r.abs().double() if name in planes_out else None
            res.append((name,) + forward_bound(g, r, ref["mag:" + name], 1.0, extra))
        else:
            r2 = r.reshape(-1, 1) if name == "rstd" and kind == "row" else r
            ratio, idx = (row_scaled if kind == "row" else col_scaled)(g.reshape(r2.shape), r2)
            res.append((name, ratio / bound_of(case, name, split, name in planes_out), idx))
    return res


def decision_threshold(case: ImgCase, ref, planes_out: bool = False) -> torch.Tensor:
    """[1, C]: below this |pre-activation| a ReLU decision may differ from the reference's -- the bound of y itself, per column"""
    scale = ref["y"].abs().double().max(0, keepdim=True).values
    return bound_of(case, "y", False, planes_out) * scale.clamp_min(FLOOR_REL * float(scale.max()))


# ================================================================================================================ family G
G_MASK_NL = ((1, 1), (5, 51), (16, 16), (1, 257), (27, 19), (16, 512), (129, 512))      # T = 1, 255, 256, 257, 513, 8192, 66048
G_MASK_P = (0.0, 0.15, 0.5, 1.0)
G_MASK_NSPECIAL = (0, 5, 8)
G_MASK_OFFSET = (0, 3, 100000)
G_MASK_CAP = ("default", "below", "T")
G_ROWS_H = (4, 8, 128, 256, 260, 512, 520, 768, 1024)
G_CAP = (1, 3, 4, 5, 37, 130)
G_KEPT = ("-2", "0", "1", "cap-1", "cap", "cap+5")      # stats[0]; the kernels clamp it to [0, cap] (csrc/mlm.hip kept_rows)
G_GAP = (0, 8, 64)
G_V = (8, 9, 15, 136, 300, 2056, 4104, 4366, 8200, 12301)
G_WIDTH = (128, 256, 2048, 4096, 4224)                  # columns per chunk; 0 in a case = one whole chunk
G_PAD = (0, 4, 8, 24)
G_PROFILES = ("randn3", "pm80", "dominant", "ties")
G_HEAD_CAP, G_HEAD_WIDTH, G_HEAD_KEPT = (5, 37), (0, 2176), ("cap-1", "cap")
G_COUNTS = (("mask_tokens", 22), ("gather", 20), ("scatter", 10), ("xent", 50), ("head", 6))
MLM_VOCAB, MLM_MASK_ID = 300, 4                         # the vocabulary of the mask cases
MLM_XENT_FLOOR = 2e-6                                   # tests/test_mlm_memory_gpu.py::test_cross_entropy_kernels
F32_TINY = 2.0 ** -126                                  # the smallest normal float32
GRAD_TILE, GRAD_STEP, STATS_STEP = 4096, 2048, 256      # csrc/mlm.hip: columns per block of xent_grad, per trip of it, per trip of the 16-byte stats loop
TIE_VALUE = 40.0


@dataclass(frozen=True)
class MlmCase:
    index: int
    op: str                 # mask_tokens, gather, scatter, xent, head
    N: int = 1              # mask_tokens: sequences, tokens per sequence
    L: int = 1
    p: float = 0.0
    given_mask: bool = False
    nspecial: int = 0
    row_offset: int = 0
    cap_mode: str = "default"
    H: int = 8              # gather, scatter, head: the hidden width
    cap: int = 1            # gather, scatter, head: slots; xent: logits rows
    kept: str = "cap"       # stats[0], one of G_KEPT
    planes: bool = False    # gather: the output is a planes tensor
    gap: int = 0            # gather: elements between the two planes
    V: int = 8              # xent, head: the vocabulary
    width: int = 0          # xent, head: columns per chunk (0: one whole chunk of V - V % 8)
    pad: int = 0            # xent: ld - widest chunk
    alpha: float = 1.0
    profile: str = "base"


def mlm_kept(c: MlmCase) -> int:
    """stats[0] as the case hands it over"""
    return {"-2": -2, "0": 0, "1": 1, "cap-1": c.cap - 1, "cap": c.cap, "cap+5": c.cap + 5}[c.kept]


def mlm_live(c: MlmCase) -> int:
    """rows that count: stats[0] clamped as csrc/mlm.hip kept_rows clamps it"""
    return max(0, min(c.cap, mlm_kept(c)))


def xent_chunks(V: int, width: int):
    """functional.mlm_vocab_chunks restated from (V, columns per chunk): (first column, columns, leading columns not counted)"""
    V8 = V // 8 * 8
    vc = width or V8
    chunks = [(v0, min(vc, V8 - v0), 0) for v0 in range(0, V8, vc)]
    if V8 != V:
        chunks.append((V - 8, 8, 8 - (V - V8)))
    return chunks


def xent_widths(V: int):
    """the chunk widths that cut this vocabulary into 2 .. 11 chunks, and the whole chunk"""
    V8 = V // 8 * 8
    return tuple(w for w in G_WIDTH if w < V8 <= 10 * w) + (0,)


def xent_needs_rows(V: int, width: int, profile: str) -> bool:
    """what shows only on rows that count -- a state carried from one whole chunk into the next, a second block of xent_grad per row
    (a chunk wider than 4096), equal maxima -- is not drawn together with stats[0] = -2 or 0; the clamp at zero is left to the
    single-chunk cases (a tail chunk of 8 columns behind them or not)"""
    main = [ch for ch in xent_chunks(V, width) if ch[2] == 0]
    return len(main) > 1 or main[0][1] > GRAD_TILE or profile == "ties"


def xent_kept(V: int, width: int, profile: str, rows: int) -> tuple:
    """the strata of stats[0] a cross-entropy case draws from: all of G_KEPT, or those that leave a row that counts"""
    if not xent_needs_rows(V, width, profile):
        return G_KEPT
    return tuple(k for k in G_KEPT[2:] if rows > 1 or k != "cap-1")


def head_chunk_bytes(c: MlmCase, split: bool) -> int:
    """the chunk_bytes that make functional.mlm_vocab_chunks cut the head case's vocabulary as xent_chunks(V, width) does"""
    return c.cap * (-(-(c.width or c.V // 8 * 8) // 128) * 128) * (8 if split else 4)


def _gen_g(i: int, sched: Schedule) -> MlmCase:
    op, k = _op_of(G_COUNTS, i)
    S = lambda dim, strata: sched(op + "." + dim, strata)      # noqa: E731
    if op == "mask_tokens":
        N, L = S("NL", G_MASK_NL)
        big = N * L > 65536                      # the strided part of the prefix over the blocks shows only where tokens behind it are placed
        p = S("p", G_MASK_P[1:] if big else G_MASK_P)
        cap = S("cap", ("default", "T") if big or p == 0.0 or N * L == 1 else G_MASK_CAP)      # "below" needs two selected tokens
        return MlmCase(i, op, N=N, L=L, p=p, given_mask=S("mask", (True, False)), nspecial=S("nspecial", G_MASK_NSPECIAL),
                       row_offset=S("row_offset", G_MASK_OFFSET), cap_mode=cap)
    if op in ("gather", "scatter"):
        planes = S("planes", (False, True)) if op == "gather" else False
        H = S("H", [h for h in G_ROWS_H if h % 8 == 0] if planes else G_ROWS_H)
        return MlmCase(i, op, H=H, cap=S("cap", G_CAP), kept=S("kept", G_KEPT), planes=planes, gap=S("gap", G_GAP) if planes else 0)
    if op == "xent":
        V = S("V", G_V)
        width = S("width", xent_widths(V))
        profile = S("profile", G_PROFILES)
        rows = S("rows", G_CAP)
        return MlmCase(i, op, V=V, width=width, cap=rows, kept=S("kept", xent_kept(V, width, profile, rows)), pad=S("pad", G_PAD),
                       alpha=S("alpha", (1.0, 0.5)), profile=profile)
    return MlmCase(i, op, H=768, V=4366, cap=S("cap", G_HEAD_CAP), width=S("width", G_HEAD_WIDTH), kept=S("kept", G_HEAD_KEPT), alpha=0.5)


def _legal_g(c: MlmCase) -> bool:
    if c.op == "mask_tokens":                    # mlm.hip:299-303 (cap itself is drawn in build(): mask_cap keeps it in [1, T])
        T = c.N * c.L
        return c.N > 0 and c.L > 0 and c.row_offset >= 0 and 0.0 <= c.p <= 1.0 and 0 <= c.nspecial <= 8 and T < (1 << 31) and 0 <= MLM_MASK_ID < MLM_VOCAB
    if c.op == "gather":                         # mlm.hip:321-322
        return c.H > 0 and c.cap > 0 and ((c.H % 8 == 0 and (c.cap * c.H + c.gap) % 8 == 0) if c.planes else c.H % 4 == 0)
    if c.op == "scatter":                        # mlm.hip:333
        return c.H > 0 and c.cap > 0 and c.H % 4 == 0
    ok = c.cap > 0 and c.V >= 8                  # functional.mlm_vocab_chunks: at least 8 ids
    width = max(cols for _, cols, _ in xent_chunks(c.V, c.width))
    for v0, cols, skip in xent_chunks(c.V, c.width):
        ok &= cols > 0 and 0 <= skip < cols and v0 >= 0 and v0 + cols <= c.V and width + c.pad >= cols       # mlm.hip:341-342, 368-369
        ok &= cols % 8 == 0 and (width + c.pad) % 4 == 0                                                     # mlm.hip:368-369
    return bool(ok)


def mask_special(c: MlmCase) -> tuple:
    return tuple(range(c.nspecial))


def mask_cap(c: MlmCase, selected: int) -> int:
    """the slots of a mask case: the library's default, half the selected tokens (an overflow), or one per token"""
    import mlm_ref
    T = c.N * c.L
    return {"default": mlm_ref.capacity(T, c.p), "below": max(1, selected // 2), "T": T}[c.cap_mode]


def mask_place(flags, ids, cap: int, blocks_summed=None):
    """sel, tgt [cap] as mlm_count_kernel + mlm_place_kernel place them: token i of block b = i // 256 goes to slot
    sum(counts[:b]) + (selected tokens of its block in front of it).  blocks_summed: a prefix that adds up only that many counts."""
    import numpy as np
    flags = np.asarray(flags, dtype=bool).reshape(-1)
    T = flags.shape[0]
    nb = (T + 255) // 256
    padded = np.zeros(nb * 256, dtype=np.int64)
    padded[:T] = flags
    counts = padded.reshape(nb, 256).sum(1)
    base = np.array([counts[:b if blocks_summed is None else min(b, blocks_summed)].sum() for b in range(nb)], dtype=np.int64)
    rank = np.cumsum(padded.reshape(nb, 256), 1) - padded.reshape(nb, 256)
    pos = (base[:, None] + rank).reshape(-1)[:T]
    sel, tgt = np.full(cap, -1, dtype=np.int32), np.full(cap, -1, dtype=np.int32)
    take = flags & (pos < cap)
    sel[pos[take]] = np.flatnonzero(take)
    tgt[pos[take]] = np.asarray(ids).reshape(-1)[take]
    return sel, tgt, counts.astype(np.int32)


def rows_list(c: MlmCase):
    """(sel int32 [cap], T) of a gather / scatter / head case: distinct tokens; among the kept slots of gather and scatter one -1
    (from two kept slots on) and one T (from three on); the tokens of the slots behind the kept ones are the poisoned ones"""
    r = _rng("G.rows", c.index)
    T = 2 * c.cap + 3
    sel = r.sample(range(T), c.cap)
    live = mlm_live(c)
    if c.op != "head" and live >= 2:
        bad = r.sample(range(live), 2)
        sel[bad[0]] = -1
        if live >= 3:
            sel[bad[1]] = T
    return torch.tensor(sel, dtype=torch.int32), T


def _stats_of(c: MlmCase) -> torch.Tensor:
    return torch.tensor([mlm_kept(c), mlm_kept(c)], dtype=torch.int32)


def xent_targets(c: MlmCase):
    """the columns a case's targets are put on before the rest is drawn: 4095 / 4096 and 2047 / 2048 inside a chunk, the first counted
    column of the tail chunk and the tail's overlap columns (counted by the chunk before), the first and the last column of every chunk"""
    chunks = xent_chunks(c.V, c.width)
    cols = []
    for v0, n, skip in chunks:
        cols += [v0 + j for j in (GRAD_TILE - 1, GRAD_TILE, GRAD_STEP - 1, GRAD_STEP) if j < n]
    v0, n, skip = chunks[-1]
    if skip:
        cols += [v0 + skip] + list(range(v0, v0 + skip))
    for v0, n, skip in chunks:
        cols += [v0 + skip, v0 + n - 1]
    return list(dict.fromkeys(cols))


def tie_columns(c: MlmCase):
    """two or three columns that hold the row maximum: in different lanes of both lane maps (group of four mod 64, column mod 64), in
    different chunks where there are several, the third among the tail chunk's counted columns where there is one"""
    r = _rng("G.ties", c.index)
    chunks = xent_chunks(c.V, c.width)
    V8 = c.V // 8 * 8
    main = [ch for ch in chunks if ch[2] == 0]
    lanes = lambda col: ((col // 4) % 64, col % 64)      # noqa: E731
    while True:
        a = r.randrange(main[0][0], main[0][0] + main[0][1])
        b = r.randrange(main[-1][0], main[-1][0] + main[-1][1])
        out = sorted({a, b}) + ([r.randrange(V8, c.V)] if V8 != c.V else [])
        seen = [lanes(col) for col in out]
        if a != b and len({s[0] for s in seen}) == len(out) and len({s[1] for s in seen}) == len(out):
            return out


def _build_g(c: MlmCase):
    g = _gen("G", c.index)
    r = _rng("G", c.index)
    if c.op == "mask_tokens":
        import mlm_ref
        inp = {"ids": torch.randint(0, MLM_VOCAB, (c.N, c.L), generator=g), "seed": torch.tensor(r.randrange(1 << 62)),
               "counter": torch.tensor(r.randrange(1 << 26))}
        if c.given_mask:
            inp["mask"] = (torch.rand(c.N, c.L, generator=g) < 0.8).long()
        every = mlm_ref.mask_tokens(inp["ids"].numpy(), inp["mask"].numpy() if c.given_mask else None, int(inp["seed"]), int(inp["counter"]), c.p,
                                    MLM_VOCAB, MLM_MASK_ID, mask_special(c), c.row_offset, cap=c.N * c.L)
        inp["cap"] = torch.tensor(mask_cap(c, every["selected"]))
        return inp
    if c.op in ("gather", "scatter"):
        sel, T = rows_list(c)
        live = mlm_live(c)
        if c.op == "gather":
            last = _randn(g, T, c.H)
            last[sel[live:].long()] = math.nan
            return {"last": last, "sel": sel, "stats": _stats_of(c)}
        dx = _randn(g, c.cap, c.H)
        dx[live:] = math.nan
        return {"dx": dx, "sel": sel, "stats": _stats_of(c), "T": torch.tensor(T)}
    if c.op == "head":
        sel, T = rows_list(c)
        live, H, V = mlm_live(c), c.H, c.V
        last = _randn(g, T, H)
        last[sel[live:].long()] = math.nan
        tgt = torch.randint(0, V, (c.cap,), generator=g).int()
        edge = xent_targets(c)
        at = r.randrange(len(edge))
        for i in range(live):
            tgt[i] = (edge[at:] + edge[:at])[i % len(edge)]
        tgt[live:] = -1
        inp = {"last": last, "sel": sel, "tgt": tgt, "stats": _stats_of(c), "scale": torch.tensor([1.0 / max(live, 1)]),
               "upstream": torch.tensor([3.0]), "wd": _randn(g, H, H) / H ** 0.5, "bd": 0.1 * _randn(g, H), "gamma": 1 + 0.1 * _randn(g, H),
               "beta": 0.1 * _randn(g, H), "wdec": _randn(g, V, H) / H ** 0.5, "bdec": 0.1 * _randn(g, V)}
        import mlm_ref
        best = mlm_ref.head_logits(last[sel[:live].long()].double(), *[inp[k].double() for k in ("wd", "bd", "gamma", "beta", "wdec", "bdec")]).argmax(1)
        tgt[1:live:2] = best[1::2].int()      # every other row's target is its arg-max: `correct` counts something
        return inp
    rows, V, live = c.cap, c.V, mlm_live(c)
    chunks = xent_chunks(V, c.width)
    S, bias = 3.0 * _randn(g, rows, V), _randn(g, V)
    tgt = torch.randint(0, V, (rows,), generator=g).int()
    edge = xent_targets(c)
    at = r.randrange(len(edge))
    for i in range(min(live, len(edge))):
        tgt[i] = (edge[at:] + edge[:at])[i]
    if c.profile in ("pm80", "dominant") and len(chunks) > 1 and live:      # one row's target in the first chunk: what every later chunk
        tgt[0] = r.randrange(chunks[0][1])                                  # must carry along
    if c.profile == "pm80":
        pool = range(chunks[0][1] if len(chunks) > 1 else 0, V)
        first, rest = r.randrange(chunks[0][1]), r.sample(pool, min(2, len(pool)))
        hot = [first] + [v for v in rest if v != first]
        bias[hot[0]], bias[hot[1]] = 80.0, -80.0
        if len(hot) > 2:
            bias[hot[2]] = 80.0
        if live >= 3:
            tgt[live - 1], tgt[live - 2] = hot[0], hot[1]
    elif c.profile == "dominant":      # the target's probability is 1 - 0.95e-6: p - 1 cancels, and the row's loss is half an ulp of its lse
        x = S.double() + bias.double()
        for i in range(live):
            others = x[i].clone()
            others[int(tgt[i])] = -math.inf
            S[i, int(tgt[i])] = float(torch.logsumexp(others, 0)) - math.log(0.95e-6) - float(bias[int(tgt[i])])
    elif c.profile == "ties":          # integers, and no bias on the columns of the maxima: their equality is exact
        S = S.round()
        ties = tie_columns(c)
        bias[ties] = 0.0
        S[:, ties] = TIE_VALUE
        for i in range(live):
            if i % 4 < 3:
                tgt[i] = ties[min(i % 4, len(ties) - 1)]
    S[live:] = math.nan
    tgt[live:] = -1
    x = (S.double() + bias.double())[:live]
    lse = torch.zeros(rows)
    lse[:live] = torch.logsumexp(x, 1).float()      # what xent_grad is handed: the float64 log-sum-exp rounded to float32
    return {"S": S, "bias": bias, "tgt": tgt, "stats": _stats_of(c), "scale": torch.tensor([1.0 / max(live, 1)]),
            "upstream": torch.tensor([0.75]), "lse_in": lse}


def _pad_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def xent_factor(c: MlmCase, inp, dt) -> torch.Tensor:
    """f = upstream * scale * alpha, in the kernel's order"""
    return inp["upstream"].to(dt)[0] * inp["scale"].to(dt)[0] * torch.tensor(c.alpha, dtype=torch.float32).to(dt)


def _eval_g(c: MlmCase, inp, dt, blocks_summed=None):
    if c.op == "mask_tokens":
        import mlm_ref
        import numpy as np
        cap = int(inp["cap"])
        ref = mlm_ref.mask_tokens(inp["ids"].numpy(), inp["mask"].numpy() if c.given_mask else None, int(inp["seed"]), int(inp["counter"]), c.p,
                                  MLM_VOCAB, MLM_MASK_ID, mask_special(c), c.row_offset, cap=cap)
        flags = (ref["kind"] != mlm_ref.KEEP).reshape(-1)
        sel, tgt, counts = mask_place(flags, inp["ids"].numpy(), cap, blocks_summed)
        if blocks_summed is None:      # the reference: the first `cap` selected tokens in token order, not the block-wise placement
            sel, tgt = ref["sel"], ref["tgt"]
        return {"ids": torch.as_tensor(ref["ids_out"]), "sel": torch.as_tensor(np.asarray(sel)), "tgt": torch.as_tensor(np.asarray(tgt)),
                "stats": torch.tensor([ref["kept"], ref["selected"]], dtype=torch.int32), "count": torch.tensor([float(ref["kept"])]),
                "blocks": torch.as_tensor(counts)}
    live = mlm_live(c)
    if c.op == "gather":
        T = inp["last"].shape[0]
        out = torch.zeros(c.cap, c.H)
        for i in range(live):
            if 0 <= int(inp["sel"][i]) < T:
                out[i] = inp["last"][int(inp["sel"][i])]
        return {"out": torch.stack(canonical_planes(out)) if c.planes else out.to(dt)}
    if c.op == "scatter":
        T = int(inp["T"])
        out = torch.zeros(T, c.H, dtype=dt)
        for i in range(live):
            if 0 <= int(inp["sel"][i]) < T:
                out[int(inp["sel"][i])] = inp["dx"][i].to(dt)
        return {"dlast": out}
    if c.op == "head":
        import mlm_ref
        params = [inp[k] for k in ("wd", "bd", "gamma", "beta", "wdec", "bdec")]
        last = torch.nan_to_num(inp["last"], nan=0.0)      # the poisoned tokens are behind the kept slots: never read
        sel, tgt = inp["sel"].numpy(), inp["tgt"].numpy()
        out = mlm_ref.head_loss(last, sel, tgt, live, params, float(inp["scale"][0]), weight=c.alpha * float(inp["upstream"][0]), dtype=dt)
        res = {"loss": torch.tensor(out["loss"], dtype=dt), "dlast": out["dlast"]}
        res.update({"d" + k: g for k, g in zip(("wd", "bd", "gamma", "beta", "wdec", "bdec"), out["dparams"])})
        logits = mlm_ref.head_logits(last[torch.as_tensor(sel[:live]).long()].double(), *[p.double() for p in params])
        t = torch.as_tensor(tgt[:live]).long()
        res["aux:correct"] = torch.tensor([mlm_ref.correct_range(logits, t, 2e-5), mlm_ref.correct_range(logits, t, 3e-4)])      # fp32, split-bf16
        return res
    rows, V = c.cap, c.V
    x = (inp["S"].to(dt) + inp["bias"].to(dt))[:live]
    tgt = inp["tgt"][:live].long()
    hot = torch.zeros(live, V, dtype=torch.bool)
    hot[torch.arange(live), tgt] = True
    lse = torch.logsumexp(x, 1)
    rowloss = lse - x[hot]
    hit = (x.argmax(1) == tgt).int()
    f = xent_factor(c, inp, dt)
    given = inp["lse_in"].to(dt)[:live, None]
    grad = (torch.exp(x - given) - hot.to(dt)) * f
    # the bound's magnitudes, and which decisions are clear, from float64 whatever dt is
    S64, b64 = inp["S"].double()[:live], inp["bias"].double()
    x64 = S64 + b64
    p64 = torch.softmax(x64, 1)
    f64 = float(xent_factor(c, inp, torch.float64).abs())
    mag = f64 * (p64 + hot.double()) * (1.0 + S64.abs() + b64.abs() + x64.abs() + torch.logsumexp(x64, 1, keepdim=True).abs())
    exact = c.profile == "ties"      # equal maxima are exact integers, every other logit lies far below them
    sure = torch.ones(live, dtype=torch.bool)
    if live and not exact:           # fl(S + bias) moves a logit by at most 2^-24 max |x|: mlm_ref.correct_range at that tolerance
        top = x64.topk(2, 1).values
        sure = (top[:, 0] - top[:, 1]) > 2.0 * U24 * float(x64.abs().max())
    if exact or not live:
        crange = (int(hit.sum()), int(hit.sum()))
    else:
        import mlm_ref
        crange = mlm_ref.correct_range(x64, tgt, U24)
    skip = xent_chunks(V, c.width)[-1][2]
    return {"lse": _pad_rows(lse, rows), "rowloss": _pad_rows(rowloss, rows), "loss": rowloss.sum() * inp["scale"].to(dt)[0],
            "hit": _pad_rows(hit, rows), "correct": hit.sum().reshape(1).int(), "grad": _pad_rows(grad, rows),
            "grad_skip": torch.zeros(rows, skip, dtype=dt), "mag:grad": _pad_rows(mag, rows), "aux:sure": torch.cat([sure, torch.ones(rows - live, dtype=torch.bool)]),
            "aux:correct": torch.tensor([crange]), "aux:tiny": _pad_rows(torch.full((live, 1), f64 * F32_TINY, dtype=torch.float64), rows)}


def grad_c(c: MlmCase) -> float:
    """the gradient's constant in units of 2^-24 mag: 8 e32, e32 measured on exp(x - lse) in float32 (E32)"""
    return 8.0 * E32[group(c, "grad")]


def grad_extra(ref, planes: bool) -> torch.Tensor:
    """products that underflow (|f| times the smallest normal float32, on the rows that count), and the planes form's storage tolerance"""
    extra = ref["aux:tiny"].expand_as(ref["grad"])
    return extra + PLANES_TOL * ref["grad"].abs().double() if planes else extra


def _check_g(case: MlmCase, ref, got, split, planes_out):
    res = []
    live = mlm_live(case)
    for name, g in got.items():
        kind, r = kind_of(case, name), ref.get(name)
        if kind == "exact":
            res.append((name,) + exact_equal(g, r))
        elif kind == "hit":            # a decision: exact wherever the reference's two largest logits are clear of each other, and the
            # zeros of the rows that do not count
            g = torch.where(ref["aux:sure"], g.cpu().to(r.dtype).reshape(r.shape), r)
            res.append((name,) + exact_equal(g, r))
        elif kind == "range":
            lo, hi = ref["aux:correct"][1 if split and case.op == "head" else 0].tolist()
            res.append((name, 0.0 if lo <= int(g.reshape(-1)[0]) <= hi else math.inf, ()))
        elif kind == "grad":
            res.append((name,) + forward_bound(g, r, ref["mag:grad"], grad_c(case) * U24, grad_extra(ref, name in planes_out)))
        else:
            g = g.detach().double().cpu().reshape(r.shape)
            if case.op == "xent" and r.dim() == 1 and bool((g[live:] != 0).any()):      # rows that do not count: exact zeros
                res.append((name, math.inf, (live + int((g[live:] != 0).nonzero()[0]),)))
                continue
            ratio, idx = (row_scaled if kind == "row" else col_scaled)(g, r)
            res.append((name, ratio / bound_of(case, name, split, name in planes_out), idx))
    return res


# ================================================================================================================ one interface
import sweep_conv_cases as _H  # noqa: E402  (family H lives there; it uses the sampling and the comparators above)

ConvCase = _H.ConvCase
_GENS = {"A": _gen_a, "B32": _gen_b, "BPL": _gen_b, "C": _gen_c, "D": _gen_d, "E": _gen_e, "F": _gen_f, "G": _gen_g,
         "H32": lambda i, sched: _H.gen(i, sched), "HPL": lambda i, sched: _H.gen(i, sched)}
_CACHE: Dict[str, list] = {}


def cases(family: str) -> list:
    if family not in _CACHE:
        sched = Schedule(family)
        _CACHE[family] = [_GENS[family](i, sched) for i in range(NCASES[family])]
    return _CACHE[family]


def family_of(case) -> str:
    return {AttnCase: "A", ColCase: "C", HeadCase: "D", RowCase: "E", ImgCase: "F", MlmCase: "G"}.get(type(case)) or case.family


def legal(case) -> bool:
    if isinstance(case, AttnCase):      # bert.hip:942,989: 4 <= dH <= 64, dH % 4 == 0, 1 <= L <= 512; bert.hip:973,1020: B, nH > 0
        return 4 <= case.dH <= 64 and case.dH % 4 == 0 and 1 <= case.L <= 512 and case.B > 0 and case.nH > 0
    return {GemmCase: _legal_b, ColCase: _legal_c, HeadCase: _legal_d, RowCase: _legal_e, ImgCase: _legal_f, MlmCase: _legal_g,
            ConvCase: _H.legal}[type(case)](case)


def build(case) -> Dict[str, torch.Tensor]:
    return {AttnCase: _build_a, GemmCase: _build_b, ColCase: _build_c, HeadCase: _build_d, RowCase: _build_e, ImgCase: _build_f,
            MlmCase: _build_g, ConvCase: _H.build}[type(case)](case)


def evaluate(case, inp, dt) -> Dict[str, torch.Tensor]:
    return {AttnCase: _eval_a, GemmCase: _eval_b, ColCase: _eval_c, HeadCase: _eval_d, RowCase: _eval_e, ImgCase: _eval_f,
            MlmCase: _eval_g, ConvCase: _H.evaluate}[type(case)](case, inp, dt)


def reference(case, inp) -> Dict[str, torch.Tensor]:
    return evaluate(case, inp, torch.float64)


def describe(case) -> str:
    return f"({family_of(case)!r}, {case.index}, {case})"


# ---------------------------------------------------------------------------------------------------------------- bounds of A, C, D
BACKWARD = {"dqkv", "dx", "dy", "dcos", "din", "grad", "dgamma", "dbeta", "dxsum", "A", "B", "Cc", "dz"}


def group(case, name: str) -> Tuple[str, str]:
    """the key of E32 an output belongs to: (family.operation.output, value profile)"""
    if isinstance(case, AttnCase):
        return "A." + name, case.profile
    if isinstance(case, ColCase):
        return f"C.{case.op}.{name}", case.profile
    if isinstance(case, ImgCase) and case.op == "bn_train" and case.rows <= 3:
        # two or three values per channel: dz and its coefficients are what a cancellation leaves (dz vanishes identically at n = 2)
        return f"F.bn_train.{name}", f"{case.profile}/n{case.rows}"
    return f"{family_of(case)}.{case.op}.{name}", case.profile


def floor_of(case, name: str, split: bool = False, planes_out: bool = False) -> float:
    """the project's existing bounds: 2e-5 forward, 5e-5 backward, 1e-6 for a column mean (test_train_mode_batchnorm_kernels), and
    3e-4 for planes tensors / split-bf16 mode; the convolutions' dgamma: 2e-3, and 2e-2 on planes operands / in split-bf16 mode
    (tests/test_kernels_gpu.py, tests/test_conv_geometry_gpu.py)"""
    if isinstance(case, ConvCase):
        return _H.floor(case, name, split)
    col_mean = name == "mean" and (isinstance(case, ColCase) or getattr(case, "op", "") == "bn_train")
    f = 1e-6 if col_mean else 5e-5 if name in BACKWARD else 2e-5
    if isinstance(case, MlmCase):      # the cross-entropy kernels: this head's own floor; the head: a gradient is every output but the loss
        f = MLM_XENT_FLOOR if case.op == "xent" else 2e-5 if name == "loss" else 5e-5
    if split or planes_out or (isinstance(case, ColCase) and case.planes):
        f = max(f, 3e-4)
    return f


# measured by tests/test_sweep_host.py::test_e32_table (evaluate(..., float32) against float64 through the family's comparator,
# maximised over the cases of the key) on two hosts -- the CPU-only one and the GPU host: the larger figure times 1.4 where twice the
# smaller allows it, else the larger figure itself, rounded up to two digits; that test keeps every entry within [measured, 2 measured]
# (2 measured times E32_HOST_RATIO for the few keys below)
E32: Dict[Tuple[str, str], float] = {
    ('A.ctx', 'base'): 2e-06,
    ('A.ctx', 'flat'): 7.6e-07,
    ('A.ctx', 'std30_outlier'): 3.7e-05,
    ('A.ctx', 'std8'): 1.1e-05,
    ('A.dqkv', 'base'): 2.2e-06,
    ('A.dqkv', 'flat'): 1.5e-06,
    ('A.dqkv', 'std30_outlier'): 0.00062,
    ('A.dqkv', 'std8'): 0.00025,
    ('A.probs', 'base'): 1.1e-06,
    ('A.probs', 'flat'): 8.1e-08,
    ('A.probs', 'std30_outlier'): 4.1e-05,
    ('A.probs', 'std8'): 8.2e-06,
    ('C.coldot.out', 'offset'): 0.00012,
    ('C.coldot.out', 'randn'): 4e-05,
    ('C.coldot_shift.out', 'offset'): 4.7e-05,
    ('C.coldot_shift.out', 'randn'): 3.8e-05,
    ('C.colstats_biased.mean', 'offset'): 1.7e-07,
    ('C.colstats_biased.mean', 'randn'): 4.5e-05,
    ('C.colstats_biased.var', 'offset'): 2.3e-07,
    ('C.colstats_biased.var', 'randn'): 3.8e-07,
    ('C.colstats_unbiased.mean', 'offset'): 3.2e-07,
    ('C.colstats_unbiased.mean', 'randn'): 7.3e-05,
    ('C.colstats_unbiased.var', 'offset'): 4.8e-07,
    ('C.colstats_unbiased.var', 'randn'): 3.2e-07,
    ('C.colsum.out', 'offset'): 1.6e-07,
    ('C.colsum.out', 'randn'): 5.4e-05,
    ('C.colvar.out', 'offset'): 5e-07,
    ('C.colvar.out', 'randn'): 3.3e-07,
    ('D.bce.dcos', 'base'): 6.9e-07,
    ('D.bce.logits', 'base'): 8.4e-08,
    ('D.bce.loss', 'base'): 1.8e-07,
    ('D.bce.score', 'base'): 5.1e-06,
    ('D.cosine.cos', 'base'): 5.7e-05,
    ('D.cosine.dx', 'base'): 4.6e-07,
    ('D.cosine.dy', 'base'): 2.2e-06,
    ('D.cosine.max', 'base'): 1.1e-05,
    ('D.cosine.mean', 'base'): 1.1e-05,
    ('D.cosine.xn', 'base'): 2.2e-07,
    ('D.cosine.yn', 'base'): 1.8e-07,
    ('D.group_mean.din', 'base'): 6.2e-08,
    ('D.group_mean.out', 'base'): 5.1e-07,
    ('D.infonce.diag', 'base'): 0,
    ('D.infonce.diag', 'sharp'): 0,
    ('D.infonce.grad', 'base'): 1.2e-07,
    ('D.infonce.grad', 'sharp'): 4.6e-08,
    ('D.infonce.loss', 'base'): 1.6e-07,
    ('D.infonce.loss', 'sharp'): 4.4e-08,
    ('D.infonce.lse', 'base'): 9e-08,
    ('D.infonce.lse', 'sharp'): 0,
    ('D.l2norm.dx', 'base'): 1.5e-07,
    ('D.l2norm.norm', 'base'): 2.1e-07,
    ('D.l2norm.xhat', 'base'): 2.4e-07,
    ('E.embed_ln_fwd.rstd', 'base'): 2.3e-07,
    ('E.embed_ln_fwd.xhat', 'base'): 3.1e-07,
    ('E.embed_ln_fwd.y', 'base'): 4.4e-07,
    ('E.ln_bwd.dbeta', 'near_constant'): 4.2e-05,
    ('E.ln_bwd.dbeta', 'outlier'): 2e-05,
    ('E.ln_bwd.dbeta', 'randn'): 6.3e-05,
    ('E.ln_bwd.dbeta', 'row_offset'): 3.6e-05,
    ('E.ln_bwd.dbeta', 'row_scale'): 4.7e-05,
    ('E.ln_bwd.dgamma', 'near_constant'): 1.2e-05,
    ('E.ln_bwd.dgamma', 'outlier'): 4.4e-05,
    ('E.ln_bwd.dgamma', 'randn'): 6.8e-05,
    ('E.ln_bwd.dgamma', 'row_offset'): 2.9e-05,
    ('E.ln_bwd.dgamma', 'row_scale'): 4.2e-05,
    ('E.ln_bwd.dx', 'near_constant'): 9e-06,
    ('E.ln_bwd.dx', 'outlier'): 5.9e-07,
    ('E.ln_bwd.dx', 'randn'): 2.9e-07,
    ('E.ln_bwd.dx', 'row_offset'): 6.2e-06,
    ('E.ln_bwd.dx', 'row_scale'): 2.7e-07,
    ('E.ln_bwd.dxsum', 'near_constant'): 4.6e-05,
    ('E.ln_bwd.dxsum', 'outlier'): 1.8e-05,
    ('E.ln_bwd.dxsum', 'randn'): 6.2e-05,
    ('E.ln_bwd.dxsum', 'row_offset'): 4.7e-05,
    ('E.ln_bwd.dxsum', 'row_scale'): 7.3e-05,
    ('E.ln_fwd.rstd', 'near_constant'): 3.4e-06,
    ('E.ln_fwd.rstd', 'outlier'): 3.1e-07,
    ('E.ln_fwd.rstd', 'randn'): 2.3e-07,
    ('E.ln_fwd.rstd', 'row_offset'): 1.5e-05,
    ('E.ln_fwd.rstd', 'row_scale'): 3e-07,
    ('E.ln_fwd.xhat', 'near_constant'): 0.00022,
    ('E.ln_fwd.xhat', 'outlier'): 2.9e-07,
    ('E.ln_fwd.xhat', 'randn'): 3.2e-07,
    ('E.ln_fwd.xhat', 'row_offset'): 9.1e-05,
    ('E.ln_fwd.xhat', 'row_scale'): 3.6e-07,
    ('E.ln_fwd.y', 'near_constant'): 0.00025,
    ('E.ln_fwd.y', 'outlier'): 3e-07,
    ('E.ln_fwd.y', 'randn'): 3e-07,
    ('E.ln_fwd.y', 'row_offset'): 9.8e-05,
    ('E.ln_fwd.y', 'row_scale'): 4.1e-07,
    ('F.bn_fold.rstd', 'base'): 1.2e-07,
    ('F.bn_fold.scale', 'base'): 1.2e-07,
    ('F.bn_fold.shift', 'base'): 2.7e-06,
    ('F.bn_fold.w_scaled', 'base'): 1.5e-07,
    ('F.bn_train.A', 'offset0'): 2.1e-07,
    ('F.bn_train.A', 'offset0/n2'): 1.6e-07,
    ('F.bn_train.A', 'offset0/n3'): 2.8e-07,
    ('F.bn_train.A', 'offset30'): 2.7e-07,
    ('F.bn_train.A', 'offset30/n2'): 2.4e-07,
    ('F.bn_train.A', 'offset300'): 2.7e-07,
    ('F.bn_train.A', 'offset300/n2'): 2.1e-07,
    ('F.bn_train.A', 'offset300/n3'): 2.4e-07,
    ('F.bn_train.A', 'offset3000'): 2.8e-07,
    ('F.bn_train.A', 'offset3000/n2'): 2.2e-07,
    ('F.bn_train.A', 'offset3000/n3'): 2.6e-07,
    ('F.bn_train.B', 'offset0'): 5.9e-06,
    ('F.bn_train.B', 'offset0/n2'): 2.2e-07,
    ('F.bn_train.B', 'offset0/n3'): 3.2e-06,
    ('F.bn_train.B', 'offset30'): 0.00023,
    ('F.bn_train.B', 'offset30/n2'): 9.1e-05,
    ('F.bn_train.B', 'offset300'): 0.0082,
    ('F.bn_train.B', 'offset300/n2'): 3.4e-05,
    ('F.bn_train.B', 'offset300/n3'): 0.0012,
    ('F.bn_train.B', 'offset3000'): 0.012,
    ('F.bn_train.B', 'offset3000/n2'): 0.00029,
    ('F.bn_train.B', 'offset3000/n3'): 0.0066,
    ('F.bn_train.Cc', 'offset0'): 1.1e-05,
    ('F.bn_train.Cc', 'offset0/n2'): 4.3e-07,
    ('F.bn_train.Cc', 'offset0/n3'): 1.5e-06,
    ('F.bn_train.Cc', 'offset30'): 0.00018,
    ('F.bn_train.Cc', 'offset30/n2'): 2.2e-05,
    ('F.bn_train.Cc', 'offset300'): 0.017,
    ('F.bn_train.Cc', 'offset300/n2'): 3.4e-05,
    ('F.bn_train.Cc', 'offset300/n3'): 0.00083,
    ('F.bn_train.Cc', 'offset3000'): 0.012,
    ('F.bn_train.Cc', 'offset3000/n2'): 0.00028,
    ('F.bn_train.Cc', 'offset3000/n3'): 0.0024,
    ('F.bn_train.dbeta', 'offset0'): 1.6e-05,
    ('F.bn_train.dbeta', 'offset0/n2'): 1.2e-07,
    ('F.bn_train.dbeta', 'offset0/n3'): 1.2e-07,
    ('F.bn_train.dbeta', 'offset30'): 3.4e-05,
    ('F.bn_train.dbeta', 'offset30/n2'): 2.3e-06,
    ('F.bn_train.dbeta', 'offset300'): 5.1e-05,
    ('F.bn_train.dbeta', 'offset300/n2'): 1.2e-07,
    ('F.bn_train.dbeta', 'offset300/n3'): 1.2e-07,
    ('F.bn_train.dbeta', 'offset3000'): 4.4e-06,
    ('F.bn_train.dbeta', 'offset3000/n2'): 1.2e-07,
    ('F.bn_train.dbeta', 'offset3000/n3'): 5.1e-06,
    ('F.bn_train.dgamma', 'offset0'): 1.1e-05,
    ('F.bn_train.dgamma', 'offset0/n2'): 1.6e-07,
    ('F.bn_train.dgamma', 'offset0/n3'): 4e-06,
    ('F.bn_train.dgamma', 'offset30'): 0.00032,
    ('F.bn_train.dgamma', 'offset30/n2'): 0.00043,
    ('F.bn_train.dgamma', 'offset300'): 0.011,
    ('F.bn_train.dgamma', 'offset300/n2'): 0.00073,
    ('F.bn_train.dgamma', 'offset300/n3'): 0.0009,
    ('F.bn_train.dgamma', 'offset3000'): 0.012,
    ('F.bn_train.dgamma', 'offset3000/n2'): 0.03,
    ('F.bn_train.dgamma', 'offset3000/n3'): 0.054,
    ('F.bn_train.dot', 'offset0'): 1.4e-05,
    ('F.bn_train.dot', 'offset0/n2'): 1.6e-07,
    ('F.bn_train.dot', 'offset0/n3'): 4e-06,
    ('F.bn_train.dot', 'offset30'): 0.00015,
    ('F.bn_train.dot', 'offset30/n2'): 3.5e-05,
    ('F.bn_train.dot', 'offset300'): 0.0035,
    ('F.bn_train.dot', 'offset300/n2'): 3.3e-05,
    ('F.bn_train.dot', 'offset300/n3'): 0.00053,
    ('F.bn_train.dot', 'offset3000'): 0.0049,
    ('F.bn_train.dot', 'offset3000/n2'): 0.00029,
    ('F.bn_train.dot', 'offset3000/n3'): 0.0066,
    ('F.bn_train.dz', 'offset0'): 3.1e-07,
    ('F.bn_train.dz', 'offset0/n3'): 4.9e-05,
    ('F.bn_train.dz', 'offset30'): 4e-06,
    ('F.bn_train.dz', 'offset300'): 4.5e-05,
    ('F.bn_train.dz', 'offset300/n3'): 0.013,
    ('F.bn_train.dz', 'offset3000'): 0.00013,
    ('F.bn_train.dz', 'offset3000/n3'): 0.073,
    ('F.bn_train.mean', 'offset0'): 0.0003,
    ('F.bn_train.mean', 'offset0/n2'): 1.2e-07,
    ('F.bn_train.mean', 'offset0/n3'): 1.8e-06,
    ('F.bn_train.mean', 'offset30'): 3.1e-07,
    ('F.bn_train.mean', 'offset30/n1'): 1.2e-07,
    ('F.bn_train.mean', 'offset30/n2'): 1.2e-07,
    ('F.bn_train.mean', 'offset300'): 3e-07,
    ('F.bn_train.mean', 'offset300/n1'): 1.2e-07,
    ('F.bn_train.mean', 'offset300/n2'): 1.2e-07,
    ('F.bn_train.mean', 'offset300/n3'): 1.2e-07,
    ('F.bn_train.mean', 'offset3000'): 2.8e-07,
    ('F.bn_train.mean', 'offset3000/n1'): 1.2e-07,
    ('F.bn_train.mean', 'offset3000/n2'): 1.2e-07,
    ('F.bn_train.mean', 'offset3000/n3'): 1.7e-07,
    ('F.bn_train.rmean', 'offset0'): 1.2e-07,
    ('F.bn_train.rmean', 'offset0/n3'): 1.2e-07,
    ('F.bn_train.rmean', 'offset30'): 1.9e-06,
    ('F.bn_train.rmean', 'offset30/n1'): 3.8e-07,
    ('F.bn_train.rmean', 'offset30/n2'): 1.2e-07,
    ('F.bn_train.rmean', 'offset300'): 1.9e-07,
    ('F.bn_train.rmean', 'offset300/n3'): 2.1e-07,
    ('F.bn_train.rmean', 'offset3000'): 2.7e-07,
    ('F.bn_train.rmean', 'offset3000/n1'): 1.2e-07,
    ('F.bn_train.rmean', 'offset3000/n2'): 1.4e-07,
    ('F.bn_train.rstd', 'offset0'): 2.3e-07,
    ('F.bn_train.rstd', 'offset0/n2'): 1.6e-07,
    ('F.bn_train.rstd', 'offset0/n3'): 2.3e-07,
    ('F.bn_train.rstd', 'offset30'): 2.5e-07,
    ('F.bn_train.rstd', 'offset30/n1'): 1.2e-07,
    ('F.bn_train.rstd', 'offset30/n2'): 2e-07,
    ('F.bn_train.rstd', 'offset300'): 2.4e-07,
    ('F.bn_train.rstd', 'offset300/n1'): 1.2e-07,
    ('F.bn_train.rstd', 'offset300/n2'): 1.6e-07,
    ('F.bn_train.rstd', 'offset300/n3'): 2e-07,
    ('F.bn_train.rstd', 'offset3000'): 2.3e-07,
    ('F.bn_train.rstd', 'offset3000/n1'): 1.2e-07,
    ('F.bn_train.rstd', 'offset3000/n2'): 2.2e-07,
    ('F.bn_train.rstd', 'offset3000/n3'): 2e-07,
    ('F.bn_train.rvar', 'offset0'): 1.2e-07,
    ('F.bn_train.rvar', 'offset0/n3'): 1.2e-07,
    ('F.bn_train.rvar', 'offset30'): 1.7e-07,
    ('F.bn_train.rvar', 'offset30/n1'): 1.2e-07,
    ('F.bn_train.rvar', 'offset30/n2'): 1.2e-07,
    ('F.bn_train.rvar', 'offset300'): 1.2e-07,
    ('F.bn_train.rvar', 'offset300/n3'): 1.9e-07,
    ('F.bn_train.rvar', 'offset3000'): 1.5e-07,
    ('F.bn_train.rvar', 'offset3000/n1'): 1.2e-07,
    ('F.bn_train.rvar', 'offset3000/n2'): 1.3e-07,
    ('F.bn_train.scale', 'offset0'): 2.1e-07,
    ('F.bn_train.scale', 'offset0/n2'): 1.6e-07,
    ('F.bn_train.scale', 'offset0/n3'): 2.8e-07,
    ('F.bn_train.scale', 'offset30'): 2.7e-07,
    ('F.bn_train.scale', 'offset30/n1'): 1.6e-07,
    ('F.bn_train.scale', 'offset30/n2'): 2.4e-07,
    ('F.bn_train.scale', 'offset300'): 2.7e-07,
    ('F.bn_train.scale', 'offset300/n1'): 1.6e-07,
    ('F.bn_train.scale', 'offset300/n2'): 2.1e-07,
    ('F.bn_train.scale', 'offset300/n3'): 2.4e-07,
    ('F.bn_train.scale', 'offset3000'): 2.8e-07,
    ('F.bn_train.scale', 'offset3000/n1'): 1.4e-07,
    ('F.bn_train.scale', 'offset3000/n2'): 2.2e-07,
    ('F.bn_train.scale', 'offset3000/n3'): 2.6e-07,
    ('F.bn_train.shift', 'offset0'): 5.5e-07,
    ('F.bn_train.shift', 'offset0/n2'): 3.4e-06,
    ('F.bn_train.shift', 'offset0/n3'): 1.1e-05,
    ('F.bn_train.shift', 'offset30'): 4.8e-07,
    ('F.bn_train.shift', 'offset30/n1'): 2.6e-07,
    ('F.bn_train.shift', 'offset30/n2'): 2.7e-07,
    ('F.bn_train.shift', 'offset300'): 4.2e-07,
    ('F.bn_train.shift', 'offset300/n1'): 2e-07,
    ('F.bn_train.shift', 'offset300/n2'): 2.7e-07,
    ('F.bn_train.shift', 'offset300/n3'): 3.2e-07,
    ('F.bn_train.shift', 'offset3000'): 5.4e-07,
    ('F.bn_train.shift', 'offset3000/n1'): 1.9e-07,
    ('F.bn_train.shift', 'offset3000/n2'): 3.4e-07,
    ('F.bn_train.shift', 'offset3000/n3'): 4.4e-07,
    ('F.bn_train.sumdy', 'offset0'): 4.5e-05,
    ('F.bn_train.sumdy', 'offset0/n2'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset0/n3'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset30'): 3.4e-05,
    ('F.bn_train.sumdy', 'offset30/n2'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset300'): 2.1e-05,
    ('F.bn_train.sumdy', 'offset300/n2'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset300/n3'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset3000'): 3.8e-06,
    ('F.bn_train.sumdy', 'offset3000/n2'): 1.2e-07,
    ('F.bn_train.sumdy', 'offset3000/n3'): 1.2e-07,
    ('F.bn_train.var', 'offset0'): 3e-07,
    ('F.bn_train.var', 'offset0/n2'): 1.8e-07,
    ('F.bn_train.var', 'offset0/n3'): 2.8e-07,
    ('F.bn_train.var', 'offset30'): 3.4e-07,
    ('F.bn_train.var', 'offset30/n1'): 1.2e-07,
    ('F.bn_train.var', 'offset30/n2'): 1.2e-07,
    ('F.bn_train.var', 'offset300'): 3.6e-07,
    ('F.bn_train.var', 'offset300/n1'): 1.2e-07,
    ('F.bn_train.var', 'offset300/n2'): 1.2e-07,
    ('F.bn_train.var', 'offset300/n3'): 2.1e-07,
    ('F.bn_train.var', 'offset3000'): 5.8e-07,
    ('F.bn_train.var', 'offset3000/n1'): 1.2e-07,
    ('F.bn_train.var', 'offset3000/n2'): 1.2e-07,
    ('F.bn_train.var', 'offset3000/n3'): 3.9e-07,
    ('F.bn_train.y', 'offset0'): 3.3e-07,
    ('F.bn_train.y', 'offset0/n2'): 2.4e-07,
    ('F.bn_train.y', 'offset0/n3'): 4.7e-07,
    ('F.bn_train.y', 'offset30'): 6.6e-06,
    ('F.bn_train.y', 'offset30/n2'): 2.4e-06,
    ('F.bn_train.y', 'offset300'): 5.8e-05,
    ('F.bn_train.y', 'offset300/n2'): 4.1e-05,
    ('F.bn_train.y', 'offset300/n3'): 4.9e-05,
    ('F.bn_train.y', 'offset3000'): 0.00051,
    ('F.bn_train.y', 'offset3000/n2'): 0.00034,
    ('F.bn_train.y', 'offset3000/n3'): 0.0012,
    # G.head: the float32 matrix products accumulate in float64 (mlm_ref.linear_wide), so that no BLAS order enters.  These eight
    # figures therefore UNDERSTATE a plain float32 evaluation (by two to three times on the hosts measured).  They only show that
    # 8 e32 lies below the head's floors; they must not be used to tighten a floor.
    ('G.head.dbd', 'base'): 2.6e-07,
    ('G.head.dbdec', 'base'): 1.5e-07,
    ('G.head.dbeta', 'base'): 2.5e-07,
    ('G.head.dgamma', 'base'): 4e-07,
    ('G.head.dlast', 'base'): 3.2e-07,
    ('G.head.dwd', 'base'): 2.5e-06,
    ('G.head.dwdec', 'base'): 1.7e-06,
    ('G.head.loss', 'base'): 1.2e-07,
    ('G.xent.grad', 'dominant'): 1.5,          # the gradient: in units of 2^-24 of its magnitudes (grad_c)
    ('G.xent.grad', 'pm80'): 1.1,
    ('G.xent.grad', 'randn3'): 1.5,
    ('G.xent.grad', 'ties'): 1.2,
    ('G.xent.loss', 'dominant'): 1.4,          # a row loss of half an ulp of its log-sum-exp: float32 returns 0 or one ulp
    ('G.xent.loss', 'pm80'): 1.2e-07,
    ('G.xent.loss', 'randn3'): 1.7e-07,
    ('G.xent.loss', 'ties'): 2.9e-06,
    ('G.xent.lse', 'dominant'): 1.2e-07,
    ('G.xent.lse', 'pm80'): 1.2e-07,
    ('G.xent.lse', 'randn3'): 1.2e-07,
    ('G.xent.lse', 'ties'): 1.2e-07,
    ('G.xent.rowloss', 'dominant'): 1.5,
    ('G.xent.rowloss', 'pm80'): 5.9e-06,
    ('G.xent.rowloss', 'randn3'): 3.2e-07,
    ('G.xent.rowloss', 'ties'): 2.9e-06,
    ('H32.dgrad.dx', 'chan_scaled'): 1.1e-07,
    ('H32.dgrad.dx', 'randn'): 9.9e-08,
    ('H32.dgrad.dx', 'relu_like'): 1.2e-07,
    ('H32.dgrad.sums', 'chan_scaled'): 2e-06,
    ('H32.dgrad.sums', 'randn'): 2.3e-05,
    ('H32.dgrad.sums', 'relu_like'): 6.8e-05,
    ('H32.fwd.y', 'chan_scaled'): 1.4e-07,
    ('H32.fwd.y', 'randn'): 1.7e-07,
    ('H32.fwd.y', 'relu_like'): 3.8e-07,
    ('H32.wgrad.dgamma', 'chan_scaled'): 1.4e-05,
    ('H32.wgrad.dgamma', 'randn'): 6.1e-06,
    ('H32.wgrad.dgamma', 'relu_like'): 3.4e-05,
    ('H32.wgrad.dw', 'chan_scaled'): 1.4e-07,
    ('H32.wgrad.dw', 'randn'): 1.5e-07,
    ('H32.wgrad.dw', 'relu_like'): 1.3e-07,
    ('HPL.dgrad.dx', 'chan_scaled'): 1.3e-07,
    ('HPL.dgrad.dx', 'randn'): 1.3e-07,
    ('HPL.dgrad.dx', 'relu_like'): 1.1e-07,
    ('HPL.dgrad.sums', 'chan_scaled'): 6.1e-06,
    ('HPL.dgrad.sums', 'randn'): 2.8e-05,
    ('HPL.dgrad.sums', 'relu_like'): 6e-05,
    ('HPL.fwd.y', 'chan_scaled'): 1.5e-07,
    ('HPL.fwd.y', 'randn'): 3.3e-07,
    ('HPL.fwd.y', 'relu_like'): 1.5e-06,
    ('HPL.wgrad.dgamma', 'chan_scaled'): 1.4e-05,
    ('HPL.wgrad.dgamma', 'randn'): 4.7e-06,
    ('HPL.wgrad.dgamma', 'relu_like'): 3.4e-05,
    ('HPL.wgrad.dw', 'chan_scaled'): 1.6e-07,
    ('HPL.wgrad.dw', 'randn'): 1.5e-07,
    ('HPL.wgrad.dw', 'relu_like'): 1.3e-07,
}


# keys whose float32 figure depends on the host beyond the factor two of test_e32_table.  The host moves the matrix products
# (attention scores and contexts, pairwise cosines: the CPU BLAS blocks them by processor model) and, by an ulp, vectorised sums and
# 1 / sqrt; the thread count moves no entry (measure_e32 runs on one thread, and 1, 8 and 16 threads measure the same).  Every entry is
# the larger host's figure.  Most then still lie within twice the smaller host's; the ones below do not (the cosines, and maxima over
# the 8 .. 24 values of a two-row BatchNorm case, where one ulp is a factor two): their upper limit is wider by this measured ratio,
# larger host / smaller host, and by nothing else.
E32_HOST_RATIO: Dict[Tuple[str, str], float] = {
    ('D.cosine.cos', 'base'): 4.50,      # 5.5e-05 / 1.23e-05
    ('D.cosine.max', 'base'): 4.29,      # 9.84e-06 / 2.31e-06
    ('D.cosine.mean', 'base'): 3.94,      # 9.84e-06 / 2.51e-06
    ('F.bn_train.dz', 'offset0/n3'): 2.16,      # 4.71e-05 / 2.2e-05
}


def bound_of(case, name: str, split: bool = False, planes_out: bool = False) -> float:
    return max(floor_of(case, name, split, planes_out), 8.0 * E32[group(case, name)])


def comparator(case):
    return col_scaled if isinstance(case, ColCase) else row_scaled


def check(case, ref, got, split: bool = False, planes_out=()) -> List[Tuple[str, float, tuple]]:
    """[(name, worst error / bound, index)] over the outputs present in `got`; <= 1 passes"""
    if isinstance(case, GemmCase):
        return _check_b(case, ref, got)
    if isinstance(case, (RowCase, ImgCase)):
        return _check_ef(case, ref, got, split, planes_out)
    if isinstance(case, MlmCase):
        return _check_g(case, ref, got, split, planes_out)
    if isinstance(case, ConvCase):
        return _H.check(case, ref, got, split)
    cmp = comparator(case)
    res = []
    for name, g in got.items():
        ratio, idx = cmp(g, ref[name])
        res.append((name, ratio / bound_of(case, name, split, name in planes_out), idx))
    return res


def failures(case, results) -> str:
    bad = [f"{n}: {r:.3g} x bound at {i}" for n, r, i in results if not r <= 1.0]
    return f"{describe(case)}: " + "; ".join(bad) if bad else ""


def uses_e32(case, name: str) -> bool:
    """outputs judged against max(floor, 8 e32): all of A, C, D; the "row" and "col" outputs of E, F and G, and G's gradient"""
    if name.startswith(("mag:", "aux:")):
        return False
    if isinstance(case, ConvCase):      # H: the outputs with a precision level (dbeta is exact)
        return name in _H.E32_OUTPUTS
    return not isinstance(case, (RowCase, ImgCase, MlmCase)) or kind_of(case, name) in ("row", "col", "grad")


def compare(case, name: str, got, ref, refs=None) -> Tuple[float, tuple]:
    """the comparator's own figure (not yet divided by a bound) of one e32 output; refs: all outputs of the reference (G's gradient is
    measured in units of 2^-24 of its magnitudes)"""
    if isinstance(case, ConvCase):
        return _H.level(case, name, got, ref)
    if isinstance(case, MlmCase) and kind_of(case, name) == "grad":
        return forward_bound(got, ref, refs["mag:grad"], U24, grad_extra(refs, False))
    if isinstance(case, (RowCase, ImgCase, MlmCase)):
        ref = ref.reshape(-1, 1) if name == "rstd" and kind_of(case, name) == "row" else ref
        return (row_scaled if kind_of(case, name) == "row" else col_scaled)(got.reshape(ref.shape), ref)
    return comparator(case)(got, ref)


def measure_e32(family: str) -> Dict[Tuple[str, str], float]:
    """the comparator's figure for the reference formula in float32 (torch, CPU) against float64, maximised per (group, profile).
    One thread while it measures (restored afterwards): a reduction split over threads sums in an order that depends on their number."""
    out: Dict[Tuple[str, str], float] = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in cases(family):
            inp = build(c)
            ref, lo = reference(c, inp), evaluate(c, inp, torch.float32)
            for name, r in ref.items():
                if uses_e32(c, name):
                    k = group(c, name)
                    out[k] = max(out.get(k, 0.0), compare(c, name, lo[name], r, ref)[0])
    finally:
        torch.set_num_threads(threads)
    return out
