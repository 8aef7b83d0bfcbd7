"""TEST-ONLY float64 restatement of A-GEM's gradient projection over flat buffers (include/cxrk.h "agem_dots" /
"agem_project"), and the error bounds of the two kernels, derived from their own roundings the way `optim_ref.sqnorm_depth` and
tests/ewc_ref.py derive theirs.  tests/test_agem_host.py pins the projection to autograd; the GPU tests compare the kernels with it."""
import numpy as np
import torch

import optim_ref as R
from ewc_ref import U, block_of, f32, gamma_k  # noqa: F401


# ---- the two kernels in float64 -----------------------------------------------------------------------------------------------
def dots_partials(g, gref, nparts: int):
    """(shares of sum g * gref, shares of sum gref^2, shares of sum |g * gref|) per block of the kernel's partition, float64"""
    gd, rd = g.double().numpy(), gref.double().numpy()
    return R.by_block(gd * rd, nparts), R.by_block(rd * rd, nparts), R.by_block(np.abs(gd * rd), nparts)


def dots(g, gref):
    """(dot, rr, sum |g * gref|) in float64"""
    gd, rd = g.double(), gref.double()
    return float((gd * rd).sum()), float((rd * rd).sum()), float((gd * rd).abs().sum())


def project(g, gref, coef=None):
    """A-GEM's update in float64: g - coef * gref when g . gref < 0, else g.  `coef` given: the axpy with that coefficient (the
    kernel's own fp32 one), taken unconditionally."""
    if coef is None:
        dot, rr, _ = dots(g, gref)
        if dot >= 0:
            return g.double().clone()
        coef = dot / rr
    return g.double() - float(coef) * gref.double()


# ---- error bounds -------------------------------------------------------------------------------------------------------------
# agem_dots: each term g * gref (gref * gref) enters its accumulator by ONE fused multiply-add, the product exact inside it, then
#   travels grad_sqnorm's tree: depth = optim_ref.sqnorm_depth(n, nparts) additions.  The terms of the dot are signed, so its bound is
#   absolute: |partial - ref| <= gamma_depth * (the block's sum of |g * gref|), not relative to the sum.  The terms of gref . gref are
#   non-negative: relative, gamma_depth, exactly grad_sqnorm's bound.
# agem_project: the partials are summed again (<= ceil(nparts / 256) per thread, 6 butterfly levels, 4 waves): depth + refold levels,
#   dot_k = D + e, |e| <= gamma_total * S with S = sum |g * gref|;  rr_k = RR (1 + d), |d| <= gamma_total.
#   coef_k = fl(dot_k / rr_k) = (D + e) / (RR (1 + d)) * (1 + eps), |eps| <= u:
#       |coef_k - D / RR| <= (|D| (u + gamma) + gamma S (1 + u)) / (RR (1 - gamma)).
#   g' = fl(g - coef_k * gref), one fused multiply-add: |g' - (g - coef_k gref)| <= gamma_1 (|g| + |coef_k gref|).
def dots_depth(n: int, nparts: int) -> int:
    return R.sqnorm_depth(n, nparts)


def refold_levels(nparts: int) -> int:
    return -(-nparts // 256) + 6 + 4


def dot_partial_bound(abs_parts: np.ndarray, n: int, nparts: int) -> np.ndarray:
    return gamma_k(dots_depth(n, nparts)) * abs_parts


def rr_partial_rtol(n: int, nparts: int) -> float:
    return R.sqnorm_rtol(n, nparts)


def total_gamma(n: int, nparts: int) -> float:
    return gamma_k(dots_depth(n, nparts) + refold_levels(nparts))


def dot_bound(g, gref, nparts: int) -> float:
    """the bound of the dot agem_project derives (and reports in stats[0]) against float64: absolute, gamma_total * sum |g * gref|"""
    return total_gamma(g.numel(), nparts) * dots(g, gref)[2]


def rr_rtol(n: int, nparts: int) -> float:
    return total_gamma(n, nparts)


def coef_bound(g, gref, nparts: int) -> float:
    D, RR, S = dots(g, gref)
    gam = total_gamma(g.numel(), nparts)
    return (abs(D) * (U + gam) + gam * S * (1.0 + U)) / (RR * (1.0 - gam))


def axpy_bound(g, gref, coef):
    return gamma_k(1) * (g.double().abs() + (float(coef) * gref.double()).abs())
