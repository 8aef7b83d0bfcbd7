"""TEST-ONLY float64 restatement of elastic weight consolidation over flat buffers (include/cxrk.h
"fisher_accumulate" / "ewc_consolidate" / "ewc_penalty"), of one penalised optimiser step, and the error bounds of the three kernels,
derived from their own roundings the way `optim_ref.sqnorm_depth` is derived.  The scalar arguments are rounded to fp32 first: that
is what the kernels receive.  tests/test_ewc_host.py pins the penalty's gradient to autograd; the GPU tests compare the kernels
with it."""
import numpy as np
import torch

import optim_ref as R

U = R.U                 # unit roundoff of fp32, 2^-24


def f32(x) -> float:
    """a host scalar as the kernel sees it"""
    return float(np.float32(x))


def gamma_k(k: int) -> float:
    """(1 + u)^k - 1 <= k u / (1 - k u) (Higham)"""
    return k * U / (1.0 - k * U)


# ---- the three kernels in float64 ---------------------------------------------------------------------------------------------
def fisher_accumulate(acc, g, w=1.0):
    """acc + w * g^2"""
    return acc.double() + f32(w) * g.double() ** 2


def consolidate(F, acc, p, gamma=1.0, scale=1.0):
    """(gamma * F + scale * acc, p) -- (None, p) with the identity Fisher (acc is None)"""
    if acc is None:
        assert F is None
        return None, p.clone()
    return f32(gamma) * F.double() + f32(scale) * acc.double(), p.clone()


def penalty_grad(g, p, anchor, F, strength):
    """g + strength * F * (p - anchor); F = None: F = 1"""
    d = p.double() - anchor.double()
    return g.double() + f32(strength) * (d if F is None else F.double() * d)


def penalty_terms(p, anchor, F):
    """F * (p - anchor)^2 per element"""
    d = p.double() - anchor.double()
    return d * d if F is None else F.double() * d * d


def penalty_partials(p, anchor, F, nparts: int) -> np.ndarray:
    """float64 partial sums of the terms over the kernel's partition (`optim_ref.by_block`)"""
    return R.by_block(penalty_terms(p, anchor, F).numpy(), nparts)


def block_of(i: int, n: int, nparts: int) -> int:
    """the partial sum element i contributes to"""
    return 0 if i >= (n // 4) * 4 else ((i // 4) % (nparts * 256)) // 256


def penalty_value(p, anchor, F, strength) -> float:
    """strength / 2 * sum F (p - anchor)^2"""
    return 0.5 * f32(strength) * float(penalty_terms(p, anchor, F).sum())


def penalised_step(p, g, anchor, F, strength, lr, optim="sgd", state=None, **adamw):
    """One optimiser step on the penalised gradient, float64 -> (p, penalised gradient, state).  "sgd": p - lr * g'.  "adamw":
    `optim_ref.adamw_step` on g' (state = (m, v, step); keyword arguments beta1, beta2, eps, weight_decay, decay, max_norm): the
    clipping norm is that of the penalised gradient, as if the penalty were part of the loss."""
    gp = penalty_grad(g, p, anchor, F, strength)
    if optim == "sgd":
        return p.double() - f32(lr) * gp, gp, None
    m, v, step = state
    pn, m, v, norm, coef = R.adamw_step(p, gp, m, v, adamw.get("decay"), f32(lr), f32(adamw.get("beta1", 0.9)), f32(adamw.get("beta2", 0.999)),
                                        f32(adamw.get("eps", 1e-8)), f32(adamw.get("weight_decay", 0.0)), step, max_norm=adamw.get("max_norm"))
    return pn, gp, (m, v, step + 1, norm, coef)


# ---- error bounds -------------------------------------------------------------------------------------------------------------
# fisher_accumulate: t = fl(g * g), acc' = fl(acc + w * t) (one fused multiply-add): two roundings,
#   |acc' - ref| <= gamma_2 * (|acc| + w * g^2).
# ewc_consolidate:   s = fl(scale * acc), F' = fl(gamma * F + s): two roundings, |F' - ref| <= gamma_2 * (|gamma * F| + |scale * acc|).
# ewc_penalty:       d = fl(p - a), t = fl(F * d), g' = fl(g + strength * t): three roundings,
#   |g' - ref| <= gamma_3 * (|g| + strength * |F * d|).
FISHER_K, CONSOLIDATE_K, PENALTY_K = 2, 2, 3


def fisher_bound(acc, g, w=1.0):
    return gamma_k(FISHER_K) * (acc.double().abs() + abs(f32(w)) * g.double() ** 2)


def consolidate_bound(F, acc, gamma=1.0, scale=1.0):
    return gamma_k(CONSOLIDATE_K) * ((f32(gamma) * F.double()).abs() + (f32(scale) * acc.double()).abs())


def penalty_grad_bound(g, p, anchor, F, strength):
    d = (p.double() - anchor.double()).abs()
    return gamma_k(PENALTY_K) * (g.double().abs() + abs(f32(strength)) * (d if F is None else F.double().abs() * d))


def penalty_partial_rtol(n: int, nparts: int) -> float:
    """A partial sum (F >= 0: non-negative terms) against float64: a term t * d = F d^2 carries the roundings of d twice and of t once
    before it enters the fused multiply-add chain, whose depth is grad_sqnorm's (`optim_ref.sqnorm_depth`): gamma_(depth + 3)."""
    return R.sqnorm_rtol(n, nparts, extra_levels=3)
