"""TEST-ONLY float64 restatement of `cxrk_ema_update` (include/cxrk.h, "ema_update") and the elementwise bound of its two roundings.

The kernel computes, in fp32 with u = 2^-24 and nothing contracted beyond the one fused multiply-add,

    c   = fl(1 - decay)                  on the host, once; `coef` forms the same fp32 number, so it enters the reference exactly
    d^  = fl(p - e)      = (p - e) (1 + d1)             |d1| <= u
    got = fl(c d^ + e)   = (c d^ + e) (1 + d2)          |d2| <= u      (an fma rounds once)

With the reference r = e + c (p - e):   got - r = c (p - e) d1 + (c (p - e) + e) d2 + c (p - e) d1 d2 = c (p - e) d1 + r d2 + c (p - e) d1 d2,
so   |got - r| <= u (c |p - e| + |r|) + u^2 c |p - e|  <=  u (c |p - e| + |r|) (1 + u).
`bound` states it with the factor (1 + 2^-20) in place of (1 + u): the slack, 2^-44 relative to the terms, covers the float64
evaluation of r itself (a few 2^-53 of c |p - e| + |e|, and |e| <= |r| + c |p - e|).  The subtraction never underflows inexactly;
a result in the subnormal range is rounded to a multiple of 2^-149, hence the additive 2^-149.  Nothing here is tuned: the bound has
no constant taken from a measurement."""
import numpy as np
import torch

U = 2.0 ** -24


def f32(x) -> float:
    """the fp32 number nearest to x, as a Python float"""
    return float(np.float32(x))


def coef(decay) -> float:
    """c = float32(1) - float32(decay), the subtraction in fp32"""
    return float(np.float32(1.0) - np.float32(decay))


def update(avg: torch.Tensor, p: torch.Tensor, decay) -> torch.Tensor:
    """r = e + c (p - e) in float64 from fp32 buffers, on the device they are on"""
    e, q = avg.detach().double(), p.detach().double()
    return e + coef(decay) * (q - e)


def bound(avg: torch.Tensor, p: torch.Tensor, decay) -> torch.Tensor:
    """|got - r| <= 2^-24 (c |p - e| + |r|) (1 + 2^-20) + 2^-149, elementwise"""
    e, q = avg.detach().double(), p.detach().double()
    c = coef(decay)
    return U * (c * (q - e).abs() + (e + c * (q - e)).abs()) * (1.0 + 2.0 ** -20) + 2.0 ** -149


def decay_at(decay: float, updates: int, warmup: bool = True) -> float:
    """d_t of update number `updates` = 1, 2, ...: min(decay, (1 + t) / (10 + t)) with warmup, else decay"""
    return min(float(decay), (1.0 + updates) / (10.0 + updates)) if warmup else float(decay)


def within(got: torch.Tensor, avg: torch.Tensor, p: torch.Tensor, decay) -> float:
    """worst |got - r| / bound over the elements (<= 1 means every element is within the bound)"""
    err = (got.detach().double().to(avg.device) - update(avg, p, decay)).abs()
    return float((err / bound(avg, p, decay)).max())
