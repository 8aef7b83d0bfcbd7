"""TEST-ONLY: tests/cpu_kernels_agem.py plus torch emulations of `kernels.ema_update` and `kernels.flat_swap`, so that `optim.EMA` and
the joint trainer's parameter average run on gloo / CPU.  The kernels' formulas and refusals (include/cxrk.h, "ema_update" /
"flat_swap"): d = p - avg in fp32, then the fused multiply-add through float64 (the product of two fp32 numbers is exact there; the
sum is rounded twice, which differs from the one rounding of the device in rare ties only).  Never imported by the package."""
import numpy as np
import torch

from cpu_kernels_agem import *  # noqa: F401,F403

_BAD = "bad argument / shape / alignment (cxrk code -1)"


def _flat_pair(a, b, name):
    if (a.dim() != 1 or b.dim() != 1 or a.numel() == 0 or b.numel() != a.numel() or a.dtype != torch.float32 or b.dtype != torch.float32
            or not a.is_contiguous() or not b.is_contiguous()):
        raise ValueError(f"{name}: " + _BAD)


def ema_update(avg, p, decay):
    _flat_pair(avg, p, "cxrk_ema_update")
    decay = np.float32(decay)
    if not (decay >= 0 and decay <= 1):
        raise ValueError("cxrk_ema_update: " + _BAD)
    c = float(np.float32(1.0) - decay)
    with torch.no_grad():
        d = p - avg
        r = (c * d.double() + avg.double()).float()
        avg.copy_(torch.where(r == avg, avg, r))               # equal as a number: avg keeps its own bits (a negative zero stays)


def flat_swap(a, b):
    _flat_pair(a, b, "cxrk_flat_swap")
    lo_a, lo_b, nbytes = a.data_ptr(), b.data_ptr(), 4 * a.numel()
    if not (lo_a + nbytes <= lo_b or lo_b + nbytes <= lo_a):
        raise ValueError("cxrk_flat_swap: " + _BAD)
    with torch.no_grad():
        ai, bi = a.view(torch.int32), b.view(torch.int32)      # moves only: every bit pattern survives
        t = ai.clone()
        ai.copy_(bi)
        bi.copy_(t)
