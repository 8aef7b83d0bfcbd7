"""Where the hand-written backward passes put parameter gradients.

PyTorch's autograd adds every gradient a `Function.backward` returns into `param.grad` with one elementwise kernel per tensor
(AccumulateGrad) — 367 launches per training step on this path in round 1.  The encoders instead hand the kernels the
parameter's own `.grad` memory (the flat gradient buffer of `optim._FlatOptimizer`) and let them ACCUMULATE into it, which is
exactly autograd's semantics; `backward` then returns None for those inputs.  A parameter whose `.grad` is missing or laid out
differently gets a fresh tensor that is returned to autograd as usual."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch


def own_layout(g: Optional[torch.Tensor], p: torch.Tensor) -> bool:
    return g is not None and g.dtype == torch.float32 and g.device == p.device and g.shape == p.shape and g.stride() == p.stride()


def dense(t: torch.Tensor) -> bool:
    """the elements occupy one gap-free block in the parameter's own order (contiguous, or channels_last for filters)"""
    return t.is_contiguous() or (t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous())


class GradSink:
    def __init__(self, params: Sequence[torch.Tensor], need: Optional[Sequence[bool]] = None):
        self.params = params
        self.need = list(need) if need is not None else [True] * len(params)
        self.ret: List[Optional[torch.Tensor]] = [None] * len(params)

    def _own_grad(self, j: int) -> Optional[torch.Tensor]:
        p = self.params[j]
        g = getattr(p, "grad", None)
        return g if own_layout(g, p) and dense(g) else None

    def dst(self, j: int, force_fresh: bool = False, zero: bool = False):
        """(tensor the kernels write, accumulate flag).  zero: a fresh tensor must start at zero (scatter-add targets)."""
        g = None if force_fresh else self._own_grad(j)
        if g is not None:
            return g, True
        p = self.params[j]
        t = torch.zeros_like(p) if zero else torch.empty_like(p)
        self.ret[j] = t
        return t, False

    def dst_group(self, *indices: int, force_fresh: bool = False):
        """([tensors the kernels write], accumulate flag) for the gradient outputs of ONE launch, which has one accumulate switch:
        every listed parameter's own `.grad`, or -- as soon as one of them does not qualify -- a fresh tensor for every one."""
        own = [None if force_fresh else self._own_grad(j) for j in indices]
        if all(g is not None for g in own):
            return own, True
        return [self.dst(j, True)[0] for j in indices], False

    def result(self) -> tuple:
        return tuple(g if n else None for g, n in zip(self.ret, self.need))
