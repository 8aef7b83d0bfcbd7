"""Optimisers on the cxrk kernels: drop-in for `optim.Adam(params, lr=lr)` / `optim.SGD(params, lr=lr)` as
constructed in the reference's `Trainer.__init__` (Trainer.py:172-178; torch defaults betas (0.9,0.999), eps 1e-8).

All parameters are re-pointed at slices of ONE flat fp32 buffer (and their `.grad` at slices of a flat gradient
buffer), so an optimiser step is a single HBM-bound kernel launch (28 B/parameter) and a data-parallel gradient
all-reduce is a handful of large contiguous RCCL calls instead of one per tensor.  Parameters that were adjacent in
memory before (the fused q/k/v projections) stay adjacent; the physical layout of each tensor (e.g. channels_last
conv filters) is preserved.

`AdamW` (decoupled weight decay with a no-decay set, global-norm clipping) and `LRSchedule` (warmup / decay) are opt-in additions
that the reference does not have; so is `EWC`, elastic weight consolidation over the same flat buffers (§5.10).  So is
`AGEM`, A-GEM's projection of the step's gradient against an episodic-memory gradient (§5.12), and `EMA`, the exponential moving
average of the flat parameter buffer (§5.14).
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional

import torch

from . import kernels as K


class _FlatOptimizer:
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float):
        plist: List[torch.nn.Parameter] = []
        seen = set()
        for p in params:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                plist.append(p)
        if not plist:
            raise ValueError("optimizer got an empty parameter list")
        dev = plist[0].device  # step() raises for non-GPU parameters (the kernels have no CPU fallback)
        for p in plist:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("all parameters must be fp32 on one device")
        self.params = plist
        self.param_groups = [{"params": plist, "lr": lr}]
        # Layout of the flat buffers: parameter-list order, except that tensors sharing one storage (the fused q/k/v
        # projections) stay together in storage order.  It must NOT depend on allocation addresses: every data-parallel
        # rank has to lay its buffers out identically, or the flat all-reduce adds gradients of different tensors
        # (tests/test_dist_gpu.py caught exactly that with an address-sorted layout).
        groups: dict = {}
        for i, p in enumerate(plist):
            groups.setdefault(p.untyped_storage().data_ptr(), []).append(i)
        order = [i for idxs in groups.values() for i in sorted(idxs, key=lambda j: plist[j].storage_offset())]
        offs, total = {}, 0
        for i in order:
            offs[i] = total
            total += (plist[i].numel() + 3) // 4 * 4
        self.numel = total
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        self._views = []
        with torch.no_grad():
            for i, p in enumerate(plist):
                o, n = offs[i], p.numel()
                if not _dense(p):
                    p.data = p.data.contiguous()
                pv = self.flat_p[o:o + n].as_strided(p.shape, p.stride())
                pv.copy_(p.data)
                p.data = pv
                gv = self.flat_g[o:o + n].as_strided(p.shape, p.stride())
                p.grad = gv
                self._views.append(gv)
        self.steps = 0

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Zero the flat gradient buffer.  `set_to_none` is ignored: gradients must stay views of the flat buffer."""
        self.flat_g.zero_()
        for p, gv in zip(self.params, self._views):
            if p.grad is not gv:
                p.grad = gv

    def _sync_grads(self) -> None:
        for p, gv in zip(self.params, self._views):
            if p.grad is None:
                continue  # never received a gradient this step: its slice of flat_g is zero
            if p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad)
                p.grad = gv

    def grad_span(self, params) -> Optional[tuple]:
        """(lo, hi) element range of the flat gradient buffer that holds exactly the gradients of `params`, or None when they
        do not form one gap-free range (then only the whole buffer can be reduced at once)."""
        ids = {id(p) for p in params}
        base = self.flat_g.data_ptr()
        lo, hi, tot = None, 0, 0
        for p, gv in zip(self.params, self._views):
            if id(p) in ids:
                o = (gv.data_ptr() - base) // 4
                n = (p.numel() + 3) // 4 * 4
                lo = o if lo is None else min(lo, o)
                hi, tot = max(hi, o + n), tot + n
        return (lo, hi) if lo is not None and hi - lo == tot else None

    def all_reduce_span(self, lo: int, hi: int, group=None, bucket_bytes: int = 256 << 20) -> list:
        """Start the sum of flat_g[lo:hi] over the group (async, ordered after the work already queued on the CURRENT stream);
        returns the work handles for `all_reduce_grads(skip=..., pending=...)` to wait on."""
        import torch.distributed as dist
        step = max(1, bucket_bytes // 4)
        return [dist.all_reduce(self.flat_g[o:min(hi, o + step)], group=group, async_op=True) for o in range(lo, hi, step)]

    def all_reduce_grads(self, group=None, bucket_bytes: int = 256 << 20, average: bool = False, skip=None,
                         pending: Optional[list] = None, pre_scale: Optional[float] = None) -> None:
        """Sum (or average) the flat gradient buffer over the data-parallel group in large contiguous buckets.  `skip` = element
        range(s) already being reduced by `all_reduce_span` (one (lo, hi) tuple or a list of them; their handles in `pending`).
        `pre_scale`: multiply this rank's gradients by it before the sum (shards of unequal size: rows / global rows)."""
        import torch.distributed as dist
        self._sync_grads()
        n = self.flat_g.numel()
        if pre_scale is not None:
            if skip:
                raise ValueError("all_reduce_grads: pre_scale cannot be combined with ranges that are already being reduced")
            K.scale_mask(self.flat_g, alpha=float(pre_scale), out=self.flat_g)
        spans = _complement(skip, n)
        works = list(pending or [])
        for lo, hi in spans:
            if hi > lo:
                works += self.all_reduce_span(lo, hi, group, bucket_bytes)
        for w in works:
            w.wait()
        if average:
            K.scale_mask(self.flat_g, alpha=1.0 / dist.get_world_size(group), out=self.flat_g)

    @property
    def lr(self) -> float:
        return float(self.param_groups[0]["lr"])


def _complement(skip, n: int) -> list:
    """[0, n) minus the (lo, hi) range(s) in `skip` (which must not overlap), as a sorted list of ranges."""
    if not skip:
        return [(0, n)]
    ranges = sorted([tuple(skip)] if isinstance(skip[0], int) else [tuple(r) for r in skip])
    out, pos = [], 0
    for lo, hi in ranges:
        if lo < pos or hi > n or hi < lo:
            raise ValueError(f"all_reduce_grads: skip ranges {ranges} overlap or leave the buffer of {n} elements")
        if lo > pos:
            out.append((pos, lo))
        pos = hi
    if pos < n:
        out.append((pos, n))
    return out


def _dense(p: torch.Tensor) -> bool:
    """True when the tensor's elements occupy one gap-free block (any dim permutation)."""
    return p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))


class Adam(_FlatOptimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        super().__init__(params, lr)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0) -> None:
        self._sync_grads()
        self.steps += 1
        K.adam_fused(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.lr, self.betas[0], self.betas[1], self.eps,
                     self.weight_decay, self.steps, grad_scale)

    def state_dict(self):
        return {"step": self.steps, "exp_avg": self.flat_m, "exp_avg_sq": self.flat_v, "lr": self.lr}


class AdamW(_FlatOptimizer):
    """`torch.optim.AdamW` (decoupled weight decay) behind `torch.nn.utils.clip_grad_norm_`, on the flat buffers.

    `no_decay`: the parameters that do not decay; default every parameter with `ndim <= 1` (biases, BatchNorm / LayerNorm gamma and
    beta, the logit scale and bias) -- embedding tables and filters decay.  `max_grad_norm`: None = no norm is taken; a positive
    number clips the global gradient norm to it; `inf` takes and reports the norm without clipping.  A step is one launch, or two
    with `max_grad_norm`: `grad_sqnorm` over the flat gradient buffer, then `adamw_clipped`, which derives the coefficient on the
    device -- no host sync.  The gradient buffer itself is left unclipped.  `last_grad_norm` / `last_clip_coef` are device views of
    the last step's norm (before clipping, `grad_scale` included) and coefficient; `current_grad_norm()` reads the norm back."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                 max_grad_norm: Optional[float] = None, no_decay=None):
        weight_decay = float(weight_decay)
        if not (weight_decay >= 0.0 and weight_decay != float("inf")):
            raise ValueError(f"AdamW: weight_decay must be finite and >= 0, got {weight_decay!r}")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"AdamW: max_grad_norm must be None, positive or inf, got {max_grad_norm!r}")
        super().__init__(params, lr)
        self.betas, self.eps, self.weight_decay, self.max_grad_norm = betas, eps, weight_decay, max_grad_norm
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        if no_decay is None:
            skip = {id(p) for p in self.params if p.ndim <= 1}
        else:
            skip = {id(p) for p in no_decay}
            unknown = skip - {id(p) for p in self.params}
            if unknown:
                raise ValueError(f"AdamW: {len(unknown)} of the no_decay parameters are not among the optimised parameters")
        self.no_decay_ids = skip
        self.decay_mask = self._build_decay_mask(skip)
        self._stats = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.flat_p.device)
        self.last_grad_norm, self.last_clip_coef = self._stats[0:1], self._stats[1:2]
        self._partials = None

    def _build_decay_mask(self, skip) -> torch.Tensor:
        """uint8 [numel / 4]: one byte per aligned group of four elements of the flat buffers, 1 = the group decays.  Every tensor is
        padded to a multiple of four, so no group holds two tensors; a tensor's padding follows the tensor."""
        mask = torch.zeros(self.numel // 4, dtype=torch.uint8)
        base = self.flat_g.data_ptr()
        for p, gv in zip(self.params, self._views):
            if id(p) not in skip:
                o = (gv.data_ptr() - base) // 4
                mask[o // 4:(o + (p.numel() + 3) // 4 * 4) // 4] = 1
        return mask.to(self.flat_p.device)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0) -> None:
        self._sync_grads()
        self.steps += 1
        partials = None
        if self.max_grad_norm is not None:
            if self._partials is None:
                self._partials = torch.empty(K.grad_sqnorm_nparts(self.numel), dtype=torch.float32, device=self.flat_p.device)
            partials = K.grad_sqnorm(self.flat_g, out=self._partials)
        K.adamw_clipped(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.lr, self.betas[0], self.betas[1], self.eps,
                        self.weight_decay, self.steps, grad_scale, 0.0 if self.max_grad_norm is None else self.max_grad_norm,
                        decay_mask=self.decay_mask, partials=partials, stats=self._stats)

    def current_grad_norm(self) -> Optional[float]:
        """the last step's gradient norm before clipping as a host float (None without `max_grad_norm`): the one read-back"""
        if self.max_grad_norm is None:
            return None
        return float(self.last_grad_norm.cpu())

    def state_dict(self):
        return {"step": self.steps, "exp_avg": self.flat_m, "exp_avg_sq": self.flat_v, "lr": self.lr}


DECAYS = ("constant", "linear", "cosine")


class LRSchedule:
    """Learning rate of optimiser step `step` (counted from 1), a pure host function: linear warmup from base_lr / warmup_steps to
    base_lr over the first `warmup_steps` steps, then constant, or a linear / cosine decay to `min_lr_ratio * base_lr` at
    `total_steps` (and constant from there on).  The learning rate is a host float argument of the update kernel already, so a
    schedule adds no launch and no sync."""

    def __init__(self, base_lr: float, warmup_steps: int = 0, total_steps: Optional[int] = None, decay: str = "constant",
                 min_lr_ratio: float = 0.0):
        if decay not in DECAYS:
            raise ValueError(f"LRSchedule: decay must be one of {DECAYS}, got {decay!r}")
        for name, val in (("warmup_steps", warmup_steps), ("total_steps", total_steps)):
            if val is not None and (isinstance(val, bool) or not isinstance(val, int) or val < 0):
                raise ValueError(f"LRSchedule: {name} must be an integer >= 0, got {val!r}")
        if decay != "constant" and total_steps is None:
            raise ValueError(f"LRSchedule: decay={decay!r} needs total_steps")
        if total_steps is not None and warmup_steps > total_steps:
            raise ValueError(f"LRSchedule: warmup_steps {warmup_steps} > total_steps {total_steps}")
        if not 0.0 <= float(min_lr_ratio) <= 1.0:
            raise ValueError(f"LRSchedule: min_lr_ratio must be in [0, 1], got {min_lr_ratio!r}")
        self.base_lr, self.warmup_steps, self.total_steps = float(base_lr), warmup_steps, total_steps
        self.decay, self.min_lr_ratio = decay, float(min_lr_ratio)

    def __call__(self, step: int) -> float:
        if step < 1:
            raise ValueError(f"LRSchedule: steps count from 1, got {step!r}")
        if step <= self.warmup_steps:
            return self.base_lr * step / self.warmup_steps
        if self.decay == "constant":
            return self.base_lr
        t = min(1.0, max(0.0, (step - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps)))
        f = 1.0 - t if self.decay == "linear" else 0.5 * (1.0 + math.cos(math.pi * t))
        return self.base_lr * (self.min_lr_ratio + (1.0 - self.min_lr_ratio) * f)


class SGD(_FlatOptimizer):
    def __init__(self, params, lr: float = 1e-3, weight_decay: float = 0.0):
        super().__init__(params, lr)
        self.weight_decay = weight_decay

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0) -> None:
        self._sync_grads()
        self.steps += 1
        K.sgd(self.flat_p, self.flat_g, self.lr, self.weight_decay, grad_scale)


FISHERS = ("empirical", "identity")


class EWC:
    """Elastic weight consolidation over the flat buffers of any `_FlatOptimizer`: after a task, `consolidate()`
    keeps the parameters as the anchor a and an importance F per parameter; from then on `apply()` adds the gradient of
    strength / 2 * sum F (p - a)^2 to the flat gradient buffer, before the optimiser's step (and its clipping norm) reads it.

    `fisher="empirical"`: F is the mean, over the batches between `begin_estimate()` and `consolidate()`, of the squared gradient
    that `accumulate()` finds in `optimizer.flat_g` -- the global-batch MEAN gradient (call it after `all_reduce_grads`), not the
    per-example Fisher.  Such an F is of the size of a squared mean gradient, so useful `strength` values are large (1e3 and far
    above, depending on the loss).  `fisher="identity"`: F = 1 (L2-SP); no F is stored and no estimate is needed.  `gamma` in [0, 1]
    merges tasks: F = gamma * F_old + F_new; the anchor is always the latest parameters.  Memory: +8 B per parameter (F and the
    anchor; +4 B with "identity"), and another +4 B while an estimate runs.  `apply()` is one launch, none before the first
    consolidation; `current_penalty()` is the one read-back and happens only when asked."""

    def __init__(self, optimizer: _FlatOptimizer, strength: float, fisher: str = "empirical", gamma: float = 1.0):
        strength, gamma = float(strength), float(gamma)
        if not (math.isfinite(strength) and strength >= 0.0):
            raise ValueError(f"EWC: strength must be finite and >= 0, got {strength!r}")
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"EWC: gamma must be in [0, 1], got {gamma!r}")
        if fisher not in FISHERS:
            raise ValueError(f"EWC: fisher must be one of {FISHERS}, got {fisher!r}")
        self.optimizer, self.strength, self.fisher, self.gamma = optimizer, strength, fisher, gamma
        self.F: Optional[torch.Tensor] = None
        self.anchor: Optional[torch.Tensor] = None
        self._acc: Optional[torch.Tensor] = None
        self._partials: Optional[torch.Tensor] = None
        self.samples, self.tasks, self.active, self._applied = 0, 0, False, False

    def begin_estimate(self) -> None:
        """allocate and zero the accumulator of an empirical estimate (a running one starts over)"""
        self._acc = torch.zeros_like(self.optimizer.flat_p)
        self.samples = 0

    @torch.no_grad()
    def accumulate(self) -> None:
        """acc += g^2 from `optimizer.flat_g` (after `all_reduce_grads` under data parallelism); counts one sample"""
        if self._acc is None:
            raise ValueError("EWC.accumulate: no estimate is running (call begin_estimate() first)")
        self.optimizer._sync_grads()
        K.fisher_accumulate(self._acc, self.optimizer.flat_g, 1.0)
        self.samples += 1

    @torch.no_grad()
    def consolidate(self) -> None:
        """F = gamma * F + acc / samples, anchor = flat_p, in one launch; frees the accumulator"""
        opt = self.optimizer
        if self.fisher == "empirical":
            if self._acc is None or self.samples == 0:
                raise ValueError("EWC.consolidate: fisher='empirical' needs at least one accumulate() since begin_estimate()")
            if self.F is None:
                self.F = torch.zeros_like(opt.flat_p)
        if self.anchor is None:
            self.anchor = torch.empty_like(opt.flat_p)
        if self.fisher == "empirical":
            K.ewc_consolidate(self.F, self._acc, self.anchor, opt.flat_p, self.gamma, 1.0 / self.samples)
        else:
            K.ewc_consolidate(None, None, self.anchor, opt.flat_p)
        self._acc, self.samples = None, 0
        self.tasks += 1
        self.active = True

    @torch.no_grad()
    def apply(self) -> None:
        """flat_g += strength * F * (flat_p - anchor); the partial sums of the penalty are kept for `current_penalty()`.  Not active
        (nothing consolidated yet): returns without a launch."""
        if not self.active:
            return
        opt = self.optimizer
        opt._sync_grads()
        if self._partials is None:
            self._partials = torch.empty(K.ewc_penalty_nparts(opt.numel), dtype=torch.float32, device=opt.flat_p.device)
        K.ewc_penalty(opt.flat_g, opt.flat_p, self.anchor, self.F, self.strength, out=self._partials)
        self._applied = True

    def current_penalty(self) -> Optional[float]:
        """strength / 2 * sum F (p - a)^2 of the last `apply()` as a host float (float64 sum of the partials; None before the first
        penalised step): the one read-back, only when asked"""
        if not (self.active and self._applied):
            return None
        return 0.5 * self.strength * float(self._partials.detach().cpu().double().sum())

    def state_dict(self) -> dict:
        """tensors and plain numbers only (loadable with weights_only=True)"""
        sd = {"tasks": int(self.tasks), "gamma": float(self.gamma), "fisher": self.fisher, "numel": int(self.optimizer.numel)}
        if self.anchor is not None:
            sd["anchor"] = self.anchor.detach().cpu()
        if self.F is not None:
            sd["F"] = self.F.detach().cpu()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """strict: the keys of `state_dict()`, the same fisher kind, and F / anchor of exactly `optimizer.numel` elements"""
        if not isinstance(sd, dict):
            raise ValueError(f"EWC.load_state_dict: expected a dict, got {type(sd).__name__}")
        want = {"tasks", "gamma", "fisher", "numel"}
        unknown = set(sd) - want - {"anchor", "F"}
        if unknown or not want <= set(sd):
            raise ValueError(f"EWC.load_state_dict: keys {sorted(sd)} (expected {sorted(want)} and, once consolidated, 'anchor' / 'F')")
        if sd["fisher"] != self.fisher:
            raise ValueError(f"EWC.load_state_dict: the state was written with fisher={sd['fisher']!r}, this object has {self.fisher!r}")
        tasks, n = int(sd["tasks"]), self.optimizer.numel
        need = set() if tasks == 0 else ({"anchor", "F"} if self.fisher == "empirical" else {"anchor"})
        if {k for k in ("anchor", "F") if k in sd} != need:
            raise ValueError(f"EWC.load_state_dict: {tasks} task(s) with fisher={self.fisher!r} need exactly the tensors {sorted(need)}")
        for k in need:
            t = sd[k]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n,):
                raise ValueError(f"EWC.load_state_dict: '{k}' must be a float32 tensor of {n} elements (this optimiser's flat buffer), "
                                 f"got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if int(sd["numel"]) != n:
            raise ValueError(f"EWC.load_state_dict: the state belongs to a flat buffer of {int(sd['numel'])} elements, this one has {n}")
        gamma = float(sd["gamma"])
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"EWC.load_state_dict: gamma must be in [0, 1], got {gamma!r}")
        dev = self.optimizer.flat_p.device
        self.anchor = sd["anchor"].to(dev).clone() if "anchor" in need else None
        self.F = sd["F"].to(dev).clone() if "F" in need else None
        self.gamma, self.tasks, self.active = gamma, tasks, tasks > 0
        self._acc, self.samples, self._applied = None, 0, False


class AGEM:
    """A-GEM's gradient projection (Chaudhry et al. 2019) over the flat gradient buffer of any `_FlatOptimizer`.
    `store_reference()` keeps a copy of `optimizer.flat_g` as the reference gradient g_ref (the gradient of a batch drawn from an
    episodic memory; call it after `all_reduce_grads` under data parallelism); `apply()` then replaces the step's gradient g, when it
    conflicts with the reference (g . g_ref < 0), by g - (g . g_ref / g_ref . g_ref) g_ref, before the optimiser's step (and its
    clipping norm) reads it.

    Memory: +4 B per parameter for g_ref, allocated at the first `store_reference()`.  `apply()` is two launches (`agem_dots`, then
    `agem_project`, which decides on the device: no host sync), none before a reference exists.  `current_interference()` is the one
    read-back and happens only when asked."""

    def __init__(self, optimizer: _FlatOptimizer):
        self.optimizer = optimizer
        self.gref: Optional[torch.Tensor] = None
        self._partials: Optional[torch.Tensor] = None
        self._stats = torch.zeros(4, dtype=torch.float32, device=optimizer.flat_p.device)
        self.valid, self.applied = False, 0

    @torch.no_grad()
    def store_reference(self) -> None:
        """g_ref = `optimizer.flat_g` (one device copy); marks the reference valid"""
        opt = self.optimizer
        opt._sync_grads()
        if self.gref is None:
            self.gref = torch.empty_like(opt.flat_g)
        self.gref.copy_(opt.flat_g)
        self.valid = True

    @torch.no_grad()
    def apply(self) -> None:
        """project `optimizer.flat_g` in place; no reference yet: returns without a launch"""
        if not self.valid:
            return
        opt = self.optimizer
        opt._sync_grads()
        if self._partials is None:
            self._partials = torch.empty(2 * K.agem_dots_nparts(opt.numel), dtype=torch.float32, device=opt.flat_p.device)
        K.agem_dots(opt.flat_g, self.gref, out=self._partials)
        K.agem_project(opt.flat_g, self.gref, self._partials, self._stats)
        self.applied += 1

    def current_interference(self) -> Optional[dict]:
        """the last `apply()` as host numbers: "dot" (g . g_ref), "ref_sqnorm", "coef" (0 when not projected), and the running counts
        "projected" / "applied" of calls (None before the first `apply()`): the one read-back, only when asked"""
        if self.applied == 0:
            return None
        s = self._stats.detach().cpu().tolist()
        return {"dot": s[0], "ref_sqnorm": s[1], "coef": s[2], "projected": int(s[3]), "applied": int(self.applied)}

    def state_dict(self) -> dict:
        """tensors and plain numbers only (loadable with weights_only=True).  The reference gradient is not saved: it is recomputed
        from the memory."""
        return {"numel": int(self.optimizer.numel), "applied": int(self.applied), "stats": self._stats.detach().cpu()}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """strict: exactly the keys of `state_dict()`, written for a flat buffer of `optimizer.numel` elements"""
        if not isinstance(sd, dict):
            raise ValueError(f"AGEM.load_state_dict: expected a dict, got {type(sd).__name__}")
        want = {"numel", "applied", "stats"}
        if set(sd) != want:
            raise ValueError(f"AGEM.load_state_dict: keys {sorted(sd)} (expected {sorted(want)})")
        if int(sd["numel"]) != self.optimizer.numel:
            raise ValueError(f"AGEM.load_state_dict: the state belongs to a flat buffer of {int(sd['numel'])} elements, this one has "
                             f"{self.optimizer.numel}")
        st = sd["stats"]
        if not isinstance(st, torch.Tensor) or st.dtype != torch.float32 or tuple(st.shape) != (4,):
            raise ValueError("AGEM.load_state_dict: 'stats' must be a float32 tensor of 4 elements")
        if int(sd["applied"]) < 0:
            raise ValueError(f"AGEM.load_state_dict: 'applied' must be >= 0, got {sd['applied']!r}")
        self._stats.copy_(st)
        self.applied, self.valid = int(sd["applied"]), False


class EMA:
    """Exponential moving average of the parameters over the flat buffer of any `_FlatOptimizer`:
    avg <- avg + (1 - d_t) (flat_p - avg) after every optimiser step, in one launch (`kernels.ema_update`).

    `begin()` allocates `avg` and sets it to `flat_p` (the one allocation, +4 B per parameter; a second call does nothing).
    `update()` counts the update and passes the step's decay d_t -- `decay`, or with `warmup` min(decay, (1 + t) / (10 + t)) at
    update t = 1, 2, ... -- as a host float argument of the launch, as the learning-rate schedule is passed: no launch and no sync
    of its own.  `last_decay` keeps it.  `swap()` exchanges `avg` and `optimizer.flat_p` exactly, in one launch, so that the modules
    (views of `flat_p`) read the averaged parameters until the next `swap()`; `swapped` says which state holds.  A parameter that
    never moved is its own average bit for bit, and so is every parameter at decay 1 (include/cxrk.h, "ema_update")."""

    def __init__(self, optimizer: _FlatOptimizer, decay: float, warmup: bool = True):
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (math.isfinite(decay) and 0.0 <= decay <= 1.0):
            raise ValueError(f"EMA: decay must be a number in [0, 1], got {decay!r}")
        if not isinstance(warmup, bool):
            raise ValueError(f"EMA: warmup must be True or False, got {warmup!r}")
        self.optimizer, self.decay, self.warmup = optimizer, float(decay), warmup
        self.avg: Optional[torch.Tensor] = None
        self.updates, self.last_decay, self.swapped = 0, None, False

    @torch.no_grad()
    def begin(self) -> None:
        """avg = a copy of `optimizer.flat_p`, once"""
        if self.avg is None:
            self.avg = self.optimizer.flat_p.detach().clone()

    def decay_at(self, updates: int) -> float:
        """d_t of update number `updates` (counted from 1), in double on the host"""
        return min(self.decay, (1.0 + updates) / (10.0 + updates)) if self.warmup else self.decay

    @torch.no_grad()
    def update(self) -> None:
        """avg += (1 - d_t) * (flat_p - avg): one launch"""
        if self.avg is None:
            raise ValueError("EMA.update: no average yet (call begin() first)")
        if self.swapped:
            raise ValueError("EMA.update: the buffers are swapped (flat_p holds the average); call swap() first")
        self.updates += 1
        self.last_decay = self.decay_at(self.updates)
        K.ema_update(self.avg, self.optimizer.flat_p, self.last_decay)

    @torch.no_grad()
    def swap(self) -> None:
        """avg <-> flat_p: one launch"""
        if self.avg is None:
            raise ValueError("EMA.swap: no average yet (call begin() first)")
        K.flat_swap(self.avg, self.optimizer.flat_p)
        self.swapped = not self.swapped

    def state_dict(self) -> dict:
        """tensors and plain numbers only (loadable with weights_only=True); refused while swapped: `avg` would hold the raw weights"""
        if self.swapped:
            raise ValueError("EMA.state_dict: the buffers are swapped (avg holds the raw parameters); call swap() first")
        sd = {"numel": int(self.optimizer.numel), "decay": float(self.decay), "warmup": bool(self.warmup), "updates": int(self.updates)}
        if self.avg is not None:
            sd["avg"] = self.avg.detach().cpu()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """strict: the keys of `state_dict()`, the same decay and warmup, and an `avg` of exactly `optimizer.numel` float32 elements;
        a refused state changes nothing.  `avg` is filled in place when it exists (a momentum teacher's parameters are views of it)."""
        if not isinstance(sd, dict):
            raise ValueError(f"EMA.load_state_dict: expected a dict, got {type(sd).__name__}")
        want = {"numel", "decay", "warmup", "updates"}
        if not want <= set(sd) or set(sd) - want - {"avg"}:
            raise ValueError(f"EMA.load_state_dict: keys {sorted(sd)} (expected {sorted(want)} and, once begun, 'avg')")
        if self.swapped:
            raise ValueError("EMA.load_state_dict: the buffers are swapped; call swap() first")
        n = self.optimizer.numel
        if isinstance(sd["numel"], bool) or not isinstance(sd["numel"], int) or sd["numel"] != n:
            raise ValueError(f"EMA.load_state_dict: the state belongs to a flat buffer of {sd['numel']!r} elements, this one has {n}")
        if isinstance(sd["decay"], bool) or not isinstance(sd["decay"], (int, float)) or float(sd["decay"]) != self.decay:
            raise ValueError(f"EMA.load_state_dict: the state was written with decay={sd['decay']!r}, this object has {self.decay!r}")
        if sd["warmup"] is not self.warmup:
            raise ValueError(f"EMA.load_state_dict: the state was written with warmup={sd['warmup']!r}, this object has {self.warmup!r}")
        updates = sd["updates"]
        if isinstance(updates, bool) or not isinstance(updates, int) or updates < 0:
            raise ValueError(f"EMA.load_state_dict: 'updates' must be an integer >= 0, got {updates!r}")
        avg = sd.get("avg")
        if avg is None:
            if updates > 0:
                raise ValueError(f"EMA.load_state_dict: {updates} update(s) need the tensor 'avg'")
        elif not isinstance(avg, torch.Tensor) or avg.dtype != torch.float32 or tuple(avg.shape) != (n,):
            raise ValueError(f"EMA.load_state_dict: 'avg' must be a float32 tensor of {n} elements (this optimiser's flat buffer), got "
                             f"{(avg.dtype, tuple(avg.shape)) if isinstance(avg, torch.Tensor) else type(avg).__name__}")
        if avg is not None:
            if self.avg is None:
                self.avg = torch.empty_like(self.optimizer.flat_p)
            self.avg.copy_(avg)
        self.updates = updates
        self.last_decay = self.decay_at(updates) if updates > 0 else None
