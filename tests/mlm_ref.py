"""TEST-ONLY numpy / float64 restatement of the masked-language-modelling loss (include/cxrk.h, "mlm"): the token draw
(HF DataCollatorForLanguageModeling's rule on the project's counter-based Philox), the capacity of the compact list, and the head's loss
by torch autograd in float64."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from dropout_ref import philox4x32_10

T80 = 3435973837          # ceil(0.8 * 2^32)
T90 = 3865470567          # ceil(0.9 * 2^32)
DOMAIN = 0xF4             # low byte of counter word 3: layer 61, site 0 (no dropout word, not the augmentation's 0xF0)
KEEP, MASK, RANDOM, SAME = 0, 1, 2, 3     # what the draw did to a token: not selected / [MASK] / random id / selected, id kept


def select_threshold(p: float) -> int:
    return int(math.floor(float(p) * 2.0 ** 32 + 0.5))


def capacity(T: int, p: float) -> int:
    need = math.ceil(p * T + 8.0 * math.sqrt(p * (1.0 - p) * T))
    return max(1, min(T, (need + 127) // 128 * 128))


def draw_words(seed: int, counter: int, n, t):
    """the four Philox words of token t of global sequence n: key = (seed lo, seed hi), counter = (0, n, t, (counter & 0xffffff) << 8 | 0xF4)"""
    c3 = ((counter & 0xFFFFFF) << 8) | DOMAIN
    return philox4x32_10(np.uint32(0), np.asarray(n, dtype=np.uint32), np.asarray(t, dtype=np.uint32), np.uint32(c3),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def mask_tokens(ids, mask, seed, counter, p, vocab, mask_id, special=(), row_offset=0, cap=None):
    """ids / mask: integer arrays [N, L] (mask may be None) -> dict(ids_out [N, L], sel, tgt (the first `cap` selections in token order,
    -1 behind them), kept, selected, kind [N, L])"""
    ids = np.asarray(ids, dtype=np.int64)
    N, L = ids.shape
    att = np.ones_like(ids, dtype=bool) if mask is None else np.asarray(mask) != 0
    cand = att & ~np.isin(ids, np.asarray(list(special), dtype=np.int64))
    n = (row_offset + np.arange(N, dtype=np.int64))[:, None] * np.ones((1, L), dtype=np.int64)
    t = np.ones((N, 1), dtype=np.int64) * np.arange(L, dtype=np.int64)[None]
    w0, w1, w2, _ = draw_words(seed, counter, n & 0xFFFFFFFF, t)
    selected = cand & (w0.astype(np.uint64) < np.uint64(select_threshold(p)))
    rand_id = ((w2.astype(np.uint64) * np.uint64(vocab)) >> np.uint64(32)).astype(np.int64)
    kind = np.where(~selected, KEEP, np.where(w1 < T80, MASK, np.where(w1 < T90, RANDOM, SAME)))
    out = np.where(kind == MASK, mask_id, np.where(kind == RANDOM, rand_id, ids))
    where = np.flatnonzero(selected.reshape(-1))
    T = N * L
    cap = capacity(T, p) if cap is None else cap
    kept = min(len(where), cap)
    sel = np.full(cap, -1, dtype=np.int32)
    tgt = np.full(cap, -1, dtype=np.int32)
    sel[:kept] = where[:kept]
    tgt[:kept] = ids.reshape(-1)[where[:kept]]
    return dict(ids_out=out, sel=sel, tgt=tgt, kept=kept, selected=len(where), kind=kind)


def linear_wide(x, w, b):
    """F.linear whose three matrix products (forward, data and weight gradient) accumulate in float64 and round once to the operands'
    dtype.  A float32 product of the CPU BLAS sums in an order that follows the processor model; this one gives every host the same
    float32 figures (float64 operands: F.linear itself)."""
    return F.linear(x.double(), w.double(), b.double()).to(x.dtype)


def head_logits(x, wd, bd, gamma, beta, wdec, bdec, eps=1e-12, linear=F.linear):
    """HF BertOnlyMLMHead on rows x [R, H] (any float dtype)"""
    h = F.gelu(linear(x, wd, bd))
    h = F.layer_norm(h, (h.shape[-1],), gamma, beta, eps)
    return linear(h, wdec, bdec)


def correct_range(logits, targets, tol):
    """(lo, hi) of the count of rows whose arg-max is the target when every logit is known to tol * max |logits| only: a row whose
    two largest logits are closer than twice that may go either way when the target is one of the two"""
    logits = logits.detach().double()
    top = logits.topk(2, dim=1)
    sure = (top.values[:, 0] - top.values[:, 1]) > 2.0 * tol * float(logits.abs().max())
    hit = top.indices[:, 0] == targets
    near = ~sure & ((top.indices[:, 0] == targets) | (top.indices[:, 1] == targets))
    return int((hit & sure).sum()), int((hit & sure).sum() + near.sum())


def head_loss(last, sel, tgt, kept, params, scale, weight=1.0, eps=1e-12, tol=0.0, dtype=torch.float64):
    """float64 autograd reference of `functional.mlm_loss`: last [T, H] and the six head parameters (cpu tensors) ->
    dict(loss (unweighted), correct = `correct_range` at `tol`, dlast, dparams) of weight * scale * sum CE over the first `kept` slots.
    `dtype`: the same formula in another precision (the differential sweep measures its float32 error, tests/sweep_cases.py), with
    the matrix products of `linear_wide`: that figure must not depend on the host's BLAS"""
    last = last.detach().to(dtype).clone().requires_grad_(True)
    ps = [p.detach().to(dtype).clone().requires_grad_(True) for p in params]
    rows = torch.as_tensor(np.asarray(sel[:kept]), dtype=torch.int64)
    t = torch.as_tensor(np.asarray(tgt[:kept]), dtype=torch.int64)
    if kept == 0:
        return dict(loss=0.0, correct=(0, 0), dlast=torch.zeros_like(last), dparams=[torch.zeros_like(p) for p in ps])
    logits = head_logits(last[rows], *ps, eps=eps, linear=F.linear if dtype == torch.float64 else linear_wide)
    loss = F.cross_entropy(logits, t, reduction="sum") * float(scale)
    (loss * weight).backward()
    return dict(loss=float(loss.detach()), correct=correct_range(logits, t, tol), dlast=last.grad,
                dparams=[p.grad if p.grad is not None else torch.zeros_like(p) for p in ps])
