"""Test-only restatement of the text encoder's dropout (include/cxrk.h, "dropout"): Philox4x32-10 and the keep rule in numpy, and
the CXR-BERT forward with explicit dropout factors in plain torch (CPU fp32), on top of oracle.ref_text."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_text

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over broadcastable uint32 counter words; returns the four output words."""
    c = [np.asarray(x).astype(np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _U32]
        k0, k1 = (k0 + np.uint64(_W0)) & _U32, (k1 + np.uint64(_W1)) & _U32
    return [x.astype(np.uint32) for x in c]


def threshold(p: float) -> int:
    return int(math.floor(float(np.float32(p)) * 2.0 ** 32 + 0.5))


def scale(p: float) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed: int, counter: int, layer: int, site: int, row_offset: int, p: float, N: int, L: int, C: int, nH: int = 1):
    """bool keep[N][nH][L][C] of one site: n = row_offset + sequence, t = token (query), h = head, c = column (key)."""
    n = (np.arange(N, dtype=np.uint64) + np.uint64(row_offset))[:, None, None, None]
    h = np.arange(nH, dtype=np.uint64)[None, :, None, None]
    t = np.arange(L, dtype=np.uint64)[None, None, :, None]
    c = np.arange(C, dtype=np.uint64)[None, None, None, :]
    shape = (N, nH, L, C)
    c3 = np.uint64(((counter & 0xFFFFFF) << 8) | (layer << 2) | site)
    out = philox4x32_10(np.broadcast_to(c >> np.uint64(2), shape), np.broadcast_to(n, shape),
                        np.broadcast_to(t | (h << np.uint64(16)), shape), np.broadcast_to(c3, shape),
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    draw = np.choose(np.broadcast_to(c & np.uint64(3), shape).astype(np.int64), out)
    return draw >= np.uint32(threshold(p)) if threshold(p) < 2 ** 32 else np.zeros(shape, bool)


def factors(keep: np.ndarray, p: float) -> torch.Tensor:
    """keep * 1/(1-p) as an fp32 tensor"""
    return torch.from_numpy(keep.astype(np.float32) * scale(p))


def model_factors(seed: int, counter: int, row_offset: int, ph: float, pa: float, N: int, L: int, H: int, nH: int, n_layers: int):
    """{(layer, site): factors} of one encoder call: site 0 (layer 0) [N, L, H], site 1 [N, nH, L, L], sites 2, 3 [N, L, H]"""
    f = {(0, 0): factors(keep_mask(seed, counter, 0, 0, row_offset, ph, N, L, H), ph).view(N, L, H)}
    for i in range(n_layers):
        f[(i, 1)] = factors(keep_mask(seed, counter, i, 1, row_offset, pa, N, L, L, nH), pa)
        for s in (2, 3):
            f[(i, s)] = factors(keep_mask(seed, counter, i, s, row_offset, ph, N, L, H), ph).view(N, L, H)
    return f


def ones_factors(N: int, L: int, H: int, nH: int, n_layers: int):
    f = {(0, 0): torch.ones(N, L, H)}
    for i in range(n_layers):
        f[(i, 1)] = torch.ones(N, nH, L, L)
        f[(i, 2)] = torch.ones(N, L, H)
        f[(i, 3)] = torch.ones(N, L, H)
    return f


def projected_with_masks(p, ids: torch.Tensor, mask: torch.Tensor, n_layers: int, n_heads: int, fac, eps: float = 1e-12):
    """HF BertModel in train mode with the dropout factors `fac` (model_factors) -> projected CLS embedding [N, P]."""
    x = ref_text.bert_embeddings(p, ids, eps) * fac[(0, 0)]
    add_mask = (1.0 - mask[:, None, None, :].to(x.dtype)) * torch.finfo(x.dtype).min
    N, L, H = x.shape
    d = H // n_heads
    for i in range(n_layers):
        pre = f"bert.encoder.layer.{i}."
        q, k, v = (F.linear(x, p[pre + f"attention.self.{nm}.weight"], p[pre + f"attention.self.{nm}.bias"])
                   .view(N, L, n_heads, d).transpose(1, 2) for nm in ("query", "key", "value"))
        pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + add_mask, dim=-1) * fac[(i, 1)]
        ctx = (pr @ v).transpose(1, 2).reshape(N, L, H)
        a = F.linear(ctx, p[pre + "attention.output.dense.weight"], p[pre + "attention.output.dense.bias"]) * fac[(i, 2)]
        x = F.layer_norm(a + x, (H,), p[pre + "attention.output.LayerNorm.weight"], p[pre + "attention.output.LayerNorm.bias"], eps)
        u = F.gelu(F.linear(x, p[pre + "intermediate.dense.weight"], p[pre + "intermediate.dense.bias"]))
        o = F.linear(u, p[pre + "output.dense.weight"], p[pre + "output.dense.bias"]) * fac[(i, 3)]
        x = F.layer_norm(o + x, (H,), p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)
    return ref_text.projection_head(p, x[:, 0])
