"""The north-star step: joint image + text embedding and symmetric InfoNCE, data-parallel over the GPUs of a node.

    images [B,3,224,224] --ImageModel--> I [B,128] \
                                                     > L2-normalise, all-gather, S = I_hat T_hat^T / tau, InfoNCE
    token ids [B,32]     --CXRBertModel-> T [B,128] /
    loss.backward() -> encoder backward (hand-written HIP) -> flat-gradient all-reduce (RCCL) -> fused Adam

One process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI).  Weights are replicated; the global
batch is sharded by rows.  Communication per step: all-gather of [B,256] normalised embeddings, all-gather of [B,2]
log-sum-exps, a scalar all-reduce for the reported loss, and the bucketed all-reduce of the ~133 M-parameter flat
gradient buffer.  This step is NOT in the reference: temperature is an explicit
argument (default 0.07, the usual CLIP-style value; the reference specifies none).

`positives="labels" | "text"`: label-aware multi-positive targets.  Every pair gets a 64-bit key (`keys_from_labels`,
`keys_from_tokens`); pairs of the global batch with equal keys are positives of each other.  One more all-gather per step, of the
[B] int64 keys.  `positives=None` (the default) is the plain loss and issues exactly the calls it always did.

`learn_temperature=True`: the temperature is a parameter.  The trainer owns `logit_scale` = theta = log(1/tau), as
CLIP parametrises it, initialised from `temperature`; it sits in the flat buffers behind the text encoder, takes the same optimiser
step, and is clamped to `log_scale_bounds` after it.  The loss kernels read theta on the device; its gradient travels in the flat
gradient all-reduce (at the end of the "text" span): no new collective, no host sync.  `learn_temperature=False` (the default) creates no parameter and issues
exactly the calls it always did.

`loss="sigmoid"`: the pairwise sigmoid loss in place of InfoNCE: every (image, report) pair of the global batch is a
binary problem on x = exp(theta) * cos + b.  With `learn_temperature` theta AND the bias b (`logit_bias`, initialised from
`sigmoid_bias`) are parameters, appended behind the text parameters in that order; otherwise both are device constants made at
construction.  Nothing is normalised over the batch, so the step has no log-sum-exp all-gather.  `loss="infonce"` (the default)
issues exactly the calls it always did.

`augment=AugmentSpec(...)`: on-device image augmentation.  The trainer owns (seed, step counter) as `augment_state`
and hands the image model one call descriptor per `step` (spec, seed, counter, this rank's first global row): the encoder's
NCHW -> NHWC boundary transform then samples each image through its own random affine map and jitters brightness / contrast.  The
draws are keyed by the global image index, so a sharded step augments exactly as the single-process step on the global batch does.
`augment=None` (the default) issues exactly the calls it always did.

`micro_batch=n`: the step runs the encoders on at most n of this rank's rows at a time (the gradient-cache scheme):
every chunk but the last is embedded without keeping activations, the loss runs once on all embeddings, and each chunk is then
run again with its graph to take its slice of dL/d(embedding) through the encoders into the flat gradient buffer.  The loss, its
collectives and the update are those of the unchunked step up to fp32 summation order; the peak memory is that of one chunk.
`micro_batch=None` (the default) or n >= this rank's rows issues exactly the calls it always did.

`distill_weight=beta`: similarity distillation from a frozen teacher (Learning without Forgetting in the
similarity-distribution form of ZSCL / Mod-X).  `snapshot_teacher()` freezes the current encoders (`FrozenTeacher`: one flat copy of the
parameters, +4 B per parameter); from then on every step also runs the teacher's two encoders save-free on the same rows and adds
beta * L_d (`functional.distill_loss`) to the objective: two more collectives than the plain step's (the [B, 4D] embedding gather and
the [B, 4] log-sum-exp gather) and one scalar all-reduce.  Before the first snapshot, and with `distill_weight=None` (the default),
a step issues exactly the calls it always did.

`mlm_weight=w`: the masked-language-modelling auxiliary loss CXR-BERT was trained with.  Every step masks its token
ids on the device (`kernels.mlm_mask_tokens`: HF DataCollatorForLanguageModeling's rule, keyed by the global sequence index, so a
sharded step masks as the single-process step does), runs the text encoder once on the masked ids through the full-sequence path, feeds
the projected CLS embedding to the contrastive head and the last hidden state to `functional.mlm_loss`, and adds w * L_mlm to the
objective as a second root of the step's one backward: one more collective than the plain step's, the scalar all-reduce of the number
of selected tokens.  With `mlm_weight=None` (the default) a step issues exactly the calls it always did.

`ema_decay=d`: an exponential moving average of every trained parameter (`optim.EMA`, +4 B per parameter).  It starts
as a copy of the parameters at the entry of the first `step` and takes one launch after each optimiser step (with `ema_warmup`, the
default, at the decay min(d, (1 + t) / (10 + t))); the training itself is not touched.  `averaged()` is a context manager inside which
the encoders read the averaged parameters (the two flat buffers are swapped, and swapped back on exit); `ema_eval=True` asks `Trainer`
to evaluate inside it.  `ema_teacher=True` (with `distill_weight`) makes the teacher a momentum teacher: its parameters ARE the average,
as of the end of the previous step.  BatchNorm running statistics are module buffers, not parameters, and are not averaged; the joint
trainers run BatchNorm in eval mode.  No collective: the replicas' averages are bit-identical because their parameters are.  With
`ema_decay=None` (the default) a step issues exactly the calls it always did.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional, Tuple

import torch

from . import functional as Fh
from . import kernels as K
from . import optim as cxr_optim
from .augment import AugmentCall, AugmentSpec, spec_from as _augment_spec_from


# ----------------------------------------------------------------------------------------------------------------
# keys of the multi-positive loss
# ----------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
KEY_GOLDEN = 0x9E3779B97F4A7C15     # position multiplier
KEY_MIX1 = 0xBF58476D1CE4E5B9       # the two multipliers of the splitmix64 finaliser
KEY_MIX2 = 0x94D049BB133111EB


def _i64(c: int) -> int:
    """the int64 (two's complement) reading of a 64-bit constant"""
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    """logical right shift of the 64-bit pattern held in an int64 tensor (torch's >> is arithmetic)"""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix64(z: torch.Tensor) -> torch.Tensor:
    z = (z ^ _lsr(z, 30)) * _i64(KEY_MIX1)
    z = (z ^ _lsr(z, 27)) * _i64(KEY_MIX2)
    return z ^ _lsr(z, 31)


def row_keys(int_rows: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int [B, L] (+ optional mask [B, L], non-zero = in) -> int64 [B]: a deterministic 64-bit hash of each row's masked-in
    integer sequence.  Integer tensor ops only, on the device of the input; the same bits on every rank, on CPU and on GPU.

    Exactly, in uint64 arithmetic (everything mod 2^64; the int64 result is the two's-complement reading of the same 64 bits):

        mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
        p_t    = number of masked-in positions among 0..t of the row (1 for the first masked-in element; all in without a mask)
        key    = mix( sum over the masked-in positions t of  mix( mix(x_t) + p_t * 0x9E3779B97F4A7C15 ) )

    with x_t the element as a 64-bit two's-complement pattern and >> the logical shift (mix is the splitmix64 finaliser, a
    bijection).  A masked-out position contributes nothing and does not advance p, so padding of any length and content leaves the
    key unchanged; an empty row has key 0.  Two rows with the same masked-in sequence always share a key; two different sequences
    share one with probability about 2^-64, so a global batch of Bg rows holds a false positive pair with probability about
    Bg^2 / 2^64 (4e-12 at Bg = 8192)."""
    if int_rows.dim() != 2:
        raise ValueError(f"row_keys: expected a [B, L] integer tensor, got shape {tuple(int_rows.shape)}")
    if int_rows.dtype.is_floating_point or int_rows.dtype.is_complex:
        raise ValueError(f"row_keys: expected an integer tensor, got {int_rows.dtype}")
    x = int_rows.to(torch.int64)
    if mask is None:
        pos = torch.arange(1, x.shape[1] + 1, dtype=torch.int64, device=x.device).expand_as(x)
        inn = None
    else:
        if tuple(mask.shape) != tuple(x.shape):
            raise ValueError(f"row_keys: mask {tuple(mask.shape)} does not match the rows {tuple(x.shape)}")
        inn = (mask != 0).to(device=x.device, dtype=torch.int64)
        pos = torch.cumsum(inn, dim=1)
    term = _mix64(_mix64(x) + pos * _i64(KEY_GOLDEN))
    if inn is not None:
        term = term * inn
    return _mix64(term.sum(dim=1))


def keys_from_labels(labels: torch.Tensor) -> torch.Tensor:
    """[B, C] label matrix -> int64 [B] keys: two rows share a key iff their label vectors are equal (up to the collision odds of
    `row_keys`).  The values must be integral (0.0 / 1.0 floats, bools and integers are fine); anything else raises ValueError."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2:
        raise ValueError(f"keys_from_labels: expected a [B, C] tensor, got {getattr(labels, 'shape', type(labels).__name__)}")
    if labels.dtype.is_complex:
        raise ValueError("keys_from_labels: complex labels")
    if labels.dtype.is_floating_point:
        if not bool((torch.isfinite(labels) & (labels == labels.round())).all()):
            raise ValueError("keys_from_labels: label values must be integral (0.0 / 1.0 floats are fine); soft labels have no "
                             "equality classes")
    return row_keys(labels.to(torch.int64))


def keys_from_tokens(input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
    """token ids [B, L] + attention mask [B, L] -> int64 [B] keys: two rows share a key iff their unpadded token sequences are
    equal (up to the collision odds of `row_keys`); the padding's length and content do not matter."""
    return row_keys(input_ids, attention_mask)


# ----------------------------------------------------------------------------------------------------------------
# kNN label probe
# ----------------------------------------------------------------------------------------------------------------
KNN_K, KNN_TEMPERATURE = 20, 0.07


def check_knn_options(k, temperature) -> Tuple[int, float]:
    """(k, temperature) of the kNN probe, validated: an int in [1, kernels.TOPK_MAX] and a finite float > 0"""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K.TOPK_MAX:
        raise ValueError(f"knn: k must be an int in [1, {K.TOPK_MAX}], got {k!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (0.0 < float(temperature) < math.inf):
        raise ValueError(f"knn: temperature must be a finite number > 0, got {temperature!r}")
    return k, float(temperature)


class KNNBank:
    """The memory of the kNN probe: [n, D] L2-normalised image embeddings and their [n, C] labels, on the device.

    `add(emb, labels)` appends this rank's rows; `finish(group)` closes the bank -- under data parallelism one all-gather of the
    rows and one of the labels (rank-major) after one MAX all-reduce over (count, -count) has checked that every rank holds the same
    number of rows, as `JointContrastiveTrainer.remember` checks its memory; `predict(emb, k, temperature)` -> [B, C], the
    weighted vote (`kernels.knn_vote`) of the k nearest bank rows of each embedding (`functional.topk_neighbours`): no [B, n]
    score block, bit-reproducible, the same on every rank for the same queries."""

    def __init__(self):
        self._emb, self._lab = [], []
        self.emb: Optional[torch.Tensor] = None
        self.labels: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self.emb.shape[0] if self.emb is not None else sum(e.shape[0] for e in self._emb)

    @property
    def width(self) -> Optional[int]:
        """the label width C (None while the bank is empty)"""
        if self.labels is not None:
            return self.labels.shape[1]
        return self._lab[0].shape[1] if self._lab else None

    @torch.no_grad()
    def add(self, emb: torch.Tensor, labels: torch.Tensor) -> None:
        if self.emb is not None:
            raise ValueError("KNNBank.add: the bank is finished")
        if emb.dim() != 2 or labels.dim() != 2 or labels.shape[0] != emb.shape[0] or emb.shape[0] == 0:
            raise ValueError(f"KNNBank.add: expected embeddings [B, D] and labels [B, C], got {tuple(emb.shape)} and {tuple(labels.shape)}")
        if self._emb and (emb.shape[1] != self._emb[0].shape[1] or labels.shape[1] != self._lab[0].shape[1]):
            raise ValueError(f"KNNBank.add: rows of width {emb.shape[1]} / labels of width {labels.shape[1]} after rows of width "
                             f"{self._emb[0].shape[1]} / labels of width {self._lab[0].shape[1]}")
        self._emb.append(Fh.K.l2norm_fwd(emb.detach().float().contiguous())[0])
        self._lab.append(labels.detach().to(device=emb.device, dtype=torch.float32).contiguous())

    @torch.no_grad()
    def finish(self, group=None) -> "KNNBank":
        if self.emb is not None:
            raise ValueError("KNNBank.finish: the bank is finished")
        if not self._emb:
            raise ValueError("KNNBank.finish: the bank is empty")
        emb, lab = torch.cat(self._emb).contiguous(), torch.cat(self._lab).contiguous()
        if group is not None:
            import torch.distributed as dist
            n = emb.shape[0]
            t = torch.tensor([n, -n], dtype=torch.int64, device=_host_collective_device(group))
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            hi, lo = int(t[0]), -int(t[1])
            if hi != lo:
                raise RuntimeError(f"KNNBank.finish: the ranks hold between {lo} and {hi} bank rows (this one {n}); every rank must "
                                   f"add the same number of rows")
            emb, lab = Fh._all_gather_rows(emb, group), Fh._all_gather_rows(lab, group)
        self.emb, self.labels = emb, lab
        self._emb, self._lab = [], []
        return self

    @torch.no_grad()
    def predict(self, emb: torch.Tensor, k: int = KNN_K, temperature: float = KNN_TEMPERATURE) -> torch.Tensor:
        if self.emb is None:
            raise ValueError("KNNBank.predict: call finish() first")
        k, temperature = check_knn_options(k, temperature)
        if emb.dim() != 2 or emb.shape[1] != self.emb.shape[1]:
            raise ValueError(f"KNNBank.predict: expected embeddings [B, {self.emb.shape[1]}], got {tuple(emb.shape)}")
        q = Fh.K.l2norm_fwd(emb.detach().float().contiguous())[0]
        score, index = Fh.topk_neighbours(q, self.emb, k, normalize=False)
        return Fh.K.knn_vote(score, index, self.labels, temperature)


# ----------------------------------------------------------------------------------------------------------------
# retrieval evaluation
# ----------------------------------------------------------------------------------------------------------------
RETRIEVAL_KS = (1, 5, 10)


def check_ks(ks) -> Tuple[int, ...]:
    """the cut-offs of Recall@K: a non-empty sequence of distinct integers >= 1 (bools and floats are refused), returned as a tuple"""
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"ks must be a sequence of positive integers, got {ks!r}") from None
    if not ks or any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in ks) or len(set(ks)) != len(ks):
        raise ValueError(f"ks must be a non-empty sequence of distinct integers >= 1, got {ks!r}")
    return ks


def rank_metrics(greater, ties, ks=RETRIEVAL_KS) -> dict:
    """Recall@K, median and mean rank of one retrieval direction from the two integer vectors of `kernels.retrieval_ranks`
    (host arithmetic; any integer tensors / arrays of one length n >= 1).  Query i has `greater[i]` gallery rows that beat its best
    positive and `ties[i]` that equal it exactly.  The rule for ties:

        R@k and median_rank use the PESSIMISTIC rank  1 + greater + ties   (every tied row is counted as ahead),
        mean_rank uses the expected rank under a random order of the tied rows,  1 + greater + ties / 2.

    With the pessimistic rule a collapsed model (all embeddings equal: every score ties) gets rank M and R@k = 0 for k < M; the
    optimistic rule would report 100 %.  R@k is a fraction in [0, 1].  If any row carries the -1 flag (it met a NaN score), every
    metric of the direction is nan: a diverged model must not report a plausible number.  Returns {"R@k"..., "median_rank",
    "mean_rank", "n"}."""
    import numpy as np
    ks = check_ks(ks)
    g = np.asarray(greater.cpu() if isinstance(greater, torch.Tensor) else greater).astype(np.int64).reshape(-1)
    t = np.asarray(ties.cpu() if isinstance(ties, torch.Tensor) else ties).astype(np.int64).reshape(-1)
    if g.shape != t.shape or g.size == 0:
        raise ValueError(f"rank_metrics: greater and ties must be two vectors of one length >= 1, got {g.shape} and {t.shape}")
    out = {}
    if bool((g < 0).any() or (t < 0).any()):
        for k in ks:
            out[f"R@{k}"] = float("nan")
        out["median_rank"] = out["mean_rank"] = float("nan")
    else:
        worst = 1 + g + t
        for k in ks:
            out[f"R@{k}"] = float((worst <= k).mean())
        out["median_rank"] = float(np.median(worst))
        out["mean_rank"] = float((1.0 + g + 0.5 * t).mean())
    out["n"] = int(g.size)
    return out


@torch.no_grad()
def retrieval_metrics(img_emb: torch.Tensor, txt_emb: torch.Tensor, keys: Optional[torch.Tensor] = None, ks=RETRIEVAL_KS, group=None,
                      normalize: bool = True) -> dict:
    """Image->text and text->image retrieval over the whole evaluation set: {"i2t": {...}, "t2i": {...}}, each the dict of
    `rank_metrics` (R@k for k in `ks`, median_rank, mean_rank, n; the tie rule is written there).  "i2t" uses the images as queries
    and the reports as the gallery, "t2i" the reverse.  `img_emb` / `txt_emb` [N,D] are this rank's paired rows, on the GPU; scores
    are cosines (`normalize=False`: plain dot products of the rows as given).  Without `keys` the positive of a query is its own
    pair; with `keys` (int64 [N]) every pair of the set with the same key is (`keys_from_labels` / `keys_from_tokens`), and the
    rank is that of the best one.  Every query is scored against the WHOLE gallery by `functional.retrieval_ranks`, which never
    forms the [N, M] block.

    Under a process `group` each rank passes its shard (equal sizes): the gallery rows and keys are all-gathered, each rank ranks
    its own queries, and the [N, 2] integer results are all-gathered (one gather per direction), so every rank returns the same
    dict, computed over all ranks' queries."""
    ks = check_ks(ks)
    out = {}
    for name, q, g in (("i2t", img_emb, txt_emb), ("t2i", txt_emb, img_emb)):
        _, greater, ties = Fh.retrieval_ranks(q, g, keys=keys, group=group, normalize=normalize)
        gt = torch.stack((greater, ties), dim=1).contiguous()
        if group is not None:
            gt = Fh._all_gather_rows(gt, group)
        gt = gt.cpu()
        out[name] = rank_metrics(gt[:, 0], gt[:, 1], ks)
    return out


POSITIVES = (None, "labels", "text")
LOSSES = ("infonce", "sigmoid")
OPTIMS = ("adam", "sgd", "adamw")
SIGMOID_BIAS = -10.0                          # SigLIP's initial bias: the Bg^2 - Bg negatives start out nearly free
LOG_SCALE_BOUNDS = (0.0, math.log(100.0))     # CLIP / open_clip: tau in [0.01, 1]


def check_micro_batch(micro_batch) -> Optional[int]:
    """None, or an integer >= 1 (bools, floats and values <= 0 are refused)"""
    if micro_batch is None:
        return None
    if isinstance(micro_batch, bool) or not isinstance(micro_batch, int) or micro_batch < 1:
        raise ValueError(f"micro_batch must be None or an integer >= 1, got {micro_batch!r}")
    return micro_batch


def micro_slices(n: int, micro_batch: int) -> Tuple[Tuple[int, int], ...]:
    """The (lo, hi) row ranges of the encoder calls of a step on n rows with at most `micro_batch` rows per call: contiguous, in
    order, the last one ragged.  (8, 3) -> ((0, 3), (3, 6), (6, 8)); any micro_batch >= n -> ((0, n),)."""
    m = check_micro_batch(micro_batch)
    if m is None:
        raise ValueError("micro_slices: micro_batch must be an integer >= 1, got None")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"micro_slices: the number of rows must be an integer >= 1, got {n!r}")
    return tuple((lo, min(lo + m, n)) for lo in range(0, n, m))


def check_distill_options(distill_weight, distill_temperature) -> Tuple[Optional[float], Optional[float]]:
    """(beta, tau_d) of `JointContrastiveTrainer(distill_weight=, distill_temperature=)` as floats or None: beta finite and >= 0
    (bools refused), tau_d positive and finite and only together with beta"""
    if distill_weight is None:
        if distill_temperature is not None:
            raise ValueError("distill_temperature is an option of similarity distillation; it was given without distill_weight")
        return None, None
    if isinstance(distill_weight, bool) or not isinstance(distill_weight, (int, float)) or not (math.isfinite(distill_weight) and distill_weight >= 0):
        raise ValueError(f"distill_weight must be finite and >= 0, got {distill_weight!r}")
    if distill_temperature is not None:
        if (isinstance(distill_temperature, bool) or not isinstance(distill_temperature, (int, float))
                or not (math.isfinite(distill_temperature) and distill_temperature > 0)):
            raise ValueError(f"distill_temperature must be positive and finite, got {distill_temperature!r}")
        distill_temperature = float(distill_temperature)
    return float(distill_weight), distill_temperature


class FrozenTeacher:
    """The frozen teacher of similarity distillation: structural copies of the two encoders whose optimised
    parameters are views of ONE flat copy of `optimizer.flat_p` (+4 B per parameter), laid out exactly as the student's are in its
    flat buffer (so fused q/k/v stay adjacent and filters keep their memory format); module buffers (BatchNorm running statistics)
    and parameters outside the optimiser are cloned.  Both copies are in eval mode for good, require no gradient, belong to no
    optimiser and no reduce span, and never take a hook, dropout or a gradient.  `refresh()` overwrites the flat copy and the cloned
    tensors IN PLACE: every tensor the copies hold keeps its identity, and the encoders derive nothing from their parameters that
    outlives a forward (q/k/v are fused by adjacency, BatchNorm is folded and planes are split per call), so nothing is stale."""

    def __init__(self, image_model: torch.nn.Module, text_model: torch.nn.Module, optimizer, flat: Optional[torch.Tensor] = None):
        """`flat`: a buffer laid out like `optimizer.flat_p` to use as the flat copy in place of a clone (the momentum teacher of
        DESIGN.md §5.14 hands in the parameter average: the teacher's parameters are then views of it, no second copy exists, and
        `refresh()` leaves it to its owner)"""
        import copy
        if flat is not None and (flat.dtype != torch.float32 or tuple(flat.shape) != (int(optimizer.numel),) or not flat.is_contiguous()
                                 or flat.device != optimizer.flat_p.device or flat.data_ptr() == optimizer.flat_p.data_ptr()):
            raise ValueError(f"FrozenTeacher: flat must be a contiguous float32 buffer of {int(optimizer.numel)} elements on the "
                             f"optimiser's device, other than its flat_p")
        self._owns_flat = flat is None
        self.flat = optimizer.flat_p.detach().clone() if flat is None else flat
        self.numel = int(optimizer.numel)
        base = optimizer.flat_p.data_ptr()
        memo = {}
        for p in optimizer.params:
            o = (p.data_ptr() - base) // 4
            view = self.flat[o:o + p.numel()].as_strided(p.shape, p.stride())
            memo[id(p)] = torch.nn.Parameter(view, requires_grad=False)
        self.image_model = copy.deepcopy(image_model, memo)
        self.text_model = copy.deepcopy(text_model, memo)
        self._pairs = []                      # (teacher tensor, student tensor) of everything that does not live in the flat copy
        shared = {id(v) for v in memo.values()}
        for tm, sm in ((self.image_model, image_model), (self.text_model, text_model)):
            tm.eval()
            tm.grad_ready_hook = None
            tm.save_free = False
            for tp, sp in zip(tm.parameters(), sm.parameters()):
                tp.requires_grad_(False)
                tp.grad = None
                if id(tp) not in shared:
                    self._pairs.append((tp, sp))
            self._pairs += list(zip(tm.buffers(), sm.buffers()))
        if hasattr(self.text_model, "_dropout"):
            self.text_model._dropout = None   # eval mode already draws none; the copy does not carry the student's stream either

    @torch.no_grad()
    def refresh(self, optimizer) -> None:
        """take the student's current parameters and buffers, in place (a flat copy handed in at construction is its owner's: only
        the cloned tensors are refreshed)"""
        if self._owns_flat:
            self.flat.copy_(optimizer.flat_p)
        for t, s in self._pairs:
            t.copy_(s)

    def state_dict(self) -> dict:
        """tensors and plain numbers only (loadable with weights_only=True): the flat copy and the cloned tensors, in module order"""
        return {"numel": self.numel, "flat": self.flat.detach().cpu(), "tensors": [t.detach().cpu() for t, _ in self._pairs]}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """strict: the keys of `state_dict()`, a flat copy of exactly this optimiser's size, the cloned tensors' number and shapes"""
        if not isinstance(sd, dict) or set(sd) != {"numel", "flat", "tensors"}:
            raise ValueError(f"FrozenTeacher.load_state_dict: expected the keys ['flat', 'numel', 'tensors'], got "
                             f"{sorted(sd) if isinstance(sd, dict) else type(sd).__name__}")
        flat, tensors = sd["flat"], sd["tensors"]
        if int(sd["numel"]) != self.numel or not isinstance(flat, torch.Tensor) or flat.dtype != torch.float32 or tuple(flat.shape) != (self.numel,):
            raise ValueError(f"FrozenTeacher.load_state_dict: 'flat' must be a float32 tensor of {self.numel} elements (this optimiser's "
                             f"flat buffer), got numel {sd['numel']!r} and {tuple(flat.shape) if isinstance(flat, torch.Tensor) else type(flat).__name__}")
        if not isinstance(tensors, (list, tuple)) or len(tensors) != len(self._pairs):
            raise ValueError(f"FrozenTeacher.load_state_dict: expected {len(self._pairs)} cloned tensors, got "
                             f"{len(tensors) if isinstance(tensors, (list, tuple)) else type(tensors).__name__}")
        for k, ((t, _), v) in enumerate(zip(self._pairs, tensors)):
            if not isinstance(v, torch.Tensor) or v.dtype != t.dtype or tuple(v.shape) != tuple(t.shape):
                raise ValueError(f"FrozenTeacher.load_state_dict: cloned tensor {k} must be {t.dtype} {tuple(t.shape)}, got "
                                 f"{getattr(v, 'dtype', type(v).__name__)} {tuple(getattr(v, 'shape', ()))}")
        self.flat.copy_(flat)
        for (t, _), v in zip(self._pairs, tensors):
            t.copy_(v)


def check_agem_options(memory, batch, every, seed) -> tuple:
    """(agem_memory, agem_batch, agem_every, agem_seed) checked, the defaults of `every` (1) and `seed` (0) filled in; options given
    without `agem_memory` are refused"""
    if memory is None:
        if batch is not None or every is not None or seed is not None:
            raise ValueError("agem_batch / agem_every / agem_seed are options of A-GEM; they were given without agem_memory")
        return None, None, None, None
    for name, v, lo in (("agem_memory", memory, 1), ("agem_batch", batch, 1), ("agem_every", every, 1), ("agem_seed", seed, 0)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < lo):
            raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return memory, batch, 1 if every is None else every, 0 if seed is None else seed


def check_ema_options(decay, warmup, ema_eval, teacher, distill_weight=None) -> tuple:
    """(ema_decay, ema_warmup, ema_eval, ema_teacher) checked, the defaults (warmup on, the other two off) filled in; options given
    without `ema_decay` are refused, and so is `ema_teacher` without `distill_weight`"""
    if decay is None:
        if warmup is not None or ema_eval is not None or teacher is not None:
            raise ValueError("ema_warmup / ema_eval / ema_teacher are options of the parameter average; they were given without ema_decay")
        return None, None, None, None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (math.isfinite(decay) and 0.0 <= decay <= 1.0):
        raise ValueError(f"ema_decay must be a number in [0, 1], got {decay!r}")
    for name, v in (("ema_warmup", warmup), ("ema_eval", ema_eval), ("ema_teacher", teacher)):
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{name} must be True or False, got {v!r}")
    if teacher and distill_weight is None:
        raise ValueError("ema_teacher makes the teacher of similarity distillation a momentum teacher; it was given without distill_weight")
    return float(decay), True if warmup is None else warmup, bool(ema_eval), bool(teacher)


def _refuse_averaged(trainer, what: str) -> None:
    """inside `JointContrastiveTrainer.averaged()` the flat parameter buffer holds the average: whatever trains on it, anchors it or
    copies it is refused (a trainer without the attribute was never inside)"""
    if getattr(trainer, "_averaging", False):
        raise RuntimeError(f"JointContrastiveTrainer.{what}: called inside averaged(); the flat parameter buffer holds the average "
                           f"until the context exits")


MLM_PROBABILITY = 0.15                        # HF DataCollatorForLanguageModeling's default
MLM_MASK_TOKEN_ID = 4                         # CXR-BERT's vocabulary: [PAD] 0, [UNK] 1, [CLS] 2, [SEP] 3, [MASK] 4
MLM_SPECIAL_IDS = (0, 1, 2, 3, 4)


def check_mlm_options(weight, probability, seed, mask_token_id, special_ids, micro_batch=None) -> tuple:
    """(mlm_weight, mlm_probability, mlm_seed, mlm_mask_token_id, mlm_special_ids) checked, the defaults filled in (the seed stays None:
    the constructor draws one); options given without `mlm_weight` are refused, and so is `mlm_weight` with `micro_batch`"""
    if weight is None:
        if any(v is not None for v in (probability, seed, mask_token_id, special_ids)):
            raise ValueError("mlm_probability / mlm_seed / mlm_mask_token_id / mlm_special_ids are options of the masked-language-"
                             "modelling loss; they were given without mlm_weight")
        return None, None, None, None, None
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not (math.isfinite(weight) and weight >= 0):
        raise ValueError(f"mlm_weight must be finite and >= 0, got {weight!r}")
    if micro_batch is not None:
        raise ValueError("mlm_weight with micro_batch is out of scope of this step: the masked-language-modelling loss needs the last "
                         "hidden state of every chunk, which the micro-batched step does not keep; construct the trainer with "
                         "micro_batch=None or without mlm_weight")
    probability = MLM_PROBABILITY if probability is None else probability
    if isinstance(probability, bool) or not isinstance(probability, (int, float)) or not 0.0 <= probability <= 1.0:
        raise ValueError(f"mlm_probability must lie in [0, 1], got {probability!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or seed < 0):
        raise ValueError(f"mlm_seed must be an integer >= 0, got {seed!r}")
    mask_token_id = MLM_MASK_TOKEN_ID if mask_token_id is None else mask_token_id
    if isinstance(mask_token_id, bool) or not isinstance(mask_token_id, int) or mask_token_id < 0:
        raise ValueError(f"mlm_mask_token_id must be an integer >= 0, got {mask_token_id!r}")
    special_ids = MLM_SPECIAL_IDS if special_ids is None else tuple(special_ids)
    if len(special_ids) > 8 or any(isinstance(s, bool) or not isinstance(s, int) or s < 0 for s in special_ids):
        raise ValueError(f"mlm_special_ids must be at most 8 integers >= 0 (they are passed to the kernel by value), got {special_ids!r}")
    return float(weight), float(probability), seed, mask_token_id, special_ids


def _host_collective_device(group) -> str:
    """where the tensor of a collective on host integers has to live: RCCL moves device memory, gloo host memory"""
    import torch.distributed as dist
    return "cuda" if dist.get_backend(group) == "nccl" else "cpu"


def _broadcast_state(seed: int, counter: int, group) -> Tuple[int, int]:
    """the (seed, counter) of a random stream -> rank 0's, on every rank: one broadcast of two int64 (the 64-bit seed travels as its
    two's-complement reading)"""
    import torch.distributed as dist
    t = torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed, counter], dtype=torch.int64, device=_host_collective_device(group))
    dist.broadcast(t, src=0 if group is None else dist.get_global_rank(group, 0), group=group)
    s, c = (int(v) for v in t.cpu())
    return s & (2 ** 64 - 1), c


class JointContrastiveTrainer:
    def __init__(self, image_model: torch.nn.Module, text_model: torch.nn.Module, lr: float = 1e-4,
                 temperature: float = 0.07, group=None, train_mlm_head: bool = False, two_streams: Optional[bool] = None,
                 optim: str = "adam", positives: Optional[str] = None, learn_temperature: bool = False,
                 log_scale_bounds: Tuple[float, float] = LOG_SCALE_BOUNDS, augment: Optional[AugmentSpec] = None,
                 augment_seed: Optional[int] = None, loss: str = "infonce", sigmoid_bias: Optional[float] = None,
                 micro_batch: Optional[int] = None, weight_decay: Optional[float] = None, max_grad_norm: Optional[float] = None,
                 warmup_steps: Optional[int] = None, total_steps: Optional[int] = None, lr_decay: Optional[str] = None,
                 min_lr_ratio: Optional[float] = None, ewc_lambda: Optional[float] = None, ewc_gamma: Optional[float] = None,
                 ewc_fisher: Optional[str] = None, distill_weight: Optional[float] = None,
                 distill_temperature: Optional[float] = None, agem_memory: Optional[int] = None,
                 agem_batch: Optional[int] = None, agem_every: Optional[int] = None, agem_seed: Optional[int] = None,
                 mlm_weight: Optional[float] = None, mlm_probability: Optional[float] = None, mlm_seed: Optional[int] = None,
                 mlm_mask_token_id: Optional[int] = None, mlm_special_ids: Optional[Tuple[int, ...]] = None,
                 ema_decay: Optional[float] = None, ema_warmup: Optional[bool] = None, ema_eval: Optional[bool] = None,
                 ema_teacher: Optional[bool] = None):
        """`optim="adamw"`: `optim.AdamW` with decoupled `weight_decay` (default 0.01; parameters with ndim <= 1 do
        not decay) and, with `max_grad_norm`, clipping of the global gradient norm (`inf`: the norm is taken and reported, nothing
        is clipped).  `warmup_steps` / `total_steps` / `lr_decay` ("constant" | "linear" | "cosine") / `min_lr_ratio`: an
        `optim.LRSchedule` around `lr`, for every optimiser; with none of them given the learning rate is never touched.
        `ewc_lambda`: elastic weight consolidation, an `optim.EWC` of that strength over the optimiser's flat
        buffers (`ewc_fisher` "empirical" | "identity", `ewc_gamma` in [0, 1]).  Until the first `consolidate(batches)` a step is
        bit for bit the step without it; afterwards `step` adds the penalty's gradient between the gradient all-reduce and the
        optimiser's step, so clipping and the update see it exactly as if the penalty were part of the loss.
        `distill_weight` = beta: similarity distillation from a frozen teacher; `distill_temperature` = tau_d
        (default: `temperature`).  Until the first `snapshot_teacher()` a step is bit for bit the step without it; afterwards the
        step's objective is contrastive + beta * L_d, with L_d of `functional.distill_loss` against the snapshot's encoders.
        `agem_memory` = M: A-GEM.  `remember(batches)` keeps M rows of a finished task per rank in an
        `memory.EpisodicMemory` (seeded by `agem_seed`, default 0); once it holds rows, every `agem_every`-th step (default 1) first
        takes the gradient of `agem_batch` memory rows (default: as many as the step's shard has, at most all stored) as the
        reference, and every step projects its gradient against the stored reference (`optim.AGEM`).  Until the first `remember()`
        a step is bit for bit the step without it.
        `mlm_weight` = w: the masked-language-modelling auxiliary loss.  Every step masks its token ids on the
        device (HF DataCollatorForLanguageModeling's rule with `mlm_probability`, default 0.15, `mlm_mask_token_id`, default 4, never
        touching `mlm_special_ids`, default (0, 1, 2, 3, 4), nor padding), runs the text encoder ONCE on the masked ids and trains
        contrastive + w * L_mlm, L_mlm the mean cross-entropy of HF's MLM head over the selected tokens of the global batch.  It
        implies that the head (`cls.predictions.*`) is trained.  `mlm_seed` (default: drawn from torch's CPU generator) seeds the
        draws; `mlm_state` is the (seed, step counter) pair.  Not with `micro_batch`.  `mlm_weight=None` (the default) issues exactly
        the calls it always did.
        `ema_decay` = d in [0, 1]: `self.ema`, an `optim.EMA` of the flat parameter buffer.  It starts at the entry of
        the first `step` (or of the first `snapshot_teacher()` with `ema_teacher`), not here: `Trainer` broadcasts the parameters
        and loads checkpoints after construction, and the average has to start from those values.  `step` updates it after the
        optimiser's step and the clamp of theta; `consolidate`, the A-GEM reference pass and `_gradient` never do.  `ema_warmup`
        (default True): the decay of update t is min(d, (1 + t) / (10 + t)).  `averaged()`: the encoders read the average.
        `ema_eval`: kept for `Trainer`, which then evaluates inside `averaged()`.  `ema_teacher` (needs `distill_weight`): the
        teacher's flat copy is the average itself.  Losses and parameters of a run with `ema_decay` and no `ema_teacher` are bit for
        bit those of the run without it."""
        self.ema_decay, self.ema_warmup, self.ema_eval, self.ema_teacher = check_ema_options(ema_decay, ema_warmup, ema_eval, ema_teacher,
                                                                                              distill_weight)
        self.ema, self._averaging = None, False
        self.agem_memory, self.agem_batch, self.agem_every, self.agem_seed = check_agem_options(agem_memory, agem_batch, agem_every,
                                                                                                agem_seed)
        self.micro_batch = check_micro_batch(micro_batch)
        (self.mlm_weight, self.mlm_probability, mlm_seed, self.mlm_mask_token_id,
         self.mlm_special_ids) = check_mlm_options(mlm_weight, mlm_probability, mlm_seed, mlm_mask_token_id, mlm_special_ids, self.micro_batch)
        self._mlm, self._mlm_version, self._mlm_synced = None, 0, None      # [seed, counter] as `_augment`
        self._mlm_off = False                # `_contrastive_only`: no masking, the counter stays
        self._mlm_call = None                # the `kernels.MlmMask` of the forward that is running
        self._pending_mlm = None             # w * L_mlm of the forward whose backward has not run yet
        self._last_mlm = None                # (L_mlm share of this rank, correct, stats, 1 / M_global) of the last step, on the device
        self.mlm_chunk_bytes = Fh.MLM_CHUNK_BYTES
        if self.mlm_weight is not None:
            train_mlm_head = True
            self._mlm_vocab = int(text_model.config.vocab_size)
            if self.mlm_mask_token_id >= self._mlm_vocab:
                raise ValueError(f"mlm_mask_token_id {self.mlm_mask_token_id} is outside the vocabulary of {self._mlm_vocab} ids")
            if mlm_seed is None:
                w = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64)
                mlm_seed = (int(w[0]) << 32) | int(w[1])
            self.mlm_state = (mlm_seed, 0)
        self.distill_weight, self.distill_temperature = check_distill_options(distill_weight, distill_temperature)
        self.teacher: Optional[FrozenTeacher] = None
        self._distill_off = False            # `consolidate` estimates the Fisher diagonal of the contrastive loss alone
        self._pending_distill = None         # beta * L_d of the forward whose backward has not run yet
        self._last_distill = None            # L_d of the last distilled step (device scalar)
        if ewc_lambda is None and (ewc_gamma is not None or ewc_fisher is not None):
            raise ValueError("ewc_gamma / ewc_fisher are options of elastic weight consolidation; they were given without ewc_lambda")
        if optim not in OPTIMS:
            raise ValueError(f"optim must be 'adam', 'sgd' or 'adamw', got {optim!r}")
        if optim != "adamw" and (weight_decay is not None or max_grad_norm is not None):
            raise ValueError(f"weight_decay / max_grad_norm are options of optim='adamw'; they were given with optim={optim!r}")
        self.schedule = None
        if any(v is not None for v in (warmup_steps, total_steps, lr_decay, min_lr_ratio)):
            self.schedule = cxr_optim.LRSchedule(lr, warmup_steps=0 if warmup_steps is None else warmup_steps, total_steps=total_steps,
                                                 decay="constant" if lr_decay is None else lr_decay,
                                                 min_lr_ratio=0.0 if min_lr_ratio is None else min_lr_ratio)
        if positives not in POSITIVES:
            raise ValueError(f"positives must be None, 'labels' or 'text', got {positives!r}")
        if loss not in LOSSES:
            raise ValueError(f"loss must be 'infonce' or 'sigmoid', got {loss!r}")
        if loss != "sigmoid" and sigmoid_bias is not None:
            raise ValueError(f"sigmoid_bias is the bias of loss='sigmoid'; it was given with loss={loss!r}")
        if loss == "sigmoid":
            sigmoid_bias = SIGMOID_BIAS if sigmoid_bias is None else float(sigmoid_bias)
            if not math.isfinite(sigmoid_bias):
                raise ValueError(f"sigmoid_bias must be finite, got {sigmoid_bias!r}")
            if not temperature > 0:
                raise ValueError(f"loss='sigmoid': the temperature must be positive, got {temperature!r}")
        self.loss = loss
        self.logit_scale = None
        self.logit_bias = None
        self._sigmoid_consts = None
        if learn_temperature:
            lo, hi = (float(v) for v in log_scale_bounds)
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError(f"log_scale_bounds must be finite with lo <= hi, got {log_scale_bounds!r}")
            if not temperature > 0:
                raise ValueError(f"learn_temperature: the initial temperature must be positive, got {temperature!r}")
            self.log_scale_bounds = (lo, hi)
        self.positives = positives
        self.augment = _augment_spec_from(augment)
        self._augment, self._augment_version, self._augment_synced = None, 0, None
        if self.augment is not None:
            if augment_seed is None:     # one 64-bit seed from torch's default CPU generator (`torch.manual_seed` makes it repeatable)
                w = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64)
                augment_seed = (int(w[0]) << 32) | int(w[1])
            self.augment_state = (augment_seed, 0)
        elif augment_seed is not None:
            raise ValueError("JointContrastiveTrainer: augment_seed given without an augment spec")
        self.image_model, self.text_model = image_model, text_model
        self.temperature, self.group = temperature, group
        import os
        self.two_streams = (os.environ.get("CXRK_TWO_STREAMS", "1") != "0") if two_streams is None else bool(two_streams)
        self._text_stream = None
        image_model.prepare_()
        text_model.prepare_()
        inamed = [(n, p) for n, p in image_model.named_parameters() if not n.startswith("encoder.encoder.fc.")]
        params = [p for _, p in inamed]
        tparams = []
        for n, p in text_model.named_parameters():
            if n.startswith("cls.predictions.") and not train_mlm_head:
                continue  # MLM head: no gradient on this path
            tparams.append(p)
        if learn_temperature:
            # behind the text parameters: the "text" reduce span stays gap-free and runs on over theta's slot (`reduce_spans`), so
            # the spans still tile the buffer and the final flat all-reduce has nothing left.  Every rank derives theta from the same
            # `temperature`; `Trainer`'s initial broadcast of the flat parameter buffer covers it as well.
            dev = next(image_model.parameters()).device
            self.logit_scale = torch.nn.Parameter(torch.tensor([math.log(1.0 / float(temperature))], dtype=torch.float32, device=dev))
            tparams = tparams + [self.logit_scale]
            if loss == "sigmoid":    # the bias is learned with the scale, and follows it: "text" runs on over both slots
                self.logit_bias = torch.nn.Parameter(torch.tensor([sigmoid_bias], dtype=torch.float32, device=dev))
                tparams = tparams + [self.logit_bias]
        elif loss == "sigmoid":
            # fixed theta and b: two device constants made once, here; no parameter and no per-step host-to-device copy
            dev = next(image_model.parameters()).device
            self._sigmoid_consts = (torch.tensor([math.log(1.0 / float(temperature))], dtype=torch.float32, device=dev),
                                    torch.tensor([sigmoid_bias], dtype=torch.float32, device=dev))
        if optim == "adam":          # the reference's `optim.Adam(params, lr)` / `optim.SGD(params, lr)` (Trainer.py:172-178)
            self.optimizer = cxr_optim.Adam(params + tparams, lr=lr)
        elif optim == "sgd":
            self.optimizer = cxr_optim.SGD(params + tparams, lr=lr)
        else:                        # "adamw": biases, norm parameters, theta and b (everything with ndim <= 1) do not decay
            self.optimizer = cxr_optim.AdamW(params + tparams, lr=lr, max_grad_norm=max_grad_norm,
                                             **({"weight_decay": weight_decay} if weight_decay is not None else {}))
        text_model.prepare_()
        self.ewc = None
        if ewc_lambda is not None:
            self.ewc = cxr_optim.EWC(self.optimizer, ewc_lambda, fisher="empirical" if ewc_fisher is None else ewc_fisher,
                                     gamma=1.0 if ewc_gamma is None else ewc_gamma)
        self.agem, self.memory, self.agem_steps = None, None, 0
        if self.agem_memory is not None:
            from .memory import EpisodicMemory
            self.agem = cxr_optim.AGEM(self.optimizer)
            self.memory = EpisodicMemory(self.agem_memory, seed=self.agem_seed)
        if self.ema_decay is not None:   # no buffer yet: `begin()` runs at the first step
            self.ema = cxr_optim.EMA(self.optimizer, self.ema_decay, warmup=self.ema_warmup)
        self.world, self.rank = 1, 0
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.world = dist.get_world_size(group)
            self.rank = dist.get_rank(group)
        self._dropout_synced = None
        self.sync_dropout_state()
        self.sync_augment_state()
        self.sync_mlm_state()
        self._spans = self.reduce_spans(inamed, tparams) if self.world > 1 else {}

    def current_temperature(self) -> float:
        """tau = exp(-theta) as a host float: the one place that reads theta back (a host sync), and only when called."""
        if self.logit_scale is None:
            return float(self.temperature)
        return math.exp(-float(self.logit_scale.detach().cpu()))

    def current_bias(self) -> Optional[float]:
        """b of the sigmoid loss as a host float (None with loss="infonce"): a host sync when b is learned, and only when called."""
        if self.loss != "sigmoid":
            return None
        b = self.logit_bias if self.logit_bias is not None else self._sigmoid_consts[1]
        return float(b.detach().cpu())

    def sync_dropout_state(self) -> None:
        """Text dropout under data parallelism: every rank takes rank 0's (seed, counter), so that with the row offset of
        `forward_loss` the masks of a sharded step are those of the single-process step on the global batch.  Runs at construction
        and at the start of every `step`; it communicates only when the text model's dropout stream was (re)seeded or assigned since
        the last time (`enable_dropout_` / `dropout_state` on every rank, in the same program order)."""
        tm = self.text_model
        version = getattr(tm, "_dropout_version", None)
        if self.world == 1 or not getattr(tm, "dropout_enabled", False) or version == self._dropout_synced:
            return
        tm.dropout_state = _broadcast_state(*tm.dropout_state, self.group)
        self._dropout_synced = tm._dropout_version

    @property
    def augment_state(self) -> Optional[Tuple[int, int]]:
        """(seed, step counter) of the next augmented `step`; None without an augment spec.  Assign a pair to resume or repeat a
        stream.  The kernels key the draws by the low 24 bits of the counter."""
        return None if self._augment is None else (self._augment[0], self._augment[1])

    @augment_state.setter
    def augment_state(self, state: Tuple[int, int]) -> None:
        if self.augment is None:
            raise RuntimeError("augment_state: this trainer was constructed without an augment spec")
        seed, counter = state
        if int(counter) < 0:
            raise ValueError("augment_state: the step counter must be >= 0")
        self._augment = [int(seed) & (2 ** 64 - 1), int(counter)]
        self._augment_version += 1

    def sync_augment_state(self) -> None:
        """Augmentation under data parallelism: every rank takes rank 0's (seed, counter), as `sync_dropout_state` does for the text
        dropout; with the row offset of `step` the draws of a sharded step are those of the single-process step on the global batch.
        Runs at construction and at the start of every `step`; it communicates only when `augment_state` was assigned since the last
        time (on every rank, in the same program order)."""
        if self.world == 1 or self._augment is None or self._augment_version == self._augment_synced:
            return
        self._augment = list(_broadcast_state(*self._augment, self.group))
        self._augment_synced = self._augment_version

    # ------------------------------------------------------------------ masked-language-modelling loss
    @property
    def mlm_state(self) -> Optional[Tuple[int, int]]:
        """(seed, step counter) of the next masked `step`; None without `mlm_weight`.  Assign a pair to resume or repeat a stream.  The
        kernel keys the draws by the low 24 bits of the counter."""
        return None if self._mlm is None else (self._mlm[0], self._mlm[1])

    @mlm_state.setter
    def mlm_state(self, state: Tuple[int, int]) -> None:
        if self.mlm_weight is None:
            raise RuntimeError("mlm_state: this trainer was constructed without mlm_weight")
        seed, counter = state
        if int(counter) < 0:
            raise ValueError("mlm_state: the step counter must be >= 0")
        self._mlm = [int(seed) & (2 ** 64 - 1), int(counter)]
        self._mlm_version += 1

    def sync_mlm_state(self) -> None:
        """Token masking under data parallelism: every rank takes rank 0's (seed, counter), exactly as `sync_augment_state` does; with
        the row offset of `step` the draws of a sharded step are those of the single-process step on the global batch.  It
        communicates only when `mlm_state` was assigned since the last time (on every rank, in the same program order)."""
        if self.world == 1 or self._mlm is None or self._mlm_version == self._mlm_synced:
            return
        self._mlm = list(_broadcast_state(*self._mlm, self.group))
        self._mlm_synced = self._mlm_version

    def _masking(self) -> bool:
        return self._mlm is not None and not self._mlm_off

    def _mask_tokens(self, input_ids, attention_mask) -> K.MlmMask:
        """this step's draw, once, before the encoders: row offset = this rank's first global row, the counter advances once"""
        seed, counter = self._mlm
        self._mlm[1] = counter + 1
        input_ids = input_ids if input_ids.dtype == torch.int64 else input_ids.to(torch.int64)
        if attention_mask is not None and attention_mask.dtype != torch.int64:
            attention_mask = attention_mask.to(torch.int64)
        return K.mlm_mask_tokens(input_ids, attention_mask, seed, counter, self.mlm_probability, self._mlm_vocab, self.mlm_mask_token_id,
                                 self.mlm_special_ids, row_offset=self.rank * int(input_ids.shape[0]))

    def _mlm_head(self, last: torch.Tensor, m: K.MlmMask) -> None:
        """w * L_mlm on the last hidden state of the masked ids (on the stream the text encoder ran on): it waits in `_pending_mlm` for
        the step's one backward.  The mean runs over the selected tokens of the GLOBAL batch: one scalar all-reduce of the count."""
        count = m.count
        if self.world > 1:
            import torch.distributed as dist
            count = count.clone()
            if count.is_cuda and dist.get_backend(self.group) == "gloo":      # rehearsals of the N > 1 path (see `_all_gather_rows`)
                host = count.cpu()
                dist.all_reduce(host, group=self.group)
                count.copy_(host)
            else:
                dist.all_reduce(count, group=self.group)
        scale = torch.reciprocal(torch.clamp(count, min=1.0))                  # 1 / max(M_global, 1), never read on the host
        weighted, loss, correct = Fh._mlm_triple(last, m.sel, m.tgt, m.stats, self.text_model.mlm_head_params(), scale,
                                                 self.mlm_chunk_bytes, self.mlm_weight, self.text_model.config.layer_norm_eps)
        self._pending_mlm = weighted if (self.mlm_weight > 0 and weighted.requires_grad) else None
        self._last_mlm = (loss, correct, m.stats, count)

    def current_mlm(self) -> Optional[dict]:
        """{"loss", "accuracy", "masked", "overflowed"} of the last masked step as host numbers (None without `mlm_weight` or before the
        first such step): L_mlm, the fraction of the counted tokens whose arg-max is the original id, the tokens counted and the
        selected tokens that found no slot, all over the global batch.  A host sync -- and, data parallel, one all-reduce of four
        numbers, so every rank has to call it -- and only when called."""
        if self._last_mlm is None:
            return None
        loss, correct, stats, _ = self._last_mlm
        t = torch.stack((loss.double().reshape(()), correct[0].double(), stats[0].double(), (stats[1] - stats[0]).double()))
        if self.world > 1:
            import torch.distributed as dist
            t = t.to(_host_collective_device(self.group))
            dist.all_reduce(t, group=self.group)
        loss, correct, kept, over = (float(v) for v in t.cpu())
        return {"loss": loss, "accuracy": correct / kept if kept > 0 else float("nan"), "masked": int(kept), "overflowed": int(over)}

    def _step_forward_loss(self, images, input_ids, attention_mask, labels, keys) -> torch.Tensor:
        """`forward_loss` of one `step`: with an augment spec the image model carries this step's call descriptor while its forward
        runs (row offset = this rank's first global row; the shards are equal and contiguous), and the counter advances once.  With
        `mlm_weight` the token ids are masked first, once (`forward_loss` finds the draw in `_mlm_call`)."""
        if self._masking():
            self._mlm_call = self._mask_tokens(input_ids, attention_mask)
            try:
                return self._augmented_forward_loss(images, input_ids, attention_mask, labels, keys)
            finally:
                self._mlm_call = None
        return self._augmented_forward_loss(images, input_ids, attention_mask, labels, keys)

    def _augmented_forward_loss(self, images, input_ids, attention_mask, labels, keys) -> torch.Tensor:
        if self._augment is None:
            return self.forward_loss(images, input_ids, attention_mask, labels, keys)
        seed, counter = self._augment
        self._augment[1] = counter + 1
        self.image_model.augment_call = AugmentCall(self.augment, seed, counter, self.rank * int(images.shape[0]))
        try:
            return self.forward_loss(images, input_ids, attention_mask, labels, keys)
        finally:
            self.image_model.augment_call = None

    def reduce_spans(self, inamed=None, tparams=None) -> dict:
        """{tag: (lo, hi)} element ranges of the flat gradient buffer that become complete together during `backward()`, in the
        order they complete: "text" (the whole text encoder: its backward is a third of the step's and ends first; with
        `learn_temperature` also theta's slot behind it, which the loss's backward has written before the text encoder's backward
        starts, on the stream that backward then waits for), then the
        image encoder from the back: "head" (projector + layer4), "layer3", "layer2", "stem" (layer1 + stem).  Each range is
        all-reduced as soon as its gradients are complete (hooks on the encoders' backward, see `step`), under the rest of the
        backward; a tag whose parameters do not form one gap-free range is left to the final reduce."""
        from .image_encoder import stage_of_param
        if inamed is None:
            inamed = [(n, p) for n, p in self.image_model.named_parameters() if not n.startswith("encoder.encoder.fc.")]
        if tparams is None:
            ids = {id(p) for p in self.optimizer.params}
            tparams = [p for p in self.text_model.parameters() if id(p) in ids]
            if self.logit_scale is not None:
                tparams.append(self.logit_scale)
            if self.logit_bias is not None:
                tparams.append(self.logit_bias)
        groups = {"text": list(tparams)}
        for n, p in inamed:
            groups.setdefault(stage_of_param(n), []).append(p)
        spans = {tag: self.optimizer.grad_span(ps) for tag, ps in groups.items()}
        return {tag: sp for tag, sp in spans.items() if sp is not None}

    def pair_keys(self, input_ids, attention_mask, labels=None, keys=None) -> Optional[torch.Tensor]:
        """The int64 [B] keys of this step's pairs, or None for the plain loss.  Explicit `keys` win; otherwise `positives` decides:
        None -> None (labels are ignored, no arithmetic is issued), "text" -> `keys_from_tokens(input_ids, attention_mask)`,
        "labels" -> `keys_from_labels(labels)` (ValueError without labels).  The hash runs on the device its inputs are on -- the
        host, when the loader's tensors are passed as they come -- and `forward_loss` moves the [B] result to the embeddings."""
        if keys is not None:
            return keys
        if self.positives is None:
            return None
        if self.positives == "text":
            return keys_from_tokens(input_ids, attention_mask)
        if labels is None:
            raise ValueError("JointContrastiveTrainer(positives='labels'): this step got no labels (pass labels=[B, C] or keys=[B])")
        return keys_from_labels(labels)

    def forward_loss(self, images: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                     labels: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The two encoders are independent up to the loss, so the text encoder runs on a second HIP stream: the tail of one
        encoder's launch (its last, partly filled round of workgroups) overlaps the head of the other's.  Autograd replays
        each encoder's backward on the stream its forward ran on and joins them again before `backward()` returns.
        Text dropout masks are keyed by the global sequence index: this rank's shard starts at rank * local rows (the shards are
        equal and contiguous, gathered in rank order).
        `labels` / `keys`: see `pair_keys`; computed once, before the encoders run.
        With a teacher (`snapshot_teacher`) its two encoders run first, save-free, and beta * L_d on the same embeddings is left for
        `_backward(loss)`, which `step` uses in place of `loss.backward()`; the returned scalar is the contrastive loss alone."""
        keys = self.pair_keys(input_ids, attention_mask, labels, keys)
        if keys is not None:
            keys = keys.to(images.device, non_blocking=True)
        self.text_model.dropout_row_offset = self.rank * int(input_ids.shape[0])
        taught = self._teacher_pair(images, input_ids, attention_mask) if self._distilling() else None   # first: it keeps nothing
        img, txt = self._encode_pair(images, input_ids, attention_mask)
        loss = self._loss(img, txt, keys)
        if taught is not None:
            self._distill_head(img, txt, *taught)
        return loss

    def _encode_pair(self, images, input_ids, attention_mask, models=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """both encoders (`models`: another pair, the teacher's) on the same rows -> (image embeddings, text embeddings), the text
        encoder on the second stream"""
        im, tm = (self.image_model, self.text_model) if models is None else models
        m = self._mlm_call

        def text():
            if m is None:
                return tm.get_projected_text_embeddings(input_ids, attention_mask, normalize_embeddings=False)
            # a masked step: every text call reads the masked ids through the full-sequence path (a teacher then gives the student's
            # bits at equal parameters); the student's last hidden state feeds the MLM head, on this stream
            txt, last = tm.get_projected_text_embeddings_and_hidden(m.ids, attention_mask, want_hidden=models is None)
            if models is None:
                self._mlm_head(last, m)
            return txt

        if not (self.two_streams and images.is_cuda):
            img = im(images)
            txt = text()
            return img, txt
        if self._text_stream is None:
            self._text_stream = torch.cuda.Stream(device=images.device)
        cur = torch.cuda.current_stream(images.device)
        self._text_stream.wait_stream(cur)                     # inputs, weights and the zeroed gradients are ready
        with torch.cuda.stream(self._text_stream):
            txt = text()
        img = im(images)
        cur.wait_stream(self._text_stream)
        txt.record_stream(cur)
        return img, txt

    # ------------------------------------------------------------------ similarity distillation
    def snapshot_teacher(self) -> None:
        """End of a task (needs `distill_weight`): freeze the current encoders as the teacher of the steps that follow.  The first
        call builds the copies (`FrozenTeacher`); a later one overwrites their flat parameter copy and buffers in place.  Under
        data parallelism every rank calls it at the same step: the replicas are identical, so are the teachers, and nothing is
        communicated.  With `ema_teacher` the copies' parameters are views of the parameter average (`self.ema.avg`, started here if
        no step has run yet): distillation begins at the first call as ever, the teacher then moves with every step's update of the
        average, and a later call refreshes only the cloned tensors (module buffers)."""
        if self.distill_weight is None:
            raise ValueError("JointContrastiveTrainer.snapshot_teacher: this trainer was constructed without distill_weight")
        _refuse_averaged(self, "snapshot_teacher")
        if self.teacher is None:
            flat = None
            if self.ema_teacher:
                self.ema.begin()
                flat = self.ema.avg
            self.teacher = FrozenTeacher(self.image_model, self.text_model, self.optimizer, flat=flat)
        else:
            self.teacher.refresh(self.optimizer)

    # ------------------------------------------------------------------ parameter average
    @contextlib.contextmanager
    def averaged(self):
        """While it is open the two encoders (and `current_temperature()`) read the averaged parameters: one `flat_swap` launch on
        entry exchanges the average and the flat parameter buffer that every trained parameter is a view of, one more on exit
        (in `finally`) puts both back bit for bit.  No copy of the model is made.  Inside, `step`, `consolidate`, `remember`,
        `snapshot_teacher` and a nested `averaged()` raise.  Module buffers (BatchNorm running statistics) are not averaged: the
        averaged model runs on the raw model's statistics.  Under data parallelism every rank enters and leaves alike."""
        if self.ema is None:
            raise ValueError("JointContrastiveTrainer.averaged: this trainer was constructed without ema_decay")
        _refuse_averaged(self, "averaged")
        self.ema.begin()
        self.ema.swap()
        self._averaging = True
        try:
            yield self
        finally:
            self.ema.swap()
            self._averaging = False

    def current_ema(self) -> Optional[dict]:
        """the parameter average as host numbers: "updates", "decay" and "last_decay" (the decay of the last update, None before it),
        all from host state: no sync.  None without `ema_decay`."""
        if self.ema is None:
            return None
        return {"updates": int(self.ema.updates), "decay": float(self.ema.decay), "last_decay": self.ema.last_decay}

    def current_distill(self) -> Optional[float]:
        """the unweighted L_d of the last distilled step as a host float (None without a teacher or before the first distilled step):
        a host sync, and only when called"""
        return None if self._last_distill is None else float(self._last_distill.detach().cpu())

    def _distilling(self) -> bool:
        return self.teacher is not None and not self._distill_off

    def _teacher_pair(self, images, input_ids, attention_mask) -> Tuple[torch.Tensor, torch.Tensor]:
        """the teacher's two encoders on the same rows, under no_grad through the save-free path (the same kernels, nothing kept).
        The teacher sees the images as the student does: it carries the student's augment call of this moment (`save_free` applies
        it under no_grad).  Eval mode: running statistics, no dropout."""
        t = self.teacher
        t.image_model.augment_call = self.image_model.augment_call
        t.image_model.save_free = t.text_model.save_free = True
        try:
            with torch.no_grad():
                return self._encode_pair(images, input_ids, attention_mask, models=(t.image_model, t.text_model))
        finally:
            t.image_model.augment_call = None
            t.image_model.save_free = t.text_model.save_free = False

    def _distill_head(self, img, txt, img_t, txt_t) -> None:
        """L_d on the step's embeddings: beta * L_d waits in `_pending_distill` for the step's one backward; beta = 0 keeps no graph"""
        tau = self.temperature if self.distill_temperature is None else self.distill_temperature
        if self.distill_weight > 0:
            self._pending_distill, self._last_distill = Fh._distill_pair(img, txt, img_t, txt_t, tau, self.distill_weight, self.group)
        else:
            with torch.no_grad():
                _, self._last_distill = Fh._distill_pair(img, txt, img_t, txt_t, tau, 0.0, self.group)

    def _backward(self, loss: torch.Tensor) -> None:
        """the step's one backward: the contrastive loss and, when a forward left one, beta * L_d, as two roots of one graph walk (each
        encoder's backward runs once, on the sum of both gradients of its embeddings)"""
        d, self._pending_distill = self._pending_distill, None
        m, self._pending_mlm = self._pending_mlm, None
        if d is None and m is None:
            loss.backward()
        else:
            torch.autograd.backward([loss] + [r for r in (d, m) if r is not None])

    def _loss(self, img, txt, keys):
        if self.loss == "sigmoid":
            theta, b = (self.logit_scale, self.logit_bias) if self.logit_scale is not None else self._sigmoid_consts
            return Fh.sigmoid_pairs_loss(img, txt, theta, b, self.group, keys=keys)
        return Fh.infonce_loss(img, txt, self.temperature, self.group, keys=keys, log_scale=self.logit_scale)

    def _gradient(self, images, input_ids, attention_mask, labels, keys) -> torch.Tensor:
        """Everything of a step up to and including the gradient all-reduce -> the loss; afterwards the flat gradient buffer holds the
        global-batch gradient, identical on every rank.  Shared by `step` and `consolidate`."""
        slices = ((0, int(images.shape[0])),) if self.micro_batch is None else micro_slices(int(images.shape[0]), self.micro_batch)
        chunked = len(slices) > 1
        self._pending_distill = None
        self._pending_mlm = None
        if chunked:
            self._require_eval_batchnorm()
        self.optimizer.zero_grad()
        self.sync_dropout_state()
        self.sync_augment_state()
        self.sync_mlm_state()
        works, fired = [], []      # without spans both stay empty: the final reduce then takes the whole buffer and waits for nothing
        on_ready = None

        if self.world > 1 and self._spans:
            def on_ready(tag: str) -> None:
                span = self._spans.get(tag)
                if span is None:
                    return
                if tag in fired:
                    raise RuntimeError(f"JointContrastiveTrainer.step: the gradients of '{tag}' were reported complete twice in one "
                                       f"backward (an encoder was called more than once in this step's graph)")
                fired.append(tag)
                works.extend(self.optimizer.all_reduce_span(span[0], span[1], self.group))

        if chunked:
            loss = self._chunked_forward_backward(images, input_ids, attention_mask, labels, keys, slices, on_ready)
        else:
            self.image_model.grad_ready_hook = self.text_model.grad_ready_hook = on_ready
            try:
                loss = self._step_forward_loss(images, input_ids, attention_mask, labels, keys)   # the hook is captured by the two autograd nodes here
            finally:
                self.image_model.grad_ready_hook = self.text_model.grad_ready_hook = None
            self._backward(loss)
        if on_ready is not None:
            self.last_overlapped = tuple(fired)
        if self.world > 1:
            self.optimizer.all_reduce_grads(self.group, skip=[self._spans[t] for t in fired], pending=works)
        return loss

    @contextlib.contextmanager
    def _contrastive_only(self):
        """While it is open `_gradient` is that of the contrastive loss alone, on the images as they are: no augmentation (its counter
        does not move) and no teacher.  What `consolidate` estimates and what the A-GEM reference is taken from."""
        augment, self._augment = self._augment, None
        self._distill_off = self._mlm_off = True
        try:
            yield
        finally:
            self._augment = augment
            self._distill_off = self._mlm_off = False

    def _stored_gradient(self, batch) -> torch.Tensor:
        """`_gradient` of a stored batch `(images, input_ids, attention_mask[, labels | keys])`: a fourth tensor of more than one
        dimension is taken as labels, a 1-D one as keys"""
        extra = batch[3] if len(batch) > 3 else None
        labels = extra if extra is not None and extra.dim() > 1 else None
        keys = extra if extra is not None and extra.dim() == 1 else None
        return self._gradient(batch[0], batch[1], batch[2], labels, keys)

    def step(self, images: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor,
             labels: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimisation step on this rank's shard; returns the global-batch loss (device scalar, no host sync).

        Data-parallel overlap (N > 1): the gradient all-reduce of a range of the flat buffer (`reduce_spans`) is started by the
        backward itself the moment that range is complete — a callable handed to THIS step's two encoder calls and carried by
        their autograd nodes (no module-level state): the text encoder's 0.44 GB under the image backward, then the image
        encoder's stages from the back (60 / 28 / 5 / 1 MB) under the layers in front of them; what is left (nothing, when every
        tag fired) is reduced after `backward()` returns.  Precondition, asserted: each encoder runs ONCE per step inside
        `forward_loss` — a second call of an encoder in the same graph would have its range reduced before the second
        contribution was accumulated.  A rank that raises inside `backward()` after a range was started leaves its peers inside that
        collective, as any failure of one data-parallel rank does: the job has to be torn down (torchrun / the RCCL watchdog).

        With `micro_batch` < this rank's rows the forward and backward run chunk by chunk (`_chunked_forward_backward`); the hook
        is then handed only to the encoder calls of the step's LAST backward, after which every range is complete.

        With `ema_decay` the parameter average starts here, at the entry of the first step (a copy of the parameters as they are
        by then), and takes its one launch at the very end, after the optimiser's step and the clamp."""
        if self.ema is not None:
            _refuse_averaged(self, "step")
            self.ema.begin()
        if self.agem is not None and len(self.memory) > 0:
            self._agem_reference(int(images.shape[0]))
        loss = self._gradient(images, input_ids, attention_mask, labels, keys)
        if self.agem is not None:        # no launch before the first reference; the penalty below is not projected: it already
            self.agem.apply()            # speaks for the old tasks
        if self.ewc is not None:         # no launch before the first consolidation
            self.ewc.apply()
        if self.schedule is not None:    # a host float that the update kernel takes as an argument: no launch, no sync
            self.optimizer.param_groups[0]["lr"] = self.schedule(self.optimizer.steps + 1)
        self.optimizer.step()
        if self.logit_scale is not None:
            K.clamp_inplace(self.logit_scale.data, *self.log_scale_bounds)
        if self.ema is not None:         # the decay is a host float argument of the one launch: no sync
            self.ema.update()
        return loss.detach()

    # ------------------------------------------------------------------ episodic memory and A-GEM
    def _agem_reference(self, rows: int) -> None:
        """The reference pass of a step: the gradient of a batch drawn from the memory, by `_gradient` (the same `micro_batch`
        chunks, the same overlapped all-reduce), kept by `optim.AGEM.store_reference()`.  Every `agem_every`-th step; in between
        the stored reference is reused.  It never augments and does not distil, as `consolidate`; no optimiser state moves.  The
        draw is keyed by (agem_seed, the count of such steps), identical on every rank."""
        k = self.agem_steps
        self.agem_steps = k + 1
        if self.agem.valid and k % self.agem_every != 0:
            return
        n = min(rows if self.agem_batch is None else self.agem_batch, len(self.memory))
        with self._contrastive_only():
            self._stored_gradient(self.memory.sample(n, step=k))
        self.agem.store_reference()

    def remember(self, batches) -> int:
        """End of a task (needs `agem_memory`): reservoir-sample `agem_memory` rows of the task's batches `(images, input_ids,
        attention_mask[, labels | keys])` -- this rank's shards, as for `step` -- into the episodic memory -> the rows stored.
        Under data parallelism every rank calls it with its own shards; one MAX all-reduce over (count, -count) then checks that
        all ranks hold the same number of rows (the sampler's indices are then the same everywhere), and raises if they do not."""
        if self.memory is None:
            raise ValueError("JointContrastiveTrainer.remember: this trainer was constructed without agem_memory")
        _refuse_averaged(self, "remember")
        kept = self.memory.add_task(batches)
        if self.world > 1:
            import torch.distributed as dist
            total = len(self.memory)
            t = torch.tensor([total, -total], dtype=torch.int64, device=_host_collective_device(self.group))
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            hi, lo = int(t[0]), -int(t[1])
            if hi != lo:
                raise RuntimeError(f"JointContrastiveTrainer.remember: the ranks hold between {lo} and {hi} memory rows (this one "
                                   f"{total}); every rank must be given the same number of rows per task")
        self.agem.valid = False              # the stored reference predates these rows
        return kept

    def current_interference(self) -> Optional[dict]:
        """`optim.AGEM.current_interference()` of the last projected-or-not step (None without `agem_memory` or before the first
        such step): a host sync, and only when called"""
        return None if self.agem is None else self.agem.current_interference()

    def consolidate(self, batches, max_batches: Optional[int] = None) -> int:
        """End of a task (needs `ewc_lambda`): estimate the Fisher diagonal and anchor the parameters -> the number of batches used.
        For each batch `(images, input_ids, attention_mask[, labels | keys])` -- this rank's shard, as for `step`; a fourth tensor
        of more than one dimension is taken as labels, a 1-D one as keys -- the gradient is computed as in `step` (the same
        `micro_batch` chunks, the same overlapped all-reduce) and its square accumulated; then `optim.EWC.consolidate()`.  No
        optimiser update, no schedule advance, no clamp: `optimizer.steps`, the moments and the parameters stay as they are.  It
        never augments and leaves the augmentation counter alone; nor does it distil (`distill_weight`): F is the Fisher diagonal of
        the contrastive loss alone.  With `ewc_fisher="identity"` no batch is read.  Under data
        parallelism every rank calls it with its shards; F comes from the all-reduced gradient, so it needs no collective of its
        own and is bit-identical on every rank."""
        if self.ewc is None:
            raise ValueError("JointContrastiveTrainer.consolidate: this trainer was constructed without ewc_lambda")
        _refuse_averaged(self, "consolidate")
        used = 0
        if self.ewc.fisher == "empirical":
            self.ewc.begin_estimate()
            with self._contrastive_only():      # the Fisher diagonal of the contrastive loss alone, of the images as they are
                for batch in batches:
                    if max_batches is not None and used >= max_batches:
                        break
                    if len(batch) < 3:
                        raise ValueError("consolidate: a batch is (images, input_ids, attention_mask[, labels | keys]); got "
                                         f"{len(batch)} tensors")
                    self._stored_gradient(batch)
                    self.ewc.accumulate()
                    used += 1
        self.ewc.consolidate()
        return used

    def current_penalty(self) -> Optional[float]:
        """the consolidation penalty of the last step as a host float (None without `ewc_lambda` or before the first penalised
        step): a host sync, and only when called"""
        return None if self.ewc is None else self.ewc.current_penalty()

    def _require_eval_batchnorm(self) -> None:
        """a micro-batched step is the unchunked step only while the rows of a batch are independent up to the loss"""
        if any(m.training for m in self.image_model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)):
            raise ValueError("JointContrastiveTrainer(micro_batch=...): the image model's BatchNorm layers are in training mode; batch "
                             "statistics depend on the chunk, so a micro-batched step would not be the step on the whole batch. "
                             "Call image_model.eval() / .train(my_freeze=True), or construct the trainer with micro_batch=None")

    def _chunked_forward_backward(self, images, input_ids, attention_mask, labels, keys, slices, on_ready) -> torch.Tensor:
        """Forward and backward of one step in the chunks `slices` -> the loss, detached.

          1. chunks 0..n-2 run through both encoders save-free (`ImageModel.save_free`, `CXRBertModel.save_free`): the same kernels
             and the same bits as a normal forward, nothing kept; their embeddings become one leaf that requires grad;
          2. the last chunk is forwarded normally; the loss head runs once on the [rows, D] pair (cache + last chunk), with its usual
             collectives; `loss.backward()` runs the last chunk's encoder backward, writes theta's and b's gradient and leaves
             dL/d(embedding) of the cached rows in the leaves' `.grad`;
          3. chunks 0..n-2 are forwarded again with their graph, and each takes its slice of the cached gradient through both
             encoders: the kernels accumulate into the flat gradient buffer (`gradsink`).

        At most one chunk's activations are alive at any time.  Every encoder call of the step uses the same dropout and augment
        (seed, counter), pinned here without going through the public setters (whose version bump would cost a broadcast), and the
        row offset rank * rows + chunk.lo; both counters advance once.  `on_ready` (data parallel) is handed only to the calls of
        the last backward, chunk n-2's: each range is reduced once, after its last contribution."""
        rows = int(images.shape[0])
        im, tm = self.image_model, self.text_model
        keys = self.pair_keys(input_ids, attention_mask, labels, keys)
        if keys is not None:
            keys = keys.to(images.device, non_blocking=True)
        aug = None
        if self._augment is not None:
            aug = (self._augment[0], self._augment[1])
            self._augment[1] = aug[1] + 1
        drop = getattr(tm, "_dropout", None)          # [seed, counter] of an opted-in text model
        drop_before = drop[1] if drop is not None else None
        base = self.rank * rows

        def encode(lo, hi, save_free=False, hook=None):
            if aug is not None:
                im.augment_call = AugmentCall(self.augment, aug[0], aug[1], base + lo)
            tm.dropout_row_offset = base + lo
            im.save_free = tm.save_free = save_free
            im.grad_ready_hook = tm.grad_ready_hook = hook
            try:
                return self._encode_pair(images[lo:hi], input_ids[lo:hi], attention_mask[lo:hi])
            finally:
                im.augment_call = None
                im.save_free = tm.save_free = False
                im.grad_ready_hook = tm.grad_ready_hook = None

        def teach(lo, hi):
            if aug is not None:       # `_teacher_pair` hands the teacher the student's call of this moment
                im.augment_call = AugmentCall(self.augment, aug[0], aug[1], base + lo)
            try:
                return self._teacher_pair(images[lo:hi], input_ids[lo:hi], attention_mask[lo:hi])
            finally:
                im.augment_call = None

        taught = None
        if self._distilling():      # the teacher's embeddings of ALL rows, chunk by chunk, next to the student's cache
            pairs = [teach(lo, hi) for lo, hi in slices]
            taught = (torch.cat([i for i, _ in pairs]), torch.cat([t for _, t in pairs]))
            del pairs
        cached = [encode(lo, hi, save_free=True) for lo, hi in slices[:-1]]            # pass 1: advances no counter
        ci = torch.cat([i for i, _ in cached]).requires_grad_()
        ct = torch.cat([t for _, t in cached]).requires_grad_()
        del cached
        img, txt = encode(*slices[-1])                                                   # advances the dropout counter, once
        drop_after = drop[1] if drop is not None else None
        img_all, txt_all = torch.cat((ci, img)), torch.cat((ct, txt))
        del img, txt
        loss = self._loss(img_all, txt_all, keys)
        if taught is not None:
            self._distill_head(img_all, txt_all, *taught)
        del img_all, txt_all, taught
        self._backward(loss)
        loss = loss.detach()
        gi, gt = ci.grad, ct.grad
        try:
            for k, (lo, hi) in enumerate(slices[:-1]):
                if drop is not None:
                    drop[1] = drop_before                                                # the masks of pass 1
                out = encode(lo, hi, hook=on_ready if k == len(slices) - 2 else None)
                pairs = [(o, g[lo:hi]) for o, g in zip(out, (gi, gt)) if o.requires_grad]   # a frozen encoder has no backward
                del out
                torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
                del pairs
        finally:
            if drop is not None:
                drop[1] = drop_after
        return loss

    def _dist_group(self):
        """the group to hand to the collectives of an evaluation: None in a single process, else this trainer's (the default group
        spelled out, because `functional.retrieval_ranks` takes `group=None` as "not distributed")"""
        if self.world == 1:
            return None
        if self.group is not None:
            return self.group
        import torch.distributed as dist
        return dist.group.WORLD

    @torch.no_grad()
    def evaluate_retrieval(self, batches, ks=RETRIEVAL_KS, return_embeddings: bool = False):
        """Image<->text retrieval of the two encoders over an evaluation set: `batches` yields
        `(images, input_ids, attention_mask[, labels])` — under data parallelism THIS rank's rows, the same number on every rank.
        Both encoders run in eval mode under no_grad (no augmentation, no dropout; the modules' previous modes are restored), the
        projected embeddings stay on the device ([N, D] each), and `retrieval_metrics` ranks every image against all reports and
        every report against all images once at the end.  With `positives` set the pairs' keys (`pair_keys`) define the positives.
        Nothing of the training state moves: parameters, optimiser, dropout and augment counters are left as they are.
        Returns the metrics dict, or (metrics, image embeddings, text embeddings) with `return_embeddings`."""
        ks = check_ks(ks)
        dev = next(self.image_model.parameters()).device
        modes = [(m, m.training) for model in (self.image_model, self.text_model) for m in model.modules()]
        imgs, txts, keys = [], [], []
        try:
            self.image_model.eval()
            self.text_model.eval()
            for batch in batches:
                if len(batch) < 3:
                    raise ValueError(f"evaluate_retrieval expects (images, input_ids, attention_mask[, labels]) batches, got {len(batch)} tensors")
                images, ids, mask = batch[0], batch[1], batch[2]
                k = self.pair_keys(ids, mask, batch[3] if len(batch) > 3 else None)
                if k is not None:
                    keys.append(k.to(dev))
                imgs.append(self.image_model(images.to(dev)))
                txts.append(self.text_model.get_projected_text_embeddings(ids.to(dev), mask.to(dev), normalize_embeddings=False))
        finally:
            for m, flag in modes:
                m.training = flag
        if not imgs:
            raise ValueError("evaluate_retrieval: no batches")
        img, txt = torch.cat(imgs).contiguous(), torch.cat(txts).contiguous()
        metrics = retrieval_metrics(img, txt, torch.cat(keys).contiguous() if keys else None, ks, self._dist_group())
        return (metrics, img, txt) if return_embeddings else metrics

    @torch.no_grad()
    def embed_images(self, batches, max_batches: Optional[int] = None):
        """(image embeddings [n, D], labels [n, C]) of `(images, ..., labels)` batches -- the labels are each batch's LAST tensor --
        with the image encoder in eval mode under no_grad (no augmentation, no dropout; the modules' previous modes are restored).
        At most `max_batches` batches are read.  Nothing of the training state moves."""
        dev = next(self.image_model.parameters()).device
        modes = [(m, m.training) for m in self.image_model.modules()]
        embs, labs = [], []
        try:
            self.image_model.eval()
            for n, batch in enumerate(batches):
                if max_batches is not None and n >= max_batches:
                    break
                if len(batch) < 2 or batch[-1].dim() != 2:
                    raise ValueError("kNN evaluation expects (images, ..., labels) batches with [B, C] labels last, got "
                                     f"{len(batch)} tensors")
                embs.append(self.image_model(batch[0].to(dev)))
                labs.append(batch[-1].to(device=dev, dtype=torch.float32))
        finally:
            for m, flag in modes:
                m.training = flag
        if not embs:
            raise ValueError("kNN evaluation: no batches")
        return torch.cat(embs).contiguous(), torch.cat(labs).contiguous()

    @torch.no_grad()
    def build_knn_bank(self, batches, max_batches: Optional[int] = None) -> KNNBank:
        """a finished `KNNBank` of the image embeddings of `batches` (this rank's shards; gathered over the trainer's group)"""
        bank = KNNBank()
        bank.add(*self.embed_images(batches, max_batches))
        return bank.finish(self._dist_group())

    @torch.no_grad()
    def evaluate_knn(self, bank_batches, eval_batches, k: int = KNN_K, temperature: float = KNN_TEMPERATURE,
                     max_bank_batches: Optional[int] = None) -> dict:
        """kNN label probe of the frozen image encoder: embed up to `max_bank_batches` of `bank_batches` into a
        `KNNBank`, then score every row of `eval_batches` by the weighted vote of its k nearest bank rows.  Both are
        `(images, ..., labels)` batches, under data parallelism THIS rank's rows.  Returns {"scores": [N, C], "labels": [N, C]} on
        the device for this rank's evaluation rows.  No text tower, no prompts, no trained head; the step counter, the dropout /
        augment / MLM counters, the optimiser and the parameter average are left as they are."""
        k, temperature = check_knn_options(k, temperature)
        bank = self.build_knn_bank(bank_batches, max_bank_batches)
        emb, labels = self.embed_images(eval_batches)
        if labels.shape[1] != bank.width:
            raise ValueError(f"evaluate_knn: the bank's labels are {bank.width} wide but the evaluation labels {labels.shape[1]}")
        return {"scores": bank.predict(emb, k, temperature), "labels": labels}
