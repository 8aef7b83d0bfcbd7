"""`Trainer` — the reference's incremental-learning trainer (`Trainer.py`, class at :100) with the hot loops on the
cxrk HIP kernels.  Same constructor, method names, argument meaning, module-level switches and error behaviour, so
`ZERO_JOINT_BOUNDS.py` / `CLASS_INCREMENTAL.py` / `DATA_INCREMENTAL.py`-style drivers run unchanged.

What changed underneath (results identical):
  * the 10 frozen CXR-BERT calls per step embed constant strings under no_grad (`Trainer.py:557-567,1657-1680`,
    `text/inference_engine.py:50`): their outputs are computed once and cached;
  * the 5x(pos,neg) Python loop of tiny cosine launches becomes one [B,128]x[128,2C] cosine kernel, and
    `nn.BCEWithLogitsLoss()` on (pos - neg) becomes one fused loss+gradient kernel (any other criterion is applied
    to the logits tensor as given);
  * `optim.Adam` / `optim.SGD` become one fused flat-buffer kernel; `myIncremental` a two-kernel reduction+restore.
Plotting / t-SNE / heat-map reporting (`Trainer.py:1074-1185,1310-1554`) is host-side visualisation and is not part
of this module; scalar metrics (sklearn) are kept.

Two extensions behind the same entry points (both off unless asked for):
  * `Trainer(..., joint_encoders={"image_model": ImageModel, "temperature": 0.07})` — the north-star step: both encoders train
    in-loop.  Loaders then yield `(images [B,3,H,W], input_ids [B,L], attention_mask [B,L][, labels [B,5]])`; `train`,
    `train_class_incremental` and `train_class_more_labels_incremental` run `contrastive.JointContrastiveTrainer.step` (ResNet-50 +
    CXR-BERT forward, InfoNCE over the global batch, hand-written backward, fused Adam) per batch, with the reference's
    iteration / logging / continual-learning bookkeeping around it; `val` / `test` embed the images with the trained image
    model and score them against the class prompts embedded by the trained text model (the zero-shot chain of
    `Trainer.py:797-837`).  The text model is the one inside `bert_encoder`.  `"positives": "labels" | "text"` in the dict makes
    pairs of the global batch with the same label vector / the same prompt tokens positives of each other (multi-positive InfoNCE,
    DESIGN.md §5.2; "labels" needs the fourth tensor of the batch); the default is one positive per row.  `"learn_temperature": True`
    (optionally `"log_scale_bounds": (lo, hi)`) makes the temperature a parameter: "temperature" is then its initial
    value, `save` / `load` carry it as `logit_scale.pt`, and `train` logs `train/temperature` once per epoch.
    `"contrastive_loss": "sigmoid"` (optionally `"sigmoid_bias": b`, default -10) trains with the pairwise sigmoid loss instead of
    InfoNCE; with "learn_temperature" its bias is learned too (`logit_bias` in `logit_scale.pt`, `train/bias`).
    `"augment": True | {...}`
    (the fields of `augment.AugmentSpec`; True = a moderate default; optionally `"augment_seed"`) augments the images on the device
    inside the training step; `val` / `test` never augment.  `"retrieval": True | (k, ...)` makes `val` / `test`
    also encode each batch's reports and add image<->text retrieval over the whole split (Recall@K, median / mean rank, both
    directions) to the returned dict and the writer as `Retrieval/i2t R@1`, ...; off by default.
    `"knn": True | {"k": 20, "temperature": 0.07, "bank_batches": 8}` adds a kNN label probe of the image embeddings (DESIGN.md
    §5.15): `knn_bank(loaders)` re-embeds up to "bank_batches" batches per loader into a bank of embeddings and labels, and from then
    on `val` / `test` label every evaluation image by the weighted vote of its k nearest bank rows and add `kNN/Accuracy`,
    `kNN/F1-macro`, `kNN/AUROC-macro`, `kNN/AUROC-weighted`; off by default, and nothing is added before `knn_bank`.
    `"micro_batch": n` runs the encoders on at most n of a rank's rows at a time (gradient cache): the same loss
    and update as the unchunked step up to fp32 summation order, at the peak memory of one chunk.
    `"optim": "adamw"` (overrides the module-level `OPTIM` for the joint trainer only) selects AdamW with decoupled
    `"weight_decay"` (default 0.01; biases and norm parameters do not decay) and, with `"max_grad_norm"`, clipping of the global
    gradient norm (`inf`: monitoring only); `"warmup_steps"`, `"total_steps"`, `"lr_decay"` ("constant" | "linear" | "cosine") and
    `"min_lr_ratio"` put a warmup / decay schedule around `lr` for any optimiser.  `train` then logs `train/lr` and,
    with "max_grad_norm", `train/grad_norm` once per epoch.
    `"ewc_lambda": s` adds elastic weight consolidation (optionally `"ewc_fisher"` "empirical" | "identity",
    `"ewc_gamma"` in [0, 1], `"ewc_batches"`: the most batches one estimate reads): `consolidate(loader)` after a task anchors the
    parameters and estimates their importance, later steps carry the quadratic penalty; `train` logs `train/ewc_penalty` once per
    epoch while it is active, `save` / `load` carry the state as `ewc.pt`.
    `"distill_weight": beta` (optionally `"distill_temperature": tau_d`, default "temperature") adds similarity distillation from a
    frozen teacher: `snapshot_teacher()` after a task freezes the current encoders, later steps add beta * L_d, the
    KL divergence of the teacher's image-text similarity distributions over the batch from the student's; `train` logs
    `train/distill` once per epoch while a teacher exists, `save` / `load` carry the teacher as `teacher.pt`.
    `"agem_memory": M` (optionally `"agem_batch"`, `"agem_every"`, `"agem_seed"`) adds A-GEM: `remember(loader)` after
    a task keeps M of its rows per rank in an episodic memory; later steps take a reference gradient on rows drawn from it and project
    the step's gradient when the two conflict; `train` logs `train/agem_projected` (the fraction of the epoch's steps projected) and
    `train/agem_dot` once per epoch while active, `save` / `load` carry the memory and the sampler's step counter as `agem.pt`.
    `"mlm_weight": w` (optionally `"mlm_probability"`, `"mlm_seed"`, `"mlm_mask_token_id"`, `"mlm_special_ids"`) adds the masked-
    language-modelling loss of CXR-BERT's own head: every step masks its token ids on the device and trains
    contrastive + w * L_mlm; `train` logs `train/mlm_loss` and `train/mlm_acc` once per epoch, `save` / `load` carry the (seed, step
    counter) of the masking stream as `mlm.pt`.
    `"ema_decay": d` (optionally `"ema_warmup"`, `"ema_eval"`, `"ema_teacher"`) keeps an exponential moving average of the trained
    parameters, updated by one launch after every step.  With `"ema_eval": True` `val` / `test` (the retrieval
    metrics included) evaluate the averaged weights under the same metric tags; with `"ema_teacher": True` (needs
    `"distill_weight"`) the distillation teacher is the average itself, a momentum teacher.  `train` logs `train/ema_decay` once per
    epoch, `save` / `load` carry the average as `ema.pt`; the saved model files stay the raw weights.
  * data parallelism: with `torch.distributed` initialised (one process per GPU) every rank draws the SAME global batch from its
    loader (same sampler seed) and trains on its contiguous row shard; adapter gradients (0.5 MB) are summed with one
    all-reduce of the flat gradient buffer, weighted by shard size, so the update equals the single-process global-batch one
    (SURVEY.md §8e).  In joint mode the shards' embeddings are all-gathered for the global similarity matrix.
"""
from __future__ import annotations

import contextlib
import copy
import inspect
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import ConcatDataset, DataLoader, RandomSampler, Subset, TensorDataset

from . import functional as Fh
from . import kernels as K
from . import optim as cxr_optim
from .contrastive import (KNN_K, KNN_TEMPERATURE, RETRIEVAL_KS, JointContrastiveTrainer, KNNBank, check_agem_options,
                          check_distill_options, check_ema_options, check_knn_options, check_ks, retrieval_metrics)
from .DataRetrieval import CHEXPERT_COMPETITION_CLASSES, basic_create_prompts, create_prompts
from .health_multimodal.text import get_cxr_bert_inference
from .models import myLinearModel, myMLP

# module-level switches, same names / defaults as the reference (Trainer.py:39-56)
SHARED = False
IMAGE_MODEL = True
TEXT_MODEL = True
MODEL_USED = "mlp"  # mlp, dense, "no-head"
OPTIM = "adam"  # sgd
MAX_EMB = False
NEW_PROMPTS = False
TRAIN_LOGIT_DIFF = True   # False <--> only POS
PRED_LOGIT_DIFF = False   # False <--> only POS
CHANGE_LABELS = False


class ScalarWriter:
    """Minimal stand-in for `torch.utils.tensorboard.SummaryWriter` (tensorboard is not installed here): keeps
    `add_scalar(tag, value, step)` and `log_dir`; values are buffered on the device and written as JSON lines on
    `flush()/close()` so logging never forces a host sync inside the training loop."""

    def __init__(self, log_dir: str):
        self.log_dir = log_dir
        os.makedirs(log_dir, exist_ok=True)
        self._rows: List[tuple] = []

    def add_scalar(self, tag, value, step=None):
        self._rows.append((tag, value.detach() if isinstance(value, torch.Tensor) else float(value), step))

    def add_figure(self, *a, **k):
        pass

    def scalars(self, tag=None):
        return [(t, float(v), s) for t, v, s in self._rows if tag is None or t == tag]

    def flush(self):
        import json
        with open(os.path.join(self.log_dir, "scalars.jsonl"), "a") as f:
            for t, v, s in self._rows:
                f.write(json.dumps({"tag": t, "value": float(v), "step": s}) + "\n")
        self._rows = []

    close = flush


def _make_writer(path: str):
    try:
        from torch.utils.tensorboard import SummaryWriter  # noqa: WPS433
        return SummaryWriter(path)
    except Exception:
        return ScalarWriter(path)


@torch.no_grad()
def change_values(tensor):
    """`Trainer.py:1708-1728`: as shipped maps 1 -> 1 and 0 -> -1, float32."""
    new_tensor = tensor.clone()
    new_tensor[tensor == 1] = 1
    new_tensor[tensor == 0] = -1
    return new_tensor.float().to(tensor.device)


# `joint_encoders` -> the keywords of `JointContrastiveTrainer.__init__`, whose signature declares (and whose body validates) the
# step's options.  A key is the keyword of the same name, except:
JOINT_RENAMED = {"contrastive_loss": "loss"}                      # key -> keyword, where the two differ
JOINT_OWN_KEYS = ("image_model", "retrieval", "ewc_batches")      # read by `Trainer` itself
JOINT_PROBE_KEYS = ("knn",)                                       # read by `Trainer` itself too, through `knn_options`
KNN_BANK_BATCHES = 8
# (master key, member keys, what the group configures, what the adapter schedules lack): a member needs its master, all need joint mode
JOINT_GROUPS = (("ewc_lambda", ("ewc_gamma", "ewc_fisher", "ewc_batches"), "elastic weight consolidation", "such penalty"),
                ("distill_weight", ("distill_temperature",), "similarity distillation", "teacher"),
                ("agem_memory", ("agem_batch", "agem_every", "agem_seed"), "A-GEM's episodic memory", "such memory"))
# the rest of the signature: the models, `lr` and the group are `Trainer`'s own arguments, the last two are not offered here
_STEP_KEYWORDS = set(inspect.signature(JointContrastiveTrainer.__init__).parameters) - {
    "self", "image_model", "text_model", "lr", "group", "train_mlm_head", "two_streams"}
JOINT_STEP_KEYS = {**{k: k for k in _STEP_KEYWORDS - set(JOINT_RENAMED.values())}, **JOINT_RENAMED}     # key -> keyword


def joint_options(joint_encoders):
    """`Trainer`'s `joint_encoders`, checked before anything is built -> (the keywords of `JointContrastiveTrainer` it sets, the values
    of `JOINT_OWN_KEYS`).  A dict, or the pair (image_model, temperature).  A key that is neither a keyword of the step's constructor
    nor in the tables above is refused; a key whose value is None counts as not given, as does "augment": False (a seed without a
    spec is then dropped); `OPTIM` is the optimiser unless "optim" names one.  The groups configure the joint trainer: without an
    "image_model" there is none, and their keys are refused."""
    if joint_encoders is None:
        return {}, dict.fromkeys(JOINT_OWN_KEYS)
    je = dict(joint_encoders) if isinstance(joint_encoders, dict) else {"image_model": joint_encoders[0], "temperature": joint_encoders[1]}
    unknown = [k for k in je if k not in JOINT_STEP_KEYS and k not in JOINT_OWN_KEYS and k not in JOINT_PROBE_KEYS]
    if unknown:
        raise ValueError(f"joint_encoders: unknown key(s) {unknown}; the valid keys are "
                         f"{sorted([*JOINT_STEP_KEYS, *JOINT_OWN_KEYS, *JOINT_PROBE_KEYS])}")
    if knn_options(je) is not None and je.get("image_model") is None:
        raise ValueError("joint_encoders: 'knn' probes the image encoder of the joint-encoder step and needs joint mode (an "
                         "'image_model'); the adapter schedules have no such encoder")
    for master, members, what, lacks in JOINT_GROUPS:
        given = [k for k in (master,) + members if je.get(k) is not None]
        if given and je.get("image_model") is None:
            raise ValueError(f"joint_encoders: {given} configure {what} of the joint-encoder step and need joint mode "
                             f"(an 'image_model'); the adapter schedules have no {lacks}")
        if given and je.get(master) is None:
            raise ValueError(f"joint_encoders: {given} are options of '{master}' and were given without it")
    nb = je.get("ewc_batches")
    if nb is not None and (isinstance(nb, bool) or not isinstance(nb, int) or nb < 1):
        raise ValueError(f"joint_encoders['ewc_batches'] must be an integer >= 1, got {nb!r}")
    kw = {JOINT_STEP_KEYS[k]: v for k, v in je.items() if k in JOINT_STEP_KEYS and v is not None}
    check_distill_options(kw.get("distill_weight"), kw.get("distill_temperature"))
    check_agem_options(*(kw.get(k) for k in ("agem_memory", "agem_batch", "agem_every", "agem_seed")))
    check_ema_options(*(kw.get(k) for k in ("ema_decay", "ema_warmup", "ema_eval", "ema_teacher", "distill_weight")))
    kw["temperature"] = float(kw.get("temperature", 0.07))
    kw.setdefault("optim", OPTIM)
    if kw.get("augment") in (None, False):
        kw.pop("augment", None)
        kw.pop("augment_seed", None)
    return kw, {k: je[k] if k == "image_model" else je.get(k) for k in JOINT_OWN_KEYS}     # (a dict without a model: KeyError)


def knn_options(joint_encoders) -> Optional[dict]:
    """the "knn" entry of `joint_encoders`: absent / None / False -> off (None); True -> the defaults; a dict with any of "k",
    "temperature", "bank_batches" -> those over the defaults {"k": 20, "temperature": 0.07, "bank_batches": 8}, validated"""
    opt = joint_encoders.get("knn") if isinstance(joint_encoders, dict) else None
    if opt is None or opt is False:
        return None
    if opt is True:
        opt = {}
    if not isinstance(opt, dict):
        raise ValueError(f"joint_encoders['knn'] must be True or a dict with 'k', 'temperature', 'bank_batches', got {opt!r}")
    unknown = [k for k in opt if k not in ("k", "temperature", "bank_batches")]
    if unknown:
        raise ValueError(f"joint_encoders['knn']: unknown key(s) {unknown}; the valid keys are ['bank_batches', 'k', 'temperature']")
    k, temperature = check_knn_options(opt.get("k", KNN_K), opt.get("temperature", KNN_TEMPERATURE))
    nb = opt.get("bank_batches", KNN_BANK_BATCHES)
    if isinstance(nb, bool) or not isinstance(nb, int) or nb < 1:
        raise ValueError(f"joint_encoders['knn']['bank_batches'] must be an integer >= 1, got {nb!r}")
    return {"k": k, "temperature": temperature, "bank_batches": nb}


class Trainer:
    def __init__(self, single_prompt, prompts, class_names, loss_name, lr, device, writer, bert_encoder=None, joint_encoders=None,
                 process_group=None):
        """Same positional arguments as the reference (`Trainer.py:101`).  `bert_encoder` (optional) injects a
        `TextInferenceEngine`; default `get_cxr_bert_inference()` as at `Trainer.py:109` (Hub fetch, or the offline
        synthetic model when CXRK_SYNTHETIC_WEIGHTS=1).  `joint_encoders` (optional, see the module docstring): a dict with
        "image_model" (an `ImageModel` on `device`) and optionally "temperature" (default 0.07) — no adapters are created, the
        trainable parameters are the two encoders; `joint_options` checks the dict before anything is built and refuses a key it does
        not know.  `process_group`: the data-parallel group (default: the default group when
        `torch.distributed` is initialised)."""
        step_options, own = joint_options(joint_encoders)
        self._ewc_batches = own["ewc_batches"]      # None: `consolidate` reads every batch of its loader
        self._agem_logged = (0, 0)         # (projected, applied) of `optim.AGEM` at the last epoch log
        self.pos_mean_counter = 0
        self.neg_mean_counter = 0
        self.n_reset = 0
        self.n_updated = 0
        self.image_adapter_copy = None
        self.text_adapter_copy = None
        self.bert_encoder = bert_encoder if bert_encoder is not None else get_cxr_bert_inference()
        self.bert_encoder.to(device)
        self.prompts = prompts
        self.class_names = class_names
        self.device = device
        self.writer = writer
        self.loss_name = loss_name
        self.change_labels = CHANGE_LABELS
        if self.change_labels:
            print("*** Watch out! Changing labels is enabled! ***")
        self.basic_prompts = single_prompt
        print("Single prompt per class" if single_prompt else "Multiple prompts per class")
        print("*** LOSS " + str(loss_name) + " ***")

        def new_adapter():
            if MODEL_USED == "mlp":
                return myMLP().to(device)
            if MODEL_USED == "dense":
                return myLinearModel().to(device)
            print("*** ERROR... ***")
            raise Exception

        import torch.distributed as dist
        self.group = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        self._joint = None
        self.image_model = None
        self._retrieval_ks = None          # joint_encoders={..., "retrieval": True | (k, ...)}: val / test add Retrieval/* metrics
        self._retrieval_result = None
        self._knn = None                   # joint_encoders={..., "knn": True | {...}}: after `knn_bank`, val / test add kNN/* metrics
        self._knn_bank = None
        self._knn_result = None
        if joint_encoders is not None:
            self.image_model = own["image_model"]
            if OPTIM not in ("adam", "sgd"):
                raise Exception
            self._joint = JointContrastiveTrainer(self.image_model, self.bert_encoder.model, lr=lr, group=process_group, **step_options)
            print("*** JOINT ENCODER TRAINING (%s over the global batch): no adapters ***"
                  % ("pairwise sigmoid loss" if self._joint.loss == "sigmoid" else "InfoNCE"))
            self._retrieval_ks = self._parse_retrieval(own["retrieval"])
            self._knn = knn_options(joint_encoders)
        params = []
        if self._joint is not None:
            self.image_adapter = self.text_adapter = None
        elif SHARED:
            print("*** SHARED MODEL !!!! ***")
            shared_model = new_adapter()
            self.image_adapter = shared_model
            self.text_adapter = shared_model
            params += list(shared_model.parameters())
        else:
            self.text_adapter = None
            if TEXT_MODEL:
                self.text_adapter = new_adapter()
                params += self.text_adapter.parameters()
            else:
                print("*** No text adapter !!!! ***")
            self.image_adapter = None
            if IMAGE_MODEL:
                self.image_adapter = new_adapter()
                params += self.image_adapter.parameters()
            else:
                print("*** No IMAGE MODEL !!!! ***")
        self._has_img = self.image_adapter is not None
        self._has_txt = self.text_adapter is not None
        print("image adapter", self.image_adapter)
        print("text adapter", self.text_adapter)
        if self._joint is not None:
            self.optimizer = self._joint.optimizer
        elif len(params) > 0:
            if OPTIM == "adam":
                print("Creating Adam optimizer...")
                self.optimizer = cxr_optim.Adam(params, lr=lr)
            elif OPTIM == "sgd":
                print("Creating SGD optimizer...")
                self.optimizer = cxr_optim.SGD(params, lr=lr)
            else:
                raise Exception
        else:
            self.optimizer = None
        if self.world > 1 and self.optimizer is not None:
            # replicas must start identical: rank 0's initial weights everywhere (the drivers seed every rank alike, this makes it
            # independent of that)
            dist.broadcast(self.optimizer.flat_p, src=dist.get_global_rank(process_group, 0) if process_group is not None else 0,
                           group=process_group)
        self.val_f1_heat_map = torch.empty((0, 5))
        self.val_auroc_heat_map = torch.empty((0, 5))
        self.test_f1_heat_map = torch.empty((0, 5))
        self.test_auroc_heat_map = torch.empty((0, 5))
        self._bert_cache: Dict[tuple, torch.Tensor] = {}
        self._flat_copy = None
        self._reset_counters = torch.zeros(2, dtype=torch.int64, device=device)
        self._reset_total = 0

    # ------------------------------------------------------------------------------------------------ data
    @staticmethod
    def _preprocessing(chex_competition, xrays_position, batch_size, dataset_root: Optional[str] = None):
        """Loaders over pre-computed `[N,128]` image embeddings + `[N,5]` labels (`Trainer.py:199-253`).
        The reference reads `embeddingDataset\\{train,val,test}\\512-chex-not-normalize[-frontal]\\
        embeddings_dataset_final_old.pt` relative to the CWD; the same layout is looked up under `dataset_root`
        (or $CXRK_EMBEDDING_DATASET).  Those files are whole-object pickles: they are opened with
        `weights_only=True` and must contain tensors only (a dict {"embs","labels"} or a tuple)."""
        if not chex_competition:
            raise Exception
        print("*** CHEX COMPETITION ***")
        class_names = list(CHEXPERT_COMPETITION_CLASSES)
        chex_str = "-chex"
        if xrays_position == "all":
            sub = "512" + chex_str + "-not-normalize"
        elif xrays_position == "frontal":
            sub = "512" + chex_str + "-not-normalize-frontal"
        else:
            raise Exception
        root = dataset_root or os.environ.get("CXRK_EMBEDDING_DATASET", "embeddingDataset")

        def load(split):
            path = os.path.join(root, split, sub, "embeddings_dataset_final_old.pt")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: pre-computed embedding dataset not found (Trainer.py:221-235); "
                                        f"use Trainer.synthetic_loaders(...) for synthetic data")
            obj = torch.load(path, map_location="cpu", weights_only=True)
            embs, labels = (obj["embs"], obj["labels"]) if isinstance(obj, dict) else obj
            return TensorDataset(embs.float(), labels.float())

        train_dataset, val_dataset, test_dataset = load("train"), load("val"), load("test")
        print("TrainBS:", batch_size, "Val/Test Batch size default set to 1024")
        mk = lambda ds, bs: DataLoader(ds, sampler=None, batch_size=bs, shuffle=True, num_workers=0, pin_memory=True,  # noqa: E731
                                       drop_last=False)
        return class_names, chex_str, mk(train_dataset, batch_size), mk(val_dataset, 1024), mk(test_dataset, 1024), None

    @staticmethod
    def synthetic_loaders(n_train: int, n_val: int, n_test: int, batch_size: int, seed: int = 29, shuffle: bool = True):
        """Synthetic stand-in for `_preprocessing`: N(0,1) embeddings, Bernoulli(0.3) labels."""
        from .synthetic import synthetic_adapter_batch
        out = []
        for i, (n, bs) in enumerate(((n_train, batch_size), (n_val, 1024), (n_test, 1024))):
            e, l, _ = synthetic_adapter_batch(n, seed=seed + i)
            g = torch.Generator().manual_seed(seed + 100 + i)
            out.append(DataLoader(TensorDataset(e, l), batch_size=bs, shuffle=shuffle, generator=g, num_workers=0,
                                  pin_memory=False, drop_last=False))
        return out

    @staticmethod
    def synthetic_joint_loaders(n_train: int, n_val: int, n_test: int, batch_size: int, image_size: int = 224, seq_len: int = 32,
                                vocab: int = 30522, seed: int = 27, eval_batch_size: int = 1024):
        """Loaders for the joint-encoder mode (SURVEY.md §8d inputs): `(images [B,3,S,S] in [0,1) with one plane replicated to 3
        channels, token ids [B,L], attention mask [B,L], multi-hot labels [B,5])`."""
        from .synthetic import synthetic_images, synthetic_tokens
        out = []
        for i, (n, bs) in enumerate(((n_train, batch_size), (n_val, eval_batch_size), (n_test, eval_batch_size))):
            ids, mask = synthetic_tokens(n, seq_len, vocab=vocab, seed=seed + 1 + 10 * i)
            g = torch.Generator().manual_seed(seed + 2 + 10 * i)
            labels = (torch.rand(n, 5, generator=g) < 0.3).float()
            ds = TensorDataset(synthetic_images(n, image_size, seed=seed + 10 * i), ids, mask, labels)
            gs = torch.Generator().manual_seed(seed + 100 + i)
            out.append(DataLoader(ds, batch_size=bs, shuffle=True, generator=gs, num_workers=0, pin_memory=False, drop_last=False))
        return out

    @staticmethod
    def _run_name(prefix, loss_name, lr, batch_size, epochs, chex_str, str_basic, xrays_position, extra=""):
        suffix = "-" + MODEL_USED
        if SHARED:
            suffix += "-SHARED-adapter"
        elif IMAGE_MODEL and TEXT_MODEL:
            suffix += "-double-adapter"
        elif IMAGE_MODEL:
            suffix += "-only-image-adapter"
        elif TEXT_MODEL:
            suffix += "-only-text-adapter"
        return (prefix + "-loss-" + str(loss_name) + "-opt-" + OPTIM + "-lr-" + str(lr) + "-bs" + str(batch_size) + "-ep"
                + str(epochs) + extra + chex_str + str_basic + "-" + str(xrays_position) + suffix)

    @staticmethod
    def _prompts_for(class_names, single_prompt):
        if single_prompt:
            return "-single-prompt", basic_create_prompts(class_names)
        return ("-MAX-prompt" if MAX_EMB else "-mean-prompt"), create_prompts(class_names, NEW_PROMPTS, TRAIN_LOGIT_DIFF)

    @staticmethod
    def _logit_suffix(w_path):
        w_path += "-NEW-PROMPTS" if NEW_PROMPTS else ""
        w_path += "-TRAIN-logit-DIFF" if TRAIN_LOGIT_DIFF else "-TRAIN-logit-POS"
        w_path += "-PRED-logit-DIFF" if PRED_LOGIT_DIFF else "-PRED-logit-POS"
        return w_path

    @staticmethod
    def preprocessing(chex_competition, xrays_position, single_prompt, batch_size, lr, epochs, loss_name,
                      dataset_root=None, log_root="."):
        """`Trainer.py:256-328`: returns (writer, class_names, train_loader, val_loader, test_loader, prompts,
        plot_tsne_array)."""
        class_names, chex_str, train_loader, val_loader, test_loader, plot_tsne_array = Trainer._preprocessing(
            chex_competition, xrays_position, batch_size, dataset_root)
        folder_name = "NUOVI_RISULTATI-3/zero-and-joint"
        str_basic, prompts = Trainer._prompts_for(class_names, single_prompt)
        if epochs > 0:
            w_path = os.path.join(log_root, folder_name, Trainer._run_name("joint-train", loss_name, lr, batch_size, epochs,
                                                                           chex_str, str_basic, xrays_position))
        else:
            if SHARED and IMAGE_MODEL and TEXT_MODEL:
                suffix = "-SHARED-adapter-" + MODEL_USED
            elif not SHARED and not IMAGE_MODEL and not TEXT_MODEL:
                suffix = "-no-head"
            else:
                raise Exception
            print("Attenzione! Zero-shot evaluation!")
            w_path = os.path.join(log_root, folder_name, "zero-shot-model" + chex_str + str_basic + "-" + str(xrays_position) + suffix)
        w_path = Trainer._logit_suffix(w_path)
        print("writer path:", w_path)
        return _make_writer(w_path), class_names, train_loader, val_loader, test_loader, prompts, plot_tsne_array

    @staticmethod
    def preprocessing_class_incremental(chex_competition, xrays_position, basic_prompts, batch_size, lr, epochs, loss_name,
                                        mode, CONTINUAL_LEARNING=None, ratio=None, threshold=None,
                                        threshold_scheduling=False, adder=0.01, MORE_LABELS=False, dataset_root=None,
                                        log_root="."):
        """`Trainer.py:330-435`: train_loader becomes a list of 5 task loaders."""
        print("**** Gradient Clipping ****\n--->" + str(CONTINUAL_LEARNING) if CONTINUAL_LEARNING is not None
              else "**** NO Gradient Clipping ****")
        class_names, chex_str, train_loader, val_loader, test_loader, plot_tsne_array = Trainer._preprocessing(
            chex_competition, xrays_position, batch_size, dataset_root)
        folder_name = "NUOVI_RISULTATI/" + mode + ("-more-labels" if MORE_LABELS else "")
        if mode == "class-pos-neg":
            train_loader = Trainer.split_dataloader_data_incremental(Trainer.concat_to_tensor_dataloader(train_loader), 5)
        elif mode == "class-pos":
            train_loader = Trainer.split_dataloader_by_label(Trainer.concat_to_tensor_dataloader(train_loader), batch_size=batch_size)
        else:
            raise Exception
        if epochs == 0:
            raise Exception
        thre_str = "-th-scheduled-" + str(adder) if (threshold_scheduling and CONTINUAL_LEARNING is not None) else ""
        cl_str = ""
        if CONTINUAL_LEARNING is not None and ratio:
            cl_str = "-" + str(CONTINUAL_LEARNING) + "-ratio-" + str(threshold)
            mode = "gradient-clipping-" + mode
        else:
            mode = "fine-tuning-" + mode
        str_basic, prompts = Trainer._prompts_for(class_names, basic_prompts)
        w_path = os.path.join(log_root, folder_name, Trainer._run_name(mode, loss_name, lr, batch_size, epochs, chex_str,
                                                                       str_basic, xrays_position)) + cl_str + thre_str
        w_path += "-MORE-LABELS" if MORE_LABELS else ""
        w_path = Trainer._logit_suffix(w_path) + "-DD"
        print("writer path:", w_path)
        return _make_writer(w_path), class_names, train_loader, val_loader, test_loader, prompts, plot_tsne_array

    @staticmethod
    def preprocessing_data_incremental(chex_competition, xrays_position, basic_prompts, batch_size, lr, parts, epochs,
                                       loss_name, mode, CONTINUAL_LEARNING=None, ratio=None, threshold=None,
                                       threshold_scheduling=False, adder=0.01, dataset_root=None, log_root="."):
        """`Trainer.py:437-523`: train_loader becomes a list of `parts` contiguous shards."""
        folder_name = "NUOVI_RISULTATI/data-incremental-" + str(parts) + "-parts"
        class_names, chex_str, train_loader, val_loader, test_loader, plot_tsne_array = Trainer._preprocessing(
            chex_competition, xrays_position, batch_size, dataset_root)
        if mode != "data-inc":
            raise Exception
        print("number of parts:", parts)
        train_loader = Trainer.split_dataloader_data_incremental(train_loader, parts)
        if epochs == 0:
            raise Exception
        thre_str = "-th-scheduled-" + str(adder) if (CONTINUAL_LEARNING is not None and threshold_scheduling) else ""
        cl_str = ""
        if CONTINUAL_LEARNING is not None and ratio:
            cl_str = "-" + str(CONTINUAL_LEARNING) + "-ratio-" + str(threshold)
            mode = "gradient-clipping-" + mode
        else:
            mode = "fine-tuning-" + mode
        str_basic, prompts = Trainer._prompts_for(class_names, basic_prompts)
        w_path = os.path.join(log_root, folder_name, Trainer._run_name(mode, loss_name, lr, batch_size, epochs, chex_str,
                                                                       str_basic, xrays_position,
                                                                       extra="-parts" + str(parts))) + cl_str + thre_str
        w_path = Trainer._logit_suffix(w_path) + "-DD"
        print("writer path:", w_path)
        return _make_writer(w_path), class_names, train_loader, val_loader, test_loader, prompts, plot_tsne_array

    # ------------------------------------------------------------------------------------------------ splitters
    @staticmethod
    def split_dataloader_by_label(dataloader, batch_size):
        """One loader per label with the samples positive for it (`Trainer.py:1187-1212`)."""
        if not isinstance(dataloader.dataset, TensorDataset):
            raise ValueError("Unsupported dataset type")
        loaders = []
        for i in range(5):
            indices = torch.where(dataloader.dataset.tensors[-1][:, i] == 1)[0]   # labels: the last tensor ([1] in the reference's pairs)
            subset = Subset(dataloader.dataset, indices)
            loaders.append(DataLoader(subset, batch_size=batch_size, sampler=RandomSampler(subset), num_workers=0,
                                      pin_memory=True, drop_last=False))
        return loaders

    @staticmethod
    def split_dataloader_data_incremental(dataloader, n):
        """N contiguous, equally sized shards (`Trainer.py:1214-1231`)."""
        dataset = dataloader.dataset
        num_samples = len(dataset)
        subset_size = math.ceil(num_samples / n)
        subsets = [Subset(dataset, range(i * subset_size, min((i + 1) * subset_size, num_samples))) for i in range(n)]
        return [DataLoader(s, batch_size=dataloader.batch_size, sampler=RandomSampler(s), num_workers=0, pin_memory=True,
                           drop_last=False) for s in subsets]

    @staticmethod
    def concat_to_tensor_dataloader(dataloader):
        """ConcatDataset of TensorDatasets -> one TensorDataset loader (`Trainer.py:1253-1271`)."""
        ds = dataloader.dataset
        if isinstance(ds, TensorDataset):
            return dataloader
        cols = [torch.cat([d.tensors[j] for d in ds.datasets]) for j in range(len(ds.datasets[0].tensors))]
        return DataLoader(TensorDataset(*cols), batch_size=dataloader.batch_size,
                          num_workers=0, pin_memory=dataloader.pin_memory, drop_last=dataloader.drop_last)

    @staticmethod
    def count_positive_labels(dataloader):
        tot = torch.zeros(5)
        for batch in dataloader:
            tot += batch[-1].sum(0)
        for i in range(5):
            print(f"Label {i}: {tot[i]}")

    # ------------------------------------------------------------------------------------------------ text side
    @torch.no_grad()
    def _bert_embed(self, prompts: Sequence[str]) -> torch.Tensor:
        """Frozen CXR-BERT embeddings of a prompt list, un-normalised (`Trainer.py:1660`); cached, since the encoder
        is frozen, in eval mode and called under no_grad (`text/inference_engine.py:50,63`)."""
        key = tuple(prompts)
        hit = self._bert_cache.get(key)
        if hit is None:
            hit = self.bert_encoder.get_embeddings_from_prompt(list(prompts), normalize=False, verbose=False).to(self.device)
            self._bert_cache[key] = hit   # (joint mode: emptied by every training step, the text encoder is no longer a constant)
        return hit

    def bert_forward_mean(self, pos_prompt, neg_prompt, use_grad, to_plot=False):
        """`Trainer.py:1657-1680`: BERT embeddings -> text adapter -> mean over prompts (unless single prompt / MAX_EMB)."""
        out = []
        with torch.set_grad_enabled(use_grad):
            for prompt in (pos_prompt, neg_prompt):
                e = self._bert_embed(prompt)
                if self._has_txt:
                    e = self.text_adapter(e)
                assert e.shape[0] == len(prompt)
                if (not self.basic_prompts and not MAX_EMB) or to_plot:
                    e = Fh.group_mean(e, 1, e.shape[0]).reshape(-1)
                out.append(e)
        return out[0], out[1]

    def myCosineSimilarity(self, x, y, use_grad, to_plot=False, train=False, pos=None):
        """`Trainer.py:1682-1704`: torchmetrics pairwise cosine of x [B,128] against y ([128] -> [1,128], or the
        un-averaged prompt set when MAX_EMB: max over prompts)."""
        with torch.set_grad_enabled(use_grad):
            if to_plot:
                return Fh.pairwise_cosine_similarity(x.reshape(1, -1), y.reshape(1, -1))
            if not MAX_EMB:
                return Fh.pairwise_cosine_similarity(x, y.reshape(1, -1))
            res, res_mean, _ = Fh.pairwise_cosine_max(x, y.reshape(-1, x.shape[1]), 1)
            res, res_mean = res.reshape(-1), res_mean.reshape(-1)
            if train and self.writer is not None:
                gap = float((res.detach().double() - res_mean.double()).mean())   # one scalar for the log, off the gradient path
                if pos:
                    self.pos_mean_counter += 1
                    self.writer.add_scalar("max-mean-comparison/pos", gap, self.pos_mean_counter)
                else:
                    self.neg_mean_counter += 1
                    self.writer.add_scalar("max-mean-comparison/neg", gap, self.neg_mean_counter)
            return res

    def _prompt_matrix(self, class_names: Sequence[str], use_grad: bool) -> torch.Tensor:
        """[2C,128]: row 2c / 2c+1 = positive / negative prompt vector of class c after the text adapter and the
        mean over prompts — the whole per-class loop of `Trainer.py:557-567` in three launches."""
        groups, n = [], None
        for c in class_names:
            pos = self.prompts[c]["positive"]
            neg = self.prompts[c]["negative"] if TRAIN_LOGIT_DIFF else self.prompts[c]["positive"]
            for pr in (pos, neg):
                if n is None:
                    n = len(pr)
                if len(pr) != n:
                    return None  # ragged prompt sets: caller falls back to the per-class path
                groups.append(self._bert_embed(pr))
        with torch.set_grad_enabled(use_grad):
            e = torch.cat(groups, dim=0)
            if self._has_txt:
                e = self.text_adapter(e)
            if MAX_EMB:
                return e   # [2C*n,128]: the max over each group's n prompts is taken on the cosines (`Trainer.py:1691-1693`)
            return Fh.group_mean(e, len(groups), n) if n > 1 else e

    def _logits_and_loss(self, new_embs, labels, class_names, criterion, use_grad):
        """logits [B,C] (+ loss).  Fast path: fused cosine + BCE kernels; otherwise the reference's per-class loop."""
        pm = self._prompt_matrix(class_names, use_grad)
        with torch.set_grad_enabled(use_grad):
            if pm is not None:
                if MAX_EMB:
                    cos, cos_mean, _ = Fh.pairwise_cosine_max(new_embs, pm, 2 * len(class_names))
                    if use_grad and self.writer is not None:   # the reference's per-call log (`Trainer.py:1694-1703`)
                        gap = (cos.detach().double() - cos_mean.double()).mean(0).tolist()
                        for g, v in enumerate(gap):
                            tag, ctr = ("pos", "pos_mean_counter") if g % 2 == 0 else ("neg", "neg_mean_counter")
                            setattr(self, ctr, getattr(self, ctr) + 1)
                            self.writer.add_scalar("max-mean-comparison/" + tag, v, getattr(self, ctr))
                else:
                    cos = Fh.pairwise_cosine_similarity(new_embs, pm)
                # the fused loss + gradient kernel serves `nn.BCEWithLogitsLoss` with reduction "mean" (the reference's criterion) or
                # "sum"; per-element weights, pos_weight, reduction "none" or any other criterion module are applied to the logits
                # tensor as the caller's module defines them
                fused = (type(criterion) is nn.BCEWithLogitsLoss and criterion.weight is None
                         and criterion.pos_weight is None and criterion.reduction in ("mean", "sum") and not self.change_labels)
                if fused:
                    lab = labels if labels.dim() == 2 else labels.unsqueeze(1)
                    loss, logits = Fh.posneg_bce_loss(cos, lab, TRAIN_LOGIT_DIFF, criterion.reduction)
                    if labels.dim() == 1:
                        logits = logits.reshape(-1)
                    return logits, loss, cos
                logits = (cos[:, 0::2] - cos[:, 1::2]) if TRAIN_LOGIT_DIFF else cos[:, 0::2]
            else:
                cols, cosl = [], []
                for c in class_names:
                    pos = self.prompts[c]["positive"]
                    neg = self.prompts[c]["negative"] if TRAIN_LOGIT_DIFF else pos
                    pe, ne = self.bert_forward_mean(pos, neg, use_grad=use_grad)
                    ps = self.myCosineSimilarity(new_embs, pe, use_grad=use_grad, train=use_grad, pos=True)
                    ns = self.myCosineSimilarity(new_embs, ne, use_grad=use_grad, train=use_grad, pos=False)
                    cols.append(ps.flatten() - ns.flatten() if TRAIN_LOGIT_DIFF else ps.flatten())
                    cosl += [ps.flatten(), ns.flatten()]
                logits = torch.stack(cols, dim=1)
                cos = torch.stack(cosl, dim=1)
            if labels.dim() == 1:
                logits = logits.reshape(-1)
            lab = change_values(labels) if self.change_labels else labels
            loss = criterion(logits, lab) if criterion is not None else None
            return logits, loss, cos

    # ------------------------------------------------------------------------------------------------ hot loops
    def _set_mode(self, train: bool):
        """adapters follow the loop (`Trainer.py:533-535,779-782`); in joint mode the encoders stay in eval mode throughout —
        BatchNorm on running statistics, dropout off (parameters still get gradients) -- except a text model that opted in to dropout
        (`CXRBertModel.enable_dropout_`, drivers `--text-dropout`): it trains in train mode and scores in eval mode"""
        for m in (self.image_adapter, self.text_adapter):
            if m is not None:
                m.train(train)
        if self._joint is not None and getattr(self.bert_encoder.model, "dropout_enabled", False):
            self.bert_encoder.model.train(train)

    def _shard(self, n: int):
        """this rank's contiguous row range of a global batch of n rows (tensor_split boundaries)"""
        return (self.rank * n) // self.world, ((self.rank + 1) * n) // self.world

    def _train_step(self, batch, class_names, criterion, label_cols=None):
        """One optimisation step on one loader batch.  Reference form: batch = (embs, labels), `label_cols` picks the label
        column(s) of the task.  Joint form: batch = (images, input_ids, attention_mask[, labels])."""
        if self.loss_name != "standard":
            raise Exception
        if self._joint is not None:
            return self._joint_step(batch)
        embs, labels = batch
        if label_cols is not None:
            labels = labels[:, label_cols]
        n = embs.shape[0]
        lo, hi = self._shard(n) if self.world > 1 else (0, n)
        self.optimizer.zero_grad()
        if hi > lo:
            embs = embs[lo:hi].to(self.device, non_blocking=True)
            labels = labels[lo:hi].to(self.device, non_blocking=True)
            new_embs = self.image_adapter(embs) if self._has_img else embs
            logits, loss, _ = self._logits_and_loss(new_embs, labels, class_names, criterion, use_grad=True)
            loss.backward()
        else:   # a ragged last batch with fewer rows than ranks: this rank contributes nothing, but takes part in the collectives
            loss = torch.zeros((), dtype=torch.float32, device=self.device)
        if self.world > 1:
            # mean over the GLOBAL batch = sum over ranks of (rows of the shard / rows of the batch) x shard mean
            import torch.distributed as dist
            w = (hi - lo) / float(n)
            self.optimizer.all_reduce_grads(self.group, pre_scale=w)
            loss = K.scale_mask(loss.detach().reshape(1), alpha=w).reshape(())
            dist.all_reduce(loss, group=self.group)
        self.optimizer.step()
        return loss.detach()

    def _joint_step(self, batch):
        """The north-star step on one batch `(images, input_ids, attention_mask[, labels])`: this rank's row shard through both
        encoders, InfoNCE over the global batch, backward, gradient all-reduce, fused optimiser step.  With
        `joint_encoders={..., "positives": "labels" | "text"}` the pairs' keys are hashed from the shard's host tensors (the labels
        need not go to the device) and the loss is the multi-positive one."""
        images, ids, mask, keys = self._joint_shard(batch)
        loss = self._joint.step(images, ids, mask, keys=keys)
        self._bert_cache.clear()
        return loss

    def _joint_shard(self, batch, who="joint-encoder training"):
        """A loader batch `(images, input_ids, attention_mask[, labels])` -> this rank's rows of it, on the device, and their keys:
        (images, input_ids, attention_mask, keys or None).  The keys (`pair_keys`: None unless the joint trainer has positives) are
        hashed once, where the loader left the tensors.  `who` names the caller in the refusals of a short batch and of rows that do
        not divide over the ranks.  The first tensor is cut and moved whatever it holds: evaluation passes the image embeddings it
        already has."""
        positives = self._joint.positives
        if len(batch) < 3:
            raise ValueError(f"{who} expects loaders that yield (images, input_ids, attention_mask[, labels]); got a batch of "
                             f"{len(batch)} tensors")
        if positives == "labels" and len(batch) < 4:
            raise ValueError(f"{who} with positives='labels' needs the labels: the loader must yield (images, input_ids, "
                             f"attention_mask, labels [B, C]); got a batch of {len(batch)} tensors")
        n = batch[0].shape[0]
        if self.world > 1 and n % self.world:
            raise ValueError(f"{who} shards the batch evenly: {n} rows over {self.world} ranks (use drop_last)")
        lo, hi = self._shard(n) if self.world > 1 else (0, n)
        images, ids, mask = (t[lo:hi] for t in batch[:3])
        keys = self._joint.pair_keys(ids, mask, batch[3][lo:hi] if positives == "labels" else None)
        return (*(t.to(self.device, non_blocking=True) for t in (images, ids, mask)), keys)

    def train(self, train_loader, criterion, epoch, CONTINUAL_LEARNING=None, threshold=None, scheduler=None, part=None,
              epochs=None, actual_task=None):
        """One epoch of joint / data-incremental training (`Trainer.py:526-606`)."""
        batch_idx = 0
        iteration = 0
        self._set_mode(True)
        cl = CONTINUAL_LEARNING == "myCL" and actual_task is not None and actual_task > 1
        for batch in train_loader:
            if cl:
                self.model_copy()
            batch_idx += 1
            loss = self._train_step(batch, self.class_names, criterion)
            if part is None:
                iteration = (epoch - 1) * len(train_loader) + batch_idx
            else:
                iteration = (part - 1) * epochs * len(train_loader) + (epoch - 1) * len(train_loader) + batch_idx
            if cl:
                self.myIncremental(threshold, iteration)
            if self.writer is not None:
                self.writer.add_scalar('train/Loss', loss, iteration)
            if scheduler is not None:
                scheduler.step()
                self.writer.add_scalar('train/LR', self.optimizer.param_groups[0]['lr'], iteration)
        if cl:
            self.myIncremental_save_log(iteration)
        self._log_temperature(epoch)

    def train_class_incremental(self, train_loader, criterion, epoch, CONTINUAL_LEARNING=None, threshold=None,
                                current_task=None, last_batch=0, actual_task=None):
        """One epoch on the single label column `current_task` (`Trainer.py:608-680`); returns the running iteration.  (Joint-encoder
        mode: the InfoNCE step has no label columns — the task is defined by what its loader yields, `current_task` only numbers it.)"""
        return self._class_incremental_epoch(train_loader, criterion, epoch, CONTINUAL_LEARNING, threshold, last_batch, actual_task,
                                             [self.class_names[current_task]], current_task)

    def train_class_more_labels_incremental(self, train_loader, criterion, epoch, CONTINUAL_LEARNING=None, threshold=None,
                                            current_task=None, last_batch=0, actual_task=None):
        """One epoch on label columns `[:current_task+1]` (`Trainer.py:682-756`); returns the running iteration.  (Joint-encoder mode:
        as in `train_class_incremental`.)"""
        return self._class_incremental_epoch(train_loader, criterion, epoch, CONTINUAL_LEARNING, threshold, last_batch, actual_task,
                                             self.class_names[:current_task + 1], slice(0, current_task + 1))

    def _class_incremental_epoch(self, train_loader, criterion, epoch, CONTINUAL_LEARNING, threshold, last_batch, actual_task, names,
                                 label_cols):
        """the epoch loop of the two class-incremental schedules: they differ in the classes `names` and the label columns of a task"""
        batch_idx = last_batch
        self._set_mode(True)
        cl = CONTINUAL_LEARNING == "myCL" and actual_task is not None and actual_task > 1
        for batch in train_loader:
            if cl:
                self.model_copy()
            batch_idx += 1
            loss = self._train_step(batch, names, criterion, label_cols=label_cols)
            if cl:
                self.myIncremental(threshold, batch_idx)
            if self.writer is not None:
                self.writer.add_scalar('train/Loss', loss, batch_idx)
        if cl:
            self.myIncremental_save_log(batch_idx)
        self._log_temperature(epoch)
        return batch_idx

    def _log_temperature(self, epoch):
        """the learned temperature, once per epoch (the one read-back of the logit scale; never inside the step loop)"""
        if self._joint is not None and self._joint.logit_scale is not None and self.writer is not None:
            self.writer.add_scalar('train/temperature', self._joint.current_temperature(), epoch)
            if self._joint.logit_bias is not None:
                self.writer.add_scalar('train/bias', self._joint.current_bias(), epoch)
        self._log_optimiser(epoch)

    def _log_optimiser(self, epoch):
        """with "optim": "adamw" or a learning-rate schedule: the learning rate of the epoch's last step, and with "max_grad_norm" that
        step's gradient norm before clipping (the one read-back of the norm), once per epoch; with "mlm_weight" the masked-language-
        modelling loss and accuracy of the epoch's last step"""
        # None without "mlm_weight" and before the first masked step; data parallel it all-reduces, so every rank asks, writer or not
        mlm = self._joint.current_mlm() if self._joint is not None else None
        if self._joint is None or self.writer is None:
            return
        opt = self._joint.optimizer
        adamw = isinstance(opt, cxr_optim.AdamW)
        if adamw or self._joint.schedule is not None:
            self.writer.add_scalar('train/lr', opt.lr, epoch)
        if adamw and opt.max_grad_norm is not None and opt.steps > 0:
            self.writer.add_scalar('train/grad_norm', opt.current_grad_norm(), epoch)
        penalty = self._joint.current_penalty()     # None without "ewc_lambda" and before the first penalised step
        if penalty is not None:
            self.writer.add_scalar('train/ewc_penalty', penalty, epoch)
        distill = self._joint.current_distill()     # None without a teacher and before the first distilled step
        if distill is not None:
            self.writer.add_scalar('train/distill', distill, epoch)
        if mlm is not None:
            self.writer.add_scalar('train/mlm_loss', mlm["loss"], epoch)
            self.writer.add_scalar('train/mlm_acc', mlm["accuracy"], epoch)
        agem = self._joint.current_interference()   # None without "agem_memory" and before the first step with a reference
        if agem is not None:
            proj, applied = agem["projected"] - self._agem_logged[0], agem["applied"] - self._agem_logged[1]
            self._agem_logged = (agem["projected"], agem["applied"])
            if applied > 0:                         # the fraction of this epoch's steps whose gradient was projected
                self.writer.add_scalar('train/agem_projected', proj / applied, epoch)
                self.writer.add_scalar('train/agem_dot', agem["dot"], epoch)
        ema = self._joint.current_ema()             # None without "ema_decay"; host numbers, no read-back
        if ema is not None and ema["last_decay"] is not None:
            self.writer.add_scalar('train/ema_decay', ema["last_decay"], epoch)

    @staticmethod
    def _parse_retrieval(opt):
        """the "retrieval" entry of `joint_encoders`: None / False -> off (None), True -> Recall@1/5/10, a sequence of positive
        integers -> those cut-offs"""
        if opt is None or opt is False:
            return None
        if opt is True:
            return RETRIEVAL_KS
        if isinstance(opt, int):
            opt = (opt,)
        return check_ks(opt)

    def _retrieval_collect(self, acc, batch, new_embs):
        """one evaluation batch of the retrieval set: this rank's shard of the image embeddings `_eval_loop` already has, and the
        paired reports through the text encoder (under no_grad, eval mode: no dropout, no augmentation)"""
        embs, ids, mask, keys = self._joint_shard((new_embs,) + tuple(batch[1:]), "retrieval evaluation")
        acc[0].append(embs)
        acc[1].append(self.bert_encoder.model.get_projected_text_embeddings(ids, mask, normalize_embeddings=False))
        if keys is not None:
            acc[2].append(keys.to(self.device))

    def _retrieval_finish(self, acc):
        if not acc[0]:
            return None
        return retrieval_metrics(torch.cat(acc[0]).contiguous(), torch.cat(acc[1]).contiguous(),
                                 torch.cat(acc[2]).contiguous() if acc[2] else None, self._retrieval_ks, self._joint._dist_group())

    def _add_retrieval(self, m, val_test, epoch):
        """`Retrieval/i2t R@1` ... `Retrieval/t2i n` of the last `_eval_loop`, into the returned dict and the writer"""
        res, self._retrieval_result = self._retrieval_result, None
        if res is None:
            return m
        for direction, d in res.items():
            for k, v in d.items():
                m[f"Retrieval/{direction} {k}"] = v
                if self.writer is not None:
                    self.writer.add_scalar(f"{val_test}/Retrieval/{direction} {k}", v, epoch)
        return m

    # ------------------------------------------------------------------------------------------------ kNN label probe
    @torch.no_grad()
    def knn_bank(self, loaders) -> int:
        """Fill the memory of the kNN probe (needs `joint_encoders={..., "knn": ...}`): re-embed up to "bank_batches" batches of each
        loader in `loaders` (one loader or a sequence of them, yielding `(images, input_ids, attention_mask, labels)`) with the image
        encoder on the weights `_eval_weights` chooses (so "ema_eval" applies), every rank its shard of each batch as `_joint_shard`
        cuts it, then gather the rows and labels of all ranks (`KNNBank.finish`) -> the bank's rows.  It replaces an earlier bank.
        From then on `val` / `test` add the kNN/* metrics.  No training state moves.  Every rank calls it."""
        if self._joint is None or self._knn is None:
            raise ValueError("Trainer.knn_bank needs joint_encoders={..., 'knn': True | {'k': ..., 'temperature': ..., 'bank_batches': ...}}")
        def is_batch(b):
            return isinstance(b, (list, tuple)) and len(b) > 0 and isinstance(b[0], torch.Tensor)

        if not isinstance(loaders, (list, tuple)) or (len(loaders) > 0 and is_batch(loaders[0])):      # one loader (a list of batches is one)
            loaders = (loaders,)
        bank = KNNBank()
        with self._eval_weights():
            self._set_mode(False)
            for loader in loaders:
                for n, batch in enumerate(loader):
                    if n >= self._knn["bank_batches"]:
                        break
                    if len(batch) < 4:
                        raise ValueError("Trainer.knn_bank needs (images, input_ids, attention_mask, labels) batches, got a batch of "
                                         f"{len(batch)} tensors")
                    images = self._joint_shard(batch, "Trainer.knn_bank")[0]
                    lo, hi = self._shard(batch[0].shape[0]) if self.world > 1 else (0, batch[0].shape[0])
                    bank.add(self.image_model(images), batch[-1][lo:hi].to(self.device))
            self._knn_bank = bank.finish(self._joint._dist_group())
        return len(self._knn_bank)

    def _knn_vote(self, new_embs, labels):
        """the vote of one evaluation batch on the image embeddings `_eval_batches` already has -> host scores [B, C]"""
        bank = self._knn_bank
        if labels.dim() != 2 or labels.shape[1] != bank.width:
            raise ValueError(f"kNN evaluation: the bank's labels are {bank.width} wide but the evaluation labels "
                             f"{labels.shape[-1] if labels.dim() else 0} (build the bank from loaders of the same label set)")
        return bank.predict(new_embs, self._knn["k"], self._knn["temperature"]).cpu().numpy()

    def _add_knn(self, m, y_true, val_test, epoch):
        """`kNN/Accuracy` ... `kNN/AUROC-weighted` of the last `_eval_loop`, computed as `evaluate_model` computes its own (a
        prediction is score > 0.5), into the returned dict and the writer"""
        score, self._knn_result = getattr(self, "_knn_result", None), None
        if score is None:
            return m
        from sklearn.metrics import accuracy_score, f1_score, roc_auc_score
        pred = (score > 0.5).astype(np.float32)
        km = {"kNN/Accuracy": accuracy_score(y_true, pred), "kNN/F1-macro": f1_score(y_true, pred, average="macro", zero_division=0)}
        try:
            km["kNN/AUROC-macro"] = roc_auc_score(y_true, score, average="macro", multi_class="ovr")
            km["kNN/AUROC-weighted"] = roc_auc_score(y_true, score, average="weighted", multi_class="ovr")
        except ValueError:  # a class without both labels in a tiny synthetic split (or a NaN score)
            pass
        for k, v in km.items():
            m[k] = v
            if self.writer is not None:
                self.writer.add_scalar(val_test + "/" + k, v, epoch)
        return m

    @contextlib.contextmanager
    def _eval_weights(self):
        """the weights an evaluation reads: with `"ema_eval": True` the parameter average (`JointContrastiveTrainer.averaged()`,
        DESIGN.md §5.14), else the parameters as they are.  The cached prompt embeddings belong to the weights they were made with:
        the cache is emptied on entry and on exit."""
        if self._joint is None or not getattr(self._joint, "ema_eval", False):
            yield
            return
        self._bert_cache.clear()
        try:
            with self._joint.averaged():
                yield
        finally:
            self._bert_cache.clear()

    @torch.no_grad()
    def _eval_loop(self, loader, criterion, epoch, log_tag):
        with self._eval_weights():
            return self._eval_batches(loader, criterion, epoch, log_tag)

    def _eval_batches(self, loader, criterion, epoch, log_tag):
        """the body of `_eval_loop` (the retrieval evaluation included), under no_grad and on the weights `_eval_weights` chose"""
        self._set_mode(False)
        y_true, y_pred, y_score = [], [], []
        batch_idx = 0
        acc = ([], [], []) if self._joint is not None and self._retrieval_ks is not None else None
        knn = [] if getattr(self, "_knn_bank", None) is not None else None      # (a bank exists only in joint mode with "knn")
        for batch in loader:
            batch_idx += 1
            labels = batch[-1].to(self.device)
            if self._joint is not None:
                if len(batch) < 4:
                    raise ValueError("joint-encoder evaluation needs (images, input_ids, attention_mask, labels) batches")
                new_embs = self.image_model(batch[0].to(self.device))   # (under no_grad: the whole loop is)
                if acc is not None:
                    self._retrieval_collect(acc, batch, new_embs)
                if knn is not None:
                    knn.append(self._knn_vote(new_embs, labels))
            else:
                embs = batch[0].to(self.device)
                new_embs = self.image_adapter(embs) if self._has_img else embs
            logits, loss, cos = self._logits_and_loss(new_embs, labels, self.class_names, criterion, use_grad=False)
            if cos.shape[1] == 2 * len(self.class_names) and TRAIN_LOGIT_DIFF:
                score, pred = K.eval_score(cos.contiguous(), PRED_LOGIT_DIFF)
            else:
                cp, cn = cos[:, 0::2], cos[:, 1::2]
                score = (cp - cn + 2) / 4 if PRED_LOGIT_DIFF else (cp + 1) / 2
                pred = (cp > cn).float()
            if loss is not None and self.writer is not None and log_tag:
                self.writer.add_scalar(log_tag + '/Loss', loss, (epoch - 1) * len(loader) + batch_idx)
            y_true.append(labels.cpu().numpy())
            y_pred.append(pred.cpu().numpy())
            y_score.append(score.cpu().numpy())
        self._retrieval_result = self._retrieval_finish(acc) if acc is not None else None
        self._knn_result = np.concatenate(knn) if knn else None
        return np.concatenate(y_true), np.concatenate(y_pred), np.concatenate(y_score)

    def val(self, val_loader, criterion, epoch, epochs, mode="joint", tasks_order=None):
        """`Trainer.py:773-866`: scores (pos+1)/2 or (pos-neg+2)/4, predictions argmax([neg,pos]), BCE logged."""
        y_true, y_pred, y_score = self._eval_loop(val_loader, criterion, epoch, "val")
        m = self._add_retrieval(self.evaluate_model(y_true, y_pred, y_score, mode, epoch, "val", epochs, tasks_order), "val", epoch)
        return self._add_knn(m, y_true, "val", epoch)

    def test(self, test_loader, criterion, epoch, epochs, mode="joint", tasks_order=None, plot_tsne_array=None):
        """`Trainer.py:989-1062` (the t-SNE / heat-map plots that follow there are out of scope)."""
        y_true, y_pred, y_score = self._eval_loop(test_loader, None, epoch, None)
        m = self._add_retrieval(self.evaluate_model(y_true, y_pred, y_score, mode, epoch, "test", epochs, tasks_order), "test", epoch)
        return self._add_knn(m, y_true, "test", epoch)

    @torch.no_grad()
    def evaluate_model(self, y_true, y_pred, y_score, mode, epoch, val_test, epochs, tasks_order):
        """Scalar metrics of `Trainer.py:869-905` (host-side sklearn); returns them as a dict."""
        from sklearn.metrics import accuracy_score, f1_score, roc_auc_score
        m = {"Accuracy": accuracy_score(y_true, y_pred),
             "F1-macro score": f1_score(y_true, y_pred, average="macro", zero_division=0),
             "F1-weighted score": f1_score(y_true, y_pred, average="weighted", zero_division=0)}
        try:
            m["AUROC-macro"] = roc_auc_score(y_true, y_score, average="macro", multi_class="ovr")
            m["AUROC-weighted"] = roc_auc_score(y_true, y_score, average="weighted", multi_class="ovr")
        except ValueError:  # a class without both labels in a tiny synthetic split
            pass
        if self.writer is not None:
            for k, v in m.items():
                self.writer.add_scalar(val_test + "/" + k, v, epoch)
        return m

    # ------------------------------------------------------------------------------------------------ continual learning
    def consolidate(self, loader) -> int:
        """End of a task with `joint_encoders={..., "ewc_lambda": s}`: the encoders in evaluation mode, each batch of
        `loader` sharded as in `_joint_step`, at most "ewc_batches" of them -> `JointContrastiveTrainer.consolidate`; returns the
        number of batches read.  Every rank calls it, as it calls the training loop."""
        if self._joint is None or self._joint.ewc is None:
            raise ValueError("Trainer.consolidate needs joint_encoders={..., 'ewc_lambda': strength}")
        self._set_mode(False)
        return self._joint.consolidate(self._joint_shards(loader, "consolidate"), max_batches=self._ewc_batches)

    def _joint_shards(self, loader, what):
        """this rank's shard of every batch of `loader`, on the device, cut as `_joint_step` cuts it (with its keys when the trainer
        has positives)"""
        for batch in loader:
            shard = self._joint_shard(batch, f"Trainer.{what}")
            yield shard if shard[3] is not None else shard[:3]

    def end_task(self, loader) -> None:
        """The task boundary of the incremental schedules: after a task that another one follows, whatever the joint trainer was
        configured with, in this order -- `consolidate(loader)` ("ewc_lambda"), `snapshot_teacher()` ("distill_weight"),
        `remember(loader)` ("agem_memory").  `loader` is the finished task's.  Nothing in adapter mode.  Every rank calls it."""
        if self._joint is None:
            return
        if self._joint.ewc is not None:               # anchor this task before the next one starts
            self.consolidate(loader)
        if self._joint.distill_weight is not None:    # this task's encoders teach the next one
            self.snapshot_teacher()
        if self._joint.memory is not None:            # rows of this task constrain the next one's updates
            self.remember(loader)

    def remember(self, loader) -> int:
        """End of a task with `joint_encoders={..., "agem_memory": M}`: each batch of `loader` sharded as in
        `_joint_step` -> `JointContrastiveTrainer.remember`, which keeps M of this rank's rows; returns the rows stored.  Every rank
        calls it, as it calls the training loop."""
        if self._joint is None or self._joint.memory is None:
            raise ValueError("Trainer.remember needs joint_encoders={..., 'agem_memory': rows}")
        return self._joint.remember(self._joint_shards(loader, "remember"))

    def snapshot_teacher(self) -> None:
        """End of a task with `joint_encoders={..., "distill_weight": beta}`: freeze the current encoders as the
        teacher of the tasks that follow (`JointContrastiveTrainer.snapshot_teacher`).  Every rank calls it, as it calls the training
        loop."""
        if self._joint is None or self._joint.distill_weight is None:
            raise ValueError("Trainer.snapshot_teacher needs joint_encoders={..., 'distill_weight': beta}")
        self._joint.snapshot_teacher()

    @torch.no_grad()
    def model_copy(self):
        """Snapshot the adapters before a step (`Trainer.py:1634-1641`)."""
        if self._has_img:
            self.image_adapter_copy = [p.detach().clone() for p in self.image_adapter.parameters()]
        if self._has_txt:
            self.text_adapter_copy = [p.detach().clone() for p in self.text_adapter.parameters()]
        if self._joint is not None:   # both encoders: one copy of the flat parameter buffer (0.5 GB)
            self._flat_copy = self.optimizer.flat_p.detach().clone()
        self.n_reset = 0
        self.n_updated = 0
        self._reset_counters.zero_()
        self._reset_total = 0

    @torch.no_grad()
    def _weight_reset(self, threshold):
        for mod, snap in ((self.image_adapter, self.image_adapter_copy), (self.text_adapter, self.text_adapter_copy)):
            if mod is None or snap is None:
                continue
            for p, old in zip(mod.parameters(), snap):
                K.weight_reset(p.data, old, threshold, self._reset_counters)
                self._reset_total += p.numel()
        if self._joint is not None and self._flat_copy is not None:
            # per parameter tensor, as in the reference: each tensor is one gap-free slice of the flat buffer and of its copy
            flat, base = self.optimizer.flat_p, self.optimizer.flat_p.data_ptr()
            for p in self.optimizer.params:
                o, n = (p.data_ptr() - base) // 4, p.numel()
                if p is self._joint.logit_scale or p is self._joint.logit_bias:
                    # one element: min = max of |new - old|, so `d < min + threshold * (max - min)` never holds and the learned
                    # temperature (or the sigmoid loss's bias) is never restored; said here instead of left to that arithmetic, and
                    # counted as updated
                    self._reset_total += n
                    continue
                K.weight_reset(flat[o:o + n], self._flat_copy[o:o + n], threshold, self._reset_counters)
                self._reset_total += n

    @torch.no_grad()
    def myIncremental(self, threshold, iteration):
        """`Trainer.py:1556-1587`: per tensor, restore entries whose |new-old| < min + threshold*(max-min)."""
        self._weight_reset(threshold)

    @torch.no_grad()
    def _reset_stats(self):
        n_reset = int(self._reset_counters[0].item())
        return n_reset, self._reset_total - n_reset

    @torch.no_grad()
    def myIncremental_save_log(self, iteration):
        self.n_reset, self.n_updated = self._reset_stats()
        tot = max(1, self.n_reset + self.n_updated)
        print("\nnumber of resets:", self.n_reset, "number of updates:", self.n_updated, "percentage resets", self.n_reset / tot)
        if self.writer is not None:
            self.writer.add_scalar("monitor-resets/resets", self.n_reset, iteration)
            self.writer.add_scalar("monitor-resets/updates", self.n_updated, iteration)
            self.writer.add_scalar("monitor-resets/percentage resets", self.n_reset / tot, iteration)

    @torch.no_grad()
    def profIncremental(self, epoch, epochs, actual_task, threshold):
        """`Trainer.py:1589-1632`: the same reset applied once per epoch, then counters logged and cleared."""
        self._weight_reset(threshold)
        self.myIncremental_save_log((actual_task - 1) * epochs + epoch)
        self.n_reset = 0
        self.n_updated = 0
        self._reset_counters.zero_()
        self._reset_total = 0

    # ------------------------------------------------------------------------------------------------ checkpoint
    @torch.no_grad()
    def save(self):
        """`Trainer.py:1643-1648`: the adapters into the writer's log dir under the reference's file names.  The reference pickles
        the whole module; here the file holds the module's state dict (tensors only), so that `load` — like every other loader of
        this package — can run with `weights_only=True`."""
        if self._has_img:
            torch.save(self.image_adapter.state_dict(), os.path.join(self.writer.log_dir, 'image_adapter.pt'))
        if self._has_txt:
            torch.save(self.text_adapter.state_dict(), os.path.join(self.writer.log_dir, 'text_adapter.pt'))
        if self._joint is not None and self.rank == 0:
            torch.save(self.image_model.state_dict(), os.path.join(self.writer.log_dir, 'image_model.pt'))
            torch.save(self.bert_encoder.model.state_dict(), os.path.join(self.writer.log_dir, 'text_model.pt'))
            if self._joint.logit_scale is not None:
                sd = {"logit_scale": self._joint.logit_scale.detach().cpu()}
                if self._joint.logit_bias is not None:
                    sd["logit_bias"] = self._joint.logit_bias.detach().cpu()
                torch.save(sd, os.path.join(self.writer.log_dir, 'logit_scale.pt'))
            if self._joint.ewc is not None:
                torch.save(self._joint.ewc.state_dict(), os.path.join(self.writer.log_dir, 'ewc.pt'))
            if self._joint.teacher is not None:
                torch.save(self._joint.teacher.state_dict(), os.path.join(self.writer.log_dir, 'teacher.pt'))
            if self._joint.mlm_state is not None:   # plain numbers: the masking stream resumes where it stopped
                seed, counter = self._joint.mlm_state
                torch.save({"seed": int(seed), "counter": int(counter)}, os.path.join(self.writer.log_dir, 'mlm.pt'))
            if self._joint.ema is not None:         # the model files above stay the raw weights; the average travels on its own
                torch.save(self._joint.ema.state_dict(), os.path.join(self.writer.log_dir, 'ema.pt'))
        if self._joint is not None and self._joint.memory is not None:   # every rank holds rows of its own shards
            torch.save({"memory": self._joint.memory.state_dict(), "agem": self._joint.agem.state_dict(),
                        "steps": int(self._joint.agem_steps)}, os.path.join(self.writer.log_dir, self._agem_file()))
        if hasattr(self.writer, "flush"):
            self.writer.flush()

    def _agem_file(self) -> str:
        return 'agem.pt' if self.rank == 0 else f'agem.rank{self.rank}.pt'

    @torch.no_grad()
    def load(self):
        """Counterpart of `save` (the reference's `load`, `Trainer.py:1650-1655`, mistakenly calls `torch.save` for the text
        adapter).  Files are opened with `weights_only=True`: a pickled module, as the reference writes, is refused."""
        for has, mod, name in ((self._has_img, self.image_adapter, 'image_adapter.pt'), (self._has_txt, self.text_adapter, 'text_adapter.pt')):
            if has:
                path = os.path.join(self.writer.log_dir, name)
                try:
                    sd = torch.load(path, map_location="cpu", weights_only=True)
                except Exception as e:   # a whole-module pickle, as the reference's save() writes (Trainer.py:1646-1648)
                    raise ValueError(f"{path}: not a tensors-only state dict ({type(e).__name__}).  This package stores "
                                     f"`module.state_dict()` under the reference's file names and opens files with weights_only=True; "
                                     f"a file written by the reference's Trainer.save() is a pickled `models.myMLP` module — convert it "
                                     f"in the reference environment (INTEGRATION.md, 'Adapter checkpoints') before loading it here") from e
                if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
                    raise ValueError(f"{path}: expected a state dict of tensors (see INTEGRATION.md, 'Adapter checkpoints')")
                mod.load_state_dict(sd)
        if self._joint is not None:   # the encoders `save` wrote in joint mode; the flat parameter buffer is updated in place
            for mod, name in ((self.image_model, 'image_model.pt'), (self.bert_encoder.model, 'text_model.pt')):
                sd = torch.load(os.path.join(self.writer.log_dir, name), map_location="cpu", weights_only=True)
                with torch.no_grad():
                    own = mod.state_dict()
                    for k, v in sd.items():
                        own[k].copy_(v)
            if self._joint.logit_scale is not None:
                sd = torch.load(os.path.join(self.writer.log_dir, 'logit_scale.pt'), map_location="cpu", weights_only=True)
                if self._joint.logit_bias is not None and "logit_bias" not in sd:
                    raise ValueError(f"{os.path.join(self.writer.log_dir, 'logit_scale.pt')}: no 'logit_bias' entry; this trainer learns "
                                     f"the sigmoid loss's bias with the logit scale (the file was written by an InfoNCE run)")
                self._joint.logit_scale.data.copy_(sd["logit_scale"].reshape(1))
                if self._joint.logit_bias is not None:
                    self._joint.logit_bias.data.copy_(sd["logit_bias"].reshape(1))
            if self._joint.ewc is not None:   # keys, fisher kind and the size of F / anchor are checked by `EWC.load_state_dict`
                self._joint.ewc.load_state_dict(torch.load(os.path.join(self.writer.log_dir, 'ewc.pt'), map_location="cpu", weights_only=True))
            tpath = os.path.join(self.writer.log_dir, 'teacher.pt')
            if self._joint.distill_weight is not None and os.path.exists(tpath):
                # (a run saved before its first snapshot wrote no file and has no teacher.)  The copies are built from the encoders
                # just loaded, then take the saved tensors; size and keys are checked by `FrozenTeacher.load_state_dict`
                self._joint.snapshot_teacher()
                self._joint.teacher.load_state_dict(torch.load(tpath, map_location="cpu", weights_only=True))
            if self._joint.ema is not None:   # keys, decay, warmup and the size of avg are checked by `EMA.load_state_dict`; with
                # "ema_teacher" the teacher's flat copy IS avg: this load and the one above land in the same storage
                self._joint.ema.load_state_dict(torch.load(os.path.join(self.writer.log_dir, 'ema.pt'), map_location="cpu", weights_only=True))
            if self._joint.mlm_state is not None:
                path = os.path.join(self.writer.log_dir, 'mlm.pt')
                sd = torch.load(path, map_location="cpu", weights_only=True)
                if not isinstance(sd, dict) or set(sd) != {"seed", "counter"} or int(sd["counter"]) < 0 or int(sd["seed"]) < 0:
                    raise ValueError(f"{path}: expected the keys ['counter', 'seed'] with both >= 0")
                self._joint.mlm_state = (int(sd["seed"]), int(sd["counter"]))
            if self._joint.memory is not None:   # the memory, the projection's counters and the sampler's step counter
                path = os.path.join(self.writer.log_dir, self._agem_file())
                sd = torch.load(path, map_location="cpu", weights_only=True)
                if not isinstance(sd, dict) or set(sd) != {"memory", "agem", "steps"} or int(sd["steps"]) < 0:
                    raise ValueError(f"{path}: expected the keys ['agem', 'memory', 'steps'] with steps >= 0")
                self._joint.memory.load_state_dict(sd["memory"], device=self.device)
                self._joint.agem.load_state_dict(sd["agem"])
                self._joint.agem_steps = int(sd["steps"])
                self._agem_logged = (int(sd["agem"]["stats"][3]), int(sd["agem"]["applied"]))
            self._bert_cache.clear()
