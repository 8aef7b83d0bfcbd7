"""Driver loops with the same schedule as the reference's `ZERO_JOINT_BOUNDS.py:62-72`, `CLASS_INCREMENTAL.py:66-97`
and `DATA_INCREMENTAL.py:74-97` (hyper-parameters as arguments instead of literals; `playsound` dropped).

    python -m incremental_multimodal_medical_learning_ii_amd.drivers zero-joint --epochs 2 --batch-size 1024
    python -m incremental_multimodal_medical_learning_ii_amd.drivers class-inc --more-labels
    python -m incremental_multimodal_medical_learning_ii_amd.drivers data-inc --parts 5

    python -m incremental_multimodal_medical_learning_ii_amd.drivers data-inc --parts 5 --joint --batch-size 1024 --epochs 1
    python -m incremental_multimodal_medical_learning_ii_amd.drivers class-inc --joint --cl ewc --ewc-lambda 1e4 --ewc-batches 8
    python -m incremental_multimodal_medical_learning_ii_amd.drivers data-inc --joint --cl lwf --distill-weight 1.0
    python -m incremental_multimodal_medical_learning_ii_amd.drivers class-inc --joint --cl agem --agem-memory 256
    python -m incremental_multimodal_medical_learning_ii_amd.drivers zero-joint --joint --ema-decay 0.999 --ema-eval
    python -m incremental_multimodal_medical_learning_ii_amd.drivers data-inc --joint --cl lwf --ema-decay 0.995 --ema-teacher
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 --master-port 29511 \
        -m incremental_multimodal_medical_learning_ii_amd.drivers class-inc --mode class-pos-neg --batch-size 2048

Without a pre-computed CheXpert embedding dataset (`--dataset-root`), synthetic loaders of the same shape are used
and CXR-BERT is the synthetic-weight model (`CXRK_SYNTHETIC_WEIGHTS=1` semantics).

`--joint`: the same schedules over the north-star step — both encoders train in-loop on `(images, token ids, mask, labels)`
batches (`Trainer(..., joint_encoders=...)`), evaluation is the zero-shot scoring of the trained encoders.
Under `torch.distributed.run` (WORLD_SIZE > 1) the process group is initialised (RCCL; CXRK_DIST_BACKEND=gloo for one-GPU
rehearsals), `--batch-size` is the GLOBAL batch and every rank trains on its row shard (BASELINE config 4: class-incremental,
global batch 2048 on 4 GPUs)."""
from __future__ import annotations

import argparse
import os
import random

import numpy as np
import torch
from torch import nn

from . import Trainer as TR
from .DataRetrieval import CHEXPERT_COMPETITION_CLASSES, basic_create_prompts, create_prompts


def _seed(seed_value: int = 27):  # the reference fixes every seed to 27 (ZERO_JOINT_BOUNDS.py:9-14)
    torch.manual_seed(seed_value)
    random.seed(seed_value)
    np.random.seed(seed_value)


def _init_distributed():
    """One process per GPU when started by `torch.distributed.run`; returns (rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("CXRK_DIST_BACKEND", "nccl")
        dev_index = int(os.environ.get("CXRK_DRIVER_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
    return dist.get_rank(), dist.get_world_size()


def _joint_models(args, device):
    """Image model + text engine for `--joint`: full ResNet-50 / 12-layer CXR-BERT with synthetic weights (or `--small-text` /
    `--pretrained-*`)."""
    from . import synthetic as syn
    from .health_multimodal import text as T
    from .health_multimodal.image.model import get_biovil_resnet
    im = get_biovil_resnet(args.pretrained_image)
    if args.pretrained_image is None:
        syn.fill_module_(im)
    im = im.eval().to(device)
    if args.small_text:
        cfg = T.CXRBertConfig(vocab_size=2048, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                              max_position_embeddings=64)
        tm = T.CXRBertModel(cfg)
        syn.fill_module_(tm)
        engine = T.TextInferenceEngine(T.SyntheticTokenizer(2048), tm.eval().to(device))
    else:
        engine = T.get_cxr_bert_inference(args.pretrained_text, device="cuda")
    if getattr(args, "text_dropout", False):   # HF train-mode dropout in the training loop (Trainer._set_mode), eval for scoring
        engine.model.enable_dropout_()
    return im, engine


def _setup(args, kind):
    device = torch.device("cuda")
    rank, world = _init_distributed()
    joint = getattr(args, "joint", False)
    if joint and args.dataset_root:
        raise SystemExit("--joint trains on (images, token ids) batches; --dataset-root holds pre-computed embeddings")
    if args.dataset_root:
        if kind == "joint":
            out = TR.Trainer.preprocessing(True, args.xrays_position, args.single_prompt, args.batch_size, args.lr, args.epochs,
                                           "standard", dataset_root=args.dataset_root, log_root=args.log_root)
        elif kind == "class":
            out = TR.Trainer.preprocessing_class_incremental(True, args.xrays_position, args.single_prompt, args.batch_size, args.lr,
                                                             args.epochs, "standard", args.mode, args.cl, True, args.threshold,
                                                             args.threshold_scheduling, args.adder, args.more_labels,
                                                             dataset_root=args.dataset_root, log_root=args.log_root)
        else:
            out = TR.Trainer.preprocessing_data_incremental(True, args.xrays_position, args.single_prompt, args.batch_size, args.lr,
                                                            args.parts, args.epochs, "standard", "data-inc", args.cl, True,
                                                            args.threshold, args.threshold_scheduling, args.adder,
                                                            dataset_root=args.dataset_root, log_root=args.log_root)
        writer, class_names, train_loader, val_loader, test_loader, prompts, _ = out
    else:
        class_names = list(CHEXPERT_COMPETITION_CLASSES)
        prompts = basic_create_prompts(class_names) if args.single_prompt else create_prompts(class_names)
        if joint:
            vocab = 2048 if args.small_text else 30522
            train_loader, val_loader, test_loader = TR.Trainer.synthetic_joint_loaders(
                args.n_train, args.n_eval, args.n_eval, args.batch_size, image_size=args.image_size, seq_len=args.seq_len, vocab=vocab,
                eval_batch_size=min(1024, args.n_eval))
        else:
            train_loader, val_loader, test_loader = TR.Trainer.synthetic_loaders(args.n_train, args.n_eval, args.n_eval, args.batch_size)
        if kind == "class":
            train_loader = (TR.Trainer.split_dataloader_data_incremental(train_loader, 5) if args.mode == "class-pos-neg"
                            else TR.Trainer.split_dataloader_by_label(train_loader, args.batch_size))
        elif kind == "data":
            train_loader = TR.Trainer.split_dataloader_data_incremental(train_loader, args.parts)
        writer = TR._make_writer(os.path.join(args.log_root, "synthetic-" + kind + ("-joint" if joint else "") + (f"-rank{rank}" if world > 1 else "")))
    os.environ.setdefault("CXRK_SYNTHETIC_WEIGHTS", "1" if not args.pretrained_text else "0")
    if joint:
        im, engine = _joint_models(args, device)
        trainer = TR.Trainer(args.single_prompt, prompts, class_names, "standard", args.lr, device, writer, bert_encoder=engine,
                             joint_encoders=joint_encoders_from_args(args, im, kind, train_loader))
    else:
        from .health_multimodal.text import get_cxr_bert_inference
        engine = get_cxr_bert_inference(args.pretrained_text, device="cuda")
        trainer = TR.Trainer(args.single_prompt, prompts, class_names, "standard", args.lr, device, writer, bert_encoder=engine)
    return trainer, writer, train_loader, val_loader, test_loader


def joint_encoders_from_args(args, image_model, kind=None, train_loader=None) -> dict:
    """the `joint_encoders` dict of `--joint`: every flag of the north-star step as the key `Trainer` reads"""
    return {"image_model": image_model, "temperature": args.temperature,
            "positives": {"pair": None}.get(getattr(args, "positives", "pair"), getattr(args, "positives", None)),
            "learn_temperature": bool(getattr(args, "learn_temperature", False)),
            "contrastive_loss": getattr(args, "contrastive_loss", None) or "infonce",
            "sigmoid_bias": getattr(args, "sigmoid_bias", None),
            "micro_batch": getattr(args, "micro_batch", None),
            **optimiser_from_args(args, kind, train_loader),
            **continual_from_args(args),
            **mlm_from_args(args),
            **ema_from_args(args),
            "augment": augment_from_args(args),
            "retrieval": retrieval_from_args(args),
            **knn_from_args(args)}


def mlm_from_args(args) -> dict:
    """`--mlm-weight W [--mlm-probability P] [--mlm-seed S]` -> the `joint_encoders` keys of the masked-language-modelling loss
    (DESIGN.md 5.13); without `--mlm-weight` an empty dict: the keys exist only when their flag is given"""
    if getattr(args, "mlm_weight", None) is None:
        return {}
    return {k: getattr(args, k) for k in ("mlm_weight", "mlm_probability", "mlm_seed") if getattr(args, k, None) is not None}


def ema_from_args(args) -> dict:
    """`--ema-decay D [--ema-no-warmup] [--ema-eval] [--ema-teacher]` -> the `joint_encoders` keys of the parameter average
    (DESIGN.md 5.14); without `--ema-decay` an empty dict: the keys exist only when their flag is given"""
    if getattr(args, "ema_decay", None) is None:
        return {}
    out = {"ema_decay": args.ema_decay}
    if getattr(args, "ema_no_warmup", False):
        out["ema_warmup"] = False
    for flag in ("ema_eval", "ema_teacher"):
        if getattr(args, flag, False):
            out[flag] = True
    return out


def retrieval_from_args(args):
    """`--retrieval [K ...]` -> None (off), True (Recall@1/5/10) or the tuple of cut-offs given"""
    ks = getattr(args, "retrieval", None)
    if ks is None:
        return None
    return True if len(ks) == 0 else tuple(ks)


def knn_from_args(args) -> dict:
    """`--knn [K] [--knn-temperature T] [--knn-bank-batches N]` -> the `joint_encoders` key of the kNN label probe;
    without `--knn` an empty dict: the key exists only when its flag is given"""
    k = getattr(args, "knn", None)
    if k is None:
        return {}
    opt = {} if k is True else {"k": k}
    if getattr(args, "knn_temperature", None) is not None:
        opt["temperature"] = args.knn_temperature
    if getattr(args, "knn_bank_batches", None) is not None:
        opt["bank_batches"] = args.knn_bank_batches
    return {"knn": opt or True}


def knn_bank(trainer, args, loaders) -> None:
    """`--knn`: refill the probe's memory from `loaders` just before a `val` / `test` pair; nothing without the flag"""
    if getattr(args, "knn", None) is not None:
        trainer.knn_bank(loaders)


def run_steps(args, kind, train_loader) -> int:
    """optimiser steps of the whole run: epochs x steps per epoch x tasks (class-inc / data-inc: one loader per task)"""
    loaders = train_loader if isinstance(train_loader, (list, tuple)) else [train_loader]
    return int(args.epochs) * sum(len(ld) for ld in loaders)


def optimiser_from_args(args, kind=None, train_loader=None) -> dict:
    """`--optim adamw` / `--weight-decay` / `--clip-grad-norm` / `--warmup-steps` / `--lr-decay` / `--min-lr-ratio` -> the
    `joint_encoders` keys they set (none of them given: an empty dict).  The schedule spans the whole run, not each task:
    total_steps is derived from the run's own length."""
    out = {}
    if getattr(args, "optim", None) is not None:
        out["optim"] = args.optim
    for flag, key in (("weight_decay", "weight_decay"), ("clip_grad_norm", "max_grad_norm"), ("warmup_steps", "warmup_steps"),
                      ("lr_decay", "lr_decay"), ("min_lr_ratio", "min_lr_ratio")):
        if getattr(args, flag, None) is not None:
            out[key] = getattr(args, flag)
    if any(k in out for k in ("warmup_steps", "lr_decay", "min_lr_ratio")) and train_loader is not None:
        out["total_steps"] = run_steps(args, kind, train_loader)
    return out


EWC_LAMBDA = 1e4         # F is a squared mean gradient, so useful strengths are large
DISTILL_WEIGHT = 1.0     # beta of --cl lwf: the distillation term enters at the weight of the contrastive loss
AGEM_MEMORY = 256        # rows kept per task and rank by --cl agem
# --cl value -> (the master key of its `joint_encoders` group, that key's default, the group's other flags); a flag and the key it
# sets share a name
CONTINUAL = {"ewc": ("ewc_lambda", EWC_LAMBDA, ("ewc_batches", "ewc_gamma", "ewc_fisher")),
             "lwf": ("distill_weight", DISTILL_WEIGHT, ("distill_temperature",)),
             "agem": ("agem_memory", AGEM_MEMORY, ("agem_batch", "agem_every"))}


def continual_from_args(args) -> dict:
    """`--cl ewc | lwf | agem` and the flags of that method (`--ewc-*`, `--distill-*`, `--agem-*`) -> the `joint_encoders` keys they
    set: the master key always (its default unless the flag is given), the others when given.  Any other `--cl`: an empty dict."""
    if getattr(args, "cl", None) not in CONTINUAL:
        return {}
    master, default, flags = CONTINUAL[args.cl]
    out = {master: default if getattr(args, master) is None else getattr(args, master)}
    for flag in flags:
        if getattr(args, flag, None) is not None:
            out[flag] = getattr(args, flag)
    return out


AUG_FLAGS = {"aug_rotate": "rotate_deg", "aug_translate": "translate", "aug_zoom": "zoom", "aug_flip": "flip_p",
             "aug_brightness": "brightness", "aug_contrast": "contrast"}


def augment_from_args(args):
    """The `--augment` / `--aug-*` flags -> None (no augmentation) or the dict of `augment.AugmentSpec` fields: `--augment` selects the
    moderate default (+-10 degrees, 0.05, zoom 0.9..1.1, no flip, 0.2, 0.2), every `--aug-*` flag overrides one field of it."""
    from .augment import DEFAULT_SPEC_ARGS
    given = {field: getattr(args, flag) for flag, field in AUG_FLAGS.items() if getattr(args, flag, None) is not None}
    if not getattr(args, "augment", False):
        if given:
            raise SystemExit("--aug-* flags set the ranges of the on-device augmentation and need --augment")
        return None
    spec = dict(DEFAULT_SPEC_ARGS)
    spec.update(given)
    spec["zoom"] = tuple(spec["zoom"])
    return spec


def zero_joint_bounds(args):
    _seed()
    if args.epochs == 0:  # zero-shot: no adapters (Trainer.py:294-303)
        TR.IMAGE_MODEL = TR.TEXT_MODEL = False
    trainer, writer, train_loader, val_loader, test_loader = _setup(args, "joint")
    criterion = nn.BCEWithLogitsLoss()
    metrics = None
    try:
        if args.epochs > 0:
            for epoch in range(1, args.epochs + 1):
                trainer.train(train_loader, criterion, epoch, args.cl, args.threshold, actual_task=epoch)
                knn_bank(trainer, args, train_loader)
                trainer.val(val_loader, criterion, epoch, args.epochs, mode="joint", tasks_order=None)
                metrics = trainer.test(test_loader, criterion, epoch, args.epochs, mode="joint", tasks_order=None)
        else:
            knn_bank(trainer, args, train_loader)
            trainer.val(val_loader, criterion, 0, 0, mode="zero", tasks_order=None)
            metrics = trainer.test(test_loader, criterion, 0, 0, mode="zero", tasks_order=None)
    finally:
        if args.epochs > 0:
            trainer.save()
    return trainer, metrics


def class_incremental(args):
    _seed()
    trainer, writer, train_loader, val_loader, test_loader = _setup(args, "class")
    criterion = nn.BCEWithLogitsLoss()
    tasks_order = [0, 1, 2, 3, 4]
    last_batch = count = 0
    threshold = args.threshold
    metrics = None
    try:
        for actual_task in range(1, len(tasks_order) + 1):
            for epoch in range(1, args.epochs + 1):
                count += 1
                threshold = threshold + args.adder
                if args.threshold_scheduling and args.cl is not None:
                    writer.add_scalar("monitor-resets/threshold-scheduling", threshold, count)
                if args.cl == "profCL" and actual_task > 1:
                    trainer.model_copy()
                fn = trainer.train_class_more_labels_incremental if args.more_labels else trainer.train_class_incremental
                last_batch = fn(train_loader[actual_task - 1], criterion, epoch, args.cl, threshold, tasks_order[actual_task - 1],
                                last_batch, actual_task)
                if args.cl == "profCL" and actual_task > 1:
                    trainer.profIncremental(epoch, args.epochs, actual_task, threshold)
            if actual_task < len(tasks_order):      # --cl ewc | lwf | agem: what the finished task leaves for the next one
                trainer.end_task(train_loader[actual_task - 1])
            knn_bank(trainer, args, list(train_loader[:actual_task]))      # the tasks seen so far
            trainer.val(val_loader, criterion, actual_task, args.epochs, mode=args.mode, tasks_order=tasks_order)
            metrics = trainer.test(test_loader, criterion, actual_task, args.epochs, mode=args.mode, tasks_order=tasks_order)
    finally:
        trainer.save()
    return trainer, metrics


def data_incremental(args):
    _seed()
    trainer, writer, train_loader, val_loader, test_loader = _setup(args, "data")
    criterion = nn.BCEWithLogitsLoss()
    count = 0
    threshold = args.threshold
    metrics = None
    try:
        for part in range(1, args.parts + 1):
            for epoch in range(1, args.epochs + 1):
                count += 1
                threshold = threshold + args.adder
                if args.cl == "profCL":
                    trainer.model_copy()
                trainer.train(train_loader[part - 1], criterion, epoch, args.cl, threshold, part=part, epochs=args.epochs,
                              actual_task=part)
                if args.cl == "profCL":
                    trainer.profIncremental(epoch, args.epochs, part, threshold)
            if part < args.parts:
                trainer.end_task(train_loader[part - 1])
            knn_bank(trainer, args, train_loader[part - 1])
            train_loader[part - 1] = None
            trainer.val(val_loader, criterion, part, args.parts, mode="data-inc", tasks_order=part)
            metrics = trainer.test(test_loader, criterion, part, args.parts, mode="data-inc", tasks_order=part)
    finally:
        trainer.save()
    return trainer, metrics


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("which", choices=["zero-joint", "class-inc", "data-inc"])
    ap.add_argument("--batch-size", type=int, default=6144)      # ZERO_JOINT_BOUNDS.py:20
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--parts", type=int, default=5)
    ap.add_argument("--mode", default="class-pos-neg", choices=["class-pos-neg", "class-pos"])
    ap.add_argument("--more-labels", action="store_true")
    ap.add_argument("--single-prompt", action="store_true")
    ap.add_argument("--xrays-position", default="all")
    ap.add_argument("--cl", default=None, choices=[None, "myCL", "profCL", "ewc", "lwf", "agem"],
                    help="continual learning: the reference's weight-reset heuristics (myCL, profCL) or, with --joint, elastic weight "
                         "consolidation (ewc, DESIGN.md 5.10), similarity distillation from the previous task's encoders (lwf, "
                         "DESIGN.md 5.11) or A-GEM's gradient projection against an episodic memory (agem, DESIGN.md 5.12)")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--adder", type=float, default=0.001)
    ap.add_argument("--threshold-scheduling", action="store_true")
    ap.add_argument("--dataset-root", default=None)
    ap.add_argument("--pretrained-text", default=None)
    ap.add_argument("--log-root", default="runs")
    ap.add_argument("--n-train", type=int, default=61440)
    ap.add_argument("--n-eval", type=int, default=4096)
    ap.add_argument("--joint", action="store_true", help="train both encoders in-loop (north-star InfoNCE step) instead of the adapters")
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--small-text", action="store_true", help="--joint: a 2-layer text model instead of the 12-layer CXR-BERT (quick runs)")
    ap.add_argument("--text-dropout", action="store_true",
                    help="--joint: train the text model in train mode with HF dropout (CXRBertModel.enable_dropout_); default: eval mode")
    ap.add_argument("--positives", default="pair", choices=["pair", "labels", "text"],
                    help="--joint: the positives of a pair in the InfoNCE loss: only itself (pair, default), every pair of the global "
                         "batch with the same label vector (labels) or the same prompt text (text)")
    ap.add_argument("--learn-temperature", action="store_true",
                    help="--joint: learn the InfoNCE temperature (logit scale log(1/tau), initialised from --temperature, clamped to "
                         "[0, ln 100] after every step); default: the temperature is fixed")
    ap.add_argument("--contrastive-loss", default=None, choices=["infonce", "sigmoid"],
                    help="--joint: the loss of the north-star step: softmax InfoNCE (infonce, default) or the pairwise sigmoid loss "
                         "(sigmoid, DESIGN.md 5.6); with --learn-temperature the sigmoid loss learns its bias too")
    ap.add_argument("--sigmoid-bias", type=float, default=None, metavar="B",
                    help="--contrastive-loss sigmoid: the (initial) bias b of the logits exp(theta) * cos + b; default -10")
    ap.add_argument("--augment", action="store_true",
                    help="--joint: augment the images on the device inside the training step (random affine + brightness / contrast, "
                         "DESIGN.md 5.4); alone it selects +-10 degrees, translate 0.05, zoom 0.9..1.1, no flip, brightness / contrast 0.2")
    ap.add_argument("--aug-rotate", type=float, default=None, metavar="DEG", help="--augment: rotation uniform in +-DEG degrees")
    ap.add_argument("--aug-translate", type=float, default=None, metavar="FRAC", help="--augment: shift uniform in +-FRAC of the image size")
    ap.add_argument("--aug-zoom", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="--augment: zoom log-uniform in [LO, HI]")
    ap.add_argument("--aug-flip", type=float, default=None, metavar="P", help="--augment: horizontal flip with probability P (default 0)")
    ap.add_argument("--aug-brightness", type=float, default=None, metavar="B", help="--augment: brightness factor uniform in 1 +- B")
    ap.add_argument("--aug-contrast", type=float, default=None, metavar="C", help="--augment: contrast factor uniform in 1 +- C")
    ap.add_argument("--retrieval", type=int, nargs="*", default=None, metavar="K",
                    help="--joint: val / test also report image<->text retrieval over the whole split (Recall@K, median / mean rank, "
                         "both directions, DESIGN.md 5.5); without values K = 1 5 10")
    ap.add_argument("--knn", type=int, nargs="?", const=True, default=None, metavar="K",
                    help="--joint: val / test also report a kNN label probe of the image embeddings against a bank re-embedded from "
                         "the training loaders (kNN/Accuracy, F1-macro, AUROC; DESIGN.md 5.15); without a value K = 20")
    ap.add_argument("--knn-temperature", type=float, default=None, metavar="T", help="--knn: the temperature of the vote's weights (default 0.07)")
    ap.add_argument("--knn-bank-batches", type=int, default=None, metavar="N",
                    help="--knn: batches of each training loader that go into the bank (default 8)")
    ap.add_argument("--micro-batch", type=int, default=None, metavar="N",
                    help="--joint: run the encoders on at most N of a rank's rows at a time (gradient cache, DESIGN.md 5.7): the loss "
                         "and update of the whole batch at the peak memory of one chunk; default: the whole batch at once")
    ap.add_argument("--optim", default=None, choices=["adam", "sgd", "adamw"],
                    help="--joint: the optimiser of the north-star step; adamw = decoupled weight decay (biases and norm parameters "
                         "do not decay) with optional clipping (DESIGN.md 5.8); default: Adam, as the reference")
    ap.add_argument("--weight-decay", type=float, default=None, metavar="W", help="--optim adamw: decoupled weight decay (default 0.01)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="C",
                    help="--optim adamw: clip the global gradient norm to C; inf = report the norm (train/grad_norm) without clipping")
    ap.add_argument("--warmup-steps", type=int, default=None, metavar="N",
                    help="--joint: linear learning-rate warmup over the first N optimiser steps of the run")
    ap.add_argument("--lr-decay", default=None, choices=["constant", "linear", "cosine"],
                    help="--joint: learning-rate decay after the warmup, to --min-lr-ratio x --lr at the run's last step")
    ap.add_argument("--min-lr-ratio", type=float, default=None, metavar="R", help="--lr-decay: the final learning rate as a fraction of --lr")
    ap.add_argument("--ewc-lambda", type=float, default=None, metavar="S",
                    help="--cl ewc: strength of the penalty S / 2 * sum F (p - anchor)^2 (default 1e4: F is a squared mean gradient)")
    ap.add_argument("--ewc-batches", type=int, default=None, metavar="N",
                    help="--cl ewc: estimate the Fisher diagonal from at most N batches of the finished task (default: all of them)")
    ap.add_argument("--ewc-gamma", type=float, default=None, metavar="G",
                    help="--cl ewc: F = G * F_old + F_new when a further task is consolidated, G in [0, 1] (default 1)")
    ap.add_argument("--ewc-fisher", default=None, choices=["empirical", "identity"],
                    help="--cl ewc: empirical Fisher diagonal (default) or identity (L2-SP: no estimate, half the memory)")
    ap.add_argument("--distill-weight", type=float, default=None, metavar="BETA",
                    help="--cl lwf: weight of the distillation term L_d in the step's objective contrastive + BETA * L_d (default 1.0; 0 "
                         "only measures the drift)")
    ap.add_argument("--distill-temperature", type=float, default=None, metavar="TAU",
                    help="--cl lwf: the fixed temperature of the distilled similarity distributions (default: --temperature)")
    ap.add_argument("--agem-memory", type=int, default=None, metavar="M",
                    help="--cl agem: rows of every finished task kept in the episodic memory, per rank (default 256)")
    ap.add_argument("--agem-batch", type=int, default=None, metavar="N",
                    help="--cl agem: memory rows of the reference gradient, per rank (default: as many as the step's shard, at most "
                         "all that are stored)")
    ap.add_argument("--agem-every", type=int, default=None, metavar="K",
                    help="--cl agem: recompute the reference gradient every K-th step and reuse it in between (default 1)")
    ap.add_argument("--mlm-weight", type=float, default=None, metavar="W",
                    help="--joint: add W times the masked-language-modelling loss of CXR-BERT's own head to the step's objective; the "
                         "token ids are masked on the device every step and the head is trained (DESIGN.md 5.13)")
    ap.add_argument("--mlm-probability", type=float, default=None, metavar="P",
                    help="--mlm-weight: the fraction of the non-special tokens selected per step (default 0.15)")
    ap.add_argument("--mlm-seed", type=int, default=None, metavar="S",
                    help="--mlm-weight: seed of the masking draws (default: drawn from torch's CPU generator)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="--joint: keep an exponential moving average of the trained parameters with decay D in [0, 1], one launch "
                         "per step (DESIGN.md 5.14)")
    ap.add_argument("--ema-no-warmup", action="store_true",
                    help="--ema-decay: use D from the first update on (default: min(D, (1 + t) / (10 + t)) at update t)")
    ap.add_argument("--ema-eval", action="store_true",
                    help="--ema-decay: val / test (and --retrieval) evaluate the averaged weights")
    ap.add_argument("--ema-teacher", action="store_true",
                    help="--ema-decay with --cl lwf: the distillation teacher is the average itself (a momentum teacher)")
    ap.add_argument("--pretrained-image", default=None)
    return ap


def parse_args(argv=None):
    """`make_parser().parse_args` plus the refusals that concern `--cl ewc`, `--cl lwf`, `--cl agem`, `--mlm-weight` and `--ema-decay`
    (parser errors: exit status 2)"""
    ap = make_parser()
    args = ap.parse_args(argv)
    given = [f for f in ("ewc_lambda", "ewc_batches", "ewc_gamma", "ewc_fisher") if getattr(args, f) is not None]
    if given and args.cl != "ewc":
        ap.error("--" + given[0].replace("_", "-") + " configures elastic weight consolidation and needs --cl ewc")
    if args.cl == "ewc":
        if args.which == "zero-joint":
            ap.error("--cl ewc consolidates between tasks; zero-joint trains a single task (use class-inc or data-inc)")
        if not args.joint:
            ap.error("--cl ewc penalises the encoders of the north-star step and needs --joint (the adapter schedules keep the "
                     "reference's weight-reset heuristics myCL / profCL)")
        if args.ewc_lambda is not None and not (args.ewc_lambda >= 0 and args.ewc_lambda != float("inf")):
            ap.error(f"--ewc-lambda must be finite and >= 0, got {args.ewc_lambda}")
        if args.ewc_gamma is not None and not 0.0 <= args.ewc_gamma <= 1.0:
            ap.error(f"--ewc-gamma must be in [0, 1], got {args.ewc_gamma}")
        if args.ewc_batches is not None and args.ewc_batches < 1:
            ap.error(f"--ewc-batches must be >= 1, got {args.ewc_batches}")
    given = [f for f in ("distill_weight", "distill_temperature") if getattr(args, f) is not None]
    if given and args.cl != "lwf":
        ap.error("--" + given[0].replace("_", "-") + " configures similarity distillation and needs --cl lwf")
    if args.cl == "lwf":
        if args.which == "zero-joint":
            ap.error("--cl lwf takes its teacher between tasks; zero-joint trains a single task (use class-inc or data-inc)")
        if not args.joint:
            ap.error("--cl lwf distils the encoders of the north-star step and needs --joint (the adapter schedules keep the "
                     "reference's weight-reset heuristics myCL / profCL)")
        if args.distill_weight is not None and not (args.distill_weight >= 0 and args.distill_weight != float("inf")):
            ap.error(f"--distill-weight must be finite and >= 0, got {args.distill_weight}")
        if args.distill_temperature is not None and not (args.distill_temperature > 0 and args.distill_temperature != float("inf")):
            ap.error(f"--distill-temperature must be positive and finite, got {args.distill_temperature}")
    given = [f for f in ("agem_memory", "agem_batch", "agem_every") if getattr(args, f) is not None]
    if given and args.cl != "agem":
        ap.error("--" + given[0].replace("_", "-") + " configures A-GEM's episodic memory and needs --cl agem")
    if args.cl == "agem":
        if args.which == "zero-joint":
            ap.error("--cl agem remembers rows between tasks; zero-joint trains a single task (use class-inc or data-inc)")
        if not args.joint:
            ap.error("--cl agem projects the gradient of the north-star step and needs --joint (the adapter schedules keep the "
                     "reference's weight-reset heuristics myCL / profCL)")
        for f in given:
            if getattr(args, f) < 1:
                ap.error(f"--{f.replace('_', '-')} must be >= 1, got {getattr(args, f)}")
    given = [f for f in ("mlm_probability", "mlm_seed") if getattr(args, f) is not None]
    if given and args.mlm_weight is None:
        ap.error("--" + given[0].replace("_", "-") + " configures the masked-language-modelling loss and needs --mlm-weight")
    if args.mlm_weight is not None:
        if not args.joint:
            ap.error("--mlm-weight adds a loss to the north-star step and needs --joint (the adapter schedules use frozen "
                     "pre-computed text embeddings)")
        if not (args.mlm_weight >= 0 and args.mlm_weight != float("inf")):
            ap.error(f"--mlm-weight must be finite and >= 0, got {args.mlm_weight}")
        if args.mlm_probability is not None and not 0.0 <= args.mlm_probability <= 1.0:
            ap.error(f"--mlm-probability must be in [0, 1], got {args.mlm_probability}")
        if args.mlm_seed is not None and args.mlm_seed < 0:
            ap.error(f"--mlm-seed must be >= 0, got {args.mlm_seed}")
        if getattr(args, "micro_batch", None) is not None:
            ap.error("--mlm-weight with --micro-batch is out of scope: the micro-batched step keeps no last hidden state")
    given = [f for f in ("ema_no_warmup", "ema_eval", "ema_teacher") if getattr(args, f)]
    if given and args.ema_decay is None:
        ap.error("--" + given[0].replace("_", "-") + " configures the parameter average and needs --ema-decay")
    if args.ema_decay is not None:
        if not args.joint:
            ap.error("--ema-decay averages the encoders of the north-star step and needs --joint (the adapter schedules have no such "
                     "average)")
        if not 0.0 <= args.ema_decay <= 1.0:
            ap.error(f"--ema-decay must be in [0, 1], got {args.ema_decay}")
        if args.ema_teacher and args.cl != "lwf":
            ap.error("--ema-teacher makes the teacher of similarity distillation a momentum teacher and needs --cl lwf")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.text_dropout and not args.joint:
        raise SystemExit("--text-dropout trains the text encoder in-loop and needs --joint (the adapter schedules use frozen "
                         "pre-computed text embeddings)")
    if args.positives != "pair" and not args.joint:
        raise SystemExit("--positives selects the targets of the north-star InfoNCE step and needs --joint (the adapter schedules "
                         "use the labels through the pos-neg BCE loss)")
    if args.learn_temperature and not args.joint:
        raise SystemExit("--learn-temperature makes the temperature of the north-star InfoNCE step a parameter and needs --joint (the "
                         "adapter schedules have no temperature)")
    if args.contrastive_loss is not None and not args.joint:
        raise SystemExit("--contrastive-loss selects the loss of the north-star step and needs --joint (the adapter schedules train "
                         "with the pos-neg BCE loss)")
    if args.sigmoid_bias is not None and not args.joint:
        raise SystemExit("--sigmoid-bias is the bias of the north-star step's pairwise sigmoid loss and needs --joint "
                         "--contrastive-loss sigmoid")
    if args.sigmoid_bias is not None and args.contrastive_loss != "sigmoid":
        raise SystemExit("--sigmoid-bias is the bias of the pairwise sigmoid loss and needs --contrastive-loss sigmoid (InfoNCE has "
                         "no bias)")
    if args.augment and not args.joint:
        raise SystemExit("--augment augments the images of the north-star step and needs --joint (the adapter schedules train on "
                         "pre-computed image embeddings)")
    if args.retrieval is not None and not args.joint:
        raise SystemExit("--retrieval ranks the reports of the evaluation batches against their images and needs --joint (the adapter "
                         "schedules evaluate on pre-computed image embeddings without reports)")
    if (args.knn is not None or args.knn_temperature is not None or args.knn_bank_batches is not None) and not args.joint:
        raise SystemExit("--knn probes the image encoder of the north-star step and needs --joint (the adapter schedules evaluate on "
                         "pre-computed image embeddings)")
    if args.knn is None and (args.knn_temperature is not None or args.knn_bank_batches is not None):
        raise SystemExit("--knn-temperature and --knn-bank-batches configure the kNN probe and need --knn")
    if args.micro_batch is not None and not args.joint:
        raise SystemExit("--micro-batch chunks the encoder calls of the north-star step and needs --joint (the adapter schedules "
                         "train on pre-computed embeddings)")
    if args.micro_batch is not None and args.micro_batch < 1:
        raise SystemExit(f"--micro-batch must be >= 1, got {args.micro_batch}")
    given = [f for f in ("optim", "weight_decay", "clip_grad_norm", "warmup_steps", "lr_decay", "min_lr_ratio") if getattr(args, f) is not None]
    if given and not args.joint:
        raise SystemExit("--" + given[0].replace("_", "-") + " configures the optimiser of the north-star step and needs --joint (the "
                         "adapter schedules keep the reference's Adam at a constant learning rate)")
    if (args.weight_decay is not None or args.clip_grad_norm is not None) and args.optim != "adamw":
        raise SystemExit("--weight-decay / --clip-grad-norm are options of AdamW and need --optim adamw")
    augment_from_args(args)      # --aug-* without --augment
    fn = {"zero-joint": zero_joint_bounds, "class-inc": class_incremental, "data-inc": data_incremental}[args.which]
    _, metrics = fn(args)
    if int(os.environ.get("RANK", "0")) == 0:
        print("final test metrics:", metrics)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
