"""Cost of similarity distillation from a frozen teacher in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 +
12-layer CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the plain Adam step (what bench.py times) and the distilled step
(the teacher's two save-free forwards on the same rows, the distillation head's forward next to the contrastive one, and its backward
inside the step's one backward).  ONE trainer serves both modes: it is built with `distill_weight`, takes one snapshot, and for the
plain steps its teacher is set aside, which is exactly the state before a first snapshot (no launch, no allocation).  Also timed,
separately and on their own: the two save-free teacher forwards (`_teacher_pair`, both streams) and the head's launches (forward and
backward of `functional.distill_loss` on detached embeddings of the batch: four normalisations, four logits GEMMs, two statistics
launches with their loss folds, two gradient transforms, two backward GEMMs, two normalisation backwards).  No pass / fail number is
fixed in advance: the yardstick is the plain step of the same run, and its own spread -- the range of its per-round medians -- is
printed beside the difference; what the distilled step costs beyond teacher forward + head is printed as `unexplained_ms`.  Prints one
JSON line.

    python scripts/distill_step_cost.py [--batch 1024] [--rounds 6] [--iters 5] [--weight 1.0]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6, help="alternations of the two modes")
    ap.add_argument("--iters", type=int, default=5, help="timed steps per mode and round")
    ap.add_argument("--precision", default="split_bf16", choices=["fp32", "split_bf16"])
    ap.add_argument("--weight", type=float, default=1.0)
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel

    dev = "cuda"
    _lib.set_precision(args.precision)
    B = args.batch
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, distill_weight=args.weight)
    images = syn.synthetic_images(B, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)
    last = {}

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    tr.step(images, ids, mask)                    # warm-up: kernels loaded, allocator settled
    torch.cuda.reset_peak_memory_stats()
    tr.step(images, ids, mask)
    torch.cuda.synchronize()
    peak_plain = torch.cuda.max_memory_allocated()
    held = torch.cuda.memory_allocated()
    tr.snapshot_teacher()
    teacher_bytes = torch.cuda.memory_allocated() - held
    teacher = tr.teacher
    torch.cuda.reset_peak_memory_stats()
    tr.step(images, ids, mask)
    torch.cuda.synchronize()
    peak_distilled = torch.cuda.max_memory_allocated()
    modes = {"plain": None, "distilled": teacher}

    def step(m):
        last[m] = tr.step(images, ids, mask)

    res = {m: {"step": [], "round_medians": []} for m in modes}
    for m, t in modes.items():
        tr.teacher = t
        timed(lambda: step(m), 2)
    tr.teacher = teacher
    with torch.no_grad():
        emb = [e.detach().clone() for e in tr._encode_pair(images, ids, mask)] + [e.clone() for e in tr._teacher_pair(images, ids, mask)]

    def head():
        i, t = emb[0].requires_grad_(True), emb[1].requires_grad_(True)
        Fh.distill_loss(i, t, emb[2], emb[3], 0.07, weight=args.weight).backward()
        i.grad = t.grad = None

    timed(head, 2)
    forward, heads = [], []
    for _ in range(args.rounds):
        for m, t in modes.items():
            tr.teacher = t
            t_ms = timed(lambda: step(m), args.iters)
            res[m]["step"] += t_ms
            res[m]["round_medians"].append(statistics.median(t_ms))
        tr.teacher = teacher
        forward += timed(lambda: tr._teacher_pair(images, ids, mask), args.iters)     # the two save-free forwards alone
        heads += timed(head, args.iters)                                               # the head's launches alone
    med = {m: statistics.median(d["step"]) for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    fwd_ms, head_ms = statistics.median(forward), statistics.median(heads)
    extra = med["distilled"] - med["plain"]
    out = {"metric": "distill_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision, "weight": args.weight,
           "parameters": tr.optimizer.numel, "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(v, 3) for m, v in med.items()},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(v, 3) for m, v in spread.items()},
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "distilled_minus_plain_step_ms": round(extra, 3),
           "teacher_forward_ms": round(fwd_ms, 3), "teacher_forward_ms_minmax": (round(min(forward), 3), round(max(forward), 3)),
           "head_ms": round(head_ms, 3), "head_ms_minmax": (round(min(heads), 3), round(max(heads), 3)),
           "unexplained_ms": round(extra - fwd_ms - head_ms, 3),
           "teacher_bytes": int(teacher_bytes), "peak_bytes": {"plain": int(peak_plain), "distilled": int(peak_distilled)},
           "last_distill": tr.current_distill(), "last_loss": {m: float(v.item()) for m, v in last.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
