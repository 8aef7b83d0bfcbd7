"""Cost of label-aware multi-positive InfoNCE in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer
CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the plain head (`positives=None`, what bench.py times) and
the label-keyed one (`positives="labels"`: host-side hashing of the [B, 5] labels, the [B] key copy, and the two multipos kernels
in place of the two plain ones).  Also times the head alone (forward + backward of `functional.infonce_loss` on fixed
embeddings) in both modes.  The allowance for the keyed step is the plain mode's own spread: the range of its per-round medians.
Prints one JSON line.

    python scripts/multipos_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]

Per-kernel attribution of the head, in a run of its own (`--head-only N` issues N head forward + backward passes per mode and
nothing else, plain first, so the trace holds the head kernels only):

    rocprofv3 --kernel-trace --stats -d prof_multipos -- python scripts/multipos_step_cost.py --head-only 50
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
    ap.add_argument("--head-only", type=int, default=0, metavar="N", help="only N head passes per mode (for a kernel trace)")
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer, keys_from_labels

    dev = "cuda"
    _lib.set_precision(args.precision)
    B = args.batch
    g = torch.Generator().manual_seed(31)
    labels = (torch.rand(B, 5, generator=g) < 0.3).float()          # five findings: at most 32 distinct vectors in the batch
    keys_dev = keys_from_labels(labels).to(dev)
    emb_i = torch.from_numpy(syn._normal("cost.I", (B, 128))).to(dev)
    emb_t = torch.from_numpy(syn._normal("cost.T", (B, 128))).to(dev)

    def head(keys):
        i, t = emb_i.clone().requires_grad_(True), emb_t.clone().requires_grad_(True)
        loss = Fh.infonce_loss(i, t, 0.07) if keys is None else Fh.infonce_loss(i, t, 0.07, keys=keys)
        loss.backward()

    if args.head_only:
        for keys in (None, keys_dev):
            for _ in range(args.head_only):
                head(keys)
        torch.cuda.synchronize()
        print(json.dumps({"metric": "multipos_head_trace", "batch": B, "passes_per_mode": args.head_only}))
        return

    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07)
    images = syn.synthetic_images(B, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)

    def step():
        tr.step(images, ids, mask, labels=labels)        # the labels stay on the host; ignored under positives=None

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    def set_mode(positives):
        tr.positives = positives

    modes = {"plain": None, "labels": "labels"}
    res = {m: {"step": [], "head": [], "round_medians": []} for m in modes}
    for m, pos in modes.items():          # warm-up: kernels loaded, allocator settled
        set_mode(pos)
        timed(step, 2)
        timed(lambda: head(None if pos is None else keys_dev), 2)
    n_groups = int(torch.unique(keys_dev).numel())
    for _ in range(args.rounds):
        for m, pos in modes.items():
            set_mode(pos)
            t = timed(step, args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
            res[m]["head"] += timed(lambda: head(None if pos is None else keys_dev), args.iters)
    set_mode(None)
    med = {m: {k: statistics.median(d[k]) for k in ("step", "head")} for m, d in res.items()}
    spread = max(res["plain"]["round_medians"]) - min(res["plain"]["round_medians"])
    delta = med["labels"]["step"] - med["plain"]["step"]
    out = {"metric": "multipos_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision, "key_groups": n_groups,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(med[m]["step"], 3) for m in med},
           "head_fwd_bwd_ms": {m: round(med[m]["head"], 3) for m in med},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "plain_spread_ms": round(spread, 3),
           "keyed_minus_plain_step_ms": round(delta, 3),
           "keyed_minus_plain_head_ms": round(med["labels"]["head"] - med["plain"]["head"], 3),
           "within_plain_spread": bool(abs(delta) <= spread),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
