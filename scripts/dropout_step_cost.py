"""Cost of train-mode text dropout in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer CXR-BERT.

Two modes, alternated in one process and timed with device events: the text model in eval mode (the headline configuration), and
in train mode with HF dropout (p = 0.1 at all four sites, `CXRBertModel.enable_dropout_`).  Also times the text encoder's forward +
backward alone in both modes.  Prints one JSON line.

    python scripts/dropout_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]
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
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel

    dev = "cuda"
    _lib.set_precision(args.precision)
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07)
    tm.enable_dropout_(seed=27)
    images = syn.synthetic_images(args.batch, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(args.batch, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)

    def step():
        tr.step(images, ids, mask)

    def text_only():
        tm.zero_grad()
        tm.get_projected_text_embeddings(ids, mask, normalize_embeddings=False).sum().backward()

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    modes = {"eval": lambda: tm.eval(), "train_p0.1": lambda: tm.train()}
    res = {m: {"step": [], "text": []} for m in modes}
    for m, setm in modes.items():          # warm-up: kernels loaded, allocator settled
        setm()
        timed(step, 2)
        timed(text_only, 2)
    for _ in range(args.rounds):
        for m, setm in modes.items():
            setm()
            res[m]["step"] += timed(step, args.iters)
            res[m]["text"] += timed(text_only, args.iters)
    tm.eval()
    med = {m: {k: statistics.median(v) for k, v in d.items()} for m, d in res.items()}
    out = {"metric": "text_dropout_cost", "batch": args.batch, "seq_len": args.seq_len, "precision": args.precision,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(med[m]["step"], 3) for m in med},
           "text_fwd_bwd_ms": {m: round(med[m]["text"], 3) for m in med},
           "dropout_cost_step_ms": round(med["train_p0.1"]["step"] - med["eval"]["step"], 3),
           "dropout_cost_text_ms": round(med["train_p0.1"]["text"] - med["eval"]["text"], 3),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
