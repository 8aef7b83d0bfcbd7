"""Cost and peak memory of the micro-batched joint step at the bench configuration: L = 32, split-bf16, ResNet-50 at
224 px + 12-layer CXR-BERT, InfoNCE.

ONE trainer serves every mode: `micro_batch` is switched between the timed runs, so all modes run the same encoders and the same
optimiser over the same elements.  The modes of one batch size are alternated in one process and timed with device events; the peak
of `torch.cuda.max_memory_allocated` is taken over the timed steps of a mode (after the warm-up, so optimiser state and workspaces
exist).  Every chunk but the last is forwarded twice, and from the profiles the forward is about a third of a step, so a step in n
chunks is expected to cost about 1 + (n - 1) / (3 n) of the unchunked one; the expectation is printed beside the measurement and is
not a gate.  Prints one JSON line per batch size.

    python scripts/microbatch_step_cost.py [--batch 1024] [--micro 0 512 256] [--rounds 4] [--iters 3]     # 0 = unchunked
    python scripts/microbatch_step_cost.py --batch 6144 --micro 1024 --rounds 1 --iters 2                   # the reference's batch
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
    ap.add_argument("--micro", type=int, nargs="+", default=[0, 512, 256], help="micro_batch of each mode; 0 = unchunked")
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the modes")
    ap.add_argument("--iters", type=int, default=3, help="timed steps per mode and round")
    ap.add_argument("--precision", default="split_bf16", choices=["fp32", "split_bf16"])
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer, micro_slices
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel

    dev = "cuda"
    _lib.set_precision(args.precision)
    B = args.batch
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07)
    images = syn.synthetic_images(B, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)
    modes = {("none" if m <= 0 else str(m)): (None if m <= 0 else m) for m in args.micro}
    last = {}

    def timed(name, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            last[name] = tr.step(images, ids, mask)
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    res = {m: {"step": [], "round_medians": [], "peak": 0} for m in modes}
    for name, mb in modes.items():          # warm-up: kernels loaded, optimiser state and workspaces allocated
        tr.micro_batch = mb
        timed(name, 1)
    for _ in range(args.rounds):
        for name, mb in modes.items():
            tr.micro_batch = mb
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t = timed(name, args.iters)
            res[name]["peak"] = max(res[name]["peak"], torch.cuda.max_memory_allocated())
            res[name]["step"] += t
            res[name]["round_medians"].append(statistics.median(t))
    med = {m: statistics.median(d["step"]) for m, d in res.items()}
    chunks = {m: (1 if mb is None else len(micro_slices(B, mb))) for m, mb in modes.items()}
    out = {"metric": "microbatch_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision,
           "samples_per_mode": args.rounds * args.iters,
           "chunks": chunks,
           "step_ms": {m: round(v, 3) for m, v in med.items()},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "peak_allocated_gib": {m: round(res[m]["peak"] / 2 ** 30, 3) for m in res},
           "input_gib": round(sum(t.numel() * t.element_size() for t in (images, ids, mask)) / 2 ** 30, 3),
           "last_loss": {m: float(v.item()) for m, v in last.items()}}
    if "none" in med:
        out["step_over_unchunked"] = {m: round(med[m] / med["none"], 4) for m in med}
        out["expected_over_unchunked"] = {m: round(1 + (chunks[m] - 1) / (3.0 * chunks[m]), 4) for m in med}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
