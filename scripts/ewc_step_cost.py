"""Cost of the elastic-weight-consolidation penalty in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer
CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the plain Adam step (what bench.py times) and the penalised
step (one `ewc_penalty` launch over the flat buffers between the backward and the update: it reads the gradient, the parameters, the
anchor and F and writes the gradient, 20 B per parameter).  ONE trainer serves both modes: it is built with `ewc_lambda`, consolidated
once on the batch, and for the plain steps its `EWC.active` flag is cleared, which is exactly the state before a first consolidation
(no launch).  Also times the penalty launch alone, against its 20 B per parameter floor, and one consolidation batch (the gradient
of a step plus `fisher_accumulate`; the final `ewc_consolidate` launch is timed on its own).  No pass / fail number is fixed in
advance: the yardstick is the plain step of the same run, and its own spread -- the range of its per-round medians -- is printed
beside the difference.  Prints one JSON line.

    python scripts/ewc_step_cost.py [--batch 1024] [--rounds 6] [--iters 5] [--strength 1e4]
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

HBM_FLOOR_GB_S = 8000.0     # the layer table's HBM floor


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6, help="alternations of the two modes")
    ap.add_argument("--iters", type=int, default=5, help="timed steps per mode and round")
    ap.add_argument("--precision", default="split_bf16", choices=["fp32", "split_bf16"])
    ap.add_argument("--strength", type=float, default=1e4)
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import kernels as K
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
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, ewc_lambda=args.strength)
    opt, ewc = tr.optimizer, tr.ewc
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
    consolidation = timed(lambda: tr.consolidate([(images, ids, mask)]), 3)[1:]
    ewc.begin_estimate()
    accumulate = timed(ewc.accumulate, 6)[1:]
    merge = timed(lambda: K.ewc_consolidate(ewc.F, ewc._acc, ewc.anchor, opt.flat_p, 1.0, 0.0), 6)[1:]    # scale 0: F is left as it is
    ewc._acc, ewc.samples = None, 0
    modes = {"plain": False, "penalised": True}

    def step(m):
        last[m] = tr.step(images, ids, mask)

    res = {m: {"step": [], "round_medians": []} for m in modes}
    for m, active in modes.items():
        ewc.active = active
        timed(lambda: step(m), 2)
    penalty = []
    for _ in range(args.rounds):
        for m, active in modes.items():
            ewc.active = active
            t = timed(lambda: step(m), args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
        penalty += timed(ewc.apply, args.iters)   # the launch alone, on the buffers the last step left
    med = {m: statistics.median(d["step"]) for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    n = opt.numel
    pen_ms = statistics.median(penalty)
    out = {"metric": "ewc_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision, "parameters": n,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(v, 3) for m, v in med.items()},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(v, 3) for m, v in spread.items()},
           "penalised_minus_plain_step_ms": round(med["penalised"] - med["plain"], 3),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "penalty_launch_ms": round(pen_ms, 4), "penalty_launch_ms_minmax": (round(min(penalty), 4), round(max(penalty), 4)),
           "penalty_bytes": 20 * n, "penalty_gb_per_s": round(20.0 * n / pen_ms / 1e6, 1),
           "penalty_floor_ms": round(20.0 * n / HBM_FLOOR_GB_S / 1e6, 4),
           "consolidation_batch_ms": round(statistics.median(consolidation), 3),
           "fisher_accumulate_ms": round(statistics.median(accumulate), 4), "ewc_consolidate_ms": round(statistics.median(merge), 4),
           "last_penalty": tr.current_penalty(), "last_loss": {m: float(v.item()) for m, v in last.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
