"""Cost of A-GEM in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the plain Adam step (what bench.py times) and the A-GEM step
(reference pass on `agem_batch` = batch memory rows with `agem_every` = 1, the copy of the reference gradient, `agem_dots` and
`agem_project` between the backward and the update).  ONE trainer serves both modes: it is built with `agem_memory`, remembers the
batch once, and for the plain steps its `agem` attribute is cleared, which is exactly the step without the option (no launch).  The
parts are also timed alone on the buffers the last step left: the reference pass (gradient of the memory rows + copy), the copy,
`agem_dots` (8 B per parameter), `agem_project` taken (8 B read + 4 B written per parameter; decided by partials of a conflicting
pair, on a scratch gradient) and not taken (the partials read and nothing else), and `ewc_penalty` (20 B per parameter, strength 0 on
scratch anchor / F) as the yardstick for a bandwidth-bound launch over the same buffers.  No pass / fail number is fixed in advance:
the yardstick is the plain step of the same run, and its own spread -- the range of its per-round medians -- is printed beside the
difference.  Prints one JSON line.

    python scripts/agem_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]
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
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, agem_memory=B)
    opt, agem = tr.optimizer, tr.agem
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
    remember = timed(lambda: tr.remember([(images, ids, mask)]), 1)[0]
    modes = {"plain": None, "agem": agem}

    def step(m):
        last[m] = tr.step(images, ids, mask)

    res = {m: {"step": [], "round_medians": []} for m in modes}
    for m, a in modes.items():
        tr.agem = a
        timed(lambda: step(m), 2)
    n = opt.numel
    # scratch for the launches timed alone: a conflicting pair's partials (taken), an agreeing pair's (not taken), the penalty's buffers
    g2 = opt.flat_g.clone()
    taken = K.agem_dots(g2, agem.gref.neg(), out=torch.empty(2 * K.agem_dots_nparts(n), device=dev)).clone()
    kept = K.agem_dots(g2, g2, out=torch.empty(2 * K.agem_dots_nparts(n), device=dev)).clone()
    stats = torch.zeros(4, device=dev)
    anchor, F = torch.zeros_like(g2), torch.zeros_like(g2)
    pen_out = torch.empty(K.ewc_penalty_nparts(n), device=dev)
    parts = {k: [] for k in ("reference_pass", "copy", "agem_dots", "agem_project_taken", "agem_project_not_taken", "ewc_penalty")}
    for _ in range(args.rounds):
        for m, a in modes.items():
            tr.agem = a
            t = timed(lambda: step(m), args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
        tr.agem = agem
        parts["reference_pass"] += timed(lambda: (setattr(agem, "valid", False), tr._agem_reference(B)), 2)
        parts["copy"] += timed(agem.store_reference, args.iters)
        parts["agem_dots"] += timed(lambda: K.agem_dots(opt.flat_g, agem.gref, out=agem._partials), args.iters)
        parts["agem_project_taken"] += timed(lambda: K.agem_project(g2, agem.gref, taken, stats), args.iters)
        parts["agem_project_not_taken"] += timed(lambda: K.agem_project(g2, agem.gref, kept, stats), args.iters)
        parts["ewc_penalty"] += timed(lambda: K.ewc_penalty(g2, opt.flat_p, anchor, F, 0.0, out=pen_out), args.iters)
    med = {m: statistics.median(d["step"]) for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    pm = {k: statistics.median(v) for k, v in parts.items()}
    gbs = lambda nbytes, ms: round(nbytes * n / ms / 1e6, 1)  # noqa: E731
    info = tr.current_interference()
    out = {"metric": "agem_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision, "parameters": n,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(v, 3) for m, v in med.items()},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(v, 3) for m, v in spread.items()},
           "agem_minus_plain_step_ms": round(med["agem"] - med["plain"], 3),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "parts_ms": {k: round(v, 4) for k, v in pm.items()},
           "parts_ms_minmax": {k: (round(min(v), 4), round(max(v), 4)) for k, v in parts.items()},
           "agem_dots_gb_per_s": gbs(8.0, pm["agem_dots"]), "agem_dots_floor_ms": round(8.0 * n / HBM_FLOOR_GB_S / 1e6, 4),
           "agem_project_taken_gb_per_s": gbs(12.0, pm["agem_project_taken"]),
           "agem_project_floor_ms": round(12.0 * n / HBM_FLOOR_GB_S / 1e6, 4),
           "copy_gb_per_s": gbs(8.0, pm["copy"]),
           "ewc_penalty_gb_per_s": gbs(20.0, pm["ewc_penalty"]),
           "agem_dots_over_ewc_penalty_bandwidth": round(gbs(8.0, pm["agem_dots"]) / gbs(20.0, pm["ewc_penalty"]), 3),
           "remember_ms": round(remember, 3), "memory_rows": len(tr.memory),
           "interference": info, "last_loss": {m: float(v.item()) for m, v in last.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
