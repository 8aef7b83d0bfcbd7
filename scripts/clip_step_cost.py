"""Cost of gradient clipping + decoupled weight decay in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer
CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the Adam step (what bench.py times: one `adam_fused` launch over
the flat buffers) and the AdamW step with clipping (`grad_sqnorm` over the flat gradient buffer, then `adamw_clipped` with the decay
mask: one more read of the gradients, 4 B per parameter beside the update's 28 B, and 0.25 B per parameter of mask).  ONE trainer
serves both modes: it is built with `optim="adamw"`, and for the Adam steps its optimiser's `step` issues `adam_fused` over the same
flat buffers, so both modes run the same encoders and loss over the same elements.  Also times the optimiser alone (its launches on
the gradients the last step left).  No pass / fail number is fixed in advance: the yardstick is the Adam step of the same run, and its
own spread -- the range of its per-round medians -- is printed beside the difference.  Prints one JSON line.

    python scripts/clip_step_cost.py [--batch 1024] [--rounds 6] [--iters 5] [--max-grad-norm 1.0]
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
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--weight-decay", type=float, default=0.01)
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import kernels as K
    from incremental_multimodal_medical_learning_ii_amd import optim as O
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
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, optim="adamw", weight_decay=args.weight_decay,
                                 max_grad_norm=args.max_grad_norm)
    opt = tr.optimizer
    images = syn.synthetic_images(B, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)
    last = {}

    def adam_step(grad_scale: float = 1.0):       # `optim.Adam.step` over this optimiser's buffers
        opt._sync_grads()
        opt.steps += 1
        K.adam_fused(opt.flat_p, opt.flat_g, opt.flat_m, opt.flat_v, opt.lr, opt.betas[0], opt.betas[1], opt.eps, 0.0, opt.steps, grad_scale)

    def set_mode(clipped):
        if clipped:
            opt.__dict__.pop("step", None)        # the class's own step: grad_sqnorm + adamw_clipped
        else:
            opt.step = adam_step

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    modes = {"adam": False, "adamw_clipped": True}

    def step(m):
        last[m] = tr.step(images, ids, mask)

    res = {m: {"step": [], "optimiser": [], "round_medians": []} for m in modes}
    for m, clipped in modes.items():              # warm-up: kernels loaded, allocator settled
        set_mode(clipped)
        timed(lambda: step(m), 2)
        timed(lambda: opt.step(), 2)
    for _ in range(args.rounds):
        for m, clipped in modes.items():
            set_mode(clipped)
            t = timed(lambda: step(m), args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
            res[m]["optimiser"] += timed(lambda: opt.step(), args.iters)
    set_mode(True)
    assert isinstance(opt, O.AdamW)
    med = {m: {k: statistics.median(d[k]) for k in ("step", "optimiser")} for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    n = opt.numel
    out = {"metric": "clip_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision, "parameters": n,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(med[m]["step"], 3) for m in med},
           "optimiser_ms": {m: round(med[m]["optimiser"], 3) for m in med},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(spread[m], 3) for m in spread},
           "clipped_minus_adam_step_ms": round(med["adamw_clipped"]["step"] - med["adam"]["step"], 3),
           "clipped_minus_adam_optimiser_ms": round(med["adamw_clipped"]["optimiser"] - med["adam"]["optimiser"], 3),
           "optimiser_gb_per_s": {"adam": round(28.0 * n / med["adam"]["optimiser"] / 1e6, 1),
                                  "adamw_clipped": round(32.25 * n / med["adamw_clipped"]["optimiser"] / 1e6, 1)},
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "last_grad_norm": opt.current_grad_norm(), "last_clip_coef": float(opt.last_clip_coef),
           "last_loss": {m: float(v.item()) for m, v in last.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
