"""Cost of the learnable InfoNCE temperature in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer CXR-BERT
(the bench configuration).

Two modes, alternated in one process and timed with device events: the fixed temperature (what bench.py times) and the learnable one
(`learn_temperature=True`: the logits GEMMs with alpha = 1, the *_scaled statistics and gradient kernels in place of the plain ones,
one single-block kernel for d theta and one clamp launch after the optimiser).  ONE trainer serves both modes: it is built with
`learn_temperature=True` and its `logit_scale` is taken away for the fixed-temperature steps, which then launch exactly the default
path's kernels (the optimiser runs over 4 more elements out of ~133 M in both modes).  theta stays in the optimiser during the fixed
steps: its gradient is zero there, its Adam moments are zeroed at every change of mode so that the fixed steps leave it where it
was, and `temperature_after` is the work of the learnable steps alone.  Also times the head alone (forward + backward of
`functional.infonce_loss` on fixed embeddings) in both modes.  No pass / fail number is fixed in advance: the yardstick is the
fixed-temperature step of the same run, and its own spread -- the range of its per-round medians -- is the allowance.
Prints one JSON line.

    python scripts/temperature_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]

Per-kernel attribution of the head, in a run of its own (`--head-only N` issues N head forward + backward passes per mode and
nothing else, fixed first, so the trace holds the head kernels only):

    rocprofv3 --kernel-trace --stats -d prof_temperature -- python scripts/temperature_step_cost.py --head-only 50
"""
from __future__ import annotations

import argparse
import json
import math
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
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer

    dev = "cuda"
    _lib.set_precision(args.precision)
    B = args.batch
    emb_i = torch.from_numpy(syn._normal("cost.I", (B, 128))).to(dev)
    emb_t = torch.from_numpy(syn._normal("cost.T", (B, 128))).to(dev)
    head_theta = torch.tensor([math.log(1.0 / 0.07)], dtype=torch.float32, device=dev, requires_grad=True)

    def head(learn):
        i, t = emb_i.clone().requires_grad_(True), emb_t.clone().requires_grad_(True)
        loss = Fh.infonce_loss(i, t, 0.07, log_scale=head_theta) if learn else Fh.infonce_loss(i, t, 0.07)
        loss.backward()
        head_theta.grad = None

    if args.head_only:
        for learn in (False, True):
            for _ in range(args.head_only):
                head(learn)
        torch.cuda.synchronize()
        print(json.dumps({"metric": "temperature_head_trace", "batch": B, "passes_per_mode": args.head_only}))
        return

    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, learn_temperature=True)
    theta = tr.logit_scale
    images = syn.synthetic_images(B, 224, seed=27).to(dev)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)

    def step():
        tr.step(images, ids, mask)

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    off = (theta.data_ptr() - tr.optimizer.flat_p.data_ptr()) // 4

    def set_mode(learn):
        tr.logit_scale = theta if learn else None
        tr.optimizer.flat_m[off:off + 4].zero_()
        tr.optimizer.flat_v[off:off + 4].zero_()

    modes = {"fixed": False, "learnable": True}
    res = {m: {"step": [], "head": [], "round_medians": []} for m in modes}
    for m, learn in modes.items():          # warm-up: kernels loaded, allocator settled
        set_mode(learn)
        timed(step, 2)
        timed(lambda: head(learn), 2)
    for _ in range(args.rounds):
        for m, learn in modes.items():
            set_mode(learn)
            t = timed(step, args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
            res[m]["head"] += timed(lambda: head(learn), args.iters)
    set_mode(True)
    med = {m: {k: statistics.median(d[k]) for k in ("step", "head")} for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    delta = med["learnable"]["step"] - med["fixed"]["step"]
    out = {"metric": "temperature_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(med[m]["step"], 3) for m in med},
           "head_fwd_bwd_ms": {m: round(med[m]["head"], 3) for m in med},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(spread[m], 3) for m in spread},
           "learnable_minus_fixed_step_ms": round(delta, 3),
           "learnable_minus_fixed_head_ms": round(med["learnable"]["head"] - med["fixed"]["head"], 3),
           "within_fixed_spread": bool(abs(delta) <= spread["fixed"]),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "temperature_after": tr.current_temperature()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
