"""Cost of the pairwise sigmoid loss in the headline step: global batch 1024, L = 32, split-bf16, ResNet-50 + 12-layer CXR-BERT (the
bench configuration).

Two modes, alternated in one process and timed with device events: the InfoNCE step (what bench.py times) and the sigmoid step
(`loss="sigmoid"` with fixed theta = log(1/0.07) and b = -10: the logits GEMMs with alpha = 1, ONE fused forward + backward kernel
per block in place of a statistics and a gradient kernel, one single-block loss fold).  ONE trainer serves both modes: it is built
for InfoNCE, and for the sigmoid steps its `loss` is switched and the two device constants (made once, before the timing) are put in
place, so both modes run the same encoders and the same optimiser over the same elements.  Also times
the head alone (forward + backward of `functional.infonce_loss` / `functional.sigmoid_pairs_loss` on fixed embeddings).  No pass /
fail number is fixed in advance: the yardstick is the InfoNCE step of the same run, and its own spread -- the range of its per-round
medians -- is the allowance.  Prints one JSON line.

    python scripts/sigmoid_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]

Per-kernel attribution of the head, in a run of its own (`--head-only N` issues N head forward + backward passes per mode and
nothing else, InfoNCE first, so the trace holds the head kernels only):

    rocprofv3 --kernel-trace --stats -d prof_sigmoid -- python scripts/sigmoid_step_cost.py --head-only 50
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
    from incremental_multimodal_medical_learning_ii_amd.contrastive import SIGMOID_BIAS, JointContrastiveTrainer

    dev = "cuda"
    _lib.set_precision(args.precision)
    B = args.batch
    emb_i = torch.from_numpy(syn._normal("cost.I", (B, 128))).to(dev)
    emb_t = torch.from_numpy(syn._normal("cost.T", (B, 128))).to(dev)
    consts = (torch.tensor([math.log(1.0 / 0.07)], dtype=torch.float32, device=dev),
              torch.tensor([SIGMOID_BIAS], dtype=torch.float32, device=dev))

    def head(sigmoid):
        i, t = emb_i.clone().requires_grad_(True), emb_t.clone().requires_grad_(True)
        loss = Fh.sigmoid_pairs_loss(i, t, consts[0], consts[1]) if sigmoid else Fh.infonce_loss(i, t, 0.07)
        loss.backward()

    if args.head_only:
        for sigmoid in (False, True):
            for _ in range(args.head_only):
                head(sigmoid)
        torch.cuda.synchronize()
        print(json.dumps({"metric": "sigmoid_head_trace", "batch": B, "passes_per_mode": args.head_only}))
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
    last = {}

    def set_mode(sigmoid):
        tr.loss = "sigmoid" if sigmoid else "infonce"
        tr._sigmoid_consts = consts if sigmoid else None

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    modes = {"infonce": False, "sigmoid": True}

    def step(m):
        last[m] = tr.step(images, ids, mask)

    res = {m: {"step": [], "head": [], "round_medians": []} for m in modes}
    for m, sigmoid in modes.items():          # warm-up: kernels loaded, allocator settled
        set_mode(sigmoid)
        timed(lambda: step(m), 2)
        timed(lambda: head(sigmoid), 2)
    for _ in range(args.rounds):
        for m, sigmoid in modes.items():
            set_mode(sigmoid)
            t = timed(lambda: step(m), args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
            res[m]["head"] += timed(lambda: head(sigmoid), args.iters)
    set_mode(False)
    med = {m: {k: statistics.median(d[k]) for k in ("step", "head")} for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    delta = med["sigmoid"]["step"] - med["infonce"]["step"]
    out = {"metric": "sigmoid_step_cost", "batch": B, "seq_len": args.seq_len, "precision": args.precision,
           "samples_per_mode": args.rounds * args.iters,
           "step_ms": {m: round(med[m]["step"], 3) for m in med},
           "head_fwd_bwd_ms": {m: round(med[m]["head"], 3) for m in med},
           "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
           "spread_ms": {m: round(spread[m], 3) for m in spread},
           "sigmoid_minus_infonce_step_ms": round(delta, 3),
           "sigmoid_minus_infonce_head_ms": round(med["sigmoid"]["head"] - med["infonce"]["head"], 3),
           "not_slower_than_infonce_spread": bool(delta <= spread["infonce"]),
           "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
           "last_loss": {m: float(v.item()) for m, v in last.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
