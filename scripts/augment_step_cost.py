"""Cost of the on-device image augmentation in the headline step: global batch 1024, 224 x 224, L = 32, split-bf16, ResNet-50 + 12-layer
CXR-BERT (the bench configuration).

Two modes, alternated in one process and timed with device events: the plain step (what bench.py times: `cxrk_nchw_to_nhwc` in front
of the stem) and the augmented one (`cxrk_augment_params` + `cxrk_augment_nhwc` in its place, the `drivers.py --augment` default
spec).  ONE trainer serves both modes: it is built with the spec and its augmentation state is taken away for the plain steps, which
then launch exactly the default path's kernels.  Also times the boundary kernels alone on the same images: `nchw_to_nhwc`,
`augment_params` (with and without the mean) and `augment_nhwc` (3- and 1-channel sources), each against its byte floor (source read
+ output written at 8 TB/s).  No pass / fail number is fixed in advance: the yardstick is the plain step of the same run, and its own
spread -- the range of its per-round medians -- is the allowance.  Prints one JSON line.

    python scripts/augment_step_cost.py [--batch 1024] [--rounds 6] [--iters 5]
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

HBM_BYTES_PER_S = 8.0e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--seq-len", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6, help="alternations of the two modes")
    ap.add_argument("--iters", type=int, default=5, help="timed steps per mode and round")
    ap.add_argument("--precision", default="split_bf16", choices=["fp32", "split_bf16"])
    ap.add_argument("--kernels-only", action="store_true", help="only the stand-alone boundary kernels")
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import kernels as K
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.augment import AugmentSpec, DEFAULT_SPEC_ARGS
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer

    dev = "cuda"
    _lib.set_precision(args.precision)
    B, S = args.batch, args.image_size
    spec = AugmentSpec(**DEFAULT_SPEC_ARGS)
    images = syn.synthetic_images(B, S, seed=27).to(dev)
    gray = images[:, :1].contiguous()

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]

    # ---- the boundary kernels alone --------------------------------------------------------------------------------
    rows = K.augment_params(images, spec, 1, 0)
    out = torch.empty(B, S, S, 4, dtype=torch.float32, device=dev)
    no_mean = AugmentSpec(**{**DEFAULT_SPEC_ARGS, "contrast": 0.0})
    src3, src1, dst = images.numel() * 4, gray.numel() * 4, out.numel() * 4
    alone = {
        "nchw_to_nhwc": (lambda: K.nchw_to_nhwc(images, 4), src3 + dst),
        "augment_nhwc": (lambda: K.augment_nhwc(images, 4, rows, out=out), src3 + dst),
        "augment_nhwc_1ch": (lambda: K.augment_nhwc(gray, 4, rows, out=out), src1 + dst),
        "augment_params": (lambda: K.augment_params(images, spec, 1, 0, out=rows), src3),
        "augment_params_no_mean": (lambda: K.augment_params(images, no_mean, 1, 0, out=rows), 0),
    }
    kernels = {}
    for name, (fn, nbytes) in alone.items():
        timed(fn, 3)
        t = timed(fn, 20)
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        kernels[name] = {"ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                         "bytes": nbytes, "floor_ms_at_8TBps": round(floor_ms, 4)}
    rows = K.augment_params(images, spec, 1, 0)
    if args.kernels_only:
        print(json.dumps({"metric": "augment_kernels", "batch": B, "image_size": S, "kernels": kernels}))
        return

    # ---- the step --------------------------------------------------------------------------------------------------
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    im, tm = get_biovil_resnet(None).eval(), CXRBertModel(CXRBertConfig()).eval()
    syn.fill_module_(im)
    syn.fill_module_(tm)
    tr = JointContrastiveTrainer(im.to(dev), tm.to(dev), lr=1e-6, temperature=0.07, augment=spec, augment_seed=1)
    ids, mask = syn.synthetic_tokens(B, args.seq_len, seed=28)
    ids, mask = ids.to(dev), mask.to(dev)
    state = tr._augment                   # [seed, counter]: the step advances it in place

    def set_mode(augmented):
        tr._augment = state if augmented else None

    def step():
        tr.step(images, ids, mask)

    modes = {"plain": False, "augmented": True}
    res = {m: {"step": [], "round_medians": []} for m in modes}
    for m, aug in modes.items():          # warm-up: kernels loaded, allocator settled
        set_mode(aug)
        timed(step, 2)
    for _ in range(args.rounds):
        for m, aug in modes.items():
            set_mode(aug)
            t = timed(step, args.iters)
            res[m]["step"] += t
            res[m]["round_medians"].append(statistics.median(t))
    set_mode(True)
    med = {m: statistics.median(d["step"]) for m, d in res.items()}
    spread = {m: max(res[m]["round_medians"]) - min(res[m]["round_medians"]) for m in res}
    delta = med["augmented"] - med["plain"]
    print(json.dumps({"metric": "augment_step_cost", "batch": B, "image_size": S, "seq_len": args.seq_len, "precision": args.precision,
                      "samples_per_mode": args.rounds * args.iters,
                      "step_ms": {m: round(v, 3) for m, v in med.items()},
                      "step_round_medians_ms": {m: [round(v, 3) for v in res[m]["round_medians"]] for m in res},
                      "spread_ms": {m: round(v, 3) for m, v in spread.items()},
                      "augmented_minus_plain_step_ms": round(delta, 3),
                      "within_plain_spread": bool(abs(delta) <= spread["plain"]),
                      "step_ms_minmax": {m: (round(min(res[m]["step"]), 3), round(max(res[m]["step"]), 3)) for m in res},
                      "augment_state_after": list(tr.augment_state), "kernels": kernels}))


if __name__ == "__main__":
    main()
