"""Cost of the fused top-k neighbour search plus the kNN vote (`kernels.topk_neighbours` + `kernels.knn_vote`) against
the path the library offered before them: materialise the [N, M] score block with the exact-fp32 GEMM (`kernels.gemm`), then
`torch.topk`, a gather of the label rows and the softmax-weighted mean in torch.

D = 128, k = 20, C = 14 labels, (N, M) in {(1024, 8192), (8192, 65536), (65536, 65536)}, unit-norm Gaussian rows.  The two paths
alternate in one process, timed with device events over enough back-to-back calls that a sample lasts milliseconds; reported per
call: median, min and max over the samples.  The materialised leg is skipped where its buffers do not fit in free memory, and beyond
2^31 block elements, a size the GEMM entry has never been run at.  Where both run, their index lists are compared (both score chains
are k-ascending fp32, so the lists differ only where torch.topk orders equal scores differently) and the votes' largest difference is
reported.  Peak extra device memory of each path is read from the allocator.  No pass / fail number is fixed in advance.  Prints one
JSON line.

    python scripts/knn_cost.py [--sizes 1024x8192 8192x65536 65536x65536] [--rounds 5]
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

MFMA_F32_FLOPS = 157.3e12      # 256 CUs x 4 SIMDs x 64 FLOP/clk (v_mfma_f32_32x32x2_f32) x 2.4 GHz


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1024x8192", "8192x65536", "65536x65536"], help="NxM pairs")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the paths")
    ap.add_argument("--sample-ms", type=float, default=20.0, help="back-to-back calls per sample are chosen to last about this long")
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import kernels as K

    dev = "cuda"
    _lib.set_precision("fp32")          # the materialising GEMM in its exact mode: the same arithmetic as the fused kernel
    D, k, C, T = args.dim, args.k, args.classes, args.temperature

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def peak_extra(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    results = []
    for size in args.sizes:
        N, M = (int(v) for v in size.lower().split("x"))
        g = torch.Generator().manual_seed(N + M)
        Q = torch.nn.functional.normalize(torch.randn(N, D, generator=g)).to(dev)
        G = torch.nn.functional.normalize(torch.randn(M, D, generator=g)).to(dev)
        labels = torch.randint(0, 2, (M, C), generator=g).float().to(dev)
        block_bytes = N * M * 4
        free, _ = torch.cuda.mem_get_info()
        materialise = N * M < 2 ** 31 and 2 * block_bytes + (1 << 30) < free       # torch.topk sorts through temporaries of its own
        S = torch.empty(N, M, dtype=torch.float32, device=dev) if materialise else None
        K.topk_neighbours(Q, G, k)          # the library's workspace exists before the memory is read: it is reused by every call

        def search():
            return K.topk_neighbours(Q, G, k)

        def fused():
            score, index = K.topk_neighbours(Q, G, k)
            return score, index, K.knn_vote(score, index, labels, T)

        def materialised():
            K.gemm(Q, G, S, N, M, D, False, True)
            score, index = torch.topk(S, k, dim=1)
            w = torch.softmax(score / T, dim=1)
            return score, index, (w[:, :, None] * labels[index]).sum(1)

        paths = {"fused": fused, "fused_search_only": search}
        if materialise:
            paths["materialised"] = materialised
        entry = {"N": N, "M": M, "D": D, "k": k, "C": C, "block_bytes": block_bytes, "inputs_bytes": (N + M) * D * 4,
                 "fused_workspace_bytes": int(_lib.load().cxrk_topk_neighbours_slab_bytes(N, M, k))}
        reps, outs = {}, {}
        for name, fn in paths.items():          # warm-up (code objects, allocator), memory, and the calls per sample
            fn()
            outs[name], entry[name + "_peak_extra_bytes"] = peak_extra(fn)
            reps[name] = max(1, min(200, int(args.sample_ms / max(timed(fn, 2), 1e-3))))
        samples = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                samples[name].append(timed(fn, reps[name]))
        for name, t in samples.items():
            entry[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                                   "calls_per_sample": reps[name], "samples": len(t)}
        flop = 2.0 * N * M * D
        entry["search_share_of_f32_mfma_peak"] = round(flop / (entry["fused_search_only_ms"]["median"] * 1e-3) / MFMA_F32_FLOPS, 3)
        if materialise:
            entry["fused_over_materialised"] = round(entry["fused_ms"]["median"] / entry["materialised_ms"]["median"], 3)
            f, m = outs["fused"], outs["materialised"]
            entry["rows_with_another_index_list"] = int((f[1].long() != m[1]).any(1).sum())
            entry["rows_with_another_score_list"] = int((f[0] != m[0]).any(1).sum())
            entry["largest_vote_difference"] = float((f[2] - m[2]).abs().max())
        else:
            entry["materialised_ms"] = None
        results.append(entry)
        del S, outs
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "knn_cost", "precision": "fp32", "results": results}))


if __name__ == "__main__":
    main()
