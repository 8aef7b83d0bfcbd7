"""Cost of the streaming retrieval ranks (`kernels.retrieval_ranks`) against the path the library offered before it:
materialise the [N, M] score block with the exact-fp32 GEMM (`kernels.gemm`), then compare-and-sum in torch.

D = 128, N = M in {1024, 8192, 65536}, unit-norm Gaussian rows, pair form (the positive of query i is gallery row i) and, for the
fused call, the keyed form too (it forms every tile twice).  The two paths alternate in one process, timed with device events over
enough back-to-back calls that a sample lasts milliseconds; reported per call: median, min and max over the samples.  The
materialised leg is skipped where its buffers (fp32 block + two boolean temporaries of torch) do not fit in free memory, and beyond
2^31 block elements, a size the GEMM entry has never been run at.  Where both run, their (greater, ties) are compared: both are
k-ascending fp32 chains, so they should agree bit for bit.  Peak extra device memory of each path is read from the allocator.
No pass / fail number is fixed in advance.  Prints one JSON line.

    python scripts/retrieval_cost.py [--sizes 1024 8192 65536] [--rounds 5]
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192, 65536])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the paths")
    ap.add_argument("--sample-ms", type=float, default=20.0, help="back-to-back calls per sample are chosen to last about this long")
    args = ap.parse_args(argv)

    from incremental_multimodal_medical_learning_ii_amd import _lib
    from incremental_multimodal_medical_learning_ii_amd import kernels as K

    dev = "cuda"
    _lib.set_precision("fp32")          # the materialising GEMM in its exact mode: the same arithmetic as the fused kernel
    D = args.dim

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
    for N in args.sizes:
        g = torch.Generator().manual_seed(N)
        Q = torch.nn.functional.normalize(torch.randn(N, D, generator=g)).to(dev)
        G = torch.nn.functional.normalize(torch.randn(N, D, generator=g)).to(dev)
        keys = torch.arange(N, dtype=torch.int64, device=dev) // 2          # pairs of pairs share a key
        block_bytes = N * N * 4
        free, _ = torch.cuda.mem_get_info()
        materialise = N * N < 2 ** 31 and block_bytes + 2 * N * N + (1 << 30) < free
        S = torch.empty(N, N, dtype=torch.float32, device=dev) if materialise else None

        def fused():
            return K.retrieval_ranks(Q, G)

        def fused_keyed():
            return K.retrieval_ranks(Q, G, keys_q=keys, keys_g=keys)

        def materialised():
            K.gemm(Q, G, S, N, N, D, False, True)
            pos = S.diagonal()
            greater = (S > pos[:, None]).sum(1, dtype=torch.int32)
            ties = (S == pos[:, None]).sum(1, dtype=torch.int32) - 1
            return pos, greater, ties

        paths = {"fused": fused, "fused_keyed": fused_keyed}
        if materialise:
            paths["materialised"] = materialised
        entry = {"N": N, "D": D, "block_bytes": block_bytes, "inputs_bytes": 2 * N * D * 4}
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
        flop = 2.0 * N * N * D
        entry["fused_share_of_f32_mfma_peak"] = round(flop / (entry["fused_ms"]["median"] * 1e-3) / MFMA_F32_FLOPS, 3)
        if materialise:
            entry["fused_over_materialised"] = round(entry["fused_ms"]["median"] / entry["materialised_ms"]["median"], 3)
            entry["mismatching_rows"] = int(((outs["fused"][1] != outs["materialised"][1]) | (outs["fused"][2] != outs["materialised"][2])).sum())
        else:
            entry["materialised_ms"] = None
        results.append(entry)
        del S, outs
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "retrieval_cost", "precision": "fp32", "results": results}))


if __name__ == "__main__":
    main()
