"""Elastic weight consolidation under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test box over gloo,
arranged as tests/test_adamw_dist_gpu.py, and each runs `JointContrastiveTrainer(ewc_lambda=...)` on its half of a global batch: a
consolidation on one batch, then two penalised steps.  F, the penalty's gradient and its partial sums come from the gradient after
the all-reduce, a buffer that is the same on every rank, through kernels whose partition depends on n alone: the ranks' parameters,
F and penalty are bit-identical, a consolidation batch and a penalised step issue exactly the collectives of the plain step, and
both agree with ONE process on the global batch within the bounds of tests/test_dist_gpu.py (loss within 1e-5 relative; > 99 % of a
strided sample of the Adam update within 2e-6 + 1e-2 |update|; sqrt(sum F), the norm of the summed gradient, within 1e-3 relative)."""
import hashlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_logit_scale_dist_gpu import B_GLOBAL, COLLECTIVES, IMG, L, ROOT, TAU, _free_port, _probe  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

RANK_TIMEOUT_S = 240
STEPS, LR, STRENGTH = 2, 1e-4, 1e6


def _build(ewc=True):
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256,
                        num_hidden_layers=2, max_position_embeddings=32)
    tm = CXRBertModel(cfg).eval()
    im = get_biovil_resnet(None).eval()
    syn.fill_module_(tm)      # name-keyed deterministic weights: identical on every process
    syn.fill_module_(im)
    images = syn.synthetic_images(B_GLOBAL, IMG, seed=3)
    ids, mask = syn.synthetic_tokens(B_GLOBAL, L, vocab=300, seed=4, ragged=True)
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=LR, temperature=TAU, **({"ewc_lambda": STRENGTH} if ewc else {}))
    return tr, images, ids, mask


def _digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _worker(rank, world, port, out_dir, precision):
    sys.path.insert(0, ROOT)
    from incremental_multimodal_medical_learning_ii_amd import _lib
    _lib.set_precision(precision)           # a spawned rank starts from the library default, not the parent's mode
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    calls = []
    for name in COLLECTIVES:          # count every collective a step issues
        def wrap(fn, name=name):
            def counted(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return counted
        setattr(dist, name, wrap(getattr(dist, name)))
    B = B_GLOBAL // world
    sl = slice(rank * B, (rank + 1) * B)
    ref, images, ids, mask = _build(ewc=False)       # the yardstick for the collectives: the plain step on the same shard
    shard = (images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
    del calls[:]
    ref.step(*shard)
    torch.cuda.synchronize()
    plain_calls = list(calls)
    del ref
    tr, _, _, _ = _build()
    assert tr.world == world
    del calls[:]
    assert tr.consolidate([shard]) == 1
    torch.cuda.synchronize()
    assert list(calls) == plain_calls, (calls, plain_calls)                   # a consolidation batch: the plain step's collectives
    out = {"F_digest": _digest(tr.ewc.F), "anchor_digest": _digest(tr.ewc.anchor), "F_sum": float(tr.ewc.F.double().sum().item()),
           "steps_after_consolidation": tr.optimizer.steps}
    for step in range(1, STEPS + 1):
        del calls[:]
        loss = tr.step(*shard)
        torch.cuda.synchronize()
        assert list(calls) == plain_calls, (calls, plain_calls)               # no collective is added
        sample, total = _probe(tr)
        out.update({f"loss{step}": float(loss.item()), f"sample{step}": sample, f"digest{step}": _digest(tr.optimizer.flat_p),
                    f"partials{step}": tr.ewc._partials.cpu().numpy(), f"penalty{step}": tr.current_penalty()})
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, args):
    """tests/test_logit_scale_dist_gpu.py's spawn: a time limit per process, a rank that hangs is ended and fails the test"""
    import time
    import torch.multiprocessing as mp
    ctx = mp.spawn(_worker, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + RANK_TIMEOUT_S
    try:
        while not ctx.join(timeout=max(0.0, min(5.0, deadline - time.monotonic()))):     # returns as soon as a rank ends; raises if one failed
            assert time.monotonic() < deadline, f"a rank did not finish within {RANK_TIMEOUT_S} s"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()


def test_two_rank_consolidation_and_penalised_steps_match_the_single_process(tmp_path, precision):
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    tr, images, ids, mask = _build()
    assert tr.world == 1
    batch = (images.to("cuda"), ids.to("cuda"), mask.to("cuda"))
    before, _ = _probe(tr)
    tr.consolidate([batch])
    # replicas: bit-identical F and anchor, nothing moved; against the single process: the norm of the summed gradient
    assert str(r[0]["F_digest"]) == str(r[1]["F_digest"]) and str(r[0]["anchor_digest"]) == str(r[1]["anchor_digest"])
    assert str(r[0]["anchor_digest"]) == _digest(tr.ewc.anchor) and int(r[0]["steps_after_consolidation"]) == 0
    n1, n2 = math.sqrt(float(tr.ewc.F.double().sum().item())), math.sqrt(float(r[0]["F_sum"]))
    print(f"sqrt(sum F): single {n1:.7e} ranks {n2:.7e}")
    assert n1 > 0 and abs(n2 - n1) <= 1e-3 * n1
    for step in range(1, STEPS + 1):
        loss = tr.step(*batch)
        torch.cuda.synchronize()
        sample, _ = _probe(tr)
        pen = tr.current_penalty()
        print(f"step {step}: loss single {loss.item():.7f} ranks {float(r[0][f'loss{step}']):.7f}; penalty single {pen:.7e} ranks "
              f"{float(r[0][f'penalty{step}']):.7e}")
        assert str(r[0][f"digest{step}"]) == str(r[1][f"digest{step}"]), f"step {step}: the ranks' parameter buffers differ"
        np.testing.assert_array_equal(r[0][f"sample{step}"], r[1][f"sample{step}"])
        assert r[0][f"partials{step}"].tobytes() == r[1][f"partials{step}"].tobytes()
        assert float(r[0][f"penalty{step}"]) == float(r[1][f"penalty{step}"])
        for k in range(world):
            assert abs(float(r[k][f"loss{step}"]) - loss.item()) / abs(loss.item()) < 1e-5
        upd_ref, upd_dp = sample - before, r[0][f"sample{step}"] - before
        agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
        print(f"step {step}: update agreement {agree:.5f}")
        assert np.abs(upd_ref).max() > 0.5e-4 and agree > 0.99, agree
    assert float(r[0]["penalty1"]) == 0.0 and float(r[0]["penalty2"]) > 0.0 and pen > 0.0    # silent at the anchor, active one step later
