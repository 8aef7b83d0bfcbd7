"""The masked joint step under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test box
over gloo, arranged as tests/test_distill_dist_gpu.py does, and each runs `JointContrastiveTrainer(mlm_weight=...).step` on its half of a
global batch (rank 1 constructed with another seed: it takes rank 0's).  Checked against ONE process on the global batch: the contrastive
loss, L_mlm, the number of masked tokens, identical replicas, and the sampled update (the bounds of tests/test_dist_gpu.py); all five
reduce spans still fire from inside the backward, the "text" span with the head and the tied word embeddings complete; a masked step
issues the plain step's collectives plus exactly one `all_reduce`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_logit_scale_dist_gpu import B_GLOBAL, COLLECTIVES, IMG, L, ROOT, TAU, _free_port, _probe  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

RANK_TIMEOUT_S = 240
SEED, P, W = 21, 0.3, 0.7


def _build(mlm, seed=SEED):
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
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=1e-4, temperature=TAU,
                                 **({"mlm_weight": W, "mlm_probability": P, "mlm_seed": seed} if mlm else {}))
    return tr, images, ids, mask


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

    def shard(images, ids, mask):
        return images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda")

    ref, images, ids, mask = _build(False)            # the yardstick: a plain step on the same shard
    del calls[:]
    ref.step(*shard(images, ids, mask))
    torch.cuda.synchronize()
    plain_calls = list(calls)
    del ref
    tr, images, ids, mask = _build(True, seed=SEED + 5 * rank)
    assert tr.world == world and tr.mlm_state == (SEED, 0)          # rank 0's state, taken at construction
    del calls[:]
    loss = tr.step(*shard(images, ids, mask))
    torch.cuda.synchronize()
    mine = list(calls)
    assert mine.count("all_reduce") == plain_calls.count("all_reduce") + 1 == 1 + 5 + 1, (mine, plain_calls)
    mine.remove("all_reduce")
    assert sorted(mine) == sorted(plain_calls), (mine, plain_calls)                       # and nothing else
    assert sorted(tr.last_overlapped) == ["head", "layer2", "layer3", "stem", "text"], tr.last_overlapped
    info = tr.current_mlm()
    sample, total = _probe(tr)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=float(loss.item()), mlm=info["loss"], acc=info["accuracy"], masked=info["masked"],
             over=info["overflowed"], sample=sample, total=total)
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


def test_two_rank_masked_step_matches_single_process_global_batch(tmp_path, precision):
    from incremental_multimodal_medical_learning_ii_amd import _lib
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    tol = 3e-4 if _lib.get_precision() == "split_bf16" else 2e-5          # the loss heads' tolerance (tests/test_logit_scale_gpu.py)
    tr, images, ids, mask = _build(True)
    assert tr.world == 1
    before, _ = _probe(tr)
    loss = float(tr.step(images.to("cuda"), ids.to("cuda"), mask.to("cuda")).item())
    info = tr.current_mlm()
    sample, _ = _probe(tr)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    print(f"loss single {loss} ranks {float(r[0]['loss'])}; L_mlm single {info['loss']} ranks {float(r[0]['mlm'])}; masked {info['masked']}")
    assert info["masked"] >= 8 and info["overflowed"] == 0
    for k in range(world):
        assert abs(float(r[k]["loss"]) - loss) / abs(loss) < 1e-5, (k, float(r[k]["loss"]), loss)
        assert int(r[k]["masked"]) == info["masked"] and int(r[k]["over"]) == 0             # the shards draw the global batch's masks
        assert abs(float(r[k]["mlm"]) - info["loss"]) <= tol * abs(info["loss"]), (k, float(r[k]["mlm"]), info["loss"])
    # replicas stay identical (same summed gradient, same update) ...
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    assert float(r[0]["mlm"]) == float(r[1]["mlm"]) and float(r[0]["total"]) == float(r[1]["total"])
    # ... and equal the single-process global-batch update (a sign-like Adam step: the bound of tests/test_dist_gpu.py)
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert np.abs(upd_ref).max() > 0.5e-4 and agree > 0.99, agree
