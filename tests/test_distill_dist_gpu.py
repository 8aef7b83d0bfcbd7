"""The distilled joint step under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test box
over gloo, arranged as tests/test_sigmoid_dist_gpu.py does, and each runs `JointContrastiveTrainer(distill_weight=1).step` on its half of
a global batch.  The compared step takes its teacher at the initial parameters and starts from a deterministic perturbation of them, so
every process starts it from the same bits.  Checked against ONE process on the global batch doing the same: the loss, L_d, the sampled
parameters, identical replicas (the bounds of tests/test_dist_gpu.py); right after a snapshot L_d is exactly 0 on every rank; all five reduce
spans still fire from inside the backward of a distilled step; a distilled step issues the plain step's collectives plus exactly two
`all_gather_into_tensor` and one `all_reduce`, and before the snapshot exactly the plain step's (counted on every rank)."""
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


def _build(distill):
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
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=1e-4, temperature=TAU, **({"distill_weight": 1.0} if distill else {}))
    return tr, images, ids, mask


def _perturb(tr):
    """move the student off its teacher by a deterministic relative perturbation of every parameter, the same in every process: the
    compared step then starts from identical parameters everywhere (the bounds of tests/test_dist_gpu.py are those of ONE step)"""
    p = tr.optimizer.flat_p
    with torch.no_grad():
        p.mul_(1.0 + 0.3 * torch.cos(0.37 * torch.arange(p.numel(), device=p.device, dtype=torch.float32)))


def _distilled_step(tr, images, ids, mask):
    """snapshot at the initial parameters, perturb the student, one distilled step -> (loss, L_d)"""
    tr.snapshot_teacher()
    _perturb(tr)
    loss = tr.step(images, ids, mask)
    torch.cuda.synchronize()
    return float(loss.item()), tr.current_distill()


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

    def distilled_calls(mine, overlapped):
        mine = list(mine)
        assert mine.count("all_gather_into_tensor") == plain_calls.count("all_gather_into_tensor") + 2, mine
        assert mine.count("all_reduce") == plain_calls.count("all_reduce") + 1 == 1 + 1 + 5, mine
        for name, n in (("all_gather_into_tensor", 2), ("all_reduce", 1)):
            for _ in range(n):
                mine.remove(name)
        assert sorted(mine) == sorted(plain_calls), (mine, plain_calls)                   # and nothing else
        assert sorted(overlapped) == ["head", "layer2", "layer3", "stem", "text"], overlapped

    ref, images, ids, mask = _build(False)            # the yardstick: a plain step on the same shard
    del calls[:]
    ref.step(*shard(images, ids, mask))
    torch.cuda.synchronize()
    plain_calls = list(calls)
    del ref
    # before the snapshot: the plain step's collectives; right after it: the distilled step's, and L_d exactly 0
    tr, images, ids, mask = _build(True)
    assert tr.world == world
    del calls[:]
    tr.step(*shard(images, ids, mask))
    torch.cuda.synchronize()
    assert list(calls) == plain_calls and tr.current_distill() is None, (calls, plain_calls)
    tr.snapshot_teacher()
    ids_opt = {id(p) for p in tr.optimizer.params}
    assert not any(id(p) in ids_opt for m in (tr.teacher.image_model, tr.teacher.text_model) for p in m.parameters())
    del calls[:]
    tr.step(*shard(images, ids, mask))
    torch.cuda.synchronize()
    distilled_calls(calls, tr.last_overlapped)
    exact = tr.current_distill()
    del tr
    # the compared step: teacher = the initial encoders, student perturbed, one step
    tr, images, ids, mask = _build(True)
    del calls[:]
    loss, ld = _distilled_step(tr, *shard(images, ids, mask))
    distilled_calls(calls, tr.last_overlapped)
    sample, total = _probe(tr)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=loss, ld=ld, exact=exact, sample=sample, total=total)
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


def test_two_rank_distilled_step_matches_single_process_global_batch(tmp_path, precision):
    from incremental_multimodal_medical_learning_ii_amd import _lib
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    tol = 3e-4 if _lib.get_precision() == "split_bf16" else 2e-5
    tr, images, ids, mask = _build(True)
    assert tr.world == 1
    tr.snapshot_teacher()
    _perturb(tr)
    before, _ = _probe(tr)
    del tr
    tr, images, ids, mask = _build(True)
    loss, ld = _distilled_step(tr, images.to("cuda"), ids.to("cuda"), mask.to("cuda"))
    sample, _ = _probe(tr)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    bound = tol * 2 * (math.log(B_GLOBAL) + 1.0 / TAU)       # the head's bound on a kl: tol * (|lse| + |lse_t|) <= tol * 2 (ln Bg + 1 / tau)
    print(f"loss single {loss} ranks {float(r[0]['loss'])}; L_d single {ld} ranks {float(r[0]['ld'])} (bound {bound:.2e})")
    assert ld > 100 * 2e-5 * 2 * (math.log(B_GLOBAL) + 1.0 / TAU)      # a distillation term worth comparing: 100 fp32 bounds
    for k in range(world):
        assert float(r[k]["exact"]) == 0.0                   # right after a snapshot, on every rank
        assert abs(float(r[k]["loss"]) - loss) / abs(loss) < 1e-5, (k, float(r[k]["loss"]), loss)
        assert abs(float(r[k]["ld"]) - ld) <= bound, (k, float(r[k]["ld"]), ld)
    # replicas stay identical (same summed gradient, same update) ...
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    assert float(r[0]["ld"]) == float(r[1]["ld"]) and float(r[0]["total"]) == float(r[1]["total"])
    # ... and equal the single-process global-batch update (a sign-like Adam step: the bound of tests/test_dist_gpu.py)
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert np.abs(upd_ref).max() > 0.5e-4 and agree > 0.99, agree
