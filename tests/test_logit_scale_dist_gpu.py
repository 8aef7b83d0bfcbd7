"""The joint step with a LEARNABLE temperature under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test
box over gloo, arranged as tests/test_multipos_dist_gpu.py does, and each runs `JointContrastiveTrainer(learn_temperature=True).step` on
its half of a global batch.  Checked against ONE process on the global batch: same loss, same sampled parameters and the same theta
after the optimiser step, identical replicas (the bounds of tests/test_dist_gpu.py); the five reduce spans still fire from inside the
backward, theta's slot rides at the end of the "text" span, nothing is left for the final flat all-reduce, and the step issues exactly
the collectives of a fixed-temperature step (counted on every rank)."""
import math
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_GLOBAL, L, TAU, IMG = 8, 16, 0.07, 64
RANK_TIMEOUT_S = 240          # per spawned process: far above the few seconds a rank takes, far below a hung collective's default
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(learn=True):
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
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=1e-4, temperature=TAU, learn_temperature=learn)
    return tr, images, ids, mask


def _probe(tr):
    """loss-independent fingerprint of the replica: a strided sample of the flat parameter buffer + its sum."""
    p = tr.optimizer.flat_p
    return p[:: max(1, p.numel() // 4096)].detach().cpu().numpy(), float(p.double().sum().item())


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
    # the yardstick: a fixed-temperature step on the same shard
    fixed, images, ids, mask = _build(learn=False)
    nf = fixed.optimizer.flat_p.numel()
    assert fixed.logit_scale is None and sorted(fixed._spans.values())[-1][1] == nf
    del calls[:]
    fixed.step(images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
    torch.cuda.synchronize()
    fixed_calls = list(calls)
    assert sorted(fixed.last_overlapped) == ["head", "layer2", "layer3", "stem", "text"], fixed.last_overlapped
    del fixed
    tr, images, ids, mask = _build()
    assert tr.world == world
    n = tr.optimizer.flat_p.numel()
    assert n == nf + 4
    spans = sorted(tr._spans.values())
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == n     # the spans tile the buffer;
    assert tr._spans["text"][1] == n and (tr.logit_scale.data_ptr() - tr.optimizer.flat_p.data_ptr()) // 4 == n - 4   # theta ends the text span
    del calls[:]
    loss = tr.step(images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
    torch.cuda.synchronize()
    # no new collective: the loss's all-reduce and one all-reduce per span, nothing after the backward, as in the fixed step
    assert list(calls) == fixed_calls, (calls, fixed_calls)
    assert calls.count("all_reduce") == 1 + 5, calls
    # every range of the flat gradient buffer was reduced from inside the backward (text encoder + the image encoder's four stages)
    assert sorted(tr.last_overlapped) == ["head", "layer2", "layer3", "stem", "text"], tr.last_overlapped
    sample, total = _probe(tr)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=float(loss.item()), sample=sample, total=total,
             theta=tr.logit_scale.detach().cpu().numpy(), dtheta=tr.logit_scale.grad.detach().cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, args):
    """tests/test_multipos_dist_gpu.py's spawn, with a time limit per process: a rank that hangs is ended and fails the test"""
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


def test_two_rank_learnable_temperature_step_matches_single_process_global_batch(tmp_path, precision):
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    tr, images, ids, mask = _build()
    assert tr.world == 1
    theta0 = tr.logit_scale.detach().cpu().numpy().copy()
    loss = tr.step(images.to("cuda"), ids.to("cuda"), mask.to("cuda"))
    torch.cuda.synchronize()
    sample, total = _probe(tr)
    theta1 = tr.logit_scale.detach().cpu().numpy()
    dtheta = tr.logit_scale.grad.detach().cpu().numpy()
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    for k in range(world):
        assert abs(float(r[k]["loss"]) - loss.item()) / abs(loss.item()) < 1e-5, (k, float(r[k]["loss"]), loss.item())
    # replicas stay identical (same summed gradient, same update), theta included ...
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    assert r[0]["theta"].tobytes() == r[1]["theta"].tobytes() and r[0]["dtheta"].tobytes() == r[1]["dtheta"].tobytes()
    # ... and equal the single-process global-batch update.  Adam's first step moves every weight by ~lr * sign(g), so
    # compare the UPDATE, with the tolerance of a sign-like step on entries whose gradient is ~0.
    tr0, _, _, _ = _build()
    before, _ = _probe(tr0)
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert agree > 0.99, agree
    print(f"theta {theta0} -> single {theta1} / two ranks {r[0]['theta']}; d theta single {dtheta} / two ranks {r[0]['dtheta']}")
    assert abs(float(theta1[0]) - float(theta0[0])) > 0.5e-4                     # theta took its Adam step (lr = 1e-4) ...
    up1, up2 = float(theta1[0]) - float(theta0[0]), float(r[0]["theta"][0]) - float(theta0[0])
    assert abs(up1 - up2) <= 2e-6 + 1e-2 * abs(up1)                              # ... the same one, by the same bound
    assert abs(float(dtheta[0])) > 1e-4 and math.isclose(float(r[0]["dtheta"][0]), float(dtheta[0]), rel_tol=1e-3)   # summed over the ranks
