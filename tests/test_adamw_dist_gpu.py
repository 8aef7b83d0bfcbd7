"""Gradient clipping under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test box over gloo, arranged
as tests/test_sigmoid_dist_gpu.py does, and each runs two steps of `JointContrastiveTrainer(optim="adamw", weight_decay, max_grad_norm)`
on its half of a global batch.  The norm is taken after the gradient all-reduce, from a buffer that is the same on every rank, by a
reduction whose shape depends on n alone: the ranks' parameter buffers and reported norms are bit-identical after two clipped steps,
the step issues exactly the collectives of the Adam step, and both agree with ONE process on the global batch within the bounds of
tests/test_dist_gpu.py (a sign-like Adam step: > 99 % of a strided sample of the update within 2e-6 + 1e-2 |update|; the norm, a sum
over the gradients, within the 1e-3 relative that file and tests/test_sigmoid_dist_gpu.py put on a summed gradient)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_logit_scale_dist_gpu import B_GLOBAL, COLLECTIVES, IMG, L, ROOT, TAU, _free_port, _probe  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

RANK_TIMEOUT_S = 240
WD, MAX_NORM, STEPS, LR = 0.05, 0.5, 2, 1e-4


def _build(optim="adamw"):
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
    kw = dict(optim="adamw", weight_decay=WD, max_grad_norm=MAX_NORM) if optim == "adamw" else {}
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=LR, temperature=TAU, **kw)
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
    ref, images, ids, mask = _build("adam")          # the yardstick for the collectives: the Adam step on the same shard
    del calls[:]
    ref.step(images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
    torch.cuda.synchronize()
    adam_calls = list(calls)
    del ref
    tr, images, ids, mask = _build()
    assert tr.world == world
    out = {}
    for step in range(1, STEPS + 1):
        del calls[:]
        loss = tr.step(images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
        torch.cuda.synchronize()
        assert list(calls) == adam_calls, (calls, adam_calls)                 # no collective is added
        sample, total = _probe(tr)
        out.update({f"loss{step}": float(loss.item()), f"sample{step}": sample, f"digest{step}": _digest(tr.optimizer.flat_p),
                    f"norm{step}": tr.optimizer.last_grad_norm.cpu().numpy(), f"coef{step}": tr.optimizer.last_clip_coef.cpu().numpy()})
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


def test_two_rank_clipped_steps_are_identical_and_match_the_single_process(tmp_path, precision):
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    tr, images, ids, mask = _build()
    assert tr.world == 1
    before, _ = _probe(tr)
    for step in range(1, STEPS + 1):
        loss = tr.step(images.to("cuda"), ids.to("cuda"), mask.to("cuda"))
        torch.cuda.synchronize()
        sample, _ = _probe(tr)
        norm, coef = float(tr.optimizer.last_grad_norm), float(tr.optimizer.last_clip_coef)
        print(f"step {step}: loss single {loss.item():.7f} ranks {float(r[0][f'loss{step}']):.7f}; norm single {norm:.7e} ranks "
              f"{float(r[0][f'norm{step}'][0]):.7e}; coef single {coef:.7f} ranks {float(r[0][f'coef{step}'][0]):.7f}")
        # replicas: bit-identical parameters, norm and coefficient
        assert str(r[0][f"digest{step}"]) == str(r[1][f"digest{step}"]), f"step {step}: the ranks' parameter buffers differ"
        np.testing.assert_array_equal(r[0][f"sample{step}"], r[1][f"sample{step}"])
        for name in ("norm", "coef"):
            assert r[0][f"{name}{step}"].tobytes() == r[1][f"{name}{step}"].tobytes(), (name, step)
        assert 0.0 < float(r[0][f"coef{step}"][0]) < 1.0 and 0.0 < coef < 1.0                    # clipping was active
        # ... and the single-process step on the global batch
        for k in range(world):
            assert abs(float(r[k][f"loss{step}"]) - loss.item()) / abs(loss.item()) < 1e-5
        assert abs(float(r[0][f"norm{step}"][0]) - norm) <= 1e-3 * norm
        assert abs(float(r[0][f"coef{step}"][0]) - coef) <= 1e-3 * coef
        upd_ref, upd_dp = sample - before, r[0][f"sample{step}"] - before
        agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
        print(f"step {step}: update agreement {agree:.5f}")
        assert np.abs(upd_ref).max() > 0.5e-4 and agree > 0.99, agree
