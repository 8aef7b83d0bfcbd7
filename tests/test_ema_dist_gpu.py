"""The parameter average under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the test box over gloo,
arranged as tests/test_ewc_dist_gpu.py, and each runs `JointContrastiveTrainer(ema_decay=...)` on its half of a global batch.  Rank 1
perturbs its parameters after construction and the ranks then broadcast rank 0's flat parameter buffer, as `Trainer` does after it
has built the joint trainer: the average begins at the entry of the first step, from the broadcast values.  It is a function of
`flat_p` (identical on every rank after the all-reduced step) and of host integers: the ranks' averages are bit-identical after each
of three steps, a step with the average issues exactly the collectives of the plain step, and both parameters and average agree with
ONE process on the global batch within the bound tests/test_dist_gpu.py sets for the parameters (> 99 % of a strided sample of the Adam
update, and of the average's displacement, within 2e-6 + 1e-2 |reference|; the losses are printed).

The optimiser is SGD: its update is linear in the gradient, so three steps of two ranks stay as close to the single process as the
all-reduced gradient is, in both contraction precisions.  Adam's sign-like step on gradients near zero amplifies the summation
order of the shards instead -- in split-bf16 mode the PARAMETERS of a two-rank Adam run, with or without the average, agree with
the single process on 96 % of the sample after the third step -- which would measure Adam, not the average.  The displacements
checked stand ten times and more above the absolute term of the bound."""
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
STEPS, LR, DECAY = 3, 1e-2, 0.9


def _build(ema=True):
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
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=LR, temperature=TAU, optim="sgd", **({"ema_decay": DECAY} if ema else {}))
    return tr, images, ids, mask


def _digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _sample(t):
    return t[:: max(1, t.numel() // 4096)].detach().cpu().numpy()


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
    ref, images, ids, mask = _build(ema=False)       # the yardstick for the collectives: the plain step on the same shard
    shard = (images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"))
    del calls[:]
    ref.step(*shard)
    torch.cuda.synchronize()
    plain_calls = list(calls)
    del ref
    tr, _, _, _ = _build()
    assert tr.world == world and tr.ema.avg is None
    start = _digest(tr.optimizer.flat_p)
    if rank == 1:                                    # a replica that is none yet ...
        with torch.no_grad():
            tr.optimizer.flat_p.mul_(1.0 + 2.0 ** -10)
    dist.broadcast(tr.optimizer.flat_p, src=0)       # ... until `Trainer`'s broadcast after construction
    assert tr.ema.avg is None and _digest(tr.optimizer.flat_p) == start
    out = {}
    for step in range(1, STEPS + 1):
        del calls[:]
        loss = tr.step(*shard)
        torch.cuda.synchronize()
        assert list(calls) == plain_calls, (calls, plain_calls)               # no collective is added
        out.update({f"loss{step}": float(loss.item()), f"sample{step}": _probe(tr)[0], f"digest{step}": _digest(tr.optimizer.flat_p),
                    f"avg_digest{step}": _digest(tr.ema.avg), f"avg_sample{step}": _sample(tr.ema.avg)})
    out["updates"], out["last_decay"] = tr.ema.updates, tr.ema.last_decay
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


def test_two_rank_average_matches_the_single_process(tmp_path, precision):
    world, port = 2, _free_port()
    _spawn(world, (world, port, str(tmp_path), precision))
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    tr, images, ids, mask = _build()
    assert tr.world == 1
    batch = (images.to("cuda"), ids.to("cuda"), mask.to("cuda"))
    before, _ = _probe(tr)
    assert int(r[0]["updates"]) == int(r[1]["updates"]) == STEPS and float(r[0]["last_decay"]) == float(r[1]["last_decay"]) == (1 + STEPS) / (10 + STEPS)
    for step in range(1, STEPS + 1):
        loss = tr.step(*batch)
        torch.cuda.synchronize()
        assert str(r[0][f"digest{step}"]) == str(r[1][f"digest{step}"]), f"step {step}: the ranks' parameter buffers differ"
        assert str(r[0][f"avg_digest{step}"]) == str(r[1][f"avg_digest{step}"]), f"step {step}: the ranks' averages differ"
        np.testing.assert_array_equal(r[0][f"avg_sample{step}"], r[1][f"avg_sample{step}"])
        upd_ref, upd_dp = _probe(tr)[0] - before, r[0][f"sample{step}"] - before
        agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
        avg_ref, avg_dp = _sample(tr.ema.avg) - before, r[0][f"avg_sample{step}"] - before
        avg_agree = np.mean(np.abs(avg_ref - avg_dp) <= 2e-6 + 1e-2 * np.abs(avg_ref))
        print(f"step {step}: loss single {loss.item():.7f} ranks {float(r[0][f'loss{step}']):.7f}; update agreement {agree:.5f}, "
              f"average agreement {avg_agree:.5f}; largest |p - start| {np.abs(upd_ref).max():.3e}, |avg - start| {np.abs(avg_ref).max():.3e}")
        assert np.abs(upd_ref).max() > 10 * 2e-6 and agree > 0.99, agree
        assert np.abs(avg_ref).max() > 10 * 2e-6 and avg_agree > 0.99, avg_agree          # the average moved, and moved alike
    assert str(r[0][f"avg_digest{STEPS}"]) != str(r[0][f"digest{STEPS}"])                 # it is not the last iterate
