"""The label-aware (multi-positive) joint step under data parallelism with the REAL HIP kernels: 2 ranks share the one GPU of the
test box over gloo, arranged exactly as tests/test_dist_gpu.py does, and each runs `JointContrastiveTrainer(positives="labels").step`
on its half of a global batch whose label groups straddle the shard boundary.  Checked against ONE process on the global batch:
same loss, same sampled parameters after the optimiser step, identical replicas (the bounds of tests/test_dist_gpu.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_GLOBAL, L, TAU, IMG = 8, 16, 0.07, 64
#          rank 0: rows 0..3                                              | rank 1: rows 4..7
LABELS = [[1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0],   [0, 1, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build():
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
    tr = JointContrastiveTrainer(im.to("cuda"), tm.to("cuda"), lr=1e-4, temperature=TAU, positives="labels")
    return tr, images, ids, mask, torch.tensor(LABELS, dtype=torch.float32)


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
    tr, images, ids, mask, labels = _build()
    assert tr.world == world
    B = B_GLOBAL // world
    sl = slice(rank * B, (rank + 1) * B)
    loss = tr.step(images[sl].to("cuda"), ids[sl].to("cuda"), mask[sl].to("cuda"), labels=labels[sl])
    torch.cuda.synchronize()
    sample, total = _probe(tr)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=float(loss.item()), sample=sample, total=total)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_label_keyed_step_matches_single_process_global_batch(tmp_path, precision):
    import torch.multiprocessing as mp
    B = B_GLOBAL // 2
    lab = torch.tensor(LABELS)
    eq = (lab[:, None, :] == lab[None, :, :]).all(-1)
    assert bool(eq[0, 1]) and not bool(eq[0, B:].any())                 # a group wholly on rank 0 ...
    assert bool(eq[2, B]) and bool(eq[2, B + 1])                        # ... one of three split across the ranks ...
    assert int((eq.sum(1) == 1).sum()) == 3                             # ... and singletons
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path), precision), nprocs=world, join=True)
    tr, images, ids, mask, labels = _build()
    assert tr.world == 1
    loss = tr.step(images.to("cuda"), ids.to("cuda"), mask.to("cuda"), labels=labels)
    torch.cuda.synchronize()
    sample, total = _probe(tr)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    for k in range(world):
        assert abs(float(r[k]["loss"]) - loss.item()) / abs(loss.item()) < 1e-5, (k, float(r[k]["loss"]), loss.item())
    # replicas stay identical (same summed gradient, same update) ...
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    # ... and equal the single-process global-batch update.  Adam's first step moves every weight by ~lr * sign(g), so
    # compare the UPDATE, with the tolerance of a sign-like step on entries whose gradient is ~0.
    tr0, _, _, _, _ = _build()
    before, _ = _probe(tr0)
    tr0.positives = None                      # the keys are in use: the plain loss of the same batch and weights is elsewhere
    plain = tr0.forward_loss(images.to("cuda"), ids.to("cuda"), mask.to("cuda")).item()
    assert abs(plain - loss.item()) > 1e-3, (plain, loss.item())
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert agree > 0.99, agree
