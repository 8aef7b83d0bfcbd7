"""The keyed (multi-positive) InfoNCE protocol on CPU: 2 processes, gloo backend, `functional._InfoNCE` driven with the test-only
torch emulation of the kernel wrappers (tests/cpu_kernels_multipos.py).  What is checked is the orchestration: the all-gather of
the keys, which slice is the row keys and which vector the column keys, the use of the stats kernel's counts, and that no exchange
of counts is needed -- every rank's loss, d img, d txt and the all-reduced weight gradient equal the single-process float64
reference (tests/multipos_ref.py) on the global batch."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, WORLD = 12, 128, 0.07, 2
#        rank 0: rows 0..5                 | rank 1: rows 6..11
KEYS = [7, 7, 7, -3, 1 << 40, 11,            -3, 12, 13, 14, (1 << 40) + (1 << 33), 15]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import cpu_kernels_multipos
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    Fh.K = cpu_kernels_multipos  # test-only emulation of the kernel wrappers
    B = BG // world
    I = torch.from_numpy(syn._normal("dist.I", (BG, D)))
    T = torch.from_numpy(syn._normal("dist.T", (BG, D)))
    w = torch.nn.Parameter(torch.from_numpy(syn._normal("dist.W", (D, D))) * 0.1)   # a shared "encoder" weight
    sl = slice(rank * B, (rank + 1) * B)
    opt = cxr_optim.SGD([w], lr=0.1)
    opt.zero_grad()
    img = (I[sl] @ w).requires_grad_(True)
    img.retain_grad()
    txt = T[sl].clone().requires_grad_(True)
    loss = Fh.infonce_loss(img, txt, TAU, keys=torch.tensor(KEYS[sl], dtype=torch.int64))
    loss.backward()
    opt.all_reduce_grads()
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=loss.item(), dimg=img.grad.numpy(), dtxt=txt.grad.numpy(),
             dw=opt.flat_g[: D * D].reshape(D, D).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_keyed_infonce_matches_single_process_reference(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import multipos_ref
    B = BG // WORLD
    keys = torch.tensor(KEYS, dtype=torch.int64)
    groups = {}
    for i, k in enumerate(KEYS):
        groups.setdefault(k, []).append(i)
    sizes = sorted(len(v) for v in groups.values())
    assert any(len(v) >= 3 and all(i < B for i in v) for v in groups.values())             # one group wholly on rank 0
    assert any(min(v) < B <= max(v) for v in groups.values())                                # one split across the ranks
    assert sizes.count(1) == len(sizes) - 2                                                  # the rest are singletons
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    I = torch.from_numpy(syn._normal("dist.I", (BG, D))).double()
    T = torch.from_numpy(syn._normal("dist.T", (BG, D))).double().requires_grad_(True)
    w = (torch.from_numpy(syn._normal("dist.W", (D, D))).double() * 0.1).requires_grad_(True)
    img = I @ w
    img.retain_grad()
    loss, _ = multipos_ref.multipos_loss(img, T, keys, TAU)
    loss.backward()
    plain, _ = multipos_ref.multipos_loss(img.detach(), T.detach(), torch.arange(BG), TAU)
    assert abs(plain.item() - loss.item()) > 1e-3                                            # the keys matter at this size
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(WORLD)]
    for k in range(WORLD):
        assert abs(float(r[k]["loss"]) - loss.item()) < 1e-5                      # every rank reports the global loss
        np.testing.assert_allclose(r[k]["dimg"], img.grad[k * B:(k + 1) * B].numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(r[k]["dtxt"], T.grad[k * B:(k + 1) * B].numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(r[k]["dw"], w.grad.numpy(), rtol=1e-4, atol=1e-6)  # summed over ranks = global grad
