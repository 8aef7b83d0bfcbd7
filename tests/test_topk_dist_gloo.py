"""The data-parallel protocol of the neighbour search and the kNN bank on CPU: 2 processes, gloo, `functional.topk_neighbours` and
`contrastive.KNNBank` driven with the test-only torch emulation of the kernel wrappers (tests/cpu_kernels_topk.py).  What is checked
is the orchestration: the all-gather of the gallery rows, the shard offset of `exclude_self`, the count check and the two gathers of
`KNNBank.finish` -- with integer embeddings every score is exact, so the shards must return EXACTLY the rows of the single-process
result on the concatenated set, index for index, and both ranks the same `predict`."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, C_, WORLD, K_ = 12, 16, 3, 2, 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def data():
    g = torch.Generator().manual_seed(31)
    emb = torch.randint(-3, 4, (N, D), generator=g).float()
    emb[7] = emb[2]                 # duplicated rows on different ranks: exact ties across the shard boundary
    emb[9] = emb[4]
    labels = torch.randint(0, 2, (N, C_), generator=g).float()
    queries = torch.randint(-3, 4, (5, D), generator=g).float()
    return emb, labels, queries


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import cpu_kernels_topk
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    Fh.K = cpu_kernels_topk  # test-only emulation of the kernel wrappers
    emb, labels, queries = data()
    B = N // world
    sl = slice(rank * B, (rank + 1) * B)
    score, index = Fh.topk_neighbours(emb[sl], emb[sl], K_, normalize=False, exclude_self=True, group=dist.group.WORLD)
    keep = Fh.topk_neighbours(emb[sl], emb[sl], K_, normalize=False, group=dist.group.WORLD)
    bank = C.KNNBank()
    bank.add(emb[sl][:2], labels[sl][:2])
    bank.add(emb[sl][2:], labels[sl][2:])
    bank.finish(dist.group.WORLD)
    pred = bank.predict(queries, K_, 0.5)
    uneven = C.KNNBank()
    uneven.add(emb[sl][:B - rank], labels[sl][:B - rank])
    try:
        uneven.finish(dist.group.WORLD)
        refused = ""
    except RuntimeError as e:
        refused = str(e)
    torch.save({"score": score, "index": index, "keep": keep, "bank_emb": bank.emb, "bank_labels": bank.labels, "pred": pred,
                "refused": refused}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_neighbours_and_bank_equal_the_single_process_whole(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpu_kernels_topk as E
    import topk_ref as T
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    emb, labels, queries = data()
    B = N // WORLD
    ws, wi = T.topk_exact(emb, emb, K_, 0)                                     # leave-one-out over the concatenated set
    ks, ki = T.topk_exact(emb, emb, K_)
    assert (np.diff(ws, axis=1) == 0).any() and not np.array_equal(wi, ki)
    assert wi[2, 0] == 7 and wi[7, 0] == 2                                     # the copy on the other rank is the nearest row
    got = [torch.load(tmp_path / f"r{rank}.pt") for rank in range(WORLD)]
    for rank, g in enumerate(got):
        sl = slice(rank * B, (rank + 1) * B)
        assert np.array_equal(g["index"].numpy(), wi[sl]) and np.array_equal(g["score"].numpy().astype(np.float64), ws[sl]), rank
        assert np.array_equal(g["keep"][1].numpy(), ki[sl]) and np.array_equal(g["keep"][0].numpy().astype(np.float64), ks[sl]), rank
        assert torch.equal(g["bank_labels"], labels) and torch.allclose(g["bank_emb"], E.l2norm_fwd(emb)[0])     # rank-major
        assert "between 5 and 6 bank rows" in g["refused"], g["refused"]
    assert torch.equal(got[0]["pred"], got[1]["pred"]) and torch.equal(got[0]["bank_emb"], got[1]["bank_emb"])
    eh, qh = E.l2norm_fwd(emb)[0], E.l2norm_fwd(queries)[0]
    s, i = E.topk_neighbours(qh, eh, K_)
    assert np.abs(got[0]["pred"].numpy() - T.vote_ref(s, i, labels, 0.5)).max() < 1e-5
