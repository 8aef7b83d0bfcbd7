"""The neighbour search and the kNN bank under data parallelism with the REAL kernels: 2 ranks share the one GPU of the test box over
gloo, arranged as tests/test_retrieval_dist_gpu.py.  Integer embeddings with normalize=False: every score is exact, so the sharded
`functional.topk_neighbours(..., exclude_self=True, group)` must equal the single-process result on the concatenated set, index for
index, and exactly the int64 reference's (tests/topk_ref.py); both ranks return the same `KNNBank.predict`, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, C_, WORLD, K_ = 300, 24, 4, 2, 10        # 150 rows per rank: each shard crosses a 128-row strip, the gallery a column tile


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def data():
    g = torch.Generator().manual_seed(37)
    emb = torch.randint(-3, 4, (N, D), generator=g).float()
    emb[200] = emb[20]              # duplicated rows on different ranks: exact ties across the shard boundary
    emb[160] = emb[140]
    labels = torch.randint(0, 2, (N, C_), generator=g).float()
    queries = torch.randn(40, D, generator=g)
    return emb, labels, queries


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    emb, labels, queries = data()
    B = N // world
    sl = slice(rank * B, (rank + 1) * B)
    e = emb[sl].to("cuda")
    score, index = Fh.topk_neighbours(e, e, K_, normalize=False, exclude_self=True, group=dist.group.WORLD)
    bank = C.KNNBank()
    bank.add(e, labels[sl].to("cuda"))
    bank.finish(dist.group.WORLD)
    pred = bank.predict(queries.to("cuda"), K_, 0.07)
    torch.cuda.synchronize()
    torch.save({"score": score.cpu(), "index": index.cpu(), "pred": pred.cpu(), "rows": len(bank)}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_neighbours_equal_one_process_on_the_whole_set(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import topk_ref as T
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    emb, labels, queries = data()
    ws, wi = T.topk_exact(emb, emb, K_, 0)
    assert wi[20, 0] == 200 and wi[200, 0] == 20 and (np.diff(ws, axis=1) == 0).any()
    e = emb.to("cuda")
    one = Fh.topk_neighbours(e, e, K_, normalize=False, exclude_self=True)
    assert np.array_equal(one[1].cpu().numpy(), wi) and np.array_equal(one[0].cpu().numpy().astype(np.float64), ws)
    bank = C.KNNBank()
    bank.add(e, labels.to("cuda"))
    want_pred = bank.finish().predict(queries.to("cuda"), K_, 0.07).cpu()
    assert bool(torch.isfinite(want_pred).all())
    B = N // WORLD
    for rank in range(WORLD):
        g = torch.load(tmp_path / f"r{rank}.pt")
        sl = slice(rank * B, (rank + 1) * B)
        assert np.array_equal(g["index"].numpy(), wi[sl]) and np.array_equal(g["score"].numpy().astype(np.float64), ws[sl]), rank
        assert g["rows"] == N and torch.equal(g["pred"], want_pred), rank
