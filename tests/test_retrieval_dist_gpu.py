"""The retrieval evaluation under data parallelism with the REAL kernel: 2 ranks share the one GPU of the test box over gloo, arranged
as tests/test_multipos_dist_gpu.py, and each calls `contrastive.retrieval_metrics(..., group)` on its half of a set whose key groups
and duplicated rows straddle the shard boundary.  Integer embeddings with normalize=False: every score is exact, so both ranks must
return EXACTLY the single-process metrics of the whole set, and exactly the int64 reference's (tests/retrieval_ref.py).  No encoder
runs here: nothing depends on the tile policy of a batch size."""
import json
import os
import socket
import sys

import pytest
import torch

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, WORLD, KS = 300, 24, 2, (1, 5, 10)       # 150 rows per rank: each shard crosses a 128-row strip, the gallery a column tile


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def data():
    g = torch.Generator().manual_seed(29)
    img = torch.randint(-3, 4, (N, D), generator=g).float()
    txt = torch.randint(-3, 4, (N, D), generator=g).float()
    txt[200] = txt[20]              # duplicated rows on different ranks: exact ties across the shard boundary
    img[160] = img[140]
    keys = 1000 + torch.arange(N, dtype=torch.int64)
    keys[149], keys[150], keys[3] = 7, 7, 7             # a group of three across the boundary
    keys[10], keys[290] = -5, -5                        # a pair across the boundary, negative key
    keys[151] = keys[152] + (1 << 33)                   # equal to its neighbour's key in the low 32 bits only
    return img, txt, keys


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    img, txt, keys = data()
    B = N // world
    sl = slice(rank * B, (rank + 1) * B)
    i, t, k = img[sl].to("cuda"), txt[sl].to("cuda"), keys[sl].to("cuda")
    out = {"pair": C.retrieval_metrics(i, t, None, KS, dist.group.WORLD, normalize=False),
           "keyed": C.retrieval_metrics(i, t, k, KS, dist.group.WORLD, normalize=False)}
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_retrieval_metrics_equal_one_process_on_the_whole_set(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import retrieval_ref as R
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    mp.spawn(_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    img, txt, keys = data()
    want = {"pair": R.metrics_both(img, txt, None, KS), "keyed": R.metrics_both(img, txt, keys, KS)}
    assert want["pair"] != want["keyed"]
    one = {"pair": C.retrieval_metrics(img.to("cuda"), txt.to("cuda"), None, KS, normalize=False),
           "keyed": C.retrieval_metrics(img.to("cuda"), txt.to("cuda"), keys.to("cuda"), KS, normalize=False)}
    assert one == want
    for rank in range(WORLD):
        with open(tmp_path / f"r{rank}.json") as f:
            got = json.load(f)
        assert got == want, (rank, got, want)
