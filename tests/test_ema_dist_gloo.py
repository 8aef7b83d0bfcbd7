"""The parameter average under data parallelism on CPU: 2 processes, gloo backend, `Trainer(joint_encoders={..., "ema_decay": d})` over
the two small CPU stand-ins for the encoders of tests/test_ema_host.py, driven with the test-only torch emulation of the kernel
wrappers (tests/cpu_kernels_ema.py).  What is checked is the protocol: the ranks are built from DIFFERENT seeds, so
only `Trainer`'s broadcast after construction makes them replicas -- the average begins at the entry of the first step, from the
broadcast values, and is then a function of `flat_p` (identical on every rank after the all-reduced step) and of host integers: it
needs no collective, and the replicas' averages stay bit-identical.  They equal the single-process run on the whole batch within
tests/test_dist_gloo.py's bound."""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, STEPS, LR, DECAY = 2, 3, 0.5, 0.9
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _trainer(seed, patch=setattr, **je):
    """`Trainer` in joint mode on the CPU stand-ins, their weights drawn from `seed`"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpu_kernels_ema as CK
    import test_ema_host as H
    from incremental_multimodal_medical_learning_ii_amd import Trainer as TR
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C, functional as Fh, optim as O
    for mod in (TR, C, Fh, O):
        patch(mod, "K", CK)                      # test-only emulation of the kernel wrappers (undone by monkeypatch in the parent)

    class Engine:
        def __init__(self, model):
            self.model = model

        def to(self, device):
            return self

    torch.manual_seed(seed)
    im, tm = H._Image(), H._Text()
    return TR.Trainer(True, {}, [], "standard", LR, torch.device("cpu"), None, bert_encoder=Engine(tm),
                      joint_encoders={"image_model": im, "temperature": 0.5, "optim": "sgd", **je})


def _batches():
    import test_ema_host as H
    return [H._cpu_batch(k) for k in range(STEPS)]                   # the GLOBAL batches: every rank draws the same ones


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    calls = []
    for name in COLLECTIVES:          # count every collective a step issues
        def wrap(fn, name=name):
            def counted(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return counted
        setattr(dist, name, wrap(getattr(dist, name)))
    ibits = lambda t: t.detach().view(torch.int32).tolist()  # noqa: E731
    out = {}
    for tag, je in (("plain", {}), ("ema", {"ema_decay": DECAY})):
        del calls[:]
        tr = _trainer(100 + rank, **je)          # another seed on every rank: replicas only through the broadcast
        assert tr.world == world and tr.rank == rank
        rec = {"construction": list(calls), "start": ibits(tr.optimizer.flat_p), "steps": []}
        for batch in _batches():
            del calls[:]
            loss = tr._train_step(batch, [], None)
            rec["steps"].append({"calls": list(calls), "loss": float(loss), "p": ibits(tr.optimizer.flat_p),
                                 "avg": None if tr._joint.ema is None else ibits(tr._joint.ema.avg)})
        rec["ema"] = tr._joint.current_ema()
        out[tag] = rec
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("ema_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def _f32(bits_list):
    return torch.tensor(bits_list, dtype=torch.int32).view(torch.float32)


def test_replicas_average_alike_from_the_broadcast_values(ranks):
    a, b = ranks
    assert a["ema"]["start"] == b["ema"]["start"] == a["plain"]["start"]                     # rank 0's weights everywhere
    for k in range(STEPS):
        assert a["ema"]["steps"][k]["avg"] == b["ema"]["steps"][k]["avg"], f"step {k + 1}: the averages differ between the ranks"
        assert a["ema"]["steps"][k]["p"] == b["ema"]["steps"][k]["p"] == a["plain"]["steps"][k]["p"]    # and training is untouched
        assert a["ema"]["steps"][k]["loss"] == a["plain"]["steps"][k]["loss"]
    assert a["ema"]["ema"] == b["ema"]["ema"] == {"updates": STEPS, "decay": DECAY, "last_decay": (1 + STEPS) / (10 + STEPS)}
    # the average began at the broadcast values: its first update is the recurrence from them (tests/ema_ref.py's bound)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ema_ref as E
    avg = _f32(a["ema"]["start"])
    for k in range(STEPS):
        s = a["ema"]["steps"][k]
        assert E.within(_f32(s["avg"]), avg, _f32(s["p"]), E.decay_at(DECAY, k + 1)) <= 1.0, k
        avg = _f32(s["avg"])
    assert float((avg - _f32(a["ema"]["start"])).abs().max()) > 1e-2 and a["ema"]["steps"][-1]["avg"] != a["ema"]["steps"][-1]["p"]


def test_the_average_adds_no_collective(ranks):
    for rk in ranks:
        assert rk["ema"]["construction"] == rk["plain"]["construction"] and rk["plain"]["construction"].count("broadcast") == 1
        plain = rk["plain"]["steps"][0]["calls"]
        assert plain.count("all_reduce") >= 2                                                 # the loss and the flat gradient buffer
        for k in range(STEPS):
            assert rk["ema"]["steps"][k]["calls"] == rk["plain"]["steps"][k]["calls"] == plain, k


def test_the_average_is_that_of_the_single_process_run(ranks, monkeypatch):
    """rank 0's seed in one process on the whole batches: parameters and average within tests/test_dist_gloo.py's bound (1e-4 relative +
    1e-6) of the two-rank run's; the average is 1e-2 and more away from where it began, so the check cannot pass with it standing"""
    tr = _trainer(100, monkeypatch.setattr, ema_decay=DECAY)
    assert tr.world == 1 and tr._joint.ema.avg is None
    for k, batch in enumerate(_batches()):
        tr._train_step(batch, [], None)
        s = ranks[0]["ema"]["steps"][k]
        torch.testing.assert_close(_f32(s["p"]), tr.optimizer.flat_p.detach(), rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(_f32(s["avg"]), tr._joint.ema.avg, rtol=1e-4, atol=1e-6)
