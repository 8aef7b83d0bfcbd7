"""The learnable-temperature InfoNCE protocol on CPU: 2 processes, gloo backend, `functional._InfoNCE(log_scale=)` driven with the
test-only torch emulation of the kernel wrappers (tests/cpu_kernels_logit_scale.py).  What is checked is the orchestration: each rank
adds (sum_S1 + sum_S2) G o S / (4 Bg) into theta's slot of the flat gradient buffer, the existing sum all-reduce of that buffer
completes d theta, and no collective is issued that the fixed-temperature step does not issue.  Loss and d theta equal the
single-process float64 reference (tests/logit_scale_ref.py) on the global batch, for the plain and the keyed loss; theta is the same
on both ranks after the optimiser step and the clamp."""
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, WORLD, LR = 12, 128, 0.07, 2, 0.05
THETA0 = math.log(1.0 / TAU)
#        rank 0: rows 0..5                 | rank 1: rows 6..11
KEYS = [7, 7, 7, -3, 1 << 40, 11,            -3, 12, 13, 14, (1 << 40) + (1 << 33), 15]
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")


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
    import cpu_kernels_logit_scale as CK
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    Fh.K = CK  # test-only emulation of the kernel wrappers
    cxr_optim.K = CK
    calls = []
    for name in COLLECTIVES:          # count every collective the step issues
        def wrap(fn, name=name):
            def counted(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return counted
        setattr(dist, name, wrap(getattr(dist, name)))
    B = BG // world
    I = torch.from_numpy(syn._normal("dist.I", (BG, D)))
    T = torch.from_numpy(syn._normal("dist.T", (BG, D)))
    sl = slice(rank * B, (rank + 1) * B)
    out = {}
    for tag, keys, learn in (("plain", None, True), ("keyed", KEYS, True), ("plain_fixed", None, False), ("keyed_fixed", KEYS, False)):
        w = torch.nn.Parameter(torch.from_numpy(syn._normal("dist.W", (D, D))) * 0.1)   # a shared "encoder" weight
        theta = torch.nn.Parameter(torch.tensor([THETA0], dtype=torch.float32))
        opt = cxr_optim.SGD([w, theta] if learn else [w], lr=LR)
        assert opt.flat_p.numel() == D * D + (4 if learn else 0)
        del calls[:]
        opt.zero_grad()
        img = (I[sl] @ w).requires_grad_(True)
        txt = T[sl].clone().requires_grad_(True)
        k = None if keys is None else torch.tensor(keys[sl], dtype=torch.int64)
        loss = Fh.infonce_loss(img, txt, TAU, keys=k, log_scale=theta if learn else None)
        (3.0 * loss).backward()                        # an upstream factor: d theta carries it through the device scalar
        if learn:
            assert theta.grad.data_ptr() == opt.flat_g[D * D:].data_ptr()            # written in place: autograd added nothing
            local = float(theta.grad.item())
        opt.all_reduce_grads()
        out[tag] = {"loss": loss.item(), "calls": list(calls)}
        if learn:
            out[tag].update(dtheta=float(opt.flat_g[D * D].item()), dtheta_local=local)
            opt.step()
            CK.clamp_inplace(theta.data, 0.0, math.log(100.0))
            out[tag]["theta"] = float(theta.item())
            out[tag]["theta_bits"] = int(theta.detach().view(torch.int32).item())
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("logit_scale_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def _reference(keys):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import logit_scale_ref as R
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    I = torch.from_numpy(syn._normal("dist.I", (BG, D))).double()
    T = torch.from_numpy(syn._normal("dist.T", (BG, D))).double()
    w = torch.from_numpy(syn._normal("dist.W", (D, D))).double() * 0.1
    theta32 = float(torch.tensor(THETA0, dtype=torch.float32))
    return R.scaled_grads(I @ w, T, theta32, None if keys is None else torch.tensor(keys, dtype=torch.int64))


@pytest.mark.parametrize("tag", ["plain", "keyed"])
def test_two_rank_learnable_temperature_matches_single_process_reference(ranks, tag):
    B = BG // WORLD
    groups = {}
    for i, k in enumerate(KEYS):
        groups.setdefault(k, []).append(i)
    assert any(min(v) < B <= max(v) for v in groups.values())                                # a key group straddles the shard boundary
    loss, _, _, dtheta, abs_sum = _reference(KEYS if tag == "keyed" else None)
    assert abs(dtheta) > 1e-3                                                                # a gradient worth checking
    r = [rk[tag] for rk in ranks]
    for k in range(WORLD):
        print(f"rank {k} {tag}: loss {r[k]['loss']:.7f} ref {loss:.7f}; d theta {r[k]['dtheta']:.7e} ref 3 x {dtheta:.7e} "
              f"(local part {r[k]['dtheta_local']:.7e}, scale {abs_sum:.3e})")
        assert abs(r[k]["loss"] - loss) < 1e-5                                               # every rank reports the global loss
        # fp32 sums against float64: 2e-5 of the summands' magnitude sum |G o S| / (2 Bg), the kernel tests' bound for d theta
        assert abs(r[k]["dtheta"] - 3.0 * dtheta) <= 2e-5 * 3.0 * abs_sum
        assert abs(r[k]["dtheta_local"]) > 0 and abs(r[k]["dtheta_local"] - r[k]["dtheta"]) > 1e-6   # one rank alone does not hold it
    assert abs(r[0]["dtheta_local"] + r[1]["dtheta_local"] - r[0]["dtheta"]) <= 1e-6 * abs(r[0]["dtheta"])   # the all-reduce is a sum
    assert r[0]["theta_bits"] == r[1]["theta_bits"]                                          # theta identical on both ranks
    want = min(max(THETA0 - LR * 3.0 * dtheta, 0.0), math.log(100.0))
    assert abs(r[0]["theta"] - want) < 1e-5, (r[0]["theta"], want)                           # SGD step + clamp


@pytest.mark.parametrize("tag", ["plain", "keyed"])
def test_no_new_collective(ranks, tag):
    for rk in ranks:
        assert rk[tag]["calls"] == rk[tag + "_fixed"]["calls"], (rk[tag]["calls"], rk[tag + "_fixed"]["calls"])
        assert rk[tag]["calls"].count("all_reduce") == 2                                     # the loss, and the ONE flat gradient bucket
    assert ranks[0]["keyed"]["calls"].count("all_gather_into_tensor") == ranks[0]["plain"]["calls"].count("all_gather_into_tensor") + 1
    np.testing.assert_allclose(ranks[0]["plain_fixed"]["loss"], ranks[0]["plain"]["loss"], rtol=1e-5)   # theta0 = log(1 / TAU)
