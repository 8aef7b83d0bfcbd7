"""The pairwise sigmoid loss's data-parallel protocol on CPU: 2 processes, gloo backend, `functional._SigmoidPairs` driven with the
test-only torch emulation of the kernel wrappers (tests/cpu_kernels_sigmoid.py).  What is checked is the orchestration: each rank's S1
block carries the complete rows of g, so each rank adds its rows' share of d theta and d b into the two slots of the flat gradient
buffer and the existing sum all-reduce of that buffer completes them; the step issues the InfoNCE step's collectives minus exactly the
two log-sum-exp `all_gather_into_tensor`.  Loss, d theta, d b and the shared weight's gradient equal the single-process float64
reference (tests/sigmoid_ref.py) on the global batch, plain and keyed; theta and b are the same on both ranks after the step."""
import json
import math
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, BIAS, WORLD, LR = 12, 128, 0.07, -2.0, 2, 0.05
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
    import cpu_kernels_sigmoid as CK
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
    for tag, keys, sigmoid in (("plain", None, True), ("keyed", KEYS, True), ("plain_infonce", None, False), ("keyed_infonce", KEYS, False)):
        w = torch.nn.Parameter(torch.from_numpy(syn._normal("dist.W", (D, D))) * 0.1)   # a shared "encoder" weight
        theta = torch.nn.Parameter(torch.tensor([THETA0], dtype=torch.float32))
        bias = torch.nn.Parameter(torch.tensor([BIAS], dtype=torch.float32))
        opt = cxr_optim.SGD([w, theta, bias] if sigmoid else [w, theta], lr=LR)
        assert opt.flat_p.numel() == D * D + (8 if sigmoid else 4)
        del calls[:]
        opt.zero_grad()
        img = (I[sl] @ w).requires_grad_(True)
        txt = T[sl].clone().requires_grad_(True)
        k = None if keys is None else torch.tensor(keys[sl], dtype=torch.int64)
        if sigmoid:
            loss = Fh.sigmoid_pairs_loss(img, txt, theta, bias, keys=k)
        else:
            loss = Fh.infonce_loss(img, txt, TAU, keys=k, log_scale=theta)
        (3.0 * loss).backward()                        # an upstream factor: d theta and d b carry it through the device scalar
        local = None
        if sigmoid:
            assert theta.grad.data_ptr() == opt.flat_g[D * D:].data_ptr()            # written in place: autograd added nothing
            assert bias.grad.data_ptr() == opt.flat_g[D * D + 4:].data_ptr()
            local = (float(theta.grad.item()), float(bias.grad.item()))
        opt.all_reduce_grads()
        out[tag] = {"loss": loss.item(), "calls": list(calls)}
        if sigmoid:
            out[tag].update(dtheta=float(opt.flat_g[D * D].item()), db=float(opt.flat_g[D * D + 4].item()), local=local,
                            dw=opt.flat_g[:D * D].double().tolist())
            opt.step()
            out[tag]["theta_bits"] = int(theta.detach().view(torch.int32).item())
            out[tag]["bias_bits"] = int(bias.detach().view(torch.int32).item())
            out[tag]["theta"], out[tag]["bias"] = float(theta.item()), float(bias.item())
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("sigmoid_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def _reference(keys):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sigmoid_ref as R
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    I = torch.from_numpy(syn._normal("dist.I", (BG, D))).double()
    T = torch.from_numpy(syn._normal("dist.T", (BG, D))).double()
    w = torch.from_numpy(syn._normal("dist.W", (D, D))).double() * 0.1
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    ref = R.sigmoid_grads(I @ w, T, f32(THETA0), f32(BIAS), None if keys is None else torch.tensor(keys, dtype=torch.int64))
    ref["dw"] = I.T @ ref["dimg"]
    return ref


@pytest.mark.parametrize("tag", ["plain", "keyed"])
def test_two_rank_sigmoid_loss_matches_single_process_reference(ranks, tag):
    B = BG // WORLD
    groups = {}
    for i, k in enumerate(KEYS):
        groups.setdefault(k, []).append(i)
    assert any(min(v) < B <= max(v) for v in groups.values())                                # a key group straddles the shard boundary
    ref = _reference(KEYS if tag == "keyed" else None)
    assert abs(ref["dtheta"]) > 1e-3 and abs(ref["db"]) > 1e-3                               # gradients worth checking
    r = [rk[tag] for rk in ranks]
    for k in range(WORLD):
        print(f"rank {k} {tag}: loss {r[k]['loss']:.7f} ref {ref['loss']:.7f}; d theta {r[k]['dtheta']:.7e} ref 3 x {ref['dtheta']:.7e}; "
              f"d b {r[k]['db']:.7e} ref 3 x {ref['db']:.7e} (local parts {r[k]['local']})")
        assert abs(r[k]["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"])                     # every rank reports the global loss
        # fp32 sums against float64: 2e-5 of the summands' magnitude, the kernel tests' bound for d theta and d b
        assert abs(r[k]["dtheta"] - 3.0 * ref["dtheta"]) <= 2e-5 * 3.0 * ref["mag_theta"]
        assert abs(r[k]["db"] - 3.0 * ref["db"]) <= 2e-5 * 3.0 * ref["mag_b"]
        for q, name in ((0, "dtheta"), (1, "db")):                                           # one rank alone does not hold them
            assert abs(r[k]["local"][q]) > 0 and abs(r[k]["local"][q] - r[k][name]) > 1e-6
        torch.testing.assert_close(torch.tensor(r[k]["dw"], dtype=torch.float64).reshape(D, D), 3.0 * ref["dw"], rtol=1e-4, atol=1e-6)   # the shared weight
    for q, name in ((0, "dtheta"), (1, "db")):                                               # the all-reduce is a sum
        assert abs(r[0]["local"][q] + r[1]["local"][q] - r[0][name]) <= 1e-6 * abs(r[0][name])
    assert r[0]["theta_bits"] == r[1]["theta_bits"] and r[0]["bias_bits"] == r[1]["bias_bits"]   # identical on both ranks
    assert abs(r[0]["theta"] - (THETA0 - LR * 3.0 * ref["dtheta"])) < 1e-5                   # the SGD step
    assert abs(r[0]["bias"] - (BIAS - LR * 3.0 * ref["db"])) < 1e-5
    if tag == "keyed":
        assert abs(r[0]["loss"] - ranks[0]["plain"]["loss"]) > 1e-3                          # the keys are not ignored


@pytest.mark.parametrize("tag", ["plain", "keyed"])
def test_two_fewer_collectives_than_infonce(ranks, tag):
    for rk in ranks:
        mine, theirs = list(rk[tag]["calls"]), list(rk[tag + "_infonce"]["calls"])
        assert theirs.count("all_gather_into_tensor") == mine.count("all_gather_into_tensor") + 2
        for _ in range(2):                                                                   # exactly the two log-sum-exp gathers: the last two
            idx = len(theirs) - 1 - theirs[::-1].index("all_gather_into_tensor")
            del theirs[idx]
        assert mine == theirs, (mine, rk[tag + "_infonce"]["calls"])
        assert mine.count("all_reduce") == 2                                                 # the loss, and the ONE flat gradient bucket
    assert ranks[0]["keyed"]["calls"].count("all_gather_into_tensor") == ranks[0]["plain"]["calls"].count("all_gather_into_tensor") + 1
