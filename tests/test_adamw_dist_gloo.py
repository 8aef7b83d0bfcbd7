"""Clipping under data parallelism on CPU: 2 processes, gloo backend, `optim.AdamW` driven with the test-only torch emulation of the two
kernel wrappers (tests/cpu_kernels_adamw.py).  What is checked is the protocol: the norm is taken after
`all_reduce_grads`, from a buffer that is identical on every rank, by a reduction whose shape depends on n alone -- so every rank
derives the same coefficient, no collective is added, and the replicas stay bit-identical over two clipped steps; the all-reduced
gradient is the CPU oracle's single-process global-batch gradient, and the update is the float64 reference's (tests/optim_ref.py)
on it."""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, WORLD, LR, WD, MAX_NORM, STEPS = 12, 128, 0.07, 2, 0.01, 0.1, 0.05, 2
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
    import cpu_kernels_adamw as CK
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    Fh.K = CK  # test-only emulation of the kernel wrappers
    cxr_optim.K = CK
    calls = []
    for name in COLLECTIVES:          # count every collective a step issues
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
    for tag, kw in (("adam", None), ("clipped", dict(weight_decay=WD, max_grad_norm=MAX_NORM))):
        w = torch.nn.Parameter(torch.from_numpy(syn._normal("dist.W", (D, D))) * 0.1)   # a shared "encoder" weight: decays
        b = torch.nn.Parameter(torch.from_numpy(syn._normal("dist.b", (D,))) * 0.1)     # and its bias: does not
        opt = cxr_optim.Adam([w, b], lr=LR) if kw is None else cxr_optim.AdamW([w, b], lr=LR, **kw)
        steps = []
        for _ in range(STEPS):
            del calls[:]
            opt.zero_grad()
            img = (I[sl] @ w + b).requires_grad_(True)
            txt = T[sl].clone().requires_grad_(True)
            loss = Fh.infonce_loss(img, txt, TAU)
            loss.backward()
            opt.all_reduce_grads()
            local_after_reduce = opt.flat_g.clone()
            opt.step()
            assert torch.equal(opt.flat_g, local_after_reduce)                           # the gradient buffer is left unclipped
            rec = {"calls": list(calls), "p": opt.flat_p.view(torch.int32).tolist(), "g": opt.flat_g.double().tolist()}
            if kw is not None:
                rec.update(norm_bits=int(opt.last_grad_norm.view(torch.int32)), norm=opt.current_grad_norm(), coef=float(opt.last_clip_coef))
            steps.append(rec)
        out[tag] = steps
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("adamw_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def test_replicas_stay_identical_over_two_clipped_steps(ranks):
    for step in range(STEPS):
        a, b = ranks[0]["clipped"][step], ranks[1]["clipped"][step]
        assert a["p"] == b["p"], f"step {step + 1}: the parameter buffers differ between the ranks"
        assert a["norm_bits"] == b["norm_bits"] and a["coef"] == b["coef"]
        assert 0.0 < a["coef"] < 1.0, a["coef"]                                            # clipping was active


def test_clipping_adds_no_collective(ranks):
    for rk in ranks:
        for step in range(STEPS):
            assert rk["clipped"][step]["calls"] == rk["adam"][step]["calls"]
            assert rk["clipped"][step]["calls"].count("all_reduce") == 2                     # the loss, and the ONE flat gradient bucket


def test_update_is_the_reference_on_the_global_batch_gradient(ranks):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import optim_ref as R
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from oracle import ref_loss
    I = torch.from_numpy(syn._normal("dist.I", (BG, D))).double()
    T = torch.from_numpy(syn._normal("dist.T", (BG, D))).double()
    w = (torch.from_numpy(syn._normal("dist.W", (D, D))) * 0.1).double()
    b = (torch.from_numpy(syn._normal("dist.b", (D,))) * 0.1).double()
    p = torch.cat([w.reshape(-1), b])
    decay = torch.cat([torch.ones(D * D, dtype=torch.bool), torch.zeros(D, dtype=torch.bool)])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    for step in range(1, STEPS + 1):
        # the oracle's global-batch gradient at the replica's own parameters: what the all-reduce must have produced
        wl, bl = p[:D * D].reshape(D, D).clone().requires_grad_(True), p[D * D:].clone().requires_grad_(True)
        loss, _ = ref_loss.infonce(I @ wl + bl, T, TAU)
        loss.backward()
        g64 = torch.cat([wl.grad.reshape(-1), bl.grad])
        r = ranks[0]["clipped"][step - 1]
        g = torch.tensor(r["g"], dtype=torch.float64)
        torch.testing.assert_close(g, g64, rtol=1e-4, atol=1e-6)                                          # tests/test_dist_gloo.py's bound
        # the update on that buffer.  (Applied to the oracle's gradient instead, Adam's eps would magnify the 1e-8 differences of the
        # two gradients where coef * |g| is of the order of eps: d update / d g = lr eps / (|g| + eps)^2.)
        p, m, v, norm, coef = R.adamw_step(p, g, m, v, decay, f32(LR), f32(0.9), f32(0.999), f32(1e-8), f32(WD), step, max_norm=f32(MAX_NORM))
        got = torch.tensor(r["p"], dtype=torch.int32).view(torch.float32).double()
        err = float((got - p).abs().max() / p.abs().max())
        print(f"step {step}: norm {r['norm']:.7e} ref {norm:.7e}; coef {r['coef']:.7f} ref {coef:.7f}; parameters rel-to-max err {err:.2e}")
        assert abs(r["norm"] - norm) <= 1e-6 * norm and abs(r["coef"] - coef) <= 1e-6 * coef             # fp32 sums of 16512 terms
        assert err < 1e-6                                                                                 # the Adam kernel tests' bound
        p = got                                                                                           # the next step starts from the replica
