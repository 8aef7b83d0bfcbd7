"""Elastic weight consolidation under data parallelism on CPU: 2 processes, gloo backend, `optim.EWC` over `optim.SGD` driven with the
test-only torch emulation of the kernel wrappers (tests/cpu_kernels_ewc.py).  What is checked is the protocol: the
Fisher estimate, the penalty's gradient and its partial sums are taken after `all_reduce_grads`, from buffers that are identical on
every rank, by kernels whose partition depends on n alone -- so no collective is added and the replicas stay bit-identical through
one plain step, an estimate over two batches, a consolidation and two penalised steps; F is the mean of the squared single-process
global-batch gradients of the CPU oracle, and the parameters follow the float64 reference (tests/ewc_ref.py)."""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, WORLD, LR, STRENGTH = 12, 128, 0.07, 2, 0.05, 3e4
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")
# batch of each phase (rows k * BG .. (k + 1) * BG of the synthetic data): step 1, two estimate batches, two penalised steps
PLAIN, ESTIMATE, PENALISED = 0, (1, 2), (3, 4)
NBATCH = 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    I = torch.from_numpy(syn._normal("ewc.I", (NBATCH * BG, D)))
    T = torch.from_numpy(syn._normal("ewc.T", (NBATCH * BG, D)))
    w = torch.from_numpy(syn._normal("ewc.W", (D, D))) * 0.1
    b = torch.from_numpy(syn._normal("ewc.b", (D,))) * 0.1
    return I, T, w, b


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import cpu_kernels_ewc as CK
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
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
    I, T, w0, b0 = _data()
    w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    opt = cxr_optim.SGD([w, b], lr=LR)
    ewc = cxr_optim.EWC(opt, STRENGTH)

    def gradient(k):
        """zero_grad .. all_reduce_grads on batch k: this rank's rows of it"""
        del calls[:]
        sl = slice(k * BG + rank * B, k * BG + (rank + 1) * B)
        opt.zero_grad()
        img = (I[sl] @ w + b).requires_grad_(True)
        txt = T[sl].clone().requires_grad_(True)
        Fh.infonce_loss(img, txt, TAU).backward()
        opt.all_reduce_grads()

    ibits = lambda t: t.view(torch.int32).tolist()  # noqa: E731
    out = {"steps": [], "estimate": []}

    def step(k):
        gradient(k)
        g = opt.flat_g.clone()
        ewc.apply()
        opt.step()
        rec = {"calls": list(calls), "g": g.double().tolist(), "g_after": ibits(opt.flat_g), "p": ibits(opt.flat_p),
               "penalty": ewc.current_penalty()}
        if ewc.active:
            rec["partials"] = ibits(ewc._partials)
        out["steps"].append(rec)

    step(PLAIN)
    assert torch.equal(opt.flat_g.view(torch.int32), torch.tensor(out["steps"][0]["g_after"], dtype=torch.int32))
    ewc.begin_estimate()
    for k in ESTIMATE:
        gradient(k)
        ewc.accumulate()
        out["estimate"].append({"calls": list(calls), "g": opt.flat_g.double().tolist()})
    del calls[:]
    ewc.consolidate()
    out["consolidate_calls"] = list(calls)
    out["F"], out["anchor"], out["steps_after_consolidation"] = ibits(ewc.F), ibits(ewc.anchor), opt.steps
    for k in PENALISED:
        step(k)
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("ewc_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def _f32(bits_list):
    return torch.tensor(bits_list, dtype=torch.int32).view(torch.float32)


def test_replicas_stay_bit_identical(ranks):
    a, b = ranks
    assert a["F"] == b["F"] and a["anchor"] == b["anchor"]
    assert a["anchor"] == a["steps"][0]["p"] and a["steps_after_consolidation"] == 1          # consolidation moved nothing
    for k in range(3):
        assert a["steps"][k]["p"] == b["steps"][k]["p"], f"step {k + 1}: the parameter buffers differ between the ranks"
        assert a["steps"][k]["g_after"] == b["steps"][k]["g_after"]
    for k in (1, 2):
        assert a["steps"][k]["partials"] == b["steps"][k]["partials"] and a["steps"][k]["penalty"] == b["steps"][k]["penalty"]
    assert a["steps"][0]["penalty"] is None and a["steps"][1]["penalty"] == 0.0 and a["steps"][2]["penalty"] > 0.0


def test_the_penalty_and_the_estimate_add_no_collective(ranks):
    for rk in ranks:
        plain = rk["steps"][0]["calls"]
        assert plain.count("all_reduce") == 2                                                  # the loss, and the ONE flat gradient bucket
        assert rk["steps"][1]["calls"] == plain and rk["steps"][2]["calls"] == plain
        assert all(e["calls"] == plain for e in rk["estimate"]) and rk["consolidate_calls"] == []


def _oracle_gradient(p, k):
    from oracle import ref_loss
    I, T, _, _ = _data()
    I, T = I[k * BG:(k + 1) * BG].double(), T[k * BG:(k + 1) * BG].double()
    wl, bl = p[:D * D].reshape(D, D).clone().requires_grad_(True), p[D * D:].clone().requires_grad_(True)
    loss, _ = ref_loss.infonce(I @ wl + bl, T, TAU)
    loss.backward()
    return torch.cat([wl.grad.reshape(-1), bl.grad])


def test_fisher_is_the_squared_global_batch_gradient(ranks):
    """F = (g_1^2 + g_2^2) / 2 with g_k the oracle's single-process gradient on estimate batch k at the anchor.  Bound: the all-reduced
    gradient is within e = 1e-4 |g| + 1e-6 of the oracle's (tests/test_dist_gloo.py's bound), so its square is within (2 |g| + e) e; the
    kernels add gamma_2 per accumulation and gamma_2 for the merge (tests/ewc_ref.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ewc_ref as E
    r = ranks[0]
    anchor = _f32(r["anchor"]).double()
    F = _f32(r["F"]).double()
    want, bound = torch.zeros_like(F), torch.zeros_like(F)
    for k, est in zip(ESTIMATE, r["estimate"]):
        g64 = _oracle_gradient(anchor, k)
        torch.testing.assert_close(torch.tensor(est["g"], dtype=torch.float64), g64, rtol=1e-4, atol=1e-6)
        e = 1e-4 * g64.abs() + 1e-6
        want += 0.5 * g64 ** 2
        bound += 0.5 * (2 * g64.abs() + e) * e
    bound += 3 * E.gamma_k(2) * want
    err = (F - want).abs()
    print(f"F: max {float(F.max()):.3e}, worst err / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert float(F.max()) > 0


def test_parameters_follow_the_reference(ranks):
    """each step from the replica's own all-reduced gradient and parameters: p' = p - lr (g + strength F (p - a)) in float64.  Bound,
    elementwise: the penalised gradient carries gamma_3 (tests/ewc_ref.py; the emulation rounds strength * t on its own: one more),
    lr * g' and the subtraction one rounding each: gamma_6 (|p| + lr (|g| + strength |F d|))."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ewc_ref as E
    r = ranks[0]
    F, anchor = _f32(r["F"]), _f32(r["anchor"])
    p = anchor
    moved = []
    for k in (1, 2):
        s = r["steps"][k]
        g = torch.tensor(s["g"], dtype=torch.float64)
        want, gp, _ = E.penalised_step(p, g, anchor, F, STRENGTH, LR)
        got = _f32(s["p"]).double()
        pen = E.f32(STRENGTH) * (F.double() * (p.double() - anchor.double())).abs()
        bound = E.gamma_k(6) * (p.double().abs() + E.f32(LR) * (g.abs() + pen))
        err = (got - want).abs()
        print(f"penalised step {k}: largest penalty gradient {float(pen.max()):.3e} vs gradient {float(g.abs().max()):.3e}; "
              f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= bound).all())
        # the penalised gradient buffer itself: gamma_3 for the kernel, one rounding more in the emulation (4 / 3 of the bound)
        assert bool((4 / 3 * E.penalty_grad_bound(g, p, anchor, F, STRENGTH) >=(_f32(s["g_after"]).double() - gp).abs()).all())
        value = E.penalty_value(p, anchor, F, STRENGTH)
        assert s["penalty"] == pytest.approx(value, rel=1e-5, abs=0)                          # fp32 sums of 16512 non-negative terms
        moved.append(float(pen.max()) / float(g.abs().max()))
        p = _f32(s["p"])
    assert moved[0] == 0.0 and moved[1] > 1e-2, moved      # at the anchor the penalty is silent; one step later it is far above the bounds
