"""A-GEM under data parallelism on CPU: 2 processes, gloo backend, `optim.AGEM` over `optim.SGD` with a `memory.EpisodicMemory` per
rank, driven with the test-only torch emulation of the kernel wrappers (tests/cpu_kernels_agem.py).  What is checked is the protocol
(DESIGN.md §5.12): every rank remembers rows of its own shards and draws the same indices from them; the reference gradient and the
step's gradient are both all-reduced before the dots are taken, by kernels whose partition depends on n alone -- so the projection
is decided identically everywhere, a projected step issues the collectives of two gradient computations and nothing more, and the
replicas stay bit-identical through a plain step, a remembered task, a step that is not projected and one that is; both gradients are
those of the CPU oracle on the single-process global batch (the memory's rows of all ranks together), and the parameters follow the
float64 projection (tests/agem_ref.py)."""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, D, TAU, WORLD, LR, SEED = 12, 128, 0.07, 2, 0.05, 5
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")
# batch of each phase (rows k * BG .. (k + 1) * BG of the synthetic data): the plain step; the remembered task, which is also the
# batch of both A-GEM steps -- as it is (the gradients agree), then with its report features negated: every pair is pushed apart
# where the memory pulls it together (the gradients conflict: g . gref = -10.4 against |gref|^2 = 12.2 in the oracle)
PLAIN, TASK = 0, 1
NBATCH = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    I = torch.from_numpy(syn._normal("agem.I", (NBATCH * BG, D)))
    T = torch.from_numpy(syn._normal("agem.T", (NBATCH * BG, D)))
    w = torch.from_numpy(syn._normal("agem.W", (D, D))) * 0.1
    b = torch.from_numpy(syn._normal("agem.b", (D,))) * 0.1
    return I, T, w, b


def _current(I, T, negate):
    """the global batch of an A-GEM step: the task's images with their own report features, or with these negated"""
    Ic, Tc = I[TASK * BG:(TASK + 1) * BG], T[TASK * BG:(TASK + 1) * BG]
    return Ic, (-Tc if negate else Tc)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import cpu_kernels_agem as CK
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
    from incremental_multimodal_medical_learning_ii_amd.memory import EpisodicMemory
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
    agem = cxr_optim.AGEM(opt)
    mem = EpisodicMemory(B, seed=SEED)
    mine = slice(rank * B, (rank + 1) * B)

    def gradient(Irows, Trows):
        """zero_grad .. all_reduce_grads on this rank's rows"""
        opt.zero_grad()
        img = (Irows @ w + b).requires_grad_(True)
        txt = Trows.clone().requires_grad_(True)
        Fh.infonce_loss(img, txt, TAU).backward()
        opt.all_reduce_grads()

    ibits = lambda t: t.view(torch.int32).tolist()  # noqa: E731
    out = {"steps": []}

    def step(Ig, Tg, k):
        """one optimiser step on this rank's rows of the global batch (Ig, Tg); with rows in the memory, A-GEM's order: the reference
        pass on memory rows drawn with step index k, the step's gradient, the projection, the update"""
        del calls[:]
        rec = {}
        if len(mem) > 0:
            rows = mem.sample(B, step=k)
            rec["memory_rows"] = rows[3].tolist()
            gradient(rows[0], rows[1])
            agem.store_reference()
            rec["gref"] = agem.gref.double().tolist()
        gradient(Ig[mine], Tg[mine])
        rec["g"] = opt.flat_g.double().tolist()
        agem.apply()
        rec["g_after"] = ibits(opt.flat_g)
        rec["p_before"] = ibits(opt.flat_p)
        opt.step()
        rec.update(calls=list(calls), p=ibits(opt.flat_p), info=agem.current_interference())
        if agem._partials is not None:
            rec["partials"] = ibits(agem._partials)
        out["steps"].append(rec)

    step(I[PLAIN * BG:(PLAIN + 1) * BG], T[PLAIN * BG:(PLAIN + 1) * BG], 0)
    del calls[:]
    # the task arrives in two batches; a row's global index travels as its key.  Token rows here are the text features themselves.
    task = slice(TASK * BG, (TASK + 1) * BG)
    Ik, Tk, idx = I[task][mine], T[task][mine], torch.arange(TASK * BG, (TASK + 1) * BG)[mine]
    # `JointContrastiveTrainer.remember` itself, on a stand-in that carries what it reads: the memory, the projection and the group
    from types import SimpleNamespace
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    joint = SimpleNamespace(memory=mem, agem=agem, world=world, group=None)
    kept = JointContrastiveTrainer.remember(joint, [(Ik[:4], Tk[:4], torch.ones_like(Tk[:4]), idx[:4]),
                                                    (Ik[4:], Tk[4:], torch.ones_like(Tk[4:]), idx[4:])])
    out["kept"], out["remember_calls"], out["steps_after_remember"] = kept, list(calls), opt.steps
    step(*_current(I, T, False), 1)
    step(*_current(I, T, True), 2)
    uneven = SimpleNamespace(memory=EpisodicMemory(B, seed=SEED), agem=cxr_optim.AGEM(opt), world=world, group=None)
    n = 3 - rank                                                     # rank 0 offers three rows of a task, rank 1 two
    try:
        JointContrastiveTrainer.remember(uneven, [(Ik[:n], Tk[:n], torch.ones_like(Tk[:n]), idx[:n])])
        out["uneven"] = None
    except RuntimeError as e:
        out["uneven"] = str(e)
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    d = tmp_path_factory.mktemp("agem_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d)), nprocs=WORLD, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)]


def _f32(bits_list):
    return torch.tensor(bits_list, dtype=torch.int32).view(torch.float32)


def test_replicas_stay_bit_identical(ranks):
    a, b = ranks
    assert a["kept"] == b["kept"] == BG // WORLD and a["steps_after_remember"] == 1
    for k in range(3):
        assert a["steps"][k]["p"] == b["steps"][k]["p"], f"step {k + 1}: the parameter buffers differ between the ranks"
        assert a["steps"][k]["g_after"] == b["steps"][k]["g_after"]
        assert a["steps"][k]["info"] == b["steps"][k]["info"]
    for k in (1, 2):
        assert a["steps"][k]["partials"] == b["steps"][k]["partials"] and a["steps"][k]["gref"] == b["steps"][k]["gref"]
    assert a["steps"][0]["info"] is None and "gref" not in a["steps"][0]                       # before the memory holds a row
    infos = [a["steps"][k]["info"] for k in (1, 2)]
    print("dots:", [i["dot"] for i in infos], "coefficients:", [i["coef"] for i in infos])
    assert infos[0]["dot"] > 0 and (infos[0]["projected"], infos[0]["applied"], infos[0]["coef"]) == (0, 1, 0.0)
    assert infos[1]["dot"] < 0 and (infos[1]["projected"], infos[1]["applied"]) == (1, 2) and infos[1]["coef"] < 0
    s = a["steps"][1]                                                # not projected: the gradient buffer is the all-reduced one, bit for bit
    assert torch.equal(_f32(s["g_after"]).double(), torch.tensor(s["g"], dtype=torch.float64))


def test_every_rank_draws_the_same_slots_of_its_own_rows(ranks):
    B = BG // WORLD
    for k in (1, 2):
        rows = [r["steps"][k]["memory_rows"] for r in ranks]
        for rk, mine in enumerate(rows):
            assert sorted(mine) == list(range(TASK * BG + rk * B, TASK * BG + (rk + 1) * B))   # its own shard, each row once
        assert [i - TASK * BG for i in rows[0]] == [i - TASK * BG - B for i in rows[1]]         # the same draw on both ranks


def test_a_projected_step_issues_the_collectives_of_two_gradients(ranks):
    for rk in ranks:
        plain = rk["steps"][0]["calls"]
        assert plain.count("all_reduce") == 2                                                  # the loss, and the ONE flat gradient bucket
        assert rk["steps"][1]["calls"] == plain + plain and rk["steps"][2]["calls"] == plain + plain
        assert rk["remember_calls"] == ["all_reduce"]                                          # the one check that the counts agree


def test_remember_refuses_ranks_with_different_row_counts(ranks):
    for rk in ranks:
        assert rk["uneven"] is not None and "between 2 and 3 memory rows" in rk["uneven"]


def _oracle_gradient(p, I, T):
    from oracle import ref_loss
    wl, bl = p[:D * D].reshape(D, D).clone().requires_grad_(True), p[D * D:].clone().requires_grad_(True)
    loss, _ = ref_loss.infonce(I.double() @ wl + bl, T.double(), TAU)
    loss.backward()
    return torch.cat([wl.grad.reshape(-1), bl.grad])


def test_both_gradients_are_the_single_process_global_batch_gradients(ranks):
    """the reference gradient is the oracle's on the memory rows of all ranks together (in rank order), the step's the oracle's on the
    global batch; tests/test_dist_gloo.py's bound for an all-reduced InfoNCE gradient"""
    I, T, _, _ = _data()
    r = ranks[0]
    for k, negate in ((1, False), (2, True)):
        s = r["steps"][k]
        p = _f32(s["p_before"]).double()
        rows = torch.tensor([i for rk in ranks for i in rk["steps"][k]["memory_rows"]])
        torch.testing.assert_close(torch.tensor(s["gref"], dtype=torch.float64), _oracle_gradient(p, I[rows], T[rows]), rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(torch.tensor(s["g"], dtype=torch.float64), _oracle_gradient(p, *_current(I, T, negate)), rtol=1e-4, atol=1e-6)


def test_parameters_follow_the_reference(ranks):
    """each step from the replica's own all-reduced gradients and parameters, in float64: p' = p - lr * project(g, gref).  The
    emulation sums the n products in torch's order, each rounded on its own: gamma_(n + 1) in the place of the kernel's gamma_total in
    the coefficient's bound (tests/agem_ref.py).  Elementwise: coef * gref, the subtraction, lr * g' and the update round once each:
    gamma_4 (|p| + lr (|g| + |coef gref|)) around the float64 step taken with the emulation's own fp32 coefficient."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import agem_ref as A
    r = ranks[0]
    for k in (1, 2):
        s = r["steps"][k]
        g, gref = torch.tensor(s["g"], dtype=torch.float64), torch.tensor(s["gref"], dtype=torch.float64)
        p = _f32(s["p_before"]).double()
        Dd, RR, S = A.dots(g, gref)
        info = s["info"]
        gam = A.gamma_k(g.numel() + 1)
        assert abs(info["dot"] - Dd) <= gam * S and abs(info["ref_sqnorm"] - RR) <= gam * RR
        assert (Dd < 0) == (k == 2) and abs(Dd) >= 1e2 * gam * S                            # no sign decided by rounding: 100 worst-case bounds away
        coef = info["coef"]
        if k == 2:
            cbound = (abs(Dd) * (A.U + gam) + gam * S * (1.0 + A.U)) / (RR * (1.0 - gam))
            print(f"coef {coef:.6e} vs {Dd / RR:.6e}: err / bound {abs(coef - Dd / RR) / cbound:.3e}")
            assert abs(coef - Dd / RR) <= cbound
            assert abs(A.dots(_f32(s["g_after"]), gref)[0]) <= 2 * gam * S                   # orthogonal to the reference now
        want = p - A.f32(LR) * (A.project(g, gref, coef) if k == 2 else g)
        bound = A.gamma_k(4) * (p.abs() + A.f32(LR) * (g.abs() + (coef * gref).abs()))
        err = (_f32(s["p"]).double() - want).abs()
        print(f"step {k + 1}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= bound).all())
        exact = p - A.f32(LR) * A.project(g, gref)                                           # and the projection proper, float64 throughout
        torch.testing.assert_close(_f32(s["p"]).double(), exact, rtol=1e-5, atol=1e-7)
