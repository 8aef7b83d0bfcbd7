"""The masked-language-modelling loss's data-parallel protocol on CPU: 2 processes, gloo backend, `JointContrastiveTrainer(mlm_weight=...)`
on two stub encoders (an embedding table and one weight matrix: what is checked is the orchestration, not the encoders), with the
test-only torch emulation of the kernel wrappers (tests/cpu_kernels_distill.py), the numpy draw (tests/mlm_ref.py) standing in for the
mask kernel and torch autograd for the head.

  * a masked step issues the plain step's collectives plus exactly ONE `all_reduce` (the scalar count of selected tokens);
  * rank 1 masks with rank 0's (seed, counter) -- constructed with another seed, it takes rank 0's in the construction's broadcast -- and
    with its row offset: the two shards' masked ids are the halves of the single-process draw on the global batch;
  * after the step the replicas are bit-identical, and the update equals the single-process update on the global batch (2e-5 of the
    largest update, the bound of tests/test_distill_dist_gloo.py), the tied embedding table and the head included."""
import json
import os
import socket
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG, L, V, D, TAU, WORLD, W, P, SEED = 12, 8, 64, 128, 0.07, 2, 0.7, 0.4, 77
COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter_tensor", "all_to_all_single", "reduce",
               "gather", "scatter")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stubs(syn):
    """two encoders with the attributes the joint trainer touches"""
    n = lambda tag, shape, s=0.1: torch.nn.Parameter(torch.from_numpy(syn._normal("mlmdist." + tag, shape)) * s)   # noqa: E731

    class Image(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = n("Wi", (D, D))
            self.grad_ready_hook, self.augment_call, self.save_free = None, None, False

        def prepare_(self):
            return self

        def forward(self, x):
            return x @ self.w

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dense_w, self.dense_b, self.bias = n("Wd", (D, D)), n("bd", (D,)), n("bdec", (V,))
            self.ln_w, self.ln_b = torch.nn.Parameter(torch.ones(D)), torch.nn.Parameter(torch.zeros(D))

    class Text(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb, self.w = n("E", (V, D), 1.0), n("Wt", (D, D))
            self.cls = torch.nn.Module()
            self.cls.predictions = Head()                      # named `cls.predictions.*`: trained only with mlm_weight
            self.config = types.SimpleNamespace(vocab_size=V, layer_norm_eps=1e-12)
            self.grad_ready_hook, self.save_free, self.dropout_row_offset = None, False, 0
            self.paths = []

        def prepare_(self):
            return self

        def get_projected_text_embeddings(self, ids, mask, normalize_embeddings=False):
            self.paths.append("cls_only")
            return self.emb[ids].mean(1) @ self.w

        def get_projected_text_embeddings_and_hidden(self, ids, mask, want_hidden=True):
            self.paths.append("full")
            h = self.emb[ids]
            return h.mean(1) @ self.w, (h if want_hidden else None)

        def mlm_head_params(self):
            hd = self.cls.predictions
            return (hd.dense_w, hd.dense_b, hd.ln_w, hd.ln_b, self.emb, hd.bias)

    return Image(), Text()


def _worker(rank, world, port, out_dir, tag):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import numpy as np
    import torch.nn.functional as F
    import cpu_kernels_distill as CK
    import mlm_ref as R
    from incremental_multimodal_medical_learning_ii_amd import contrastive as C
    from incremental_multimodal_medical_learning_ii_amd import functional as Fh
    from incremental_multimodal_medical_learning_ii_amd import kernels as K
    from incremental_multimodal_medical_learning_ii_amd import optim as cxr_optim
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    drawn = []

    def mask_tokens(ids, mask, seed, counter, p, vocab_size, mask_id, special_ids=(), row_offset=0, cap=None):
        r = R.mask_tokens(ids.numpy(), None if mask is None else mask.numpy(), seed, counter, p, vocab_size, mask_id, special_ids, row_offset, cap)
        drawn.append((seed, counter, row_offset, r["ids_out"].tolist()))
        return K.MlmMask(torch.as_tensor(r["ids_out"]), torch.as_tensor(r["sel"]), torch.as_tensor(r["tgt"]),
                         torch.tensor([r["kept"], r["selected"]], dtype=torch.int32), torch.tensor([float(r["kept"])]))

    def triple(last, sel, tgt, stats, params, scale, chunk_bytes=0, weight=1.0, eps=1e-12):
        kept = int(stats[0])
        flat = last.reshape(-1, last.shape[-1])
        logits = R.head_logits(flat[sel[:kept].long()], *params, eps=eps)
        t = tgt[:kept].long()
        loss = F.cross_entropy(logits, t, reduction="sum") * scale.reshape(())
        return loss * weight, loss.detach(), (logits.argmax(dim=1) == t).sum().reshape(1).to(torch.int32)

    CK.mlm_mask_tokens = mask_tokens          # test-only emulation of the kernel wrappers
    Fh.K = CK
    cxr_optim.K = CK
    C.K = CK
    Fh._mlm_triple = triple
    calls = []
    for name in COLLECTIVES:                  # count every collective the step issues
        def wrap(fn, name=name):
            def counted(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return counted
        setattr(dist, name, wrap(getattr(dist, name)))
    B = BG // world
    sl = slice(rank * B, (rank + 1) * B)
    X = torch.from_numpy(syn._normal("mlmdist.X", (BG, D)))
    ids = torch.as_tensor(np.random.default_rng(3).integers(5, V, size=(BG, L)))
    ids[:, 0] = 2
    amask = torch.ones(BG, L, dtype=torch.int64)

    def trainer(**kw):
        im, tm = _stubs(syn)
        return C.JointContrastiveTrainer(im, tm, lr=0.05, temperature=TAU, optim="sgd", **kw)

    def step(tr):
        before = tr.optimizer.flat_p.detach().clone()
        del calls[:]
        loss = tr.step(X[sl], ids[sl], amask[sl])
        return list(calls), float(loss), (tr.optimizer.flat_p.detach() - before).double().tolist(), tr.optimizer.flat_p.view(torch.int32).tolist()

    plain = trainer()
    masked = trainer(mlm_weight=W, mlm_probability=P, mlm_seed=SEED + rank)       # the ranks seed differently: rank 0's counts
    state0 = masked.mlm_state
    c0, l0, _, _ = step(plain)
    c1, l1, upd, bits = step(masked)
    info = masked.current_mlm()
    names = [n for n, _ in masked.text_model.named_parameters()]
    out = {"plain": c0, "masked": c1, "loss_plain": l0, "loss": l1, "update": upd, "bits": bits, "state0": list(state0),
           "state1": list(masked.mlm_state), "drawn": drawn, "mlm": info, "paths": [plain.text_model.paths, masked.text_model.paths],
           "numel": [int(plain.optimizer.numel), int(masked.optimizer.numel)], "names": names}
    with open(os.path.join(out_dir, f"{tag}{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlm_gloo")
    mp.spawn(_worker, args=(WORLD, _free_port(), str(d), "r"), nprocs=WORLD, join=True)
    mp.spawn(_worker, args=(1, _free_port(), str(d), "s"), nprocs=1, join=True)
    return [json.load(open(d / f"r{k}.json")) for k in range(WORLD)], json.load(open(d / "s0.json"))


def test_a_masked_step_adds_exactly_one_scalar_all_reduce(runs):
    ranks, single = runs
    for rk in ranks:
        mine = list(rk["masked"])
        assert mine.count("all_reduce") == rk["plain"].count("all_reduce") + 1, (mine, rk["plain"])
        mine.remove("all_reduce")
        assert sorted(mine) == sorted(rk["plain"]), (rk["masked"], rk["plain"])                # and nothing else
        assert rk["paths"] == [["cls_only"], ["full"]]                                          # one text call per step, either way
        assert rk["numel"][1] - rk["numel"][0] == D * D + D + D + D + V                         # the head joins the optimiser
    assert single["masked"] == single["plain"] == []                                            # a single process: no collective at all


def test_the_shards_mask_as_the_global_batch_does(runs):
    ranks, single = runs
    assert [rk["state0"] for rk in ranks] == [[SEED, 0], [SEED, 0]] and all(rk["state1"] == [SEED, 1] for rk in ranks)
    (seed, counter, off, whole), = single["drawn"]
    assert (seed, counter, off) == (SEED, 0, 0)
    B = BG // WORLD
    for k, rk in enumerate(ranks):
        (s, c, o, part), = rk["drawn"]
        assert (s, c, o) == (SEED, 0, k * B) and part == whole[k * B:(k + 1) * B]
    assert ranks[0]["mlm"] == ranks[1]["mlm"] and ranks[0]["mlm"]["masked"] == single["mlm"]["masked"] >= 8
    assert abs(ranks[0]["mlm"]["loss"] - single["mlm"]["loss"]) < 2e-5 * single["mlm"]["loss"]
    assert ranks[0]["mlm"]["accuracy"] == single["mlm"]["accuracy"] and ranks[0]["mlm"]["overflowed"] == 0


def test_replicas_stay_identical_and_the_update_is_the_single_process_update(runs):
    ranks, single = runs
    assert ranks[0]["bits"] == ranks[1]["bits"]
    want = torch.tensor(single["update"], dtype=torch.float64)
    scale = float(want.abs().max())
    assert scale > 0
    for rk in ranks:
        got = torch.tensor(rk["update"], dtype=torch.float64)
        assert float((got - want).abs().max()) < 2e-5 * scale
        assert abs(rk["loss"] - single["loss"]) < 2e-5 * abs(single["loss"])                    # `step` reports the contrastive loss
    assert ranks[0]["loss"] != ranks[0]["loss_plain"]                                           # of the MASKED ids
    assert any(n.startswith("cls.predictions.") for n in ranks[0]["names"])
