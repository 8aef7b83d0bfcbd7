"""What A-GEM and the episodic memory promise without a device: the float64 reference (tests/agem_ref.py) pinned to
autograd, the entry points in the header and the ctypes table, `optim.AGEM` on CPU buffers with the test-only emulation of the kernel
wrappers (tests/cpu_kernels_agem.py) for both signs of the dot, `memory.EpisodicMemory`, and the ValueError / SystemExit paths of
the trainers and the drivers that need no kernel."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agem_ref as A  # noqa: E402
import cpu_kernels_agem as CK  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, optim as O  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd.memory import EpisodicMemory  # noqa: E402

ENTRY_POINTS = {"cxrk_agem_dots_partials_bytes": 1, "cxrk_agem_dots": 6, "cxrk_agem_project": 6}


def bits(t):
    return t.detach().reshape(-1).view(torch.int32)


class NoKernels:
    def __getattr__(self, name):
        raise AssertionError(f"kernel wrapper {name} was reached")


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(O, "K", CK)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_projection_against_autograd():
    """A-GEM's update is the minimiser of |g~ - g|^2 / 2 subject to g~ . gref >= 0: where the constraint binds, g~ - g is parallel
    to gref (the gradient of the constraint, taken by autograd) and g~ . gref = 0; where it does not, g~ = g."""
    gen = torch.Generator().manual_seed(0)
    r = torch.randn(41, generator=gen, dtype=torch.float64)
    noise = 0.1 * torch.randn(41, generator=gen, dtype=torch.float64)
    for sign in (-1.0, 1.0):
        g = sign * 0.5 * r + noise
        out = A.project(g, r)
        if sign > 0:
            assert torch.equal(out, g)
            continue
        x = out.clone().requires_grad_()
        (dc,) = torch.autograd.grad((x * r).sum(), x)                 # gradient of the constraint: gref
        lam = ((out - g) * dc).sum() / (dc * dc).sum()
        torch.testing.assert_close(out - g, lam * dc, rtol=1e-13, atol=1e-15)
        assert float(lam) > 0 and abs(float((out * r).sum())) < 1e-13
    D, RR, S = A.dots(g, r)
    for nparts in (1, 3):
        d, rr, a = A.dots_partials(g, r, nparts)
        assert d.sum() == pytest.approx(D, rel=1e-13) and rr.sum() == pytest.approx(RR, rel=1e-13) and a.sum() == pytest.approx(S, rel=1e-13)
    assert A.dots_depth(4097, 2) == A.R.sqnorm_depth(4097, 2) and A.refold_levels(1024) == 4 + 6 + 4


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        if nargs > 1:
            assert args[-1] == "hipStream_t stream"
    assert "agem_dots:" in hdr and "agem_project:" in hdr                                                # the contract comments
    assert "agem.hip" in open(os.path.join(ROOT, "incremental_multimodal_medical_learning_ii_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    for n in (1, 3, 4096, 4100, 65923, 4 * (1 << 20) + 3, 135_000_000):      # one partition for the norm, the penalty and the dots
        assert lib.cxrk_agem_dots_partials_bytes(n) == 2 * lib.cxrk_grad_sqnorm_partials_bytes(n) == 8 * CK.agem_dots_nparts(n), n
    from incremental_multimodal_medical_learning_ii_amd import kernels
    assert all(callable(getattr(kernels, f)) for f in ("agem_dots", "agem_project"))
    assert kernels.agem_dots_nparts(4100) == 2


# ------------------------------------------------------------------------------------------------ optim.AGEM
def _model(seed=3):
    torch.manual_seed(seed)
    return torch.nn.Linear(6, 3)


def _loss(model, x, y):
    return ((model(x) - y) ** 2).mean()


@pytest.mark.parametrize("conflict", [True, False], ids=["conflicting", "agreeing"])
def test_agem_over_sgd_on_a_linear_model(emulated, conflict):
    """the reference gradient from a memory batch, the step's from another: the flat gradient after `apply()` is the float64
    projection of the two autograd gradients, and the SGD step moves the parameters along it"""
    model = _model()
    opt = O.SGD(model.parameters(), lr=0.1)
    agem = O.AGEM(opt)
    gen = torch.Generator().manual_seed(1)
    xm, ym = torch.randn(8, 6, generator=gen), torch.randn(8, 3, generator=gen)
    x2 = torch.randn(4, 6, generator=gen)
    y2 = model(x2).detach() + 0.1 * torch.randn(4, 3, generator=gen)
    xc = torch.cat([xm, x2])                                          # the memory's rows, their residual mirrored when the batch is
    yc = torch.cat([2 * model(xm).detach() - ym if conflict else ym, y2])   # to conflict, and four rows of its own
    assert agem.current_interference() is None
    opt.zero_grad()
    _loss(model, xm, ym).backward()
    gref = opt.flat_g.clone()
    agem.store_reference()
    assert agem.valid and torch.equal(agem.gref, gref) and agem.gref.data_ptr() != opt.flat_g.data_ptr()
    opt.zero_grad()
    _loss(model, xc, yc).backward()
    g = opt.flat_g.clone()
    D, RR, _ = A.dots(g, gref)
    assert (D < 0) == conflict and abs(D) > 1e-3
    agem.apply()
    assert torch.equal(agem.gref, gref)
    info = agem.current_interference()
    assert set(info) == {"dot", "ref_sqnorm", "coef", "projected", "applied"}
    assert info["dot"] == pytest.approx(D, rel=1e-5) and info["ref_sqnorm"] == pytest.approx(RR, rel=1e-5)
    assert (info["projected"], info["applied"]) == (int(conflict), 1)
    want = A.project(g, gref)
    if conflict:
        assert info["coef"] == pytest.approx(D / RR, rel=1e-5)
        assert float((opt.flat_g.double() - want).abs().max()) <= 1e-5 * float(g.abs().max())
        assert abs(A.dots(opt.flat_g, gref)[0]) <= 1e-5 * A.dots(g, gref)[2]
    else:
        assert info["coef"] == 0.0 and torch.equal(bits(opt.flat_g), bits(g))
    p0 = opt.flat_p.clone()
    opt.step()
    assert float((opt.flat_p.double() - (p0.double() - 0.1 * want)).abs().max()) <= 1e-6


def test_apply_before_a_reference_issues_no_kernel_call(monkeypatch):
    monkeypatch.setattr(O, "K", NoKernels())
    opt = O.SGD(_model().parameters(), lr=0.1)
    agem = O.AGEM(opt)
    opt.flat_g.normal_()
    g = opt.flat_g.clone()
    agem.apply()
    assert torch.equal(opt.flat_g, g) and agem.gref is None and agem._partials is None and agem.current_interference() is None


def test_agem_state_round_trip_and_refusals(emulated):
    opt = O.SGD(_model().parameters(), lr=0.1)
    agem = O.AGEM(opt)
    opt.flat_g.normal_()
    agem.store_reference()
    opt.flat_g.neg_()
    agem.apply()
    sd = agem.state_dict()
    assert set(sd) == {"numel", "applied", "stats"} and all(isinstance(v, (int, torch.Tensor)) for v in sd.values())
    other = O.AGEM(O.SGD(_model(5).parameters(), lr=0.1))
    other.load_state_dict(sd)
    assert other.applied == 1 and not other.valid and other.gref is None      # the reference is recomputed, never loaded
    assert other.current_interference()["projected"] == 1
    for bad, what in ((dict(sd, extra=1), "keys"), ({k: v for k, v in sd.items() if k != "stats"}, "keys"),
                      (dict(sd, numel=sd["numel"] + 4), "flat buffer"), (dict(sd, stats=sd["stats"][:3]), "4 elements"),
                      (dict(sd, stats=sd["stats"].double()), "float32"), (dict(sd, applied=-1), "applied"), ([1], "dict")):
        target = O.AGEM(O.SGD(_model().parameters(), lr=0.1))
        with pytest.raises(ValueError, match=what):
            target.load_state_dict(bad)
        assert target.applied == 0 and bool((target._stats == 0).all())


# ------------------------------------------------------------------------------------------------ memory.EpisodicMemory
def _stream(rows_per_batch, width=5, seed=0, labels=False, base=0):
    """batches whose image rows carry their own stream index (so a stored row names where it came from)"""
    gen = torch.Generator().manual_seed(seed)
    out, start = [], base
    for rows in rows_per_batch:
        idx = torch.arange(start, start + rows)
        images = idx.float().view(rows, 1, 1, 1).expand(rows, 1, 2, 2).contiguous()
        lens = torch.randint(1, width + 1, (rows,), generator=gen)
        mask = (torch.arange(width)[None, :] < lens[:, None]).long()
        ids = torch.randint(1, 100, (rows, width), generator=gen) * mask
        batch = (images, ids, mask)
        if labels:
            batch += (torch.randint(0, 2, (rows, 5), generator=gen).float(),)
        out.append(batch)
        start += rows
    return out


def test_memory_add_task_is_a_deterministic_reservoir():
    a, b = EpisodicMemory(6, seed=3), EpisodicMemory(6, seed=3)
    stream = _stream([4, 7, 1, 9])
    assert a.add_task(stream) == 6 and b.add_task(_stream([4, 7, 1, 9])) == 6 and len(a) == 6
    for k in ("images", "input_ids", "attention_mask"):
        assert torch.equal(a.tasks[0][k], b.tasks[0][k])
    src = a.tasks[0]["images"][:, 0, 0, 0].long()
    assert len(set(src.tolist())) == 6 and int(src.max()) < 21                   # six distinct rows of the stream
    allrows = {k: torch.cat([bt[i] for bt in stream]) for i, k in enumerate(("images", "input_ids", "attention_mask"))}
    for k in allrows:                                                             # every field of a slot comes from the same row
        assert torch.equal(a.tasks[0][k], allrows[k][src])
    other = EpisodicMemory(6, seed=4)
    other.add_task(stream)
    assert not torch.equal(other.tasks[0]["images"], a.tasks[0]["images"])       # another seed, another choice
    assert a.add_task(_stream([3], base=100)) == 3 and len(a) == 9               # a short stream: all of it, in order
    assert a.tasks[1]["images"][:, 0, 0, 0].tolist() == [100.0, 101.0, 102.0]
    a.add_task(_stream([5, 5], base=200))
    assert len(a) == 15 and [int(t["images"].shape[0]) for t in a.tasks] == [6, 3, 6]
    # the same stream as the next task draws differently: the generator is keyed by the task index
    c = EpisodicMemory(6, seed=3)
    c.add_task(_stream([3], base=100))
    c.add_task(stream)
    assert not torch.equal(c.tasks[1]["images"], a.tasks[0]["images"])


def test_memory_reservoir_is_uniform():
    """every row of a 40-row stream is kept with probability 8 / 40: over 300 seeds the counts stay within 5 sigma"""
    counts = torch.zeros(40)
    stream = _stream([16, 16, 8])
    for seed in range(300):
        m = EpisodicMemory(8, seed=seed)
        m.add_task(stream)
        counts[m.tasks[0]["images"][:, 0, 0, 0].long()] += 1
    p = 8 / 40
    sigma = (300 * p * (1 - p)) ** 0.5
    assert float((counts - 300 * p).abs().max()) <= 5 * sigma, counts.tolist()


def test_memory_pads_narrower_and_widens_for_wider_token_rows():
    m = EpisodicMemory(4, seed=0)
    wide = _stream([4], width=7)
    m.add_task(wide)
    narrow = _stream([4], width=3, seed=1, base=50)
    m.add_task(narrow)
    assert m.width == 7 and tuple(m.tasks[1]["input_ids"].shape) == (4, 7)
    src = (m.tasks[1]["images"][:, 0, 0, 0].long() - 50)
    assert torch.equal(m.tasks[1]["input_ids"][:, :3], narrow[0][1][src]) and bool((m.tasks[1]["input_ids"][:, 3:] == 0).all())
    assert torch.equal(m.tasks[1]["attention_mask"][:, :3], narrow[0][2][src]) and bool((m.tasks[1]["attention_mask"][:, 3:] == 0).all())
    assert torch.equal(C.keys_from_tokens(m.tasks[1]["input_ids"], m.tasks[1]["attention_mask"]),
                       C.keys_from_tokens(narrow[0][1][src], narrow[0][2][src]))  # the padding does not reach the keys
    wider = _stream([2, 2], width=9, seed=2, base=80)
    m.add_task(wider)
    assert m.width == 9 and all(tuple(t["input_ids"].shape)[1] == 9 and tuple(t["attention_mask"].shape)[1] == 9 for t in m.tasks)
    assert bool((m.tasks[0]["input_ids"][:, 7:] == 0).all()) and bool((m.tasks[0]["attention_mask"][:, 7:] == 0).all())
    assert torch.equal(m.tasks[0]["input_ids"][:, :7], wide[0][1][m.tasks[0]["images"][:, 0, 0, 0].long()])
    batch = m.sample(12, step=0)
    assert tuple(batch[1].shape) == (12, 9) and batch[1].dtype == torch.int64 and batch[0].dtype == torch.float32


def test_memory_sample_is_deterministic_distinct_and_uniform():
    m = EpisodicMemory(6, seed=1)
    m.add_task(_stream([10], labels=True))
    m.add_task(_stream([10], seed=1, labels=True, base=100))
    assert len(m) == 12
    s0, s0b, s1 = m.sample(5, step=0), m.sample(5, step=0), m.sample(5, step=1)
    assert len(s0) == 4 and tuple(s0[3].shape) == (5, 5)
    assert all(torch.equal(x, y) for x, y in zip(s0, s0b))
    assert not torch.equal(s0[0], s1[0])
    stored = torch.cat([t["images"][:, 0, 0, 0] for t in m.tasks]).tolist()
    seen = torch.zeros(12)
    for step in range(400):
        rows = m.sample(5, step=step)[0][:, 0, 0, 0].tolist()
        assert len(set(rows)) == 5 and set(rows) <= set(stored)                  # distinct rows of the memory
        for r in rows:
            seen[stored.index(r)] += 1
    p = 5 / 12
    assert float((seen - 400 * p).abs().max()) <= 5 * (400 * p * (1 - p)) ** 0.5, seen.tolist()
    every = m.sample(12, step=7)[0][:, 0, 0, 0].tolist()
    assert sorted(every) == sorted(stored)
    for bad in (0, 13, 2.0, True):
        with pytest.raises(ValueError, match="sample"):
            m.sample(bad, step=0)
    full = m.sample(12, step=3)                                                   # the fields of a sampled row belong together
    for i, r in enumerate(full[0][:, 0, 0, 0].tolist()):
        t, j = (0, stored.index(r)) if stored.index(r) < 6 else (1, stored.index(r) - 6)
        assert torch.equal(full[1][i], m.tasks[t]["input_ids"][j]) and torch.equal(full[3][i], m.tasks[t]["extra"][j])


def test_memory_refusals():
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="rows_per_task"):
            EpisodicMemory(bad)
    with pytest.raises(ValueError, match="seed"):
        EpisodicMemory(4, seed=1.5)
    m = EpisodicMemory(4)
    with pytest.raises(ValueError, match="no row"):
        m.add_task([])
    with pytest.raises(ValueError, match="batch is"):
        m.add_task([(torch.zeros(2, 1), torch.zeros(2, 3, dtype=torch.long))])
    with pytest.raises(ValueError, match="same number of rows"):
        m.add_task([(torch.zeros(2, 1), torch.zeros(3, 3, dtype=torch.long), torch.zeros(3, 3, dtype=torch.long))])
    assert len(m) == 0
    m.add_task(_stream([4]))
    with pytest.raises(ValueError, match="differ"):
        m.add_task(_stream([4], labels=True))                                     # a field the stored rows do not have
    assert len(m) == 4


def test_memory_state_round_trip_is_strict(tmp_path):
    m = EpisodicMemory(5, seed=2)
    m.add_task(_stream([8], labels=True))
    m.add_task(_stream([3], width=7, seed=1, labels=True, base=30))
    path = os.path.join(tmp_path, "memory.pt")
    torch.save(m.state_dict(), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)                  # tensors, lists and plain numbers only
    other = EpisodicMemory(5, seed=2)
    other.load_state_dict(sd)
    assert len(other) == 8 and other.width == 7
    for a, b in zip(m.tasks, other.tasks):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert all(torch.equal(x, y) for x, y in zip(m.sample(6, step=4), other.sample(6, step=4)))
    assert other.tasks[0]["images"].data_ptr() != sd["tasks"][0]["images"].data_ptr()
    empty = EpisodicMemory(5, seed=2)
    empty.load_state_dict(EpisodicMemory(5, seed=2).state_dict())
    assert len(empty) == 0
    t0 = sd["tasks"][0]
    for bad, what in ((dict(sd, extra=1), "keys"), ({k: v for k, v in sd.items() if k != "width"}, "keys"),
                      (dict(sd, rows_per_task=6), "rows_per_task"), (dict(sd, seed=9), "seed"),
                      (dict(sd, width=8), "token rows"), (dict(sd, tasks=[dict(t0, images=t0["images"][:2])] + sd["tasks"][1:]), "rows"),
                      (dict(sd, tasks=[{k: v for k, v in t0.items() if k != "extra"}] + sd["tasks"][1:]), "must hold"),
                      (dict(sd, tasks=[dict(t0, extra=[1, 2])] + sd["tasks"][1:]), "tensors"),
                      (dict(sd, tasks=[t0, dict(sd["tasks"][1], images=sd["tasks"][1]["images"].double())]), "dtype"),
                      (dict(sd, tasks="x"), "list"), ("x", "keys")):
        target = EpisodicMemory(5, seed=2)
        with pytest.raises(ValueError, match=what):
            target.load_state_dict(bad)
        assert len(target) == 0 and target.width == 0                              # a refused state changes nothing


# ------------------------------------------------------------------------------------------------ trainers and drivers
def test_joint_trainer_arguments(monkeypatch):
    monkeypatch.setattr(C, "K", NoKernels())
    for kw in ({"agem_batch": 4}, {"agem_every": 2}, {"agem_seed": 1}):
        with pytest.raises(ValueError, match="agem_memory"):
            C.JointContrastiveTrainer(None, None, **kw)
    for kw, what in (({"agem_memory": 0}, "agem_memory"), ({"agem_memory": 2.5}, "agem_memory"), ({"agem_memory": True}, "agem_memory"),
                     ({"agem_memory": 4, "agem_batch": 0}, "agem_batch"), ({"agem_memory": 4, "agem_every": 0}, "agem_every"),
                     ({"agem_memory": 4, "agem_seed": -1}, "agem_seed")):
        with pytest.raises(ValueError, match=what):
            C.JointContrastiveTrainer(None, None, **kw)
    assert C.check_agem_options(8, None, None, None) == (8, None, 1, 0)
    assert C.check_agem_options(8, 4, 3, 7) == (8, 4, 3, 7)
    assert C.check_agem_options(None, None, None, None) == (None, None, None, None)


def test_trainer_refuses_the_keys_without_joint_mode():
    for je in ({"agem_memory": 16}, {"agem_batch": 4}, {"image_model": None, "agem_every": 2}):
        with pytest.raises(ValueError, match="joint mode"):
            TR.Trainer(True, [], [], "standard", 1e-3, "cpu", None, bert_encoder=object(), joint_encoders=je)
    im = object()
    for key in ("agem_batch", "agem_every", "agem_seed"):
        with pytest.raises(ValueError, match="agem_memory"):
            TR.joint_options({"image_model": im, key: 2})
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="agem_memory"):
            TR.joint_options({"image_model": im, "agem_memory": bad})
        with pytest.raises(ValueError, match="agem_every"):
            TR.joint_options({"image_model": im, "agem_memory": 8, "agem_every": bad})
    # (the removed checker returned None for what it accepted; the one function returns what it passes on)
    step, own = TR.joint_options({"image_model": im, "agem_memory": 8, "agem_batch": 4})
    assert (step["agem_memory"], step["agem_batch"]) == (8, 4) and "agem_every" not in step and own["image_model"] is im
    assert "agem_memory" not in TR.joint_options({"image_model": im})[0] and TR.joint_options(None)[0] == {}


def test_drivers_arguments():
    a = drivers.parse_args(["class-inc", "--joint"])
    assert drivers.continual_from_args(a) == {}
    a = drivers.parse_args(["class-inc", "--joint", "--cl", "agem"])
    # the whole dict: no "ewc_*" and no "distill_*" key
    assert drivers.continual_from_args(a) == {"agem_memory": drivers.AGEM_MEMORY} and drivers.AGEM_MEMORY == 256
    a = drivers.parse_args(["data-inc", "--joint", "--cl", "agem", "--agem-memory", "64", "--agem-batch", "32", "--agem-every", "4"])
    assert drivers.continual_from_args(a) == {"agem_memory": 64, "agem_batch": 32, "agem_every": 4}
    for argv in (["class-inc", "--cl", "agem"],                                    # needs --joint
                 ["zero-joint", "--joint", "--cl", "agem"],                         # a single task: nothing to remember between
                 ["class-inc", "--joint", "--agem-memory", "10"],                   # the options need --cl agem
                 ["class-inc", "--joint", "--cl", "ewc", "--agem-every", "2"],
                 ["class-inc", "--joint", "--cl", "agem", "--ewc-lambda", "10"],
                 ["class-inc", "--joint", "--cl", "agem", "--agem-memory", "0"],
                 ["class-inc", "--joint", "--cl", "agem", "--agem-batch", "-1"],
                 ["class-inc", "--joint", "--cl", "agem", "--agem-every", "0"]):
        with pytest.raises(SystemExit):
            drivers.parse_args(argv)
        with pytest.raises(SystemExit):
            drivers.main(argv)
