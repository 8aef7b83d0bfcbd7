"""The masked-language-modelling loss without a device: the numpy restatement of the token draw (tests/mlm_ref.py) --
its key layout, shard invariance and, at 65536 tokens, its selected fraction and 80 / 10 / 10 split --, the capacity formula, the
chunk list of the vocabulary sweep, the CPU models of the compaction and of the per-lane folding (tests/cpu_kernels_mlm.py), the
option refusals, the drivers' flags and the C ABI's arity."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cpu_kernels_mlm as CK  # noqa: E402
import mlm_ref as R  # noqa: E402
from dropout_ref import philox4x32_10  # noqa: E402

from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh, kernels as K  # noqa: E402

SPECIAL = (0, 1, 2, 3, 4)
SEED = 0x1234ABCD5678EF01


def _tokens(N, L, vocab, seed=0, pads=True):
    g = np.random.default_rng(seed)
    ids = g.integers(5, vocab, size=(N, L))
    ids[:, 0] = 2
    mask = np.ones((N, L), dtype=np.int64)
    if pads:
        for n in range(N):
            ln = int(g.integers(3, L + 1))
            ids[n, ln - 1] = 3
            ids[n, ln:] = 0
            mask[n, ln:] = 0
    return ids, mask


def test_the_key_layout_of_one_draw():
    """one Philox block per token: key = the seed's two words, counter = (0, global sequence, token, (counter & 0xffffff) << 8 | 0xF4);
    word 0 selects, word 1 decides what happens, word 2 is the random id"""
    ids, mask = _tokens(3, 7, 300, pads=False)
    p, counter, off = 0.5, 0x1ABCDEF, 11
    out = R.mask_tokens(ids, mask, SEED, counter, p, 300, 4, SPECIAL, row_offset=off)
    for n in range(3):
        for t in range(7):
            w = philox4x32_10(np.uint32(0), np.uint32(off + n), np.uint32(t), np.uint32(((counter & 0xFFFFFF) << 8) | 0xF4),
                              SEED & 0xFFFFFFFF, SEED >> 32)
            w = [int(x) for x in w]
            cand = ids[n, t] not in SPECIAL
            sel = cand and w[0] < int(math.floor(p * 2 ** 32 + 0.5))
            want = ids[n, t]
            if sel and w[1] < R.T80:
                want = 4
            elif sel and w[1] < R.T90:
                want = (w[2] * 300) >> 32
            assert out["ids_out"][n, t] == want and (out["kind"][n, t] != R.KEEP) == sel
    assert (R.T80, R.T90) == (math.ceil(0.8 * 2 ** 32), math.ceil(0.9 * 2 ** 32))
    # counters that differ above bit 24 draw alike; a different seed word or counter does not
    again = R.mask_tokens(ids, mask, SEED, counter + (1 << 24), p, 300, 4, SPECIAL, row_offset=off)
    assert np.array_equal(again["ids_out"], out["ids_out"])
    assert not np.array_equal(R.mask_tokens(ids, mask, SEED, counter + 1, p, 300, 4, SPECIAL, row_offset=off)["kind"], out["kind"])
    assert not np.array_equal(R.mask_tokens(ids, mask, SEED ^ (1 << 40), counter, p, 300, 4, SPECIAL, row_offset=off)["kind"], out["kind"])


def test_pads_and_special_tokens_are_never_drawn_and_the_list_is_in_token_order():
    ids, mask = _tokens(6, 19, 300, seed=1)
    out = R.mask_tokens(ids, mask, SEED, 3, 1.0, 300, 4, SPECIAL)                 # p = 1: every candidate
    cand = (mask != 0) & ~np.isin(ids, SPECIAL)
    assert np.array_equal(out["kind"] != R.KEEP, cand) and out["selected"] == int(cand.sum()) == out["kept"]
    assert np.array_equal(out["ids_out"][~cand], ids[~cand])
    k = out["kept"]
    assert np.all(np.diff(out["sel"][:k]) > 0) and np.array_equal(out["tgt"][:k], ids.reshape(-1)[out["sel"][:k]])
    assert np.all(out["sel"][k:] == -1) and np.all(out["tgt"][k:] == -1)
    none = R.mask_tokens(ids, mask, SEED, 3, 0.0, 300, 4, SPECIAL)
    assert none["selected"] == 0 and np.array_equal(none["ids_out"], ids)
    small = R.mask_tokens(ids, mask, SEED, 3, 1.0, 300, 4, SPECIAL, cap=5)         # overflow: the first five keep their targets
    assert small["kept"] == 5 < small["selected"] and np.array_equal(small["sel"], out["sel"][:5])
    assert np.array_equal(small["ids_out"], out["ids_out"])                        # the rest stay corrupted


def test_shard_invariance_of_the_reference():
    ids, mask = _tokens(8, 16, 300, seed=2)
    whole = R.mask_tokens(ids, mask, SEED, 9, 0.3, 300, 4, SPECIAL, row_offset=4)
    parts = [R.mask_tokens(ids[lo:hi], mask[lo:hi], SEED, 9, 0.3, 300, 4, SPECIAL, row_offset=4 + lo) for lo, hi in ((0, 3), (3, 8))]
    assert np.array_equal(np.concatenate([q["ids_out"] for q in parts]), whole["ids_out"])
    sel = np.concatenate([parts[0]["sel"][:parts[0]["kept"]], parts[1]["sel"][:parts[1]["kept"]] + 3 * 16])
    assert np.array_equal(sel, whole["sel"][:whole["kept"]]) and parts[0]["selected"] + parts[1]["selected"] == whole["selected"]


def test_selected_fraction_and_split_at_65536_tokens():
    """every token a candidate: selected ~ Binomial(T, p), and among the M selected the three fates ~ Binomial(M, 0.8 / 0.1 / 0.1);
    each within five standard deviations (the seed is fixed: this is a property of the stated rule, checked once on the CPU)"""
    T, p, V = 65536, 0.15, 30522
    ids = np.random.default_rng(5).integers(5, V, size=(T // 32, 32))
    out = R.mask_tokens(ids, None, 20240607, 0, p, V, 4, SPECIAL)
    M = out["selected"]
    assert abs(M - p * T) <= 5 * math.sqrt(p * (1 - p) * T), M
    for kind, q in ((R.MASK, 0.8), (R.RANDOM, 0.1), (R.SAME, 0.1)):
        n = int((out["kind"] == kind).sum())
        assert abs(n - q * M) <= 5 * math.sqrt(q * (1 - q) * M), (kind, n, M)
    rnd = out["ids_out"][out["kind"] == R.RANDOM]
    assert rnd.min() >= 0 and rnd.max() < V and abs(rnd.mean() - V / 2) <= 5 * (V / math.sqrt(12)) / math.sqrt(len(rnd))
    assert out["kept"] == M <= R.capacity(T, p)                                     # no overflow at the default capacity


@pytest.mark.parametrize("T, p, want", [(65536, 0.15, 10624), (32768, 0.15, 5504), (95, 0.15, 95), (95, 0.5, 95), (4096, 0.0, 1),
                                        (1024, 1.0, 1024), (128, 0.15, 128), (1 << 20, 0.15, 160256)])
def test_capacity_formula(T, p, want):
    """min(T, roundup128(ceil(p T + 8 sqrt(p (1 - p) T)))), at least one slot"""
    need = math.ceil(p * T + 8 * math.sqrt(p * (1 - p) * T))
    assert K.mlm_capacity(T, p) == R.capacity(T, p) == max(1, min(T, -(-need // 128) * 128)) == want
    assert K.mlm_capacity(T, p) % 128 == 0 or K.mlm_capacity(T, p) in (T, 1)


def test_capacity_refusals():
    for T, p in ((0, 0.1), (True, 0.1), (10, -0.1), (10, 1.5)):
        with pytest.raises(ValueError):
            K.mlm_capacity(T, p)


@pytest.mark.parametrize("V, rows, chunk_bytes, planes", [(300, 37, 37 * 128 * 4, False), (300, 37, 1 << 30, False), (300, 37, 1, True),
                                                          (30522, 5504, 128 << 20, False), (30522, 5504, 128 << 20, True), (296, 8, 1, False),
                                                          (8, 1, 1, False), (15, 3, 1, False)])
def test_vocab_chunks_tile_the_vocabulary_in_multiples_of_eight(V, rows, chunk_bytes, planes):
    chunks = Fh.mlm_vocab_chunks(V, rows, chunk_bytes, planes)
    assert chunks == CK.vocab_chunks(V, rows, chunk_bytes, planes)
    counted = np.zeros(V, dtype=int)
    for v0, cols, skip in chunks:
        assert cols % 8 == 0 and v0 + cols <= V
        assert (skip == 0 and v0 % 8 == 0) or (V % 8 != 0 and (v0, cols, skip) == (V - 8, 8, 8 - V % 8))
        counted[v0 + skip: v0 + cols] += 1
    assert np.all(counted == 1)                                                    # every column exactly once
    width = max(c for _, c, _ in chunks)
    assert width % 128 == 0 or width == V // 8 * 8 or width == 8
    assert width <= 128 or rows * width * (8 if planes else 4) <= chunk_bytes      # the workspace follows chunk_bytes, never V
    with pytest.raises(ValueError):
        Fh.mlm_vocab_chunks(7, rows, chunk_bytes, planes)


def test_cpu_model_of_the_compaction_is_the_token_order():
    g = np.random.default_rng(3)
    for T, q, cap in ((95, 0.5, 37), (1000, 0.15, 256), (777, 0.0, 8), (513, 1.0, 513), (2048, 0.9, 100)):
        flags = g.random(T) < q
        sel, kept, total = CK.place(flags, cap)
        where = np.flatnonzero(flags)
        assert total == len(where) and kept == min(total, cap)
        assert np.array_equal(sel[:kept], where[:kept]) and np.all(sel[kept:] == -1)


def test_cpu_model_of_the_lane_folding_does_not_depend_on_the_chunk_size():
    """the per-lane sequence of additions is a function of the absolute column alone, so chunks of 128 columns and one whole chunk give
    the same float32 bits; and both give the float64 log-sum-exp to float32 accuracy, +-80 logits and a NaN included"""
    g = np.random.default_rng(4)
    V = 300
    for case in range(4):
        x = (g.standard_normal(V) * 3).astype(np.float32)
        if case == 1:
            x[[0, 127, 128, 299]] = [80.0, -80.0, 80.0, -80.0]
        if case == 2:
            x[297] = 50.0                                                         # the maximum in the unaligned tail chunk
        if case == 3:
            x[200] = np.nan
        a = CK.fold_row(x, CK.vocab_chunks(V, 37, 37 * 128 * 4))
        b = CK.fold_row(x, CK.vocab_chunks(V, 37, 1 << 30))
        assert len(CK.vocab_chunks(V, 37, 37 * 128 * 4)) == 4 and len(CK.vocab_chunks(V, 37, 1 << 30)) == 2
        assert np.array_equal(np.float32(a[0]).view(np.int32), np.float32(b[0]).view(np.int32)) and a[1] == b[1]
        if case == 3:
            assert np.isnan(a[0]) and a[1] == 200
        else:
            x64 = x.astype(np.float64)
            want = x64.max() + math.log(np.exp(x64 - x64.max()).sum())
            assert abs(float(a[0]) - want) <= 4e-6 * max(1.0, abs(want)) and a[1] == int(np.argmax(x64))


def test_option_refusals():
    ok = C.check_mlm_options(0.5, None, None, None, None)
    assert ok == (0.5, 0.15, None, 4, (0, 1, 2, 3, 4))
    assert C.check_mlm_options(None, None, None, None, None) == (None,) * 5
    assert C.check_mlm_options(0, 0.3, 7, 103, (0, 100, 101, 102, 103)) == (0.0, 0.3, 7, 103, (0, 100, 101, 102, 103))
    for member in ({"probability": 0.2}, {"seed": 3}, {"mask_token_id": 4}, {"special_ids": (0,)}):
        kw = dict(probability=None, seed=None, mask_token_id=None, special_ids=None)
        kw.update(member)
        with pytest.raises(ValueError, match="without mlm_weight"):
            C.check_mlm_options(None, **kw)
    for bad in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight=True), dict(weight="1"), dict(probability=1.5), dict(probability=-0.1),
                dict(seed=-1), dict(seed=1.5), dict(mask_token_id=-1), dict(special_ids=tuple(range(9))), dict(special_ids=(0, -1))):
        kw = dict(weight=1.0, probability=None, seed=None, mask_token_id=None, special_ids=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            C.check_mlm_options(**kw)
    with pytest.raises(ValueError, match="micro_batch.*out of scope"):
        C.check_mlm_options(1.0, None, None, None, None, micro_batch=4)
    assert C.check_mlm_options(None, None, None, None, None, micro_batch=4) == (None,) * 5


def test_the_keywords_reach_trainer_and_no_group_is_added():
    keywords = set(inspect.signature(C.JointContrastiveTrainer.__init__).parameters)
    new = {"mlm_weight", "mlm_probability", "mlm_seed", "mlm_mask_token_id", "mlm_special_ids"}
    assert new <= keywords and new <= set(TR.JOINT_STEP_KEYS)
    assert "train_mlm_head" not in TR.JOINT_STEP_KEYS and not any(g[0].startswith("mlm") for g in TR.JOINT_GROUPS)
    im = object()
    step, _ = TR.joint_options({"image_model": im, "mlm_weight": 0.5, "mlm_probability": 0.2, "mlm_seed": None})
    assert step["mlm_weight"] == 0.5 and step["mlm_probability"] == 0.2 and "mlm_seed" not in step
    sig = inspect.signature(C.JointContrastiveTrainer.__init__).parameters
    assert all(sig[k].default is None for k in new)                               # not given = the step as it always was


@pytest.mark.parametrize("argv, extra", [
    (["class-inc", "--joint"], {}),
    (["class-inc", "--joint", "--mlm-weight", "0.5"], {"mlm_weight": 0.5}),
    (["data-inc", "--joint", "--mlm-weight", "1", "--mlm-probability", "0.2", "--mlm-seed", "7"],
     {"mlm_weight": 1.0, "mlm_probability": 0.2, "mlm_seed": 7})])
def test_the_drivers_flags(argv, extra):
    je = drivers.joint_encoders_from_args(drivers.parse_args(argv), object())
    assert {k: v for k, v in je.items() if k.startswith("mlm")} == extra          # the keys exist only when their flag is given
    step, _ = TR.joint_options(je)
    assert {k: v for k, v in step.items() if k.startswith("mlm")} == extra


@pytest.mark.parametrize("argv", [["class-inc", "--joint", "--mlm-probability", "0.2"], ["class-inc", "--joint", "--mlm-seed", "1"],
                                  ["class-inc", "--mlm-weight", "1"], ["class-inc", "--joint", "--mlm-weight", "-1"],
                                  ["class-inc", "--joint", "--mlm-weight", "1", "--mlm-probability", "2"],
                                  ["class-inc", "--joint", "--mlm-weight", "1", "--micro-batch", "4"]])
def test_the_drivers_refusals(argv):
    with pytest.raises(SystemExit) as e:
        drivers.parse_args(argv)
    assert e.value.code == 2


def test_abi_arity_and_no_scratch_memory():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    want = {"cxrk_mlm_mask_tokens": 20, "cxrk_mlm_gather_rows": 9, "cxrk_mlm_scatter_rows": 8, "cxrk_mlm_xent_stats": 13,
            "cxrk_mlm_xent_finish": 12, "cxrk_mlm_xent_grad": 17}
    for name, nargs in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip()]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert sorted(n for n in _lib.SIGNATURES if "mlm" in n) == sorted(want)
    assert not [n for n in _lib.SIGNATURES if "mlm" in n and n.endswith("_bytes")]   # no scratch memory: nothing to size
    src = open(os.path.join(ROOT, "incremental_multimodal_medical_learning_ii_amd", "csrc", "mlm.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)                                  # no atomic decides anything
