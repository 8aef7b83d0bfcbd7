"""The kernels of the masked-language-modelling loss on the device (csrc/mlm.hip), in both precisions.

Mask kernel: bit for bit the numpy restatement (tests/mlm_ref.py) at N = 5, L = 19, row offset 3, with pads and special tokens; one call
equals two sharded calls; a forced small capacity keeps the first selections in token order and reports the overflow; p = 0 selects
nothing.  Head (`functional.mlm_loss`): H = 128, V = 300 with the chunk forced to 128 vocabulary rows (chunks 128 / 128 / 40 and the
unaligned tail of 4 columns), 37 slots of which 29 count, targets at the chunk edges, +-80 logits, NaN propagation, inert padding,
no slot counting, and the chunked sweep against one whole chunk.  Parity: loss, accuracy and every head gradient against
`oracle.ref_text.mlm_logits` + `F.cross_entropy(ignore_index=-100)` on the CPU.  Tolerances: those of the loss-head tests
(tests/test_logit_scale_gpu.py `close`: 2e-5 of the reference's largest magnitude, 3e-4 in split-bf16 mode)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mlm_ref as R  # noqa: E402
from test_logit_scale_gpu import _bits, _split, _tol, close  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
SPECIAL = (0, 1, 2, 3, 4)
SEED = 0x1234ABCD5678EF01
N_M, L_M, OFF_M, V_M = 5, 19, 3, 300


def _tokens(N=N_M, L=L_M, vocab=V_M, seed=0):
    g = np.random.default_rng(seed)
    ids = g.integers(5, vocab, size=(N, L))
    ids[:, 0] = 2
    mask = np.ones((N, L), dtype=np.int64)
    for n in range(N):
        ln = int(g.integers(4, L + 1))
        ids[n, ln - 1] = 3
        ids[n, ln:] = 0
        mask[n, ln:] = 0
    ids[1, 2], ids[2, 3] = 1, 4                                    # an [UNK] and a [MASK] already in the text: never drawn
    return ids, mask


def _run_mask(ids, mask, p, counter=5, row_offset=OFF_M, cap=None):
    m = K.mlm_mask_tokens(torch.as_tensor(ids, device=DEV), None if mask is None else torch.as_tensor(mask, device=DEV), SEED, counter, p,
                          V_M, 4, SPECIAL, row_offset=row_offset, cap=cap)
    return {k: getattr(m, k).cpu().numpy() for k in ("ids", "sel", "tgt", "stats", "count")}


def _same_mask(got, ref):
    assert np.array_equal(got["ids"], ref["ids_out"])
    assert np.array_equal(got["sel"], ref["sel"]) and np.array_equal(got["tgt"], ref["tgt"])
    assert got["stats"].tolist() == [ref["kept"], ref["selected"]] and got["count"].tolist() == [float(ref["kept"])]


@pytest.mark.parametrize("p", [0.15, 0.5, 1.0])
def test_mask_kernel_is_the_numpy_draw_bit_for_bit(p):
    ids, mask = _tokens()
    ref = R.mask_tokens(ids, mask, SEED, 5, p, V_M, 4, SPECIAL, row_offset=OFF_M)
    assert ref["selected"] > 0 and ref["sel"].shape[0] == K.mlm_capacity(N_M * L_M, p)
    _same_mask(_run_mask(ids, mask, p), ref)
    _same_mask(_run_mask(ids, None, p), R.mask_tokens(ids, None, SEED, 5, p, V_M, 4, SPECIAL, row_offset=OFF_M))   # no mask: all attended


def test_mask_kernel_one_call_equals_two_sharded_calls():
    ids, mask = _tokens()
    whole = _run_mask(ids, mask, 0.5)
    a, b = _run_mask(ids[:2], mask[:2], 0.5, row_offset=OFF_M), _run_mask(ids[2:], mask[2:], 0.5, row_offset=OFF_M + 2)
    assert np.array_equal(np.concatenate([a["ids"], b["ids"]]), whole["ids"])
    ka, kb = int(a["stats"][0]), int(b["stats"][0])
    assert ka == a["stats"][1] and kb == b["stats"][1] and ka + kb == whole["stats"][1]
    assert np.array_equal(np.concatenate([a["sel"][:ka], b["sel"][:kb] + 2 * L_M]), whole["sel"][:ka + kb])
    assert np.array_equal(np.concatenate([a["tgt"][:ka], b["tgt"][:kb]]), whole["tgt"][:ka + kb])
    assert not np.array_equal(_run_mask(ids, mask, 0.5, counter=6)["ids"], whole["ids"])          # the counter is part of the key


def test_mask_kernel_overflow_and_nothing_selected():
    ids, mask = _tokens()
    full = R.mask_tokens(ids, mask, SEED, 5, 0.5, V_M, 4, SPECIAL, row_offset=OFF_M)
    cap = 7
    assert full["selected"] > cap
    got = _run_mask(ids, mask, 0.5, cap=cap)
    _same_mask(got, R.mask_tokens(ids, mask, SEED, 5, 0.5, V_M, 4, SPECIAL, row_offset=OFF_M, cap=cap))
    assert np.array_equal(got["sel"], full["sel"][:cap]) and got["stats"][1] > got["stats"][0] == cap    # selected > kept: the report
    assert np.array_equal(got["ids"], full["ids_out"])                                                # the rest stay corrupted
    none = _run_mask(ids, mask, 0.0)
    assert none["stats"].tolist() == [0, 0] and np.array_equal(none["ids"], ids) and np.all(none["sel"] == -1) and np.all(none["tgt"] == -1)
    # 2 blocks of 256 tokens: the second block's offset comes from the first block's count
    big_ids, big_mask = _tokens(N=20, L=19, seed=9)
    _same_mask(_run_mask(big_ids, big_mask, 0.5), R.mask_tokens(big_ids, big_mask, SEED, 5, 0.5, V_M, 4, SPECIAL, row_offset=OFF_M))


def test_mask_kernel_refusals():
    ids = torch.as_tensor(_tokens()[0], device=DEV)
    for kw in (dict(p=1.5), dict(p=-0.1), dict(mask_id=V_M), dict(cap=0), dict(cap=N_M * L_M + 1)):
        a = dict(p=0.15, mask_id=4, cap=None)
        a.update(kw)
        with pytest.raises(ValueError):
            K.mlm_mask_tokens(ids, None, SEED, 0, a["p"], V_M, a["mask_id"], SPECIAL, cap=a["cap"])
    with pytest.raises(ValueError, match="at most 8"):
        K.mlm_mask_tokens(ids, None, SEED, 0, 0.15, V_M, 4, tuple(range(9)))


# ------------------------------------------------------------------------------------------------ the head
H_H, V_H, T_H, CAP_H, KEPT_H = 128, 300, 95, 37, 29
EDGE_TARGETS = (0, 127, 128, 299, 295, 296)       # chunk edges, and both sides of the unaligned tail chunk [292, 300) with skip 4


def _chunk_bytes(rows=CAP_H, cols=128):
    return rows * cols * (8 if _split() else 4)


def _head_case(seed=0, kept=KEPT_H, big=False):
    g = torch.Generator().manual_seed(seed)
    last = torch.randn(T_H, H_H, generator=g)
    params = [torch.randn(H_H, H_H, generator=g) / H_H ** 0.5, 0.1 * torch.randn(H_H, generator=g), 1 + 0.1 * torch.randn(H_H, generator=g),
              0.1 * torch.randn(H_H, generator=g), torch.randn(V_H, H_H, generator=g) / H_H ** 0.5, 0.1 * torch.randn(V_H, generator=g)]
    if big:                                        # logits of about +80 and -80 in every row
        params[5][5], params[5][6], params[5][298] = 80.0, -80.0, 80.0
    sel = np.full(CAP_H, -1, dtype=np.int32)
    tgt = np.full(CAP_H, -1, dtype=np.int32)
    rows = np.sort(np.random.default_rng(seed).choice(T_H, size=kept, replace=False))
    sel[:kept] = rows
    tgt[:kept] = np.random.default_rng(seed + 1).integers(0, V_H, size=kept)
    tgt[:min(kept, len(EDGE_TARGETS))] = EDGE_TARGETS[:kept]
    if big and kept > 8:
        tgt[6], tgt[7], tgt[8] = 5, 6, 298
    return last, params, sel, tgt


def _run_head(last, params, sel, tgt, kept, scale, weight=1.0, chunk_bytes=None, upstream=None):
    ld = last.to(DEV).requires_grad_(True)
    ps = [p.to(DEV).requires_grad_(True) for p in params]
    stats = torch.tensor([kept, kept], dtype=torch.int32, device=DEV)
    weighted, loss, correct = Fh._mlm_triple(ld, torch.as_tensor(sel, device=DEV), torch.as_tensor(tgt, device=DEV), stats, ps,
                                             torch.tensor([scale], dtype=torch.float32, device=DEV),
                                             _chunk_bytes() if chunk_bytes is None else chunk_bytes, weight)
    assert not loss.requires_grad and not correct.requires_grad
    (weighted if upstream is None else weighted * upstream).backward()
    return dict(weighted=weighted.detach(), loss=loss.detach(), correct=int(correct.cpu()), dlast=ld.grad, dparams=[p.grad for p in ps])


NAMES = ("transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight", "transform.LayerNorm.bias", "decoder.weight",
         "decoder.bias")


def _check(got, ref, weight=1.0):
    close(got["loss"].reshape(1), torch.tensor([ref["loss"]]), "loss")
    close(got["weighted"].reshape(1), torch.tensor([ref["loss"] * weight]), "weighted loss")
    assert ref["correct"][0] <= got["correct"] <= ref["correct"][1], (got["correct"], ref["correct"])
    close(got["dlast"], ref["dlast"], "d last")
    for name, a, b in zip(NAMES, got["dparams"], ref["dparams"]):
        close(a, b, "d " + name)


@pytest.mark.parametrize("big", [False, True], ids=["plain", "pm80"])
def test_head_against_float64(big):
    """chunks of 128 vocabulary rows (the last ragged), 37 slots of which 29 count, targets at v = 0, 127, 128, 299 and around the
    unaligned tail; `big`: logits of +-80; a weight and an upstream factor reach every gradient"""
    last, params, sel, tgt = _head_case(big=big)
    assert [c for c in Fh.mlm_vocab_chunks(V_H, CAP_H, _chunk_bytes(), _split())] == [(0, 128, 0), (128, 128, 0), (256, 40, 0), (292, 8, 4)]
    scale = 1.0 / KEPT_H
    got = _run_head(last, params, sel, tgt, KEPT_H, scale, weight=0.5, upstream=3.0)
    ref = R.head_loss(last, sel, tgt, KEPT_H, params, scale, weight=1.5, tol=_tol())
    if big:
        lg = R.head_logits(last[sel[:KEPT_H].astype(np.int64)].double(), *[p.double() for p in params])
        assert float(lg.max()) > 70 and float(lg.min()) < -70
    _check(got, ref, weight=0.5)
    # rows that do not count get no gradient, and the unselected tokens none either
    rows = torch.as_tensor(sel[:KEPT_H].astype(np.int64))
    rest = torch.ones(T_H, dtype=torch.bool)
    rest[rows] = False
    assert torch.equal(got["dlast"].cpu()[rest], torch.zeros(int(rest.sum()), H_H)) and float(got["dlast"].cpu()[rows].abs().min(dim=1)[0].min()) > 0


def test_no_slot_counting_gives_exact_zeros():
    """kept = 0 (M_global = 0: the scale is 1 / max(0, 1) = 1): the loss and every gradient are exactly 0, not NaN"""
    last, params, sel, tgt = _head_case(kept=0)
    got = _run_head(last, params, sel, tgt, 0, 1.0)
    assert float(got["loss"]) == 0.0 and float(got["weighted"]) == 0.0 and got["correct"] == 0
    assert not bool(got["dlast"].any()) and all(not bool(g.any()) and bool(torch.isfinite(g).all()) for g in got["dparams"])


def test_nan_in_a_counted_row_reaches_the_loss_and_padding_is_inert():
    last, params, sel, tgt = _head_case()
    scale = 1.0 / KEPT_H
    clean = _run_head(last, params, sel, tgt, KEPT_H, scale)
    # poison in tokens that are not selected, and in tokens that the slots BEHIND the kept ones point at: nothing may change, bit for bit
    free = np.setdiff1d(np.arange(T_H), sel[:KEPT_H])
    poisoned = last.clone()
    poisoned[torch.as_tensor(free)] = float("nan")
    sel2, tgt2 = sel.copy(), tgt.copy()
    sel2[KEPT_H:] = free[:CAP_H - KEPT_H]
    tgt2[KEPT_H:] = 7
    inert = _run_head(poisoned, params, sel2, tgt2, KEPT_H, scale)
    assert torch.equal(_bits(inert["loss"]), _bits(clean["loss"])) and inert["correct"] == clean["correct"]
    rows = torch.as_tensor(sel[:KEPT_H].astype(np.int64))
    assert torch.equal(_bits(inert["dlast"][rows.to(DEV)]), _bits(clean["dlast"][rows.to(DEV)]))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(inert["dparams"], clean["dparams"]))
    # a NaN in a row that counts reaches the loss
    bad = last.clone()
    bad[int(sel[3]), 17] = float("nan")
    assert not bool(torch.isfinite(_run_head(bad, params, sel, tgt, KEPT_H, scale)["loss"]))


def test_chunked_sweep_against_one_whole_chunk():
    """The forward statistics do not depend on the chunk size by construction (a lane's sequence of additions is a function of the
    absolute column): loss, accuracy and, through the log-sum-exps, every element of the logits gradient are bit-identical in fp32
    mode; so is the decoder bias gradient (a column sum of that block).  The data gradient is accumulated chunk by chunk, which rounds
    differently from one long contraction, and the weight gradient's split-K follows the chunk's width: those agree to the head's
    tolerance.  Two runs of one configuration are bit-identical throughout, in both modes."""
    last, params, sel, tgt = _head_case(seed=3)
    scale = 1.0 / KEPT_H
    a = _run_head(last, params, sel, tgt, KEPT_H, scale)
    again = _run_head(last, params, sel, tgt, KEPT_H, scale)
    whole = _run_head(last, params, sel, tgt, KEPT_H, scale, chunk_bytes=1 << 30)
    assert len(Fh.mlm_vocab_chunks(V_H, CAP_H, 1 << 30, _split())) == 2
    assert torch.equal(_bits(a["loss"]), _bits(again["loss"])) and torch.equal(_bits(a["dlast"]), _bits(again["dlast"]))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a["dparams"], again["dparams"]))
    if not _split():
        assert torch.equal(_bits(a["loss"]), _bits(whole["loss"])) and torch.equal(_bits(a["dparams"][5]), _bits(whole["dparams"][5]))
    else:
        close(a["loss"].reshape(1), whole["loss"].reshape(1), "loss, chunked vs whole")
    assert a["correct"] == whole["correct"]
    close(a["dlast"], whole["dlast"], "d last, chunked vs whole")
    for name, x, y in zip(NAMES, a["dparams"], whole["dparams"]):
        close(x, y, f"d {name}, chunked vs whole")


def test_parity_with_the_oracle_head_and_cross_entropy():
    """loss, accuracy and all head gradients against `oracle.ref_text.mlm_logits` + `F.cross_entropy(ignore_index=-100)` (HF
    `BertForMaskedLM.forward(labels=)`'s loss) on a CPU copy, on the last hidden state of a 2-layer 128-wide CXR-BERT with a vocabulary
    of 300 whose ids were masked by the kernel"""
    from oracle import ref_text
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal import text as T
    cfg = dict(vocab_size=V_H, hidden_size=H_H, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=32)
    tm = T.CXRBertModel(T.CXRBertConfig(**cfg)).eval()
    syn.fill_module_(tm)
    sd = {k: v.detach().clone().double() for k, v in tm.state_dict().items()}
    tm.to(DEV)
    ids, mask = _tokens(N=8, L=16, seed=6)
    m = K.mlm_mask_tokens(torch.as_tensor(ids, device=DEV), torch.as_tensor(mask, device=DEV), SEED, 2, 0.3, V_H, 4, SPECIAL)
    kept = int(m.stats[0])
    assert 8 < kept == int(m.stats[1]) < m.sel.shape[0]
    proj, last = tm.get_projected_text_embeddings_and_hidden(m.ids, torch.as_tensor(mask, device=DEV))
    last = last.detach().requires_grad_(True)
    head = tm.mlm_head_params()
    scale = torch.reciprocal(torch.clamp(m.count, min=1.0))
    weighted, loss, correct = Fh._mlm_triple(last, m.sel, m.tgt, m.stats, head, scale, _chunk_bytes(m.sel.shape[0]), 1.0,
                                             tm.config.layer_norm_eps)
    grads = torch.autograd.grad(weighted, [last] + list(head))
    # the CPU copy: labels = -100 everywhere but at the selected tokens
    labels = torch.full((8 * 16,), -100, dtype=torch.int64)
    labels[m.sel[:kept].long().cpu()] = m.tgt[:kept].long().cpu()
    leaves = {k: sd[k].requires_grad_(True) for k in ("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
                                                      "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias",
                                                      "bert.embeddings.word_embeddings.weight", "cls.predictions.bias")}
    hidden = last.detach().cpu().double().requires_grad_(True)
    logits = ref_text.mlm_logits(sd, hidden).reshape(-1, V_H)
    ref = F.cross_entropy(logits, labels, ignore_index=-100)
    ref.backward()
    close(loss.reshape(1), ref.detach().reshape(1), "L_mlm")
    counted = labels >= 0
    lo, hi = R.correct_range(logits[counted], labels[counted], _tol())
    assert lo <= int(correct.cpu()) <= hi and hi - lo <= 2, (int(correct.cpu()), lo, hi)
    close(grads[0].reshape(-1, H_H), hidden.grad.reshape(-1, H_H), "d last hidden")
    for (name, leaf), g in zip(leaves.items(), grads[1:]):
        close(g, leaf.grad, "d " + name)
