"""Text-encoder dropout on the GPU: the mask generator against its numpy restatement, the dropout kernels against torch CPU fp32
with the same masks, the model against a CPU restatement with explicit masks, the determinism / invariance contract, and the joint
step (two streams, two data-parallel ranks)."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_ref import factors, keep_mask, model_factors, ones_factors, projected_with_masks
from incremental_multimodal_medical_learning_ii_amd import _lib
from incremental_multimodal_medical_learning_ii_amd import kernels as K
from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.image.model import get_biovil_resnet
from incremental_multimodal_medical_learning_ii_amd.health_multimodal.text import CXRBertConfig, CXRBertModel
from oracle import ref_text

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3                      # test_models_gpu.test_text_tiny_forward_backward_vs_reference


def _split() -> bool:
    return _lib.get_precision() == "split_bf16"


def close(a, b, tol=2e-5, what=""):   # tests/test_kernels_gpu.py tolerances
    if _split():
        tol = max(tol, 3e-4)
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), what
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    assert err < tol, (what, err)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ 1. mask generator
@pytest.mark.parametrize("seed,counter,layer,site,off,p,N,L,nH,C", [
    (0, 0, 0, 0, 0, 0.1, 3, 7, 1, 768),
    (0xDEADBEEFCAFEF00D, 17, 11, 3, 5, 0.1, 4, 32, 1, 64),
    (2 ** 64 - 1, 0xFFFFFF, 63, 2, 1000, 0.5, 2, 13, 1, 36),
    (12345, 3, 5, 1, 7, 0.1, 3, 33, 12, 33),
    (987654321987, 2 ** 24 + 9, 1, 1, 0, 0.5, 2, 65, 4, 65),
])
def test_mask_generator_matches_numpy(seed, counter, layer, site, off, p, N, L, nH, C):
    d = K.Drop(seed, counter, layer, site, off, p)
    got = K.dropout_mask(d, N, L, C, nH=nH).cpu().numpy().astype(bool)
    ref = keep_mask(seed, counter, layer, site, off, p, N, L, C, nH)
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_keep_rate(p):
    N, L, C = 64, 32, 768
    k = K.dropout_mask(K.Drop(42, 1, 2, 3, 0, p), N, L, C).float()
    n = k.numel()
    assert abs(float(k.mean()) - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n)


# ------------------------------------------------------------------------------------------------ 2. kernels
def _hidden_fac(d: K.Drop, N, L, H):
    return factors(keep_mask(d.seed, d.counter, d.layer, d.site, d.row_offset, d.p, N, L, H), d.p).view(N * L, H)


@pytest.mark.parametrize("planes", [False, True])
def test_embed_ln_dropout(planes):
    V, H, L, B = 50, 64, 8, 3
    word, pos, typ = rnd(V, H), rnd(16, H, seed=1), rnd(2, H, seed=2)
    g, b = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(5))
    d = K.Drop(77, 4, 0, K.DROP_EMBED, 3, 0.1)
    fac = _hidden_fac(d, B, L, H)
    ln = F.layer_norm(word[ids] + pos[:L][None] + typ[0], (H,), g, b, 1e-12).view(B * L, H)
    y, xhat, rstd = K.embed_ln_fwd(ids.view(-1).to(DEV), word.to(DEV), pos.to(DEV), typ[0].contiguous().to(DEV), g.to(DEV), b.to(DEV),
                                   1e-12, L, out_planes=planes, drop=d)
    close(y.float() if planes else y, ln * fac, what="embed ln dropout")
    _, xh0, rs0 = K.embed_ln_fwd(ids.view(-1).to(DEV), word.to(DEV), pos.to(DEV), typ[0].contiguous().to(DEV), g.to(DEV), b.to(DEV),
                                 1e-12, L)
    assert torch.equal(xhat, xh0) and torch.equal(rstd, rs0)      # saved statistics stay pre-dropout
    # backward in front of the embedding LayerNorm: dy masked on load
    s = (word[ids] + pos[:L][None] + typ[0]).view(B * L, H).requires_grad_(True)
    gg, bb = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    gy = rnd(B * L, H, seed=6)
    (F.layer_norm(s, (H,), gg, bb, 1e-12) * fac).backward(gy)
    dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    dx, none = K.residual_ln_bwd_drop(gy.to(DEV), xhat, rstd, g.to(DEV), dg, db, d, L, mask_dy=True)
    assert none is None
    close(dx, s.grad, what="embed ln dropout bwd")
    close(dg, gg.grad, what="embed ln dropout dgamma")
    close(db, bb.grad, what="embed ln dropout dbeta")


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("cls_rows", [False, True])
def test_residual_ln_dropout_fwd_bwd(planes, cls_rows):
    N, L, H = 5, 12, 128
    rows, rps = (N, 1) if cls_rows else (N * L, L)
    d = K.Drop(0x1234_5678_9ABC, 9, 4, K.DROP_FFN_OUT, 2, 0.1)
    x, resfull = rnd(rows, H), rnd(N * L, H, seed=1)
    res = resfull.view(N, L * H)[:, :H] if cls_rows else resfull          # CLS rows: a strided view, row stride L*H
    g, b = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    fac_full = _hidden_fac(d, N, L, H)
    fac = fac_full.view(N, L, H)[:, 0] if cls_rows else fac_full          # the CLS rows draw the full path's masks
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True)
    gg, bb = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.layer_norm(xr * fac + rr, (H,), gg, bb, 1e-12)
    gy = rnd(rows, H, seed=4)
    y.backward(gy)
    res_d = resfull.to(DEV)
    res_d = res_d.view(N, L * H)[:, :H] if cls_rows else res_d
    if planes:
        rp = K.split_planes(resfull.to(DEV))
        res_d = K.Planes(rp.t.view(2, N, L * H)[:, :, :H]) if cls_rows else rp
    yd, xhat, rstd = K.residual_ln_fwd(x.to(DEV), res_d, g.to(DEV), b.to(DEV), 1e-12, out_planes=planes, drop=d, rows_per_seq=rps)
    close(yd.float() if planes else yd, y, what="residual ln dropout fwd")
    dg, db, bs = torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.full((H,), 3.0, device=DEV)
    dsum, dxm = K.residual_ln_bwd_drop(gy.to(DEV), xhat, rstd, g.to(DEV), dg, db, d, rps, out_planes=planes, dxsum=bs)
    dsum, dxm = (dsum.float(), dxm.float()) if planes else (dsum, dxm)
    close(dsum, rr.grad, what="residual path gradient")
    close(dxm, xr.grad, what="dense output gradient (masked)")
    close(bs, xr.grad.sum(0), what="fused column sums of the masked gradient")
    close(dg, gg.grad, what="dgamma")
    close(db, bb.grad, what="dbeta")
    K.residual_ln_bwd_drop(gy.to(DEV), xhat, rstd, g.to(DEV), dg, db, d, rps, out_planes=planes, dxsum=bs, dxsum_accumulate=True)
    close(bs, 2 * xr.grad.sum(0), what="fused column sums, accumulated")


@pytest.mark.parametrize("L,ragged", [(16, "empty"), (32, True), (64, False), (65, True), (200, "empty"), (512, True)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_fwd_bwd(L, ragged, p):
    B, nH, dH = 3, 4, 64
    d = K.Drop(0xFEEDFACE12345, 6, 7, K.DROP_ATTN_PROBS, 10, p)
    qkv = rnd(B * L, 3 * nH * dH, scale=0.7).requires_grad_(True)
    mask = torch.ones(B, L, dtype=torch.int64)
    if ragged:
        for i in range(B):
            mask[i, max(1, L - 3 * i - 2):] = 0
    if ragged == "empty":
        mask[1] = 0
    fac = factors(keep_mask(d.seed, d.counter, d.layer, d.site, d.row_offset, p, B, L, L, nH), p)
    q, k, v = qkv.view(B, L, 3, nH, dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(dH) + (1.0 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    P = torch.softmax(s, -1)
    ctx = ((P * fac) @ v).transpose(1, 2).reshape(B * L, nH * dH)
    gc = rnd(B * L, nH * dH, seed=2)
    ctx.backward(gc)
    qd = qkv.detach().to(DEV)
    cd, probs = K.attn_fwd(qd, mask.to(DEV), B, L, nH, dH, drop=d)
    close(cd, ctx, what="attn dropout fwd")
    close(probs, P, what="saved probs stay undropped")
    close(K.attn_bwd(qd, probs, gc.to(DEV), B, L, nH, dH, drop=d), qkv.grad, tol=5e-5, what="attn dropout bwd")
    cp, _ = K.attn_fwd(qd, mask.to(DEV), B, L, nH, dH, out_planes=True, drop=d)
    close(cp.float(), ctx, what="attn dropout fwd -> planes")
    close(K.attn_bwd(qd, probs, gc.to(DEV), B, L, nH, dH, out_planes=True, drop=d).float(), qkv.grad, tol=5e-5,
          what="attn dropout bwd -> planes")


# ------------------------------------------------------------------------------------------------ 3. model
def _model(n_layers, H=64, nH=4, inter=256, vocab=128, seed=None):
    cfg = CXRBertConfig(vocab_size=vocab, hidden_size=H, num_attention_heads=nH, intermediate_size=inter, num_hidden_layers=n_layers,
                        max_position_embeddings=64, projection_size=128)
    m = CXRBertModel(cfg)
    syn.fill_module_(m)
    m.to(DEV).prepare_()
    if seed is not None:
        m.enable_dropout_(seed)
    return m


def _params_cpu(m):
    return {n: t.detach().cpu().clone().requires_grad_(True) for n, t in m.named_parameters()}


def test_restatement_with_unit_masks_is_the_oracle():
    m = _model(2)
    p = {n: t.detach().cpu() for n, t in m.named_parameters()}
    ids, mask = syn.synthetic_tokens(4, 16, vocab=128, seed=3, ragged=True)
    a = projected_with_masks(p, ids, mask, 2, 4, ones_factors(4, 16, 64, 4, 2))
    b = ref_text.cxrbert_projected(p, ids, mask, 2, 4)
    assert torch.equal(a, b) or rel(a, b) < 1e-6


@pytest.mark.parametrize("n_layers,L", [(1, 16), (2, 32)])
def test_model_train_dropout_vs_cpu_restatement(n_layers, L):
    N, H, nH = 6, 64, 4
    m = _model(n_layers, seed=0xABCDEF0123456789).train()
    m.dropout_state = (0xABCDEF0123456789, 5)
    ids, mask = syn.synthetic_tokens(N, L, vocab=128, seed=8, ragged=True)
    probe = rnd(N, 128, seed=9)
    m.zero_grad()
    proj = m.get_projected_text_embeddings(ids.to(DEV), mask.to(DEV), normalize_embeddings=False)
    (proj * probe.to(DEV)).sum().backward()
    assert m.dropout_state == (0xABCDEF0123456789, 6)
    p = _params_cpu(m)
    fac = model_factors(0xABCDEF0123456789, 5, 0, 0.1, 0.1, N, L, H, nH, n_layers)
    ref = projected_with_masks(p, ids, mask, n_layers, nH, fac)
    (ref * probe).sum().backward()
    assert rel(proj, ref) < TOL
    checked = 0
    for name, t in m.named_parameters():
        if name.startswith("cls.predictions") or p[name].grad is None:
            continue
        refg = p[name].grad
        assert t.grad is not None, name
        if refg.abs().max() < 1e-5:
            assert t.grad.abs().max() < 1e-5, name
        else:
            assert rel(t.grad, refg) < TOL, (name, rel(t.grad, refg))
        checked += 1
    assert checked >= 5 + 16 * n_layers + 6
    # the full forward (all token rows in the last layer) draws the same masks: same projected embedding
    m.dropout_state = (0xABCDEF0123456789, 5)
    out = m(ids.to(DEV), mask.to(DEV), output_cls_projected_embedding=True, output_mlm_logits=False)
    assert rel(out.cls_projected_embedding, ref) < TOL


# ------------------------------------------------------------------------------------------------ 4. invariants
def _run(m, ids, mask, state, cls_only=True):
    m.dropout_state = state
    m.zero_grad()
    if cls_only:
        out = m.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    else:
        out = m(ids, mask, output_cls_projected_embedding=True, output_mlm_logits=False).cls_projected_embedding
    out.square().sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), [t.grad.detach().clone() for n, t in m.named_parameters() if t.grad is not None]


def test_dropout_determinism_and_invariants():
    m = _model(2, seed=11).train()
    ids, mask = syn.synthetic_tokens(8, 24, vocab=128, seed=12, ragged=True)
    ids, mask = ids.to(DEV), mask.to(DEV)
    o1, g1 = _run(m, ids, mask, (11, 3))
    o2, g2 = _run(m, ids, mask, (11, 3))
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))     # same state: bit-identical
    o3, _ = _run(m, ids, mask, (11, 4))
    assert not torch.equal(o1, o3)                                                      # advanced counter: new masks
    o4, g4 = _run(m, ids, mask, (11, 3), cls_only=False)                                # full path == cls_only path
    assert rel(o4, o1) < 1e-5
    assert all(rel(a, b) < TOL for a, b in zip(g4, g1) if b.abs().max() > 1e-5)
    # eval after opting in == a model that never opted in, bit for bit (no counter advance)
    m.eval()
    e1, ge1 = _run(m, ids, mask, (11, 9))
    assert m.dropout_state == (11, 9)
    ref = _model(2).eval()
    ref.zero_grad()
    r = ref.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    r.square().sum().backward()
    assert torch.equal(e1, r.detach())
    assert all(torch.equal(a, b.grad) for a, b in zip(ge1, [t for t in ref.parameters() if t.grad is not None]))
    # train mode with both probabilities 0: exactly the eval computation
    z = _model(2)
    z.config.hidden_dropout_prob = z.config.attention_probs_dropout_prob = 0.0
    z.train().enable_dropout_(1)
    assert torch.equal(z.get_projected_text_embeddings(ids, mask, normalize_embeddings=False), r.detach())


def test_seed_none_reproducible_with_manual_seed():
    ids, mask = syn.synthetic_tokens(4, 16, vocab=128, seed=13, ragged=True)
    outs = []
    for _ in range(2):
        m = _model(1)
        torch.manual_seed(2024)
        m.enable_dropout_().train()
        with torch.no_grad():
            outs.append(m.get_projected_text_embeddings(ids.to(DEV), mask.to(DEV), normalize_embeddings=False))
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 5. joint step
def _joint_models(seed=99):
    cfg = CXRBertConfig(vocab_size=300, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=32)
    tm, im = CXRBertModel(cfg), get_biovil_resnet(None).eval()
    syn.fill_module_(tm)
    syn.fill_module_(im)
    return im, tm.train().enable_dropout_(seed)


def test_joint_step_two_streams_equals_one_stream_with_dropout():
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    B, L = 8, 16
    images = syn.synthetic_images(B, 64, seed=5).to(DEV)
    ids, mask = syn.synthetic_tokens(B, L, vocab=300, seed=6, ragged=True)
    ids, mask = ids.to(DEV), mask.to(DEV)
    runs = []
    for two in (False, True):
        im, tm = _joint_models()
        tr = JointContrastiveTrainer(im.to(DEV), tm.to(DEV), lr=1e-4, temperature=0.07, two_streams=two)
        losses = [float(tr.step(images, ids, mask).item()) for _ in range(3)]
        torch.cuda.synchronize()
        assert tm.dropout_state == (99, 3)
        runs.append((losses, tr.optimizer.flat_p.detach().clone()))
    (l0, p0), (l1, p1) = runs
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-6 * abs(a), (l0, l1)
    d = (p0 - p1).abs()
    assert float((d > 1e-6 + 1e-3 * p0.abs()).float().mean()) < 1e-3


B_GLOBAL, L_DP = 8, 16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_build(seed):
    from incremental_multimodal_medical_learning_ii_amd.contrastive import JointContrastiveTrainer
    im, tm = _joint_models(seed)
    images = syn.synthetic_images(B_GLOBAL, 64, seed=3)
    ids, mask = syn.synthetic_tokens(B_GLOBAL, L_DP, vocab=300, seed=4, ragged=True)
    tr = JointContrastiveTrainer(im.to(DEV), tm.to(DEV), lr=1e-4, temperature=0.07)
    return tr, images, ids, mask


def _probe(tr):
    p = tr.optimizer.flat_p
    return p[:: max(1, p.numel() // 4096)].detach().cpu().numpy()


def _dp_worker(rank, world, port, out_dir, precision):
    sys.path.insert(0, ROOT)
    from incremental_multimodal_medical_learning_ii_amd import _lib as lib
    lib.set_precision(precision)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    tr, images, ids, mask = _dp_build(seed=4321 if rank == 0 else 1)    # rank 0's seed must win
    assert tr.text_model.dropout_state == (4321, 0)
    B = B_GLOBAL // world
    sl = slice(rank * B, (rank + 1) * B)
    loss = tr.step(images[sl].to(DEV), ids[sl].to(DEV), mask[sl].to(DEV))
    torch.cuda.synchronize()
    assert tr.text_model.dropout_row_offset == rank * B
    assert tr.text_model.dropout_state == (4321, 1)
    # re-seeding after the trainer was built (each rank draws its own seed): the next step starts from rank 0's again
    torch.manual_seed(100 + rank)
    tr.text_model.enable_dropout_()
    mine = tr.text_model.dropout_state
    tr.sync_dropout_state()
    states = [None] * world
    dist.all_gather_object(states, tr.text_model.dropout_state)
    assert states[0] == states[1] and (rank != 0 or states[0] == mine), states
    tr.sync_dropout_state()                                             # nothing changed since: no further broadcast needed
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), loss=float(loss.item()), sample=_probe(tr))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_dropout_step_matches_single_process_global_batch(tmp_path, precision):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path), precision), nprocs=world, join=True)
    tr, images, ids, mask = _dp_build(seed=4321)
    loss = tr.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    torch.cuda.synchronize()
    sample = _probe(tr)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(world)]
    for k in range(world):
        assert abs(float(r[k]["loss"]) - loss.item()) / abs(loss.item()) < 1e-5, (k, float(r[k]["loss"]), loss.item())
    np.testing.assert_array_equal(r[0]["sample"], r[1]["sample"])
    tr0, _, _, _ = _dp_build(seed=4321)
    before = _probe(tr0)
    upd_ref, upd_dp = sample - before, r[0]["sample"] - before
    agree = np.mean(np.abs(upd_ref - upd_dp) <= 2e-6 + 1e-2 * np.abs(upd_ref))
    assert agree > 0.99, agree
    # a different seed gives a different step: the masks matter
    tr2, _, _, _ = _dp_build(seed=4322)
    loss2 = tr2.step(images.to(DEV), ids.to(DEV), mask.to(DEV))
    assert abs(float(loss2.item()) - loss.item()) > 1e-6 * abs(loss.item())


# ------------------------------------------------------------------------------------------------ 6. Trainer / driver wiring
def test_trainer_runs_an_opted_in_text_model_in_train_mode_and_scores_in_eval(tmp_path):
    """`Trainer(..., joint_encoders=...)` (drivers --joint --text-dropout): the loop trains the opted-in text model in train mode
    (its dropout counter advances once per step) and the scoring loop puts it back into eval mode, which
    `TextInferenceEngine.get_embeddings_from_prompt` asserts."""
    from incremental_multimodal_medical_learning_ii_amd import Trainer as TR
    from incremental_multimodal_medical_learning_ii_amd.DataRetrieval import CHEXPERT_COMPETITION_CLASSES, create_prompts
    from incremental_multimodal_medical_learning_ii_amd.health_multimodal import text as T
    cfg = CXRBertConfig(vocab_size=2048, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                        max_position_embeddings=32)
    tm, im = CXRBertModel(cfg).eval(), get_biovil_resnet(None).eval()
    syn.fill_module_(tm)
    syn.fill_module_(im)
    tm.enable_dropout_(seed=5)
    engine = T.TextInferenceEngine(T.SyntheticTokenizer(2048), tm.to(DEV))
    names = list(CHEXPERT_COMPETITION_CLASSES)
    tr = TR.Trainer(False, create_prompts(names), names, "standard", 1e-5, torch.device(DEV), TR.ScalarWriter(str(tmp_path / "t")),
                    bert_encoder=engine, joint_encoders={"image_model": im.to(DEV), "temperature": 0.07})
    train, val, _ = TR.Trainer.synthetic_joint_loaders(8, 8, 8, 4, image_size=64, seq_len=16, vocab=2048, eval_batch_size=8)
    crit = torch.nn.BCEWithLogitsLoss()
    tr._set_mode(True)
    assert tm.training
    tr.train(list(train), crit, 1)
    assert tm.dropout_state == (5, 2)                      # two steps, one train-mode forward each
    m = tr.val(list(val), crit, 1, 1)
    assert not tm.training and "Accuracy" in m
    assert tm.dropout_state == (5, 2)                      # scoring draws no masks
    # a text model that did not opt in stays in eval mode throughout, as before
    tm2, im2 = CXRBertModel(cfg).eval(), get_biovil_resnet(None).eval()
    syn.fill_module_(tm2)
    syn.fill_module_(im2)
    tr2 = TR.Trainer(False, create_prompts(names), names, "standard", 1e-5, torch.device(DEV), TR.ScalarWriter(str(tmp_path / "u")),
                     bert_encoder=T.TextInferenceEngine(T.SyntheticTokenizer(2048), tm2.to(DEV)),
                     joint_encoders={"image_model": im2.to(DEV), "temperature": 0.07})
    tr2._set_mode(True)
    assert not tm2.training
