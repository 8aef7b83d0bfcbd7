"""The pairwise sigmoid loss on the GPU: the fused forward + backward kernel and the loss fold against float64, their
memory contract and non-finite behaviour, the autograd head `functional.sigmoid_pairs_loss`, and
`JointContrastiveTrainer(loss="sigmoid")` / `Trainer`.  The float64 reference is tests/sigmoid_ref.py (autograd over
exp(theta) * I_hat T_hat^T + b with F.logsigmoid)."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import memguard as MG  # noqa: E402
import sigmoid_ref as R  # noqa: E402
from test_logit_scale_gpu import (B_T, CFG, G2, G3, HI, LABELS, NEG, TAU_T, THETA_T, _batch, _bits, _host_batch, _joint, _trainer,  # noqa: E402
                                  cosines, head_inputs, head_keys, key_vector, pitched_dev)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("precision")]

from incremental_multimodal_medical_learning_ii_amd import _lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
TOL = 2e-5          # the head is exact fp32 in both precision modes: no GEMM is involved in the kernel tests
EMU = 5.8e-6        # the fp32 emulation of the kernel's formulas on the CPU against float64


def _tol():
    """functional / trainer tests, where the logits GEMMs take part: 3e-4 in split-bf16 mode"""
    return 3e-4 if _lib.get_precision() == "split_bf16" else 2e-5


def close(a, b, what="", tol=TOL):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    print(f"{what}: rel-to-max err {err:.3e} (tol {tol})")
    assert torch.isfinite(a).all(), what
    assert err < tol, f"{what}: rel-to-max err {err:.3e} (tol {tol})"


#          rows cols diag_off ld
SHAPES = [(1, 1, 0, 1),
          (8, 8, 0, 8),
          (8, 24, 16, 24),          # a DP shard
          (5, 7, 0, 9),             # scalar path, ragged, ld % 4 != 0
          (3, 1030, 0, 1032),       # crosses the 1024-column chunk and leaves a cut last group
          (4, 260, 256, 260)]
THETAS = [0.0, math.log(1.0 / 0.07), math.log(100.0)]
BIASES = [-10.0, 0.0, 3.0]
NOMATCH = 999                        # key_vector's keys are 1000 + 3 c and its four constants: no column carries this one


def block_keys(rows, cols, off):
    """tests/test_logit_scale_gpu.py's `key_vector` (a group of 3, a group of 2, a negative key, a pair that differs above bit 32),
    the row keys its slice [off, off + rows), plus ONE row -- the last -- whose key matches no column"""
    if cols < 7:
        kc = torch.tensor([G3] * cols, dtype=torch.int64)
    else:
        kc = key_vector(rows, cols, off)
    kr = kc[off:off + rows].clone()
    kr[rows - 1] = NOMATCH
    assert not bool((kc == NOMATCH).any())
    return kr, kc


def chunk_sums(v):
    nchunk = (v.shape[1] + 1023) // 1024
    return torch.stack([v[:, k * 1024:(k + 1) * 1024].sum(1) for k in range(nchunk)], 1).reshape(-1)


def scalars(theta, bias):
    th, b = torch.tensor([theta], dtype=torch.float32, device=DEV), torch.tensor([bias], dtype=torch.float32, device=DEV)
    return th, b, float(th.item()), float(b.item())


def misaligned_dev(S, ld):
    """a [rows, cols] view, rows ld apart, whose base is 4 bytes off a 16-byte boundary"""
    rows, cols = S.shape
    flat = torch.full((rows * ld + 4,), float("nan"), device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(S)
    assert v.data_ptr() % 16 == 4
    return v, flat


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
@pytest.mark.parametrize("rows,cols,off,ld", SHAPES)
def test_kernel_against_float64(rows, cols, off, ld, keyed):
    """t * g in the block, the loss, d theta and d b from the three planes of partial sums, over theta x b; every kernel run twice:
    bit-identical; `partials=False` leaves the same block; a base 4 bytes off 16-byte alignment (scalar path) gives the same values"""
    Cm = cosines(rows, cols)
    kr, kc = block_keys(rows, cols, off) if keyed else (None, None)
    krd, kcd = (kr.to(DEV), kc.to(DEV)) if keyed else (None, None)
    nchunk = (cols + 1023) // 1024
    up = torch.tensor(-1.75, device=DEV)
    for theta in THETAS:
        for bias in BIASES:
            th, b, th32, b32 = scalars(theta, bias)
            tg64, l64, gx64, g64 = R.block(Cm, th32, b32, off, kr, kc)
            what = f"[theta {theta:.3f} b {bias}]"
            # the kernel's formulas in fp32 on the CPU: within 5.8e-6 on all four quantities
            e_tg, e_l, e_gx, e_g = R.block_fp32(Cm, th32, b32, off, kr, kc)
            emu = (float((e_tg.double() - tg64).abs().max() / tg64.abs().max()),
                   abs(float(e_l.double().sum() - l64.sum())) / float(l64.sum()),
                   abs(float(e_gx.double().sum() - gx64.sum())) / max(float(gx64.abs().sum()), 1e-30),
                   abs(float(e_g.double().sum() - g64.sum())) / float(g64.abs().sum()))
            print(f"{what} fp32 emulation: block {emu[0]:.2e} loss {emu[1]:.2e} d theta {emu[2]:.2e} d b {emu[3]:.2e} (bound {EMU})")
            assert max(emu) <= EMU, emu
            Cd = pitched_dev(Cm, ld)
            assert Cd.stride(0) == ld or rows == 1
            G, part = K.sigmoid_pairs_fwd_bwd_inplace(Cd, off, krd, kcd, th, b)
            assert G.data_ptr() == Cd.data_ptr()
            assert tuple(part.shape) == (3, rows * nchunk) and part.numel() == K.sigmoid_partials_numel(rows, cols) and part.is_contiguous()
            close(G, tg64, what=f"{what} t*g")
            if ld > cols:
                assert bool(torch.isnan(Cd._base[:, cols:]).all()), "pitch padding of C written"
            Cd2 = pitched_dev(Cm, ld)
            G2_, part2 = K.sigmoid_pairs_fwd_bwd_inplace(Cd2, off, krd, kcd, th, b)
            assert torch.equal(G, G2_) and torch.equal(part, part2), "two runs of the kernel differ"
            Cd3 = pitched_dev(Cm, ld)
            G3_, none = K.sigmoid_pairs_fwd_bwd_inplace(Cd3, off, krd, kcd, th, b, partials=False)
            assert none is None and torch.equal(G, G3_), "partials = NULL changes the block"
            # each partial: a fixed-order fp32 sum of its chunk's summands
            for q, (name, v64) in enumerate((("l", l64), ("g*(t c)", gx64), ("g", g64))):
                perr = float((part[q].double().cpu() - chunk_sums(v64)).abs().max())
                assert perr <= TOL * float(v64.abs().sum(1).max()), (what, name, perr)
            # the loss: 2e-5 relative, fresh and accumulated
            lval = 0.25 * float(l64.sum())
            for acc, start in ((False, 2.5), (True, 2.5)):
                outs = []
                for _ in range(2):
                    loss = torch.tensor(start, device=DEV)
                    K.sigmoid_pairs_loss(part[0], 0.25, out=loss, accumulate=acc)
                    outs.append(loss)
                assert torch.equal(outs[0], outs[1]), "two runs of sigmoid_pairs_loss differ"
                got = outs[0].item() - (start if acc else 0.0)
                print(f"{what} loss accumulate={acc}: {got} vs {lval} rel {abs(got - lval) / lval:.3e}")
                assert abs(got - lval) <= TOL * max(lval, start if acc else 0.0)
            fresh = K.sigmoid_pairs_loss(part[0], 0.25)
            assert fresh.shape == () and abs(fresh.item() - lval) <= TOL * lval
            # d theta / d b through the unchanged cxrk_logit_scale_grad: 2e-5 of scale * sum |summands|
            for q, name, v64 in ((1, "d theta", gx64), (2, "d b", g64)):
                mag = 1.75 * 0.25 * float(v64.abs().sum())
                for acc, start in ((False, 0.5), (True, 0.5)):
                    outs = []
                    for _ in range(2):
                        d = torch.tensor([start], device=DEV)
                        K.logit_scale_grad(part[q], None, up, 0.25, d, acc)
                        outs.append(d)
                    assert torch.equal(outs[0], outs[1])
                    want = -1.75 * 0.25 * float(v64.sum()) + (start if acc else 0.0)
                    err = abs(float(outs[0].item()) - want)
                    print(f"{what} {name} accumulate={acc}: {outs[0].item()} vs {want}; err {err:.3e} = {err / max(mag, 1e-30):.3e} of the magnitude")
                    assert err <= TOL * mag + (1e-7 * start if acc else 0.0)
    # a base pointer 4 bytes off 16-byte alignment: the scalar kernel, same values (theta, b: the last of the sweep)
    Cu, flat = misaligned_dev(Cm, ld)
    Gu, partu = K.sigmoid_pairs_fwd_bwd_inplace(Cu, off, krd, kcd, th, b)
    close(Gu, tg64, what="misaligned t*g")
    close(partu[0].sum(), l64.sum(), what="misaligned sum l")
    assert bool(torch.isnan(flat[0]).all()) and bool(torch.isnan(flat[1 + rows * ld:]).all())
    if ld > cols:
        assert bool(torch.isnan(flat[1:1 + rows * ld].view(rows, ld)[:, cols:]).all()), "pitch padding of C written"


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
@pytest.mark.parametrize("rows,cols,off,ld", SHAPES)
def test_guarded_outputs(rows, cols, off, ld, keyed):
    """both entry points between guard regions (tests/memguard.py), outputs starting from the sentinel: guards and the pitch padding
    intact, every element of the exact-size partials written, results bit-identical between the runs (independent of stale memory)"""
    Cm = cosines(rows, cols)
    kr, kc = block_keys(rows, cols, off) if keyed else (None, None)
    krd, kcd = (kr.to(DEV), kc.to(DEV)) if keyed else (None, None)
    th, b, th32, b32 = scalars(THETAS[1], BIASES[0])
    tg64, l64, gx64, g64 = R.block(Cm, th32, b32, off, kr, kc)
    lib = _lib.load()
    st = K._stream
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    runs = ("session", "nan")
    nchunk = (cols + 1023) // 1024
    n = rows * nchunk

    def call(name, *args):
        _lib.check(getattr(lib, name)(*args, st()), name)

    def fused(o):
        call("cxrk_sigmoid_pairs_fwd_bwd_inplace", P(o["C"]), ld, rows, cols, off, P(krd), P(kcd), P(th), P(b), P(o.get("partials")))

    og = MG.run_contract(fused, {"C": Out((rows, cols), ld=ld, init=Cm), "partials": Out((3 * n,))}, {"C": tg64}, TOL, module=K, device=DEV,
                         runs=runs)
    want = torch.cat([chunk_sums(l64), chunk_sums(gx64), chunk_sums(g64)])
    scale = torch.cat([v.abs().sum(1).max().expand(n) for v in (l64, gx64, g64)])
    assert bool(((og["partials"].value() - want).abs() <= TOL * scale).all())
    MG.run_contract(fused, {"C": Out((rows, cols), ld=ld, init=Cm)}, {"C": tg64}, TOL, module=K, device=DEV, runs=runs)      # partials = NULL
    part_d = og["partials"].t.clone()
    lval = 0.5 * l64.sum()
    MG.run_contract(lambda o: call("cxrk_sigmoid_pairs_loss", P(part_d), n, 0.5, P(o["loss"]), 0), {"loss": Out(())}, {"loss": lval}, TOL,
                    module=K, device=DEV, runs=runs)
    MG.run_contract(lambda o: call("cxrk_sigmoid_pairs_loss", P(part_d), n, 0.5, P(o["loss"]), 1), {"loss": Out((), init=torch.tensor(2.5))},
                    {"loss": 2.5 + lval}, TOL, module=K, device=DEV, runs=runs)


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
def test_one_nan_cosine(keyed):
    """a NaN cosine: its own element, its row's three partial sums, the loss, d theta and d b are non-finite; every other element of
    the block is finite and equal to the reference"""
    rows, cols, off, ld = 8, 24, 16, 24
    Cm = cosines(rows, cols)
    kr, kc = block_keys(rows, cols, off) if keyed else (None, None)
    krd, kcd = (kr.to(DEV), kc.to(DEV)) if keyed else (None, None)
    th, b, th32, b32 = scalars(THETAS[1], BIASES[0])
    tg64 = R.block(Cm, th32, b32, off, kr, kc)[0]
    for (r, c) in ((2, 5), (1, off + 1)):                        # a negative and (plain form) a positive position
        bad = Cm.clone()
        bad[r, c] = float("nan")
        Cd = pitched_dev(bad, ld)
        G, part = K.sigmoid_pairs_fwd_bwd_inplace(Cd, off, krd, kcd, th, b)
        G, part = G.cpu(), part.cpu()
        assert not math.isfinite(G[r, c].item())
        ok = torch.ones(rows, cols, dtype=torch.bool)
        ok[r, c] = False
        assert bool(torch.isfinite(G[ok]).all())
        err = float((G.double()[ok] - tg64[ok]).abs().max() / tg64[ok].abs().max())
        assert err < TOL, err
        rows_ok = torch.arange(rows) != r
        for q in range(3):
            assert not math.isfinite(part[q, r].item()) and bool(torch.isfinite(part[q][rows_ok]).all()), (q, part[q])
        part = part.to(DEV)
        assert not math.isfinite(K.sigmoid_pairs_loss(part[0], 1.0 / cols).item())
        one = torch.tensor(1.0, device=DEV)
        for q in (1, 2):
            d = torch.zeros(1, device=DEV)
            K.logit_scale_grad(part[q], None, one, 1.0 / cols, d, False)
            assert not math.isfinite(d.item())
        G0, none = K.sigmoid_pairs_fwd_bwd_inplace(pitched_dev(bad, ld), off, krd, kcd, th, b, partials=False)
        assert none is None and not math.isfinite(G0[r, c].item()) and torch.equal(G0.cpu()[ok], G[ok])


def test_bad_arguments_return_error_codes():
    lib = _lib.load()
    st = K._stream()
    Cm = torch.zeros(4, 8, device=DEV)
    k4, k8 = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    th, b, o1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    part = torch.zeros(12, device=DEV)
    P = lambda t: t.data_ptr()   # noqa: E731

    def sweep(fn, good, bads):
        assert fn(*good, st) == 0
        for idx, bad in bads:
            a = list(good)
            a[idx] = bad
            assert fn(*a, st) == -1, (fn.__name__, idx, bad)

    sweep(lib.cxrk_sigmoid_pairs_fwd_bwd_inplace, [P(Cm), 8, 4, 8, 2, None, None, P(th), P(b), P(part)],
          ((0, None), (7, None), (8, None), (2, 0), (2, -1), (3, 0), (3, -2), (1, 7), (4, -1), (4, 5), (5, P(k4)), (6, P(k8))))
    sweep(lib.cxrk_sigmoid_pairs_fwd_bwd_inplace, [P(Cm), 8, 4, 8, 0, P(k4), P(k8), P(th), P(b), P(part)],
          ((0, None), (7, None), (8, None), (2, 0), (3, 0), (1, 7), (5, None), (6, None)))
    assert lib.cxrk_sigmoid_pairs_fwd_bwd_inplace(P(Cm), 8, 4, 8, 2, None, None, P(th), P(b), None, st) == 0      # partials = NULL is a mode
    assert lib.cxrk_sigmoid_pairs_fwd_bwd_inplace(P(Cm), 8, 4, 8, -1, P(k4), P(k8), P(th), P(b), None, st) == 0   # keyed: diag_off is ignored
    sweep(lib.cxrk_sigmoid_pairs_loss, [P(part), 12, 1.0, P(o1), 0], ((0, None), (1, 0), (1, -1), (3, None)))
    torch.cuda.synchronize()
    for bad in (th.double(), torch.zeros(2, device=DEV), th.cpu()):            # the wrappers: a scalar of the wrong dtype / shape / device
        with pytest.raises(ValueError):
            K.sigmoid_pairs_fwd_bwd_inplace(Cm, 0, None, None, bad, b)
        with pytest.raises(ValueError):
            K.sigmoid_pairs_fwd_bwd_inplace(Cm, 0, None, None, th, bad)
    with pytest.raises(ValueError):
        K.sigmoid_pairs_fwd_bwd_inplace(Cm, 0, k4, None, th, b)
    with pytest.raises(ValueError):
        K.sigmoid_pairs_fwd_bwd_inplace(Cm, 0, k4, k8.int(), th, b)
    with pytest.raises(ValueError):
        K.sigmoid_pairs_fwd_bwd_inplace(Cm.cpu(), 0, None, None, th, b)
    with pytest.raises(ValueError):
        K.sigmoid_pairs_loss(part, 1.0, out=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        K.sigmoid_pairs_loss(part.cpu(), 1.0)


# ------------------------------------------------------------------------------------------------ the autograd head
def run_head(I0, T0, theta, bias, keys=None, factor=1.0, params=(True, True)):
    I = I0.to(DEV).requires_grad_(True)
    Tt = T0.to(DEV).requires_grad_(True)
    th = torch.tensor([theta], dtype=torch.float32, device=DEV).requires_grad_(params[0])
    b = torch.tensor([bias], dtype=torch.float32, device=DEV).requires_grad_(params[1])
    loss = Fh.sigmoid_pairs_loss(I, Tt, th, b, keys=None if keys is None else keys.to(DEV))
    (loss * factor if factor != 1.0 else loss).backward()
    gr = lambda p: None if p.grad is None else p.grad.cpu().reshape(())   # noqa: E731
    return loss.detach().cpu(), I.grad.cpu(), Tt.grad.cpu(), gr(th), gr(b)


@pytest.mark.parametrize("dup", [False, True], ids=["distinct", "duplicates"])
@pytest.mark.parametrize("B", [8, 24])
def test_sigmoid_pairs_loss_against_reference(B, dup):
    """loss (1e-5 relative), d img / d txt (rtol 1e-4, atol 1e-6), d theta and d b against float64; run-to-run bit equality; constants
    in place of parameters give the same loss and embedding gradients and no scalar gradient"""
    I0, T0 = head_inputs(B)
    keys = head_keys(B) if dup else None
    for theta, bias in ((math.log(1.0 / 0.07), -10.0), (math.log(10.0), 0.0)):
        th32, b32 = float(torch.tensor(theta, dtype=torch.float32)), float(torch.tensor(bias, dtype=torch.float32))
        got = run_head(I0, T0, theta, bias, keys)
        ref = R.sigmoid_grads(I0, T0, th32, b32, keys)
        print(f"B={B} dup={dup} theta={theta:.3f} b={bias}: loss {got[0].item():.8f} ref {ref['loss']:.8f}; d theta {got[3].item():.8e} ref "
              f"{ref['dtheta']:.8e} (mag {ref['mag_theta']:.3e}); d b {got[4].item():.8e} ref {ref['db']:.8e} (mag {ref['mag_b']:.3e}); "
              f"max |d img - ref| {float((got[1].double() - ref['dimg']).abs().max()):.2e} (scale {float(ref['dimg'].abs().max()):.2e})")
        assert abs(got[0].item() - ref["loss"]) < 1e-5 * abs(ref["loss"])
        np.testing.assert_allclose(got[1].numpy(), ref["dimg"].numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(got[2].numpy(), ref["dtxt"].numpy(), rtol=1e-4, atol=1e-6)
        assert abs(got[3].item() - ref["dtheta"]) <= _tol() * ref["mag_theta"]
        assert abs(got[4].item() - ref["db"]) <= _tol() * ref["mag_b"]
        again = run_head(I0, T0, theta, bias, keys)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
        const = run_head(I0, T0, theta, bias, keys, params=(False, False))
        assert const[3] is None and const[4] is None and all(torch.equal(a, b) for a, b in zip(got[:3], const[:3]))
        only_b = run_head(I0, T0, theta, bias, keys, params=(False, True))
        assert only_b[3] is None and torch.equal(only_b[4], got[4])
        if dup:
            assert abs(got[0].item() - run_head(I0, T0, theta, bias, None)[0].item()) > 1e-3       # silently ignored keys fail here


def test_upstream_factor_reaches_d_theta_and_d_b():
    I0, T0 = head_inputs(8)
    one = run_head(I0, T0, math.log(1.0 / 0.07), -10.0, head_keys(8))
    three = run_head(I0, T0, math.log(1.0 / 0.07), -10.0, head_keys(8), factor=3.0)
    for q in (3, 4):
        a, b = float(three[q].double()), 3.0 * float(one[q].double())
        print(f"x3: {a:.9e} vs {b:.9e}")
        assert abs(b) > 1e-3 and abs(a - b) <= 1e-6 * abs(b)
    np.testing.assert_allclose(three[1].numpy(), 3.0 * one[1].numpy(), rtol=1e-5, atol=1e-9)


def test_scalars_need_not_be_leaves_and_bad_ones_are_refused():
    import warnings
    g = torch.Generator().manual_seed(5)
    I0, T0 = torch.randn(8, 128, generator=g), torch.randn(8, 128, generator=g)
    base = torch.tensor([1.3], device=DEV, requires_grad=True)
    bb = torch.tensor([-2.0], device=DEV, requires_grad=True)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*not a leaf Tensor.*")
        Fh.sigmoid_pairs_loss(I0.to(DEV).requires_grad_(True), T0.to(DEV).requires_grad_(True), base * 2.0, bb * 3.0).backward()
    ref = R.sigmoid_grads(I0, T0, float((base.detach() * 2.0).item()), float((bb.detach() * 3.0).item()))
    assert abs(base.grad.item() / 2.0 - ref["dtheta"]) <= _tol() * ref["mag_theta"]
    assert abs(bb.grad.item() / 3.0 - ref["db"]) <= _tol() * ref["mag_b"]
    th = torch.tensor([2.6], device=DEV, requires_grad=True)
    loss = Fh.sigmoid_pairs_loss(I0.to(DEV).requires_grad_(True), T0.to(DEV).requires_grad_(True), th, bb.detach())
    with torch.no_grad():
        th.add_(0.1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    I, Tt, ok = I0.to(DEV), T0.to(DEV), torch.zeros(1, device=DEV)
    for bad in (torch.zeros(1), torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(2, device=DEV), torch.zeros(1, 1, device=DEV), 2.66):
        with pytest.raises(ValueError, match="log_scale"):
            Fh.sigmoid_pairs_loss(I, Tt, bad, ok)
        with pytest.raises(ValueError, match="logit_bias"):
            Fh.sigmoid_pairs_loss(I, Tt, ok, bad)


# ------------------------------------------------------------------------------------------------ the joint trainer
def _embeddings(tr, images, ids, mask):
    with torch.no_grad():
        img = tr.image_model(images)
        txt = tr.text_model.get_projected_text_embeddings(ids, mask, normalize_embeddings=False)
    return img.cpu(), txt.cpu()


def test_first_adam_step_moves_theta_and_b_against_the_reference_gradient():
    """Adam's first step is lr * g / (|g| + eps): theta_1 = theta_0 - lr * sign(d theta_ref), b_1 = b_0 - lr * sign(d b_ref), within
    1e-3 * lr (lr = 1e-3: the bound 1e-6 is at the fp32 spacing of b near -10, 9.5e-7, and above theta's near 2.66)"""
    lr = 1e-3
    tr = _joint(lr=lr, learn_temperature=True, loss="sigmoid")
    images, ids, mask = _batch()
    for p in (tr.logit_scale, tr.logit_bias):
        assert isinstance(p, torch.nn.Parameter) and tuple(p.shape) == (1,)
    assert float(tr.logit_scale.item()) == THETA_T and tr.current_bias() == -10.0 and abs(tr.current_temperature() - TAU_T) < 1e-7
    n, base = tr.optimizer.flat_p.numel(), tr.optimizer.flat_p.data_ptr()
    assert (tr.logit_scale.data_ptr() - base) // 4 == n - 8 and (tr.logit_bias.data_ptr() - base) // 4 == n - 4   # theta, then b, last
    ref = R.sigmoid_grads(*_embeddings(tr, images, ids, mask), THETA_T, -10.0)
    print(f"reference d theta {ref['dtheta']:.6e} d b {ref['db']:.6e}")
    assert abs(ref["dtheta"]) > 1e-4 and abs(ref["db"]) > 1e-4
    tr.step(images, ids, mask)
    th1, b1 = float(tr.logit_scale.detach().double().item()), float(tr.logit_bias.detach().double().item())
    want_t, want_b = THETA_T - lr * math.copysign(1.0, ref["dtheta"]), -10.0 - lr * math.copysign(1.0, ref["db"])
    print(f"theta {THETA_T:.9f} -> {th1:.9f}, want {want_t:.9f}; b -10 -> {b1:.9f}, want {want_b:.9f}")
    assert abs(th1 - want_t) <= 1e-3 * lr
    assert abs(b1 - want_b) <= 1e-3 * lr + 9.6e-7                      # half a spacing of b on each side of the bound
    assert tr.current_bias() == float(tr.logit_bias.item())


def test_bounds_pin_theta_but_not_b():
    images, ids, mask = _batch()
    pinned = _joint(learn_temperature=True, loss="sigmoid", sigmoid_bias=-5.0, log_scale_bounds=(THETA_T, THETA_T))
    th0, b0 = _bits(pinned.logit_scale), _bits(pinned.logit_bias)
    assert pinned.current_bias() == -5.0
    for _ in range(3):
        pinned.step(images, ids, mask)
        assert torch.equal(_bits(pinned.logit_scale), th0)
    assert not torch.equal(_bits(pinned.logit_bias), b0)               # b is not clamped


def test_fixed_scalars_are_device_constants():
    """learn_temperature=False: no parameter, two constants made at construction; the step's loss is the reference's"""
    tr = _joint(loss="sigmoid", sigmoid_bias=-3.0)
    images, ids, mask = _batch()
    assert tr.logit_scale is None and tr.logit_bias is None and tr.current_bias() == -3.0 and tr.current_temperature() == TAU_T
    consts = tr._sigmoid_consts
    assert all(c.is_cuda and not c.requires_grad for c in consts)
    ref = R.sigmoid_grads(*_embeddings(tr, images, ids, mask), THETA_T, -3.0)
    n = tr.optimizer.flat_p.numel()
    loss = tr.step(images, ids, mask)
    assert abs(loss.item() - ref["loss"]) <= 2e-4 * abs(ref["loss"])   # the joint tests' loss bound (tests/test_multipos_gpu.py)
    assert tr._sigmoid_consts[0] is consts[0] and tr._sigmoid_consts[1] is consts[1] and tr.optimizer.flat_p.numel() == n
    assert float(consts[0].item()) == THETA_T and float(consts[1].item()) == -3.0


def test_twenty_steps_on_one_batch():
    tr = _joint(lr=1e-5, learn_temperature=True, loss="sigmoid")
    images, ids, mask = _batch(32)
    losses = [tr.step(images, ids, mask) for _ in range(20)]
    losses = [float(v.item()) for v in losses]
    print("losses", [f"{v:.5f}" for v in losses], "tau", tr.current_temperature(), "b", tr.current_bias())
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_composes_with_label_positives_and_text_dropout():
    tr = _joint(positives="labels", learn_temperature=True, loss="sigmoid")
    images, ids, mask = _batch()
    loss = tr.forward_loss(images, ids, mask, labels=LABELS)
    img, txt = _embeddings(tr, images, ids, mask)
    ref = R.sigmoid_grads(img, txt, THETA_T, -10.0, C.keys_from_labels(LABELS))
    plain = R.sigmoid_grads(img, txt, THETA_T, -10.0)
    assert abs(loss.item() - ref["loss"]) / abs(ref["loss"]) < 2e-4    # the joint test's loss bound (tests/test_multipos_gpu.py)
    assert abs(ref["loss"] - plain["loss"]) > 1e-3
    tr.text_model.enable_dropout_(seed=5)
    tr.text_model.train()
    th0, b0 = _bits(tr.logit_scale), _bits(tr.logit_bias)
    out = tr.step(images, ids, mask, labels=LABELS)
    assert math.isfinite(out.item()) and not torch.equal(_bits(tr.logit_scale), th0) and not torch.equal(_bits(tr.logit_bias), b0)


def test_default_trainer_is_untouched(monkeypatch):
    """loss="infonce" spelled out against a trainer built without the new arguments: the same sequence of kernel-wrapper calls, the
    same bits in loss and parameters, and no sigmoid wrapper among the calls"""
    calls = []
    for name, fn in list(vars(K).items()):
        if inspect.isfunction(fn) and fn.__module__ == K.__name__ and not name.startswith("_"):
            def wrap(fn, name=name):
                def recorded(*a, **k):
                    calls.append(name)
                    return fn(*a, **k)
                return recorded
            monkeypatch.setattr(K, name, wrap(fn))
    images, ids, mask = _batch()
    res = []
    for kw in ({}, {"loss": "infonce"}, {"learn_temperature": True}, {"learn_temperature": True, "loss": "infonce"}):
        del calls[:]
        tr = _joint(**kw)
        assert tr.loss == "infonce" and tr.logit_bias is None and tr._sigmoid_consts is None and tr.current_bias() is None
        loss = tr.step(images, ids, mask)
        loss2 = tr.step(images, ids, mask)
        res.append((list(calls), _bits(loss), _bits(loss2), _bits(tr.optimizer.flat_p)))
    for a, b in ((res[0], res[1]), (res[2], res[3])):
        assert a[0] == b[0], "the sequence of kernel-wrapper calls changed"
        assert len(a[0]) > 50 and not [n for n in a[0] if "sigmoid" in n]
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), "loss or parameters differ"
    del calls[:]
    sg = _joint(loss="sigmoid")                                         # the recorder does see the sigmoid path
    sg.step(images, ids, mask)
    assert calls.count("sigmoid_pairs_fwd_bwd_inplace") == 2 and calls.count("sigmoid_pairs_loss") == 1
    assert not [n for n in calls if n.startswith(("infonce_", "multipos_"))]


# ------------------------------------------------------------------------------------------------ Trainer
def test_trainer_save_load_and_epoch_log(tmp_path):
    crit = torch.nn.BCEWithLogitsLoss()
    tr = _trainer(tmp_path, "w", learn_temperature=True, contrastive_loss="sigmoid", sigmoid_bias=-6.0)
    assert tr._joint.loss == "sigmoid" and tr._joint.current_bias() == -6.0
    tr.train([_host_batch(), _host_batch()], crit, 1)               # one epoch of two steps
    th, b = _bits(tr._joint.logit_scale), _bits(tr._joint.logit_bias)
    assert not torch.equal(th, _bits(torch.tensor([THETA_T]))) and not torch.equal(b, _bits(torch.tensor([-6.0])))
    for tag, want in (("train/temperature", tr._joint.current_temperature()), ("train/bias", tr._joint.current_bias())):
        logged = tr.writer.scalars(tag)
        assert len(logged) == 1 and logged[0][2] == 1 and abs(logged[0][1] - want) < 1e-9, tag     # once per epoch
    tr.save()
    sd = torch.load(tmp_path / "w" / "logit_scale.pt", map_location="cpu", weights_only=True)
    assert set(sd) == {"logit_scale", "logit_bias"}
    fresh = _trainer(tmp_path, "w", learn_temperature=True, contrastive_loss="sigmoid")
    assert fresh._joint.current_bias() == -10.0
    fresh.load()
    assert torch.equal(_bits(fresh._joint.logit_scale), th) and torch.equal(_bits(fresh._joint.logit_bias), b)      # bit for bit
    torch.save({"logit_scale": sd["logit_scale"]}, tmp_path / "w" / "logit_scale.pt")                                # an InfoNCE run's file
    with pytest.raises(ValueError, match="logit_bias"):
        fresh.load()
    # the fixed form: nothing of it is written or logged
    fixed = _trainer(tmp_path, "p", contrastive_loss="sigmoid")
    fixed.train([_host_batch()], crit, 1)
    assert fixed.writer.scalars("train/temperature") == [] and fixed.writer.scalars("train/bias") == [] and len(fixed.writer.scalars("train/Loss")) == 1
    fixed.save()
    assert not os.path.exists(tmp_path / "p" / "logit_scale.pt")
    with pytest.raises(ValueError, match="sigmoid_bias"):
        _trainer(tmp_path, "q", sigmoid_bias=-10.0)


def test_weight_reset_leaves_theta_and_b_and_counts_them(tmp_path, monkeypatch):
    from incremental_multimodal_medical_learning_ii_amd import Trainer as TR
    crit = torch.nn.BCEWithLogitsLoss()
    tr = _trainer(tmp_path, "w", learn_temperature=True, contrastive_loss="sigmoid")
    theta, b = tr._joint.logit_scale, tr._joint.logit_bias
    tr.model_copy()
    tr._train_step(_host_batch(), tr.class_names, crit)
    moved = (_bits(theta), _bits(b))
    assert not torch.equal(moved[0], _bits(torch.tensor([THETA_T]))) and not torch.equal(moved[1], _bits(torch.tensor([-10.0])))
    seen = []
    real = TR.K.weight_reset

    def recorded(pnew, pold, threshold, counters):
        seen.append((pnew.data_ptr(), pnew.numel()))
        return real(pnew, pold, threshold, counters)
    monkeypatch.setattr(TR.K, "weight_reset", recorded)
    tr._weight_reset(0.5)
    torch.cuda.synchronize()
    assert torch.equal(_bits(theta), moved[0]) and torch.equal(_bits(b), moved[1])                          # untouched
    ptrs = [p for p, _ in seen]
    assert theta.data_ptr() not in ptrs and b.data_ptr() not in ptrs and len(seen) == len(tr.optimizer.params) - 2
    assert tr._reset_total == sum(p.numel() for p in tr.optimizer.params) == sum(n for _, n in seen) + 2    # ... and counted
    n_reset, n_updated = tr._reset_stats()
    assert n_reset + n_updated == tr._reset_total and n_updated >= 2
