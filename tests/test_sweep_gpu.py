"""Seeded differential sweep of the attention, GEMM, column-reduction and head kernels, the BERT row kernels (LayerNorm, embedding,
gelu', planes_add_rows), the image-side non-GEMM kernels (max-pool, layout transforms, spatial mean, BatchNorm folding and the
train-mode BatchNorm chain) and the masked-language-modelling kernels (token masking, gather / scatter of the selected rows, the
chunked vocabulary cross-entropy and its gradient, the whole head) (cases, float64 references, comparators and bounds:
tests/sweep_cases.py; what the sweep can see: tests/test_sweep_host.py).  Families A to D run in both contraction precisions; the
kernels of E, F and G neither dispatch nor store by that mode (kernels.py: only the GEMM and convolution launches read it; the
masked-LM kernels take their storage form from their arguments), so they run once -- but for G's head cases, whose GEMMs do.

Every input sits in a `memguard.Guarded` allocation and every output goes through `memguard.run_contract` (guards and pitch padding
intact, every element written, bit-identical over an ordinary and a NaN-poisoned exact-size workspace, and a +-1e30 one where the
call takes a workspace), so a stray access lands in memory the test owns.  Every generated case is legal under include/cxrk.h:
nothing is skipped, and a refusal by a wrapper fails the test.  Each test id is a chunk of at most 16 cases and prints its worst
error / bound per output before it asserts.

Family H (tests/sweep_conv_cases.py) is the convolutions, one operation per case: `test_conv_f32` the fp32 entry points and the stem's
form of the planes forward, `test_conv_planes` the planes entry points under the library's tile policy and with the 256x256 tile
forced.  Planes inputs keep tests/test_conv_geometry_gpu.py's gap between their planes.  Every output passes the elementwise derived
bound AND the per-channel / per-filter level; after every call the library's launch count, label and split-K are held to the Python
restatement of the dispatch (sweep_conv_cases.predict); decision bits, masked elements, the pixels of a stride-2 class that no tap
reaches, dx with and without fused sums, and the window-resident weight gradient against its implicit-GEMM twin are compared bit for
bit."""
import ctypes

import pytest
import torch

import memguard as MG
import sweep_cases as S

pytestmark = [pytest.mark.gpu]
both_precisions = pytest.mark.usefixtures("precision")

from incremental_multimodal_medical_learning_ii_amd import _lib as _cxr_lib  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import functional as Fh  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import kernels as K  # noqa: E402

DEV = "cuda"
Out = MG.Out
BF, U8, I32, I64 = torch.bfloat16, torch.uint8, torch.int32, torch.int64
CHUNK = 16

# (family, case): cases the sweep once failed on, with the cause; they run first in their family's test
REGRESSIONS = [
    # colstats took the block mean from sums shifted by the block's first row: on zero-mean columns their rounding was 23 e32 of the mean
    ("C", S.ColCase(index=55, op="colstats_biased", planes=True, rows=257, C=2048, pad=0, gap=0, alpha=1.0, accumulate=False, profile="randn")),
    ("C", S.ColCase(index=77, op="colstats_unbiased", planes=False, rows=1023, C=1024, pad=0, gap=0, alpha=1.0, accumulate=False, profile="randn")),
]


def _split() -> bool:
    return _cxr_lib.get_precision() == "split_bf16"


def cabi(name, *args):
    """a direct C-ABI call on the current stream (wrappers that allocate their outputs themselves)"""
    _cxr_lib.check(getattr(_cxr_lib.load(), name)(*args, K._stream()), name)


def P(t):
    return None if t is None else (t.ptr() if isinstance(t, K.Planes) else t.data_ptr())


def chunk_ids(family):
    return [f"chunk{i}" for i in range(-(-S.NCASES[family] // CHUNK))]


def chunk_cases(family, chunk_id):
    i = int(chunk_id[5:])
    first = [c for f, c in REGRESSIONS if f == family] if i == 0 else []
    return first + S.cases(family)[i * CHUNK:(i + 1) * CHUNK]


class Inputs:
    """the guarded inputs of one case; `check()` once the kernels have run"""

    def __init__(self):
        self.guards = []

    def put(self, t, name, ld=None, gap=0):
        g = MG.Guarded(t.shape, t.dtype, ld=ld, gap=gap, device=DEV, name=name).load(t)
        self.guards.append(g)
        return g.t

    def planes(self, t32, name, ld=None, gap=0):
        """the canonical split of an fp32 CPU tensor (what K.split_planes gives: tests/test_exact_planes_gpu.py) as guarded Planes"""
        hi, lo = S.canonical_planes(t32.contiguous())
        return K.Planes(self.put(torch.stack([hi, lo]), name, ld, gap))

    def check(self):
        for g in self.guards:
            g.check()


def run(call, outs, ws):
    return MG.run_contract(call, outs, module=K, device=DEV, runs=("session", "nan", "alt") if ws else ("session", "nan"))


class Report:
    def __init__(self, tag, mode=True):
        self.tag, self.worst, self.bad, self.mode = tag, {}, [], mode      # mode: the test runs per contraction precision

    def add(self, case, results, form=""):
        for name, ratio, _ in results:
            k = (name if self.mode else f"{case.op}.{name}") + form      # E and F hold several operations: figures per operation
            self.worst[k] = max(self.worst.get(k, 0.0), ratio)
        msg = S.failures(case, results)
        if msg:
            self.bad.append(form + " " + msg)

    def finish(self):
        print(f"{self.tag}{' [' + _cxr_lib.get_precision() + ']' if self.mode else ''} worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))
        assert not self.bad, "\n".join(self.bad)


def _like(got, ref):
    return {k: v.reshape(ref[k].shape) for k, v in got.items()}


# ================================================================================================================ A: attention
def _attention(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    B, L, nH, dH = c.B, c.L, c.nH, c.dH
    T, W = B * L, nH * dH
    G = Inputs()
    qd, md, gd = G.put(inp["qkv"], "qkv"), G.put(inp["mask"], "mask"), G.put(inp["dctx"], "dctx")
    o = run(lambda o: cabi("cxrk_attn_fwd", P(qd), P(md), B, L, nH, dH, P(o["ctx"]), 0, P(o["probs"])),
            {"ctx": Out((T, W)), "probs": Out((B, nH, L, L))}, False)
    probs = o["probs"].t
    got = {"ctx": o["ctx"].value(), "probs": o["probs"].value()}
    p64, live = got["probs"], inp["mask"].bool()
    assert float((p64.sum(-1) - 1).abs().max()) <= (L + 8) * 2.0 ** -23, f"{S.describe(c)}: probability rows do not sum to 1"
    dead = (~live & live.any(1, keepdim=True))[:, None, None, :].expand_as(p64)
    assert float(p64[dead].abs().max()) == 0.0 if bool(dead.any()) else True, f"{S.describe(c)}: a masked key has a probability"
    ws = L > 64      # the dS workspace of the tiled form
    o = run(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=o["dqkv"]), {"dqkv": Out((T, 3 * W))}, ws)
    got["dqkv"] = o["dqkv"].value()
    rep.add(c, S.check(c, ref, got, _split()))
    o = run(lambda o: cabi("cxrk_attn_fwd", P(qd), P(md), B, L, nH, dH, P(o["ctx"]), o["ctx"].stride(0), None), {"ctx": Out((2, T, W), BF)}, False)
    o2 = run(lambda o: K.attn_bwd(qd, probs, gd, B, L, nH, dH, out=K.Planes(o["dqkv"])), {"dqkv": Out((2, T, 3 * W), BF)}, ws)
    rep.add(c, S.check(c, ref, {"ctx": o["ctx"].value(), "dqkv": o2["dqkv"].value()}, _split(), planes_out=("ctx", "dqkv")), "->planes")
    G.check()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("A"))
def test_attention(chunk):
    rep = Report("attention " + chunk)
    for c in chunk_cases("A", chunk):
        _attention(c, rep)
    rep.finish()


# ================================================================================================================ B: dense GEMM
def _gemm(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    pl = c.family == "BPL"
    M, N, Kd = c.M, c.N, c.K
    ld = S.gemm_lds(c)
    G = Inputs()
    if pl:
        a, b = G.planes(inp["a"], "a", ld["lda"], c.gap_a), G.planes(inp["b"], "b", ld["ldb"], c.gap_b)
    else:
        a, b = G.put(inp["a"], "a", ld["lda"]), G.put(inp["b"], "b", ld["ldb"])
    bias = G.put(inp["bias"], "bias") if c.bias else None
    res = None
    if c.residual == "f32":
        res = G.put(inp["residual"], "residual", ld["ldr"])
    elif c.residual == "pl":
        res = G.planes(inp["residual"], "residual", ld["ldr"], c.gap_r)
    aux = G.put(inp["aux"], "aux", ld["ldaux"]) if c.auxmode in (1, 2) else None
    maskin = G.put(inp["maskin"], "maskin") if c.auxmode == 3 else None
    outs = {"out": Out((2, M, N), BF, ld=ld["ldc"], gap=c.gap_c) if c.out_planes else Out((M, N), ld=ld["ldc"], init=inp.get("c0"))}
    if c.preact:
        outs["preact"] = Out((M, N), ld=ld["ldc2"])
    if c.maskout:
        outs["bits"] = Out((M, N // 8), U8)
    if c.colsum != "none":
        outs["colsum"] = Out((N,), init=inp.get("colsum0"))

    def call(o):
        if pl:
            K.gemm_pl(a, b, M, N, Kd, c.ta, c.tb, out=K.Planes(o["out"]) if c.out_planes else o["out"], bias=bias, residual=res, aux=aux,
                      auxmode=c.auxmode, maskin=maskin, maskout=o.get("bits"), preact_out=o.get("preact"), act=c.act, alpha=c.alpha,
                      accumulate=c.accumulate, splitk=c.splitk, colsum=o.get("colsum"), colsum_accumulate=c.colsum == "acc")
        else:
            K.gemm(a, b, o["out"], M, N, Kd, c.ta, c.tb, bias=bias, residual=res, aux=aux, auxmode=c.auxmode, preact_out=o.get("preact"),
                   act=c.act, alpha=c.alpha, accumulate=c.accumulate, splitk=c.splitk)

    o = run(call, outs, c.splitk > 1 or c.colsum != "none")
    got = {k: o[k].value() for k in ("out", "preact", "colsum") if k in o}
    rep.add(c, S.check(c, ref, got))
    if c.maskout:      # the bits are the decisions of the values this launch stored
        assert torch.equal(S.unpack_bits(o["bits"].t.cpu(), N), got["out"] > 0), f"{S.describe(c)}: decision bits differ from the stored output"
    G.check()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("B32"))
def test_gemm_f32(chunk):
    rep = Report("gemm fp32 " + chunk)
    for c in chunk_cases("B32", chunk):
        _gemm(c, rep)
    rep.finish()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("BPL"))
def test_gemm_planes(chunk, wide):
    rep = Report(f"gemm planes {chunk} [{wide}]")
    for c in chunk_cases("BPL", chunk):
        _gemm(c, rep)
    rep.finish()


# ================================================================================================================ C: column reductions
def _columns(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    ldx = c.C + c.pad
    put = (lambda t, n: G.planes(t, n, ldx, c.gap)) if c.planes else (lambda t, n: G.put(t, n, ldx))
    x = put(inp["x"], "x")
    vec = Out((c.C,))
    if c.op == "colsum":
        o = run(lambda o: K.colsum(x, o["out"], alpha=c.alpha, accumulate=c.accumulate), {"out": Out((c.C,), init=inp.get("out0"))}, True)
    elif c.op == "colvar":
        mean = G.put(inp["mean"], "mean")
        o = run(lambda o: K.colvar(x, mean, o["out"], alpha=c.alpha), {"out": vec}, True)
    elif c.op.startswith("colstats"):
        o = run(lambda o: K.colstats(x, unbiased=c.op == "colstats_unbiased", out=(o["mean"], o["var"])), {"mean": vec, "var": Out((c.C,))}, True)
    else:
        a = put(inp["a"], "a")
        shift = G.put(inp["bshift"], "bshift") if c.op == "coldot_shift" else None
        o = run(lambda o: K.coldot(a, x, shift, out=o["out"]), {"out": vec}, True)
    rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}, _split()))
    G.check()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("C"))
def test_column_reductions(chunk):
    rep = Report("columns " + chunk)
    for c in chunk_cases("C", chunk):
        _columns(c, rep)
    rep.finish()


# ================================================================================================================ D: row-wise heads
def _heads(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    rows, cols = c.rows, c.cols
    got = {}
    if c.op == "l2norm":
        ldh = cols + c.pad
        xd, dd, nd = G.put(inp["x"], "x"), G.put(inp["dxhat"], "dxhat"), G.put(inp["norm"], "norm")
        xh = G.put(inp["xhat"], "xhat", ldh)
        o = run(lambda o: cabi("cxrk_l2norm_fwd", P(xd), rows, cols, 1e-12, P(o["xhat"]), ldh, P(o["norm"])),
                {"xhat": Out((rows, cols), ld=ldh), "norm": Out((rows,))}, False)
        got = {k: g.value() for k, g in o.items()}
        o = run(lambda o: cabi("cxrk_l2norm_bwd", P(dd), P(xh), ldh, P(nd), rows, cols, P(o["dx"])), {"dx": Out((rows, cols))}, False)
        got["dx"] = o["dx"].value()
    elif c.op == "infonce":
        ld = cols + c.pad
        Sd, lr, lc = G.put(inp["S"], "S", ld), G.put(inp["lse_row"], "lse_row"), G.put(inp["lse_col"], "lse_col")
        o = run(lambda o: cabi("cxrk_infonce_row_lse", P(Sd), ld, rows, cols, c.diag_off, P(o["lse"]), P(o["diag"]), P(o["loss"]), 0.5 / rows, int(c.flag_a)),
                {"lse": Out((rows,)), "diag": Out((rows,)), "loss": Out((), init=inp["loss0"] if c.flag_a else None)}, False)
        got = {k: g.value() for k, g in o.items()}
        o = run(lambda o: cabi("cxrk_infonce_grad_inplace", P(o["grad"]), ld, rows, cols, c.diag_off, P(lr), P(lc)),
                {"grad": Out((rows, cols), ld=ld, init=inp["S"])}, False)
        got["grad"] = o["grad"].value()
    elif c.op == "cosine":
        Pn, Gr = c.n, c.groups
        xd, yd = G.put(inp["x"], "x"), G.put(inp["y"], "y")
        spec = {"cos": Out((rows, Pn)), "xn": Out((rows,)), "yn": Out((Pn,))}
        if Gr:
            spec.update(max=Out((rows, Gr)), mean=Out((rows, Gr)), arg=Out((rows, Gr), I32))
            o = run(lambda o: cabi("cxrk_pairwise_cosine_max_fwd", P(xd), P(yd), rows, Gr, Pn // Gr, cols, P(o["cos"]), P(o["xn"]), P(o["yn"]),
                                   P(o["max"]), P(o["mean"]), P(o["arg"])), spec, False)
            won = ref["cos"].view(rows, Gr, -1).gather(2, o["arg"].t.cpu().long()[:, :, None])[:, :, 0]
            assert bool((won >= ref["max"] - 2e-5).all()), f"{S.describe(c)}: the winner's index does not point at the group's maximum"
        else:
            o = run(lambda o: cabi("cxrk_pairwise_cosine_fwd", P(xd), P(yd), rows, Pn, cols, P(o["cos"]), P(o["xn"]), P(o["yn"])), spec, False)
        got = {k: g.value() for k, g in o.items() if k != "arg"}
        cd, xn, yn, dc = G.put(inp["cos"], "cos"), G.put(inp["xn"], "xn"), G.put(inp["yn"], "yn"), G.put(inp["dcos"], "dcos")
        spec = {"dy": Out((Pn, cols), init=inp["dy0"] if c.flag_a else None)}
        if c.flag_b:
            spec["dx"] = Out((rows, cols))
        if Gr:
            arg = G.put(inp["arg"], "arg")
            o = run(lambda o: K.pairwise_cosine_max_bwd(xd, yd, cd, dc, arg, xn, yn, need_dx=c.flag_b, out=(o.get("dx"), o["dy"]), accumulate_dy=c.flag_a), spec, True)
        else:
            o = run(lambda o: K.pairwise_cosine_bwd(xd, yd, cd, dc, xn, yn, need_dx=c.flag_b, out=(o.get("dx"), o["dy"]), accumulate_dy=c.flag_a), spec, True)
        got.update({k: g.value() for k, g in o.items()})
    elif c.op == "bce":
        cd = G.put(inp["cos"], "cos")
        lab = G.put(inp["labels"], "labels")[:, :cols]          # a column slice of a wider label matrix: ldlab > C
        o = run(lambda o: K.bce_posneg_fwd_bwd(cd, lab, diff=c.flag_a, out=(o["logits"], o["dcos"], o["loss"])),
                {"logits": Out((rows, cols)), "dcos": Out((rows, 2 * cols)), "loss": Out(())}, True)
        got = {k: g.value() for k, g in o.items()}
        o = run(lambda o: cabi("cxrk_eval_score", P(cd), rows, cols, int(c.flag_b), P(o["score"]), P(o["pred"])),
                {"score": Out((rows, cols)), "pred": Out((rows, cols))}, False)
        got["score"] = o["score"].value()
        assert torch.equal(o["pred"].t.cpu(), (inp["cos"][:, 0::2] > inp["cos"][:, 1::2]).float()), f"{S.describe(c)}: pred"
    else:
        xd, gd = G.put(inp["x"], "x"), G.put(inp["dout"], "dout")
        o = run(lambda o: cabi("cxrk_group_mean_fwd", P(xd), rows, c.n, cols, P(o["out"])), {"out": Out((rows, cols))}, False)
        got["out"] = o["out"].value()
        o = run(lambda o: cabi("cxrk_group_mean_bwd", P(gd), rows, c.n, cols, P(o["din"])), {"din": Out((rows * c.n, cols))}, False)
        got["din"] = o["din"].value()
    rep.add(c, S.check(c, ref, _like(got, ref), _split()))
    G.check()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("D"))
def test_heads(chunk):
    rep = Report("heads " + chunk)
    for c in chunk_cases("D", chunk):
        _heads(c, rep)
    rep.finish()


# ================================================================================================================ E: BERT row kernels
def _ln_forward(c, inp, ref, G, rep):
    rows, H = c.rows, c.H
    gam, bet = G.put(inp["gamma"], "gamma"), G.put(inp["beta"], "beta")
    if c.op == "ln_fwd":
        xd, rd = G.put(inp["x"], "x"), (G.put(inp["res"], "res") if c.res else None)
        call = lambda y, yplane, o: cabi("cxrk_residual_ln_fwd", P(xd), P(rd), P(gam), P(bet), c.eps, rows, H, P(y), yplane, P(o["xhat"]), P(o["rstd"]))      # noqa: E731
    else:
        ids, word, pos, typ = (G.put(inp[k], k) for k in ("ids", "word", "pos", "type"))
        call = lambda y, yplane, o: cabi("cxrk_embed_ln_fwd", P(ids), P(word), P(pos), P(typ), P(gam), P(bet), c.eps, rows, c.L, H, P(y), yplane,      # noqa: E731
                                         P(o["xhat"]), P(o["rstd"]))
    saved = {"xhat": Out((rows, H)), "rstd": Out((rows,))}
    o = run(lambda o: call(o["y"], 0, o), dict(saved, y=Out((rows, H))), False)
    rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}))
    if H % 8 == 0:      # the planes output exists in the 8-column kernel only (bert.hip:874,883)
        o = run(lambda o: call(o["y"], o["y"].stride(0), o), dict(saved, y=Out((2, rows, H), BF)), False)
        rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}, planes_out=("y",)), "->planes")


def _rows(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    rows, H = c.rows, c.H
    if c.op in ("ln_fwd", "embed_ln_fwd"):
        _ln_forward(c, inp, ref, G, rep)
    elif c.op == "ln_bwd":
        dy, xhat, rstd, gam = (G.put(inp[k], k) for k in ("dy", "xhat", "rstd", "gamma"))
        add = G.put(inp["dx_add"], "dx_add") if c.res else None
        outs = {"dx": Out((2, rows, H), BF) if c.planes else Out((rows, H)), "dgamma": Out((H,), init=inp.get("dgamma0")),
                "dbeta": Out((H,), init=inp.get("dbeta0"))}
        if c.dxsum != "none":
            outs["dxsum"] = Out((H,), init=inp.get("dxsum0"))
        o = run(lambda o: K.residual_ln_bwd(dy, xhat, rstd, gam, o["dgamma"], o["dbeta"], dx_add=add, accumulate=c.accumulate,
                                            out=K.Planes(o["dx"]) if c.planes else o["dx"], dxsum=o.get("dxsum"), dxsum_accumulate=c.dxsum == "acc"),
                outs, True)
        rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}, planes_out=("dx",) if c.planes else ()))
    elif c.op == "embed_bwd":      # the three workspace runs are three launches: bit-identical (run_contract)
        ids, dx = G.put(inp["ids"], "ids"), G.put(inp["dx"], "dx")
        o = run(lambda o: K.embed_bwd(ids, dx, o["dword"]), {"dword": Out((c.V, H), init=inp["dword0"])}, True)
        rep.add(c, S.check(c, ref, {"dword": o["dword"].value()}))
    elif c.op == "gelu_bwd":
        dy, pre = G.put(inp["dy"], "dy"), G.put(inp["pre"], "pre")
        o = run(lambda o: cabi("cxrk_gelu_bwd", P(dy), P(pre), rows, P(o["dx"])), {"dx": Out((rows,))}, False)
        rep.add(c, S.check(c, ref, {"dx": o["dx"].value()}))
    else:
        src = G.planes(inp["src"], "src")
        o = run(lambda o: K.planes_add_rows(src, o["dst"]), {"dst": Out((rows, H), ld=H + c.pad, init=inp["dst0"])}, False)
        rep.add(c, S.check(c, ref, {"dst": o["dst"].value()}))
    G.check()


@pytest.mark.parametrize("chunk", chunk_ids("E"))
def test_rows(chunk):
    rep = Report("rows " + chunk, mode=False)
    for c in chunk_cases("E", chunk):
        _rows(c, rep)
    rep.finish()


# ================================================================================================================ F: image-side kernels
def _maxpool(c, inp, ref, G, rep):
    N, H, W, C = c.N, c.H, c.W, c.C
    Ho, Wo = S.pool_out(H), S.pool_out(W)
    xd, dyd = G.put(inp["x"], "x"), G.put(inp["dy"], "dy")
    o = run(lambda o: cabi("cxrk_maxpool_fwd", P(xd), P(o["y"]), P(o["idx"]), N, H, W, C), {"y": Out((N, Ho, Wo, C)), "idx": Out((N, Ho, Wo, C), U8)}, False)
    idx = o["idx"].t
    got = {"y": o["y"].value(), "idx": idx.cpu()}
    o = run(lambda o: cabi("cxrk_maxpool_bwd", P(dyd), P(idx), P(xd), P(o["dx"]), N, H, W, C, int(c.relu == "mask")), {"dx": Out((N, H, W, C))}, False)
    got["dx"] = o["dx"].value()
    rep.add(c, S.check(c, ref, got))
    if C % 8:
        return
    xp, dyp = G.planes(inp["x"], "x planes"), G.planes(inp["dy"], "dy planes")
    o = run(lambda o: cabi("cxrk_maxpool_fwd_pl", xp.ptr(), xp.plane, P(o["y"]), o["y"].stride(0), P(o["idx"]), N, H, W, C),
            {"y": Out((2, N, Ho, Wo, C), BF), "idx": Out((N, Ho, Wo, C), U8)}, False)
    idx, pooled = o["idx"].t, K.Planes(o["y"].t)
    got = {"y": o["y"].value(), "idx": idx.cpu()}
    o = run(lambda o: cabi("cxrk_maxpool_bwd_pl", dyp.ptr(), dyp.plane, P(idx), pooled.ptr(), P(o["dx_pl"]), N, H, W, C), {"dx_pl": Out((N, H, W, C))}, False)
    got["dx_pl"] = o["dx_pl"].value()
    rep.add(c, S.check(c, ref, got), "[planes]")


def _bn_train(c, inp, ref, G, rep):
    rows, C = c.rows, c.C
    put = (lambda t, n: G.planes(t, n)) if c.planes else (lambda t, n: G.put(t, n))
    fmt = lambda t: (t.ptr(), t.plane) if isinstance(t, K.Planes) else (t.data_ptr(), 0)      # noqa: E731
    act = lambda: Out((2, rows, C), BF) if c.planes else Out((rows, C))      # noqa: E731
    vec = lambda init=None: Out((C,), init=init)      # noqa: E731
    zd, gam, bet = put(inp["z"], "z"), G.put(inp["gamma"], "gamma"), G.put(inp["beta"], "beta")
    st = run(lambda o: K.colstats(zd, out=(o["mean"], o["var"])), {"mean": vec(), "var": vec()}, True)
    mean, var = st["mean"].t, st["var"].t
    outs = {"scale": vec(), "shift": vec(), "rstd": vec()}
    if c.running:
        outs.update(rmean=vec(inp["rmean0"]), rvar=vec(inp["rvar0"]))
    co = run(lambda o: cabi("cxrk_bn_train_fwd_coeffs", P(mean), P(var), P(gam), P(bet), S.BN_EPS, rows, c.momentum, P(o["scale"]), P(o["shift"]),
                            P(o["rstd"]), P(o.get("rmean")), P(o.get("rvar")), C), outs, False)
    got = {k: g.value() for k, g in list(st.items()) + list(co.items())}
    if rows == 1:      # one value per channel: the statistics and the coefficients are all that is defined
        rep.add(c, S.check(c, ref, got))
        return
    res = None if c.residual == "none" else G.planes(inp["res"], "res") if c.residual == "pl" else G.put(inp["res"], "res")
    rp, rpl = fmt(res) if res is not None else (None, 0)
    outs = {"y": act()}
    if c.relu == "mask":
        outs["bits"] = Out((rows, C // 8), U8)
    zp, zpl = fmt(zd)
    ya = run(lambda o: cabi("cxrk_bn_apply", zp, zpl, P(co["scale"].t), P(co["shift"].t), rp, rpl, P(o["y"]), o["y"].stride(0) if c.planes else 0,
                            P(o.get("bits")), rows, C, int(c.relu != "none")), outs, False)
    got["y"] = ya["y"].value()
    bits = None
    if c.relu != "none":      # the decisions are those of the stored values, and the reference's wherever it is clear of zero by y's bound
        bits = got["y"] > 0
        if c.relu == "mask":
            assert torch.equal(S.unpack_bits(ya["bits"].t.cpu(), C), bits), f"{S.describe(c)}: decision bits differ from the stored output"
        clear = ref["aux:pre"].abs() > S.decision_threshold(c, ref, c.planes)
        assert torch.equal(bits[clear], (ref["aux:pre"] > 0)[clear]), f"{S.describe(c)}: a ReLU decision differs where the reference is clear of zero"
    back = S.bn_backward(c, inp, torch.float64, ref, bits)      # from the kernel's own decisions
    dyd = put(inp["dy"] * bits.float() if bits is not None else inp["dy"], "dy")
    dp, dpl = fmt(dyd)
    sm = run(lambda o: K.colsum(dyd, o["sumdy"]), {"sumdy": vec()}, True)
    dt = run(lambda o: K.coldot(dyd, zd, mean, out=o["dot"]), {"dot": vec()}, True)
    outs = {"A": vec(), "B": vec(), "Cc": vec(), "dgamma": vec(inp["dgamma0"] if c.accumulate else None), "dbeta": vec(inp["dbeta0"] if c.accumulate else None)}
    bc = run(lambda o: cabi("cxrk_bn_train_bwd_coeffs", P(gam), P(mean), P(co["rstd"].t), P(sm["sumdy"].t), P(dt["dot"].t), rows, P(o["A"]), P(o["B"]),
                            P(o["Cc"]), P(o["dgamma"]), P(o["dbeta"]), int(c.accumulate), C), outs, False)
    dz = run(lambda o: cabi("cxrk_bn_train_dz", dp, dpl, zp, zpl, P(bc["A"].t), P(bc["B"].t), P(bc["Cc"].t), P(o["dz"]), o["dz"].stride(0) if c.planes else 0,
                            rows, C), {"dz": act()}, False)
    got.update({k: g.value() for k, g in list(sm.items()) + list(dt.items()) + list(bc.items()) + list(dz.items())})
    rep.add(c, S.check(c, dict(ref, **back), got, planes_out=("y", "dz") if c.planes else ()))


def _image_side(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    if c.op == "maxpool":
        _maxpool(c, inp, ref, G, rep)
    elif c.op == "bn_train":
        _bn_train(c, inp, ref, G, rep)
    elif c.op == "layout":
        N, C, H, W = c.N, c.C, c.H, c.W
        xd, x2 = G.put(inp["x"], "x"), G.put(inp["x2"], "x2")
        o = run(lambda o: cabi("cxrk_nchw_to_nhwc", P(xd), P(o["nhwc"]), N, C, H, W, c.Cpad), {"nhwc": Out((N, H, W, c.Cpad))}, False)
        o2 = run(lambda o: cabi("cxrk_nhwc_to_nchw", P(x2), P(o["nchw"]), N, C, H, W), {"nchw": Out((N, C, H, W))}, False)
        rep.add(c, S.check(c, ref, {"nhwc": o["nhwc"].t.cpu(), "nchw": o2["nchw"].t.cpu()}))
    elif c.op == "spatial_mean":
        N, Pn, C = c.N, c.P, c.C
        xd, dyd = G.put(inp["x"], "x"), G.put(inp["dy"], "dy")
        o = run(lambda o: cabi("cxrk_spatial_mean_fwd", P(xd), P(o["y"]), N, Pn, C), {"y": Out((N, C))}, False)
        o2 = run(lambda o: cabi("cxrk_spatial_mean_bwd", P(dyd), P(o["dx"]), N, Pn, C), {"dx": Out((N, Pn, C))}, False)
        rep.add(c, S.check(c, ref, {"y": o["y"].value(), "dx": o2["dx"].value()}))
        if C % 8 == 0:
            add = G.put(inp["add"], "add") if c.add else None
            o = run(lambda o: cabi("cxrk_spatial_mean_bwd_pl", P(dyd), P(add), P(o["dx_pl"]), o["dx_pl"].stride(0), N, Pn, C),
                    {"dx_pl": Out((2, N, Pn, C), BF)}, False)
            rep.add(c, S.check(c, ref, {"dx_pl": o["dx_pl"].value()}, planes_out=("dx_pl",)), "[planes]")
    else:
        Ko, n = c.Ko, c.taps * c.Cpad
        w, gam, bet, rm, rv = (G.put(inp[k], k) for k in ("w", "gamma", "beta", "rmean", "rvar"))
        vecs = {"scale": Out((Ko,)), "shift": Out((Ko,)), "rstd": Out((Ko,))}
        o = run(lambda o: cabi("cxrk_bn_fold", P(w), P(gam), P(bet), P(rm), P(rv), S.BN_EPS, Ko, c.taps, c.C, c.Cpad, P(o["w_scaled"]), P(o["scale"]),
                               P(o["shift"]), P(o["rstd"])), dict(vecs, w_scaled=Out((Ko, n))), False)
        rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}))
        if c.Cpad % 8 == 0:
            o = run(lambda o: cabi("cxrk_bn_fold_pl", P(w), P(gam), P(bet), P(rm), P(rv), S.BN_EPS, Ko, c.taps, c.C, c.Cpad, P(o["w_scaled"]),
                                   o["w_scaled"].stride(0), P(o["scale"]), P(o["shift"]), P(o["rstd"])), dict(vecs, w_scaled=Out((2, Ko, n), BF)), False)
            rep.add(c, S.check(c, ref, {k: g.value() for k, g in o.items()}, planes_out=("w_scaled",)), "[planes]")
    G.check()


@pytest.mark.parametrize("chunk", chunk_ids("F"))
def test_image_side(chunk):
    rep = Report("image side " + chunk, mode=False)
    for c in chunk_cases("F", chunk):
        _image_side(c, rep)
    rep.finish()


# ================================================================================================================ G: masked-LM kernels
def _mlm_mask(c, inp, ref, G, rep):
    N, L, cap = c.N, c.L, int(inp["cap"])
    ids, mask = G.put(inp["ids"], "ids"), (G.put(inp["mask"], "mask") if c.given_mask else None)
    special = S.mask_special(c)
    sp = (ctypes.c_long * 8)(*(special + (-1,) * (8 - len(special))))
    outs = {"ids": Out((N, L), I64), "sel": Out((cap,), I32), "tgt": Out((cap,), I32), "stats": Out((2,), I32), "count": Out((1,)),
            "blocks": Out(((N * L + 255) // 256,), I32)}
    o = run(lambda o: cabi("cxrk_mlm_mask_tokens", P(ids), P(mask), N, L, c.row_offset, int(inp["seed"]), int(inp["counter"]) & 0xFFFFFFFF, c.p,
                           S.MLM_VOCAB, S.MLM_MASK_ID, ctypes.cast(sp, ctypes.c_void_p), len(special), cap,
                           *(P(o[k]) for k in ("ids", "sel", "tgt", "stats", "count", "blocks"))), outs, False)
    rep.add(c, S.check(c, ref, {k: g.t.cpu() for k, g in o.items()}))


def _mlm_rows(c, inp, ref, G, rep):
    cap, H = c.cap, c.H
    sel, stats = G.put(inp["sel"], "sel"), G.put(inp["stats"], "stats")
    if c.op == "gather":
        last = G.put(inp["last"], "last")
        T = last.shape[0]
        spec = {"out": Out((2, cap, H), BF, gap=c.gap) if c.planes else Out((cap, H))}
        o = run(lambda o: cabi("cxrk_mlm_gather_rows", P(last), T, H, P(sel), P(stats), cap, P(o["out"]), o["out"].stride(0) if c.planes else 0), spec, False)
        rep.add(c, S.check(c, ref, {"out": o["out"].t.cpu()}), "->planes" if c.planes else "")      # the planes: bit for bit the canonical split
    else:
        dx, T = G.put(inp["dx"], "dx"), int(inp["T"])
        o = run(lambda o: cabi("cxrk_mlm_scatter_rows", P(dx), P(sel), P(stats), cap, T, H, P(o["dlast"])), {"dlast": Out((T, H), init=torch.zeros(T, H))}, False)
        rep.add(c, S.check(c, ref, {"dlast": o["dlast"].t.cpu()}))


def _mlm_xent(c, inp, ref, G, rep):
    """one vocabulary sweep at kernel level: stats chunk by chunk through one shared workspace, finish, then the gradient of every chunk
    from the float32 rounding of the reference's log-sum-exp, in place and as planes"""
    rows, V = c.cap, c.V
    chunks = S.xent_chunks(V, c.width)
    width = max(n for _, n, _ in chunks)
    ld = width + c.pad
    bias, tgt, stats, scale, up, lse_in = (G.put(inp[k], k) for k in ("bias", "tgt", "stats", "scale", "upstream", "lse_in"))
    logits = inp["S"].to(DEV)
    spec = {"state": Out((4, rows, 64), written=False), "tl": Out((rows,), written=False), "lse": Out((rows,)), "rowloss": Out((rows,)),
            "hit": Out((rows,), I32), "loss": Out(()), "correct": Out((1,), I32)}
    # the workspace of _MLMLoss (ws[:, :cols] of one block for every chunk); then with ld % 4 != 0 and from a base 4 bytes off a
    # 16-byte boundary: the column-by-column kernel takes every chunk, not only the tail
    for form, ldw, off in (("", ld, 0), ("[ld % 4]", ld + 1, 0), ("[base + 4]", ld, 1)):
        if off:
            ws = MG.Guarded(((rows - 1) * ldw + width + off,), device=DEV, name="logits workspace " + form)
            block = ws.t[off:].as_strided((rows, width), (ldw, 1))
        else:
            ws = MG.Guarded((rows, width), ld=ldw, device=DEV, name="logits workspace " + form)
            block = ws.t
        ws.must_write = False

        def sweep(o):
            for k, (v0, n, skip) in enumerate(chunks):
                block[:, :n].copy_(logits[:, v0:v0 + n])
                cabi("cxrk_mlm_xent_stats", P(block), ldw, rows, n, skip, v0, P(bias), P(tgt), P(stats), P(o["state"]), P(o["tl"]), int(k == 0))
            cabi("cxrk_mlm_xent_finish", P(o["state"]), P(o["tl"]), P(tgt), P(stats), rows, P(scale), P(o["lse"]), P(o["rowloss"]), P(o["hit"]),
                 P(o["loss"]), P(o["correct"]))

        o = run(sweep, spec, False)
        ws.check()
        got = {k: o[k].value() for k in ("lse", "rowloss", "loss")}
        got.update(hit=o["hit"].t.cpu(), correct=o["correct"].t.cpu())
        rep.add(c, S.check(c, ref, got), form)
    alpha = float(torch.tensor(c.alpha, dtype=torch.float32))
    ldg = (ld + 7) // 8 * 8 + 8
    for form in ("", "->planes"):
        grad, skipped = torch.zeros(rows, V, dtype=torch.float64), []
        for v0, n, skip in chunks:
            if form:
                src = G.put(inp["S"][:, v0:v0 + n], "logits", ld)
                o = run(lambda o: cabi("cxrk_mlm_xent_grad", P(src), ld, P(o["g"]), ldg, o["g"].stride(0), rows, n, skip, v0, P(bias), P(tgt), P(stats),
                                       P(lse_in), P(up), P(scale), alpha), {"g": Out((2, rows, n), BF, ld=ldg, gap=8)}, False)
            else:
                o = run(lambda o: cabi("cxrk_mlm_xent_grad", P(o["g"]), ld, None, 0, 0, rows, n, skip, v0, P(bias), P(tgt), P(stats), P(lse_in), P(up),
                                       P(scale), alpha), {"g": Out((rows, n), ld=ld, init=inp["S"][:, v0:v0 + n])}, False)
            g = o["g"].value()
            grad[:, v0 + skip:v0 + n] = g[:, skip:]
            skipped.append(g[:, :skip])
        rep.add(c, S.check(c, ref, {"grad": grad, "grad_skip": skipped[-1]}, planes_out=("grad",) if form else ()), form)


def _mlm_head(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    names = ("wd", "bd", "gamma", "beta", "wdec", "bdec")
    last, params = G.put(inp["last"], "last"), [G.put(inp[k], k) for k in names]
    sel, tgt, stats, scale, up = (G.put(inp[k], k) for k in ("sel", "tgt", "stats", "scale", "upstream"))
    T, H, V = last.shape[0], c.H, c.V
    assert Fh.mlm_vocab_chunks(V, c.cap, S.head_chunk_bytes(c, _split()), _split()) == S.xent_chunks(V, c.width)
    spec = {"loss": Out(()), "correct": Out((1,), I32), "dlast": Out((T, H)), "dwd": Out((H, H)), "dbd": Out((H,)), "dgamma": Out((H,)),
            "dbeta": Out((H,)), "dwdec": Out((V, H)), "dbdec": Out((V,))}

    def call(o):      # autograd allocates its results: copied into the guarded outputs, whose three runs must agree bit for bit
        x = last.detach().requires_grad_(True)
        leaves = [p.detach().requires_grad_(True) for p in params]
        weighted, loss, correct = Fh._mlm_triple(x, sel, tgt, stats, leaves, scale, S.head_chunk_bytes(c, _split()), c.alpha)
        (weighted * up[0]).backward()
        o["loss"].copy_(loss)
        o["correct"].copy_(correct)
        o["dlast"].copy_(x.grad)
        for k, p in zip(names, leaves):
            o["d" + k].copy_(p.grad)

    o = run(call, spec, True)
    got = {k: g.value() for k, g in o.items() if k != "correct"}
    got["correct"] = o["correct"].t.cpu()
    rep.add(c, S.check(c, ref, got, _split()))
    G.check()


def _mlm(c, rep):
    inp = S.build(c)
    ref = S.reference(c, inp)
    G = Inputs()
    {"mask_tokens": _mlm_mask, "gather": _mlm_rows, "scatter": _mlm_rows, "xent": _mlm_xent}[c.op](c, inp, ref, G, rep)
    G.check()


@pytest.mark.parametrize("chunk", chunk_ids("G"))
def test_mlm(chunk):
    """mask, gather, scatter and the cross-entropy kernels take their storage form from their arguments: once (the head cases that fall
    into the chunk run in test_mlm_head)"""
    rep = Report("mlm " + chunk, mode=False)
    for c in chunk_cases("G", chunk):
        if c.op != "head":
            _mlm(c, rep)
    rep.finish()


@both_precisions
def test_mlm_head():
    rep = Report("mlm head")
    for c in [c for f, c in REGRESSIONS if f == "G"] + S.cases("G"):
        if c.op == "head":
            _mlm_head(c, rep)
    rep.finish()


# ================================================================================================================ grid-stride wraps
WRAP_ROWS, WRAP_C = 32768 + 8, 1024      # 8 * 256 * BN_GRID_CAP = 33 554 432 elements fill the capped grid once; 8192 lie past it


def _pattern(n, mul, mod, dev):
    """((i * mul) % mod - mod / 2) / 64 for i < n: exact in float32 on either device"""
    i = torch.arange(n, dtype=torch.int64, device=dev)
    return ((i * mul) % mod - mod // 2).float() / 64.0


@pytest.mark.parametrize("op", ("bn_apply", "bn_train_dz"))
def test_grid_stride_wrap(op):
    """bn_apply and bn_train_dz cap their grids at 16384 blocks (csrc/bn_train.hip grid_for): one fp32 tensor just past
    8 * 256 * 16384 elements, a strided sample and the whole second pass against float64.  The bounds are the roundings of the
    kernels' own forms: fma(z, scale, shift) rounds once (2 * 2^-24 on |z scale| + |shift|, twice what it needs);
    fma(A, dy, fma(Cc, z, B)) twice (3 * 2^-24 on the three magnitudes)."""
    rows, C = WRAP_ROWS, WRAP_C
    n = rows * C
    assert n > 8 * 256 * S.BN_GRID_CAP
    pick = torch.cat([torch.arange(0, 8 * 256 * S.BN_GRID_CAP, 997), torch.arange(8 * 256 * S.BN_GRID_CAP, n)])
    cols = pick % C
    vec = lambda k: _pattern(C, 29 + 2 * k, 257, "cpu") + 0.015625 * (k + 1)      # noqa: E731
    G = Inputs()
    z = MG.Guarded((rows, C), device=DEV, name="z")
    z.t.view(-1).copy_(_pattern(n, 37, 1021, DEV))
    z.must_write = False
    zs = _pattern(n, 37, 1021, "cpu")[pick].double()
    out = MG.Guarded((rows, C), device=DEV, name=op)
    if op == "bn_apply":
        sc, sh = vec(0), vec(1)
        cabi("cxrk_bn_apply", z.data_ptr(), 0, P(G.put(sc, "scale")), P(G.put(sh, "shift")), None, 0, out.data_ptr(), 0, None, rows, C, 1)
        a, b = zs * sc.double()[cols], sh.double()[cols]
        ref, mag, cst = torch.relu(a + b), a.abs() + b.abs(), 2.0
    else:
        dy = MG.Guarded((rows, C), device=DEV, name="dy")
        dy.t.view(-1).copy_(_pattern(n, 53, 509, DEV))
        dy.must_write = False
        A, B, Cc = vec(0), vec(1), vec(2)
        cabi("cxrk_bn_train_dz", dy.data_ptr(), 0, z.data_ptr(), 0, P(G.put(A, "A")), P(G.put(B, "B")), P(G.put(Cc, "Cc")), out.data_ptr(), 0, rows, C)
        ds = _pattern(n, 53, 509, "cpu")[pick].double()
        t = [A.double()[cols] * ds, Cc.double()[cols] * zs, B.double()[cols]]
        ref, mag, cst = t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs(), 3.0
        dy.check()
    torch.cuda.synchronize()
    out.check()
    z.check()
    G.check()
    got = out.t.view(-1)[pick.to(DEV)].cpu()
    ratio, at = S.forward_bound(got, ref, mag, cst * S.U24)
    print(f"{op} wrap: worst error / bound {ratio:.3g} over {pick.numel()} elements, {n - 8 * 256 * S.BN_GRID_CAP} past the cap")
    assert ratio <= 1.0, f"{op}: {ratio:.3g} x bound at flat index {int(pick[at[0]])}"


# ================================================================================================================ H: convolutions
import os  # noqa: E402

import sweep_conv_cases as HC  # noqa: E402
from test_conv_geometry_gpu import plane_gap  # noqa: E402


@pytest.fixture
def window_wgrad_switch():
    """CXRK_HALO_WGRAD, read by the library on every call (as tests/test_exact_planes_gpu.py switches it)"""
    old = os.environ.get("CXRK_HALO_WGRAD")

    def set_(v):
        if v is None:
            os.environ.pop("CXRK_HALO_WGRAD", None)
        else:
            os.environ["CXRK_HALO_WGRAD"] = v
    yield set_
    set_(old)


def _launched(c, pred, what=""):
    """the Python restatement of the dispatch (sweep_conv_cases.predict) against what the library says it launched"""
    lib = _cxr_lib.load()
    got = (lib.cxrk_last_launch_label().decode(), lib.cxrk_last_launch_count(), lib.cxrk_last_launch_split_bf16())
    want = (pred["label"], pred["count"], pred["split_bf16"])
    assert got == want, f"{S.describe(c)}{what}: launched {got}, predicted {want}"


def _zero_bits(g, sel):
    """every bit of the selected pixels of a guarded [.., N, H, W, C] output is zero"""
    b = g.bits()
    b = b[(slice(None),) + sel] if g.dtype == BF else b[sel]
    return not bool(b.any())


def _conv(c, rep, wide=False, switch=None):
    inp = S.build(c)
    ref = S.reference(c, inp)
    pred = HC.predict(c, wide)
    pl = c.family == "HPL"
    N, H, W, C, Cp, Ko, R, Sf, st, pad = c.N, c.H, c.W, c.C, c.Cpad, c.Ko, c.R, c.S, c.stride, c.pad
    Ho, Wo = c.out_hw
    geo = (N, H, W, Cp, Ko, R, Sf, st, pad)
    G = Inputs()
    planes = lambda t, n: G.planes(t, n, gap=plane_gap(t.shape))      # noqa: E731
    put = planes if pl else G.put
    form = f" [{c.op}:{pred['path']}]"
    if c.op == "fwd":
        x, w = put(inp["x"], "x"), put(inp["w"].reshape(Ko, -1) if pl else inp["w"], "w_scaled")
        shift = G.put(inp["shift"], "shift") if c.shift else None
        res = None if c.residual == "none" else G.put(inp["residual"], "residual") if c.form == "f32" else planes(inp["residual"], "residual")
        if c.form == "f32":
            o = run(lambda o: K.conv_fwd(x, w, shift, res, o["y"], *geo, c.relu), {"y": Out((N, Ho, Wo, Ko))}, False)
        else:
            spec = {"y": Out((2, N, Ho, Wo, Ko), BF)}
            if c.bits:
                spec["bits"] = Out((N * Ho * Wo, Ko // 8), U8)
            o = run(lambda o: K.conv_fwd_pl(x, w, shift, res, K.Planes(o["y"]), o.get("bits"), *geo, c.relu), spec, False)
        _launched(c, pred)
        got = {"y": o["y"].value()}
        if c.bits:      # the decisions of the values this launch stored
            assert torch.equal(S.unpack_bits(o["bits"].t.cpu(), Ko), got["y"].reshape(-1, Ko) > 0), f"{S.describe(c)}: decision bits differ from the stored output"
    elif c.op == "dgrad":
        dy, w = put(inp["dy"], "dy"), put(inp["w"].reshape(Ko, -1) if pl else inp["w"], "w_scaled")
        res = put(inp["residual"], "residual") if c.residual != "none" else None
        side = G.put(inp["maskin" if pl else "relu_src"], "mask") if c.mask else None
        dx = Out((2, N, H, W, Cp), BF) if pl else Out((N, H, W, Cp))

        def call(o):
            if pl:
                K.conv_bwd_data_pl(dy, w, res, side, K.Planes(o["dx"]), *geo, sums=o.get("sums"), residual_s2=c.residual == "compact")
            else:
                K.conv_bwd_data(dy, w, res, side, o["dx"], *geo, sums=o.get("sums"))

        o = run(call, {"dx": dx, "sums": Out((Cp,))} if c.sums else {"dx": dx}, c.sums)
        _launched(c, pred)
        got = {k: g.value() for k, g in o.items()}
        if c.sums:      # the fused column sums leave dx alone
            o2 = run(call, {"dx": dx}, False)
            _launched(c, pred, " without sums")
            assert torch.equal(o["dx"].bits(), o2["dx"].bits()), f"{S.describe(c)}: dx with sums differs from dx without"
        keep = HC.dgrad_mask(c, inp)
        if keep is not None:
            assert not bool(got["dx"][~keep].any()), f"{S.describe(c)}: a masked element of dx is not zero"
        if st == 2:     # the pixels of a class that no tap reaches: zero in every bit
            for ph, pw, _, _, tr, ts in HC.s2_classes(c):
                if not (tr and ts):
                    sel = (slice(None), slice(ph, None, 2), slice(pw, None, 2))
                    assert _zero_bits(o["dx"], sel), f"{S.describe(c)}: class ({ph}, {pw}) has no tap and is not zero"
    else:
        x, dy = put(inp["x"], "x"), put(inp["dy"], "dy")
        wraw = G.put(inp["w"], "w")
        scale = G.put(inp["scale"], "scale") if c.bn != "noscale" else None
        rstd, rmean, sumdy = (G.put(inp[k], k) for k in ("rstd", "rmean", "sumdy"))
        spec = {"dw": Out((Ko, R, Sf, C), init=inp.get("dw0"))}
        if c.bn != "none":
            spec.update(dgamma=Out((Ko,), init=inp.get("dgamma0")), dbeta=Out((Ko,), init=inp.get("dbeta0")))

        def call(o):
            if pl:
                K.conv_bwd_params_pl(x, dy, wraw, scale, rstd, rmean, sumdy, o["dw"], o.get("dgamma"), o.get("dbeta"), c.accumulate, N, H, W, C, Ko,
                                     R, Sf, st, pad)
            else:
                K.conv_bwd_params(x, dy, wraw, scale, rstd, rmean, sumdy, o["dw"], o.get("dgamma"), o.get("dbeta"), c.accumulate, N, H, W, C, Cp,
                                  Ko, R, Sf, st, pad)

        o = run(call, spec, True)
        _launched(c, pred)
        sk = _cxr_lib.load().cxrk_gemm_wgrad_splitk(Ko, R * Sf * Cp, N * Ho * Wo, int(pl))
        assert sk == pred["splitk"], f"{S.describe(c)}: the library splits K by {sk}, the restated policy by {pred['splitk']}"
        got = {k: g.value() for k, g in o.items()}
        if pred["path"] == "window":      # include/cxrk.h: the implicit GEMM's slabs, bit-identical result
            switch("0")
            try:
                o2 = run(call, spec, True)
                _launched(c, HC.predict(c, wide, window_wgrad=False), " with CXRK_HALO_WGRAD=0")
            finally:
                switch(None)
            for k in spec:
                assert torch.equal(o[k].bits(), o2[k].bits()), f"{S.describe(c)}: {k} of the window kernel differs from the implicit GEMM's"
    rep.add(c, S.check(c, ref, got, _split()), form)
    G.check()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("H32"))
def test_conv_f32(chunk):
    rep = Report("conv fp32 " + chunk)
    for c in chunk_cases("H32", chunk):
        _conv(c, rep)
    rep.finish()


@both_precisions
@pytest.mark.parametrize("chunk", chunk_ids("HPL"))
def test_conv_planes(chunk, wide, window_wgrad_switch):
    rep = Report(f"conv planes {chunk} [{wide}]")
    for c in chunk_cases("HPL", chunk):
        _conv(c, rep, wide == "wide", window_wgrad_switch)
    rep.finish()
