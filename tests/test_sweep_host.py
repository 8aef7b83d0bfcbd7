"""The differential sweep without a GPU: the generators of tests/sweep_cases.py are deterministic, legal and cover their strata and the
kernels' dispatch thresholds; the float64 references agree with independent formulations; the table E32 is what this machine
measures; and -- as tests/test_memguard_host.py does for the memory contract -- deliberately wrong CPU "kernels" run through the
same comparators and bounds as the GPU tests: each is caught on at least one generated case, the correct float32 evaluation passes
on every case."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_cases as S  # noqa: E402

F32, F64 = torch.float32, torch.float64
FAMILIES = tuple(S.NCASES)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- generators
@pytest.mark.parametrize("family", FAMILIES)
def test_generators_are_deterministic_and_legal(family):
    first = list(S.cases(family))
    S._CACHE.clear()
    again = S.cases(family)
    assert first == again and len(first) == S.NCASES[family] and 96 <= len(first) <= 128
    assert [c.index for c in first] == list(range(len(first)))
    bad = [c for c in first if not S.legal(c)]
    assert not bad, f"illegal under include/cxrk.h: {bad[:3]}"
    for c in first[::3]:
        a, b = S.build(c), S.build(c)
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a), S.describe(c)
        biggest = max(t.numel() * t.element_size() for t in a.values())
        assert biggest < (64 << 20), S.describe(c)


def _dims(family):
    """dimension -> (strata, value of a case)"""
    if family == "A":
        return {"L": (S.A_L, lambda c: c.L), "dH": (S.A_DH, lambda c: c.dH), "nH": (S.A_NH, lambda c: c.nH), "B": (S.A_B, lambda c: c.B),
                "mask": (S.A_MASKS, lambda c: c.mask), "profile": (S.A_PROFILES, lambda c: c.profile)}
    if family in ("B32", "BPL"):
        d = {"M": (S.B_MN, lambda c: c.M), "N": (S.B_MN, lambda c: c.N), "K": (S.B_K, lambda c: c.K), "form": (S.B_FORMS[family], lambda c: c.form),
             "epi": (S.B_EPI[family], lambda c: c.epi), "alpha": (S.ALPHAS, lambda c: c.alpha), "profile": (S.B_PROFILES, lambda c: c.profile),
             "splitk": ((1, 2, 3, 7), lambda c: c.splitk), "act": ((0, 1, 2), lambda c: c.act),
             "auxmode": ((0, 2, 3) if family == "BPL" else (0, 1, 2), lambda c: c.auxmode)}
        for k in ("pad_a", "pad_b", "pad_c", "pad_r", "pad_aux", "pad_c2") + (("gap_a", "gap_b", "gap_c", "gap_r") if family == "BPL" else ()):
            d[k] = (S.PADS, lambda c, k=k: getattr(c, k))
        return d
    if family == "C":
        return {"rows": (S.C_ROWS, lambda c: c.rows), "C": (S.C_COLS, lambda c: c.C), "op": (S.C_OPS, lambda c: c.op),
                "planes": ((False, True), lambda c: c.planes), "profile": (S.C_PROFILES, lambda c: c.profile)}
    return {}


@pytest.mark.parametrize("family", ("A", "B32", "BPL", "C"))
def test_first_cases_hit_every_stratum(family):
    dims = _dims(family)
    scheduled = {k: v for k, v in dims.items() if k not in ("splitk", "act", "auxmode")}      # those three are drawn inside `epi`
    first = S.cases(family)[:max(len(s) for s, _ in scheduled.values())]
    for name, (strata, get) in scheduled.items():
        missing = set(strata) - {get(c) for c in first}
        assert not missing, f"{family}.{name}: strata {sorted(missing, key=str)} not among the first {len(first)} cases"
    for name, (strata, get) in dims.items():
        assert set(strata) <= {get(c) for c in S.cases(family)}, f"{family}.{name}"


def test_head_strata_are_hit():
    by = {}
    for c in S.cases("D"):
        by.setdefault(c.op, []).append(c)
    assert {op: len(v) for op, v in by.items()} == dict(S.D_COUNTS)
    has = lambda op, f, strata: set(strata) <= {f(c) for c in by[op]}      # noqa: E731
    assert has("l2norm", lambda c: c.cols, S.D_L2_D) and has("l2norm", lambda c: c.rows, S.D_L2_ROWS)
    assert {c.pad == 0 for c in by["l2norm"]} == {True, False}
    assert has("infonce", lambda c: c.cols, S.D_NCE_COLS) and has("infonce", lambda c: c.rows, S.D_NCE_ROWS)
    assert has("infonce", lambda c: c.profile, ("base", "sharp")) and has("infonce", lambda c: c.pad, S.PADS)
    wide = [c for c in by["infonce"] if c.cols - c.rows >= 2]
    assert any(c.diag_off == 0 for c in wide) and any(c.diag_off == c.cols - c.rows for c in wide)
    assert any(0 < c.diag_off < c.cols - c.rows for c in wide)
    assert has("cosine", lambda c: c.rows, S.D_COS_B) and has("cosine", lambda c: c.cols, S.D_COS_D) and has("cosine", lambda c: c.n, S.D_COS_P)
    for f in (lambda c: c.flag_a, lambda c: c.flag_b, lambda c: c.groups > 0):
        assert {f(c) for c in by["cosine"]} == {True, False}
    assert has("bce", lambda c: c.rows * c.cols, S.D_BCE_N) and all(c.pad > 0 for c in by["bce"])
    for f in (lambda c: c.flag_a, lambda c: c.flag_b):
        assert {f(c) for c in by["bce"]} == {True, False}
    assert has("group_mean", lambda c: c.rows, S.D_GM_G) and has("group_mean", lambda c: c.n, S.D_GM_N) and has("group_mean", lambda c: c.cols, S.D_GM_D)


def test_dispatch_coverage():
    """conditions on the generated lists: every kernel and tile form the library chooses between is reached"""
    A = S.cases("A")
    assert any(c.L <= 64 for c in A) and any(c.L > 64 for c in A)
    assert {c.mask for c in A if c.L > 128} == set(S.A_MASKS)
    # a live row of the tiled kernels with a fully masked 64-key tile, a sequence with a single key, left padding, the outlier profile
    masks = {c.index: S.attention_mask(c) for c in A}
    def dead_tile(c):      # noqa: E306
        m = masks[c.index]
        return any(bool(m[b].any()) and any(not bool(m[b, t:t + 64].any()) for t in range(0, c.L - 63, 64)) for b in range(c.B))
    assert sum(dead_tile(c) for c in A if c.L > 64) >= 5
    assert any(int(masks[c.index][b].sum()) == 1 for c in A if c.L > 64 for b in range(c.B))
    assert any(int(masks[c.index][b, 0]) == 0 and bool(masks[c.index][b].any()) for c in A for b in range(c.B))
    for c in A:
        if c.mask == "empty":
            live = masks[c.index].any(1)
            assert (~live).sum() == 1 and live.sum() >= 1, S.describe(c)
    P = S.cases("BPL")
    assert any(c.N <= 64 for c in P) and any(c.M <= 64 and c.N > 64 for c in P) and any(c.M > 64 and c.N > 64 for c in P)
    for fam in ("B32", "BPL"):
        cs = S.cases(fam)
        for form in S.B_FORMS[fam]:
            assert any(c.form == form and c.splitk == 1 for c in cs) and any(c.form == form and c.splitk > 1 for c in cs), (fam, form)
        for pad in ("pad_a", "pad_b", "pad_c"):
            assert any(getattr(c, pad) == 0 for c in cs) and any(getattr(c, pad) > 0 for c in cs)
        assert any(c.K < 32 for c in cs) and any(c.K % 32 for c in cs if c.K > 32)
    assert any(c.residual == "pl" and c.pad_r for c in P) and any(c.residual == "f32" and c.pad_r == 0 for c in P)
    assert any(c.out_planes for c in P) and any(c.maskout for c in P) and {c.colsum for c in P} == {"none", "fresh", "acc"}
    assert any(c.form == "TT" for c in S.cases("B32"))
    D = [c for c in S.cases("D") if c.op == "cosine"]
    assert any(S.cosine_chunks(c) > 1 and c.flag_b for c in D) and any(S.cosine_chunks(c) > 1 and c.groups for c in D)
    assert any(c.rows * c.cols > 65536 for c in S.cases("D") if c.op == "bce")
    Cc = S.cases("C")
    assert {c.op for c in Cc if c.planes} == set(S.C_OPS) == {c.op for c in Cc if not c.planes}
    assert any(c.op == "colsum" and c.accumulate for c in Cc) and any(c.op == "colsum" and c.planes and c.pad for c in Cc)


# ---------------------------------------------------------------------------------------------------------------- references
def _pick(family, pred, n=3):
    out = [c for c in S.cases(family) if pred(c)][:n]
    assert out
    return out


def test_attention_reference_against_explicit_loop():
    for c in _pick("A", lambda c: c.L <= 33 and c.mask != "ones", 4) + _pick("A", lambda c: c.mask == "empty" and c.L <= 65, 1):
        inp = S.build(c)
        ref = S.reference(c, inp)
        qkv, mask = inp["qkv"].double().view(c.B, c.L, 3, c.nH, c.dH), inp["mask"]
        for b in range(c.B):
            live = mask[b].nonzero().flatten().tolist() or list(range(c.L))       # no key at all: uniform over all L
            for h in range(c.nH):
                for i in range(c.L):
                    sc = [float(qkv[b, i, 0, h] @ qkv[b, j, 1, h]) / math.sqrt(c.dH) if mask[b].any() else 0.0 for j in live]
                    mx = max(sc)
                    w = [math.exp(v - mx) for v in sc]
                    tot = sum(w)
                    row = torch.zeros(c.L, dtype=F64)
                    row[live] = torch.tensor([v / tot for v in w], dtype=F64)
                    assert float((ref["probs"][b, h, i] - row).abs().max()) < 1e-12, S.describe(c)
                    ctx = sum(row[j] * qkv[b, j, 2, h] for j in live)
                    assert float((ref["ctx"][b * c.L + i, h * c.dH:(h + 1) * c.dH] - ctx).abs().max()) < 1e-12
        # the backward from given probabilities (what the GPU test's kernel reads) is the autograd gradient
        assert S.row_scaled(S.attn_backward(c, inp, ref["probs"]), ref["dqkv"])[0] < 1e-12, S.describe(c)


def test_attention_reference_is_hf_on_today_s_masks():
    """on a suffix mask the live-key softmax is HuggingFace's additive finfo.min form (tests/kernel_refs.py), the empty sequence included"""
    c = next(c for c in S.cases("A") if c.mask == "empty" and c.L <= 129)
    inp = S.build(c)
    x = inp["qkv"].clone().requires_grad_(True)
    q, k, v = x.view(c.B, c.L, 3, c.nH, c.dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(c.dH) + (1.0 - inp["mask"][:, None, None, :].float()) * torch.finfo(F32).min
    ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(c.B * c.L, -1)
    ctx.backward(inp["dctx"])
    ref = S.reference(c, inp)
    assert S.row_scaled(ctx, ref["ctx"])[0] < 1e-5 and S.row_scaled(x.grad, ref["dqkv"])[0] < 1e-4


@pytest.mark.parametrize("family", ("B32", "BPL"))
def test_gemm_reference_against_einsum(family):
    for c in _pick(family, lambda c: c.epi == "plain", 2) + _pick(family, lambda c: c.bias and c.residual != "none", 2):
        inp = S.build(c)
        ref = S.reference(c, inp)
        a, b = inp["a"], inp["b"]
        if family == "BPL":      # the three plane terms sum to the product of the merged values minus a_lo b_lo
            (ah, al), (bh, bl) = S.canonical_planes(a), S.canonical_planes(b)
            ea, eb = ("km" if c.ta else "mk"), ("nk" if c.tb else "kn")
            full = torch.einsum(f"{ea},{eb}->mn", ah.double() + al.double(), bh.double() + bl.double())
            acc = full - torch.einsum(f"{ea},{eb}->mn", al.double(), bl.double())
        else:
            acc = torch.einsum(f"{'km' if c.ta else 'mk'},{'nk' if c.tb else 'kn'}->mn", a.double(), b.double())
        exp = c.alpha * acc
        if c.bias:
            exp = exp + inp["bias"].double()
        if c.residual == "f32":
            exp = exp + inp["residual"].double()
        elif c.residual == "pl":
            hi, lo = S.canonical_planes(inp["residual"])
            exp = exp + hi.double() + lo.double()
        pre = ref["preact"] if c.preact else None
        if c.act == 0 and c.auxmode == 0:
            assert float(((ref["out"] - exp).abs() / ref["mag:out"].clamp_min(1e-300)).max()) < 1e-13, S.describe(c)
        elif pre is not None:
            assert float(((pre - exp).abs() / ref["mag:pre"].clamp_min(1e-300)).max()) < 1e-13, S.describe(c)
    c = _pick(family, lambda c: c.act == S.ACT_GELU, 1)[0]
    x = torch.linspace(-6, 6, 97, dtype=F64).requires_grad_(True)
    F.gelu(x).sum().backward()
    assert float((S._gelu(x.detach()) - F.gelu(x.detach())).abs().max()) < 1e-14 and float((S._gelu_grad(x.detach()) - x.grad).abs().max()) < 1e-14


def test_column_references_against_torch():
    for c in _pick("C", lambda c: c.op.startswith("colstats") and 1 < c.rows <= 4097, 4):
        inp = S.build(c)
        ref = S.reference(c, inp)
        x = S._seen(None, inp["x"], c.planes, F64)
        assert float((ref["mean"] - x.mean(0)).abs().max()) < 1e-10
        assert S.col_scaled(ref["var"], torch.var(x, 0, unbiased=c.op == "colstats_unbiased"))[0] < 1e-12, S.describe(c)
    for c in _pick("C", lambda c: c.op in ("colsum", "colvar", "coldot_shift"), 6):
        inp = S.build(c)
        out = S.reference(c, inp)["out"]
        x = S._seen(None, inp["x"], c.planes, F64)
        if c.op == "colsum":
            exp = c.alpha * torch.einsum("rc->c", x) + (inp["out0"].double() if c.accumulate else 0)
        elif c.op == "colvar":
            exp = c.alpha * c.rows * ((x * x).mean(0) - 2 * inp["mean"].double() * x.mean(0) + inp["mean"].double() ** 2)
        else:
            a = S._seen(None, inp["a"], c.planes, F64)
            exp = torch.einsum("rc,rc->c", a, x) - inp["bshift"].double() * a.sum(0)
        assert S.col_scaled(out, exp)[0] < 1e-8, S.describe(c)


def test_cosine_references_against_the_oracle():
    from oracle import ref_loss
    for c in _pick("D", lambda c: c.op == "cosine" and c.rows <= 65, 6):
        inp = S.build(c)
        ref = S.reference(c, inp)
        x, y = inp["x"].double().requires_grad_(True), inp["y"].double().requires_grad_(True)
        cos = ref_loss.pairwise_cosine_similarity(x, y)
        assert float((cos - ref["cos"]).abs().max()) < 1e-13
        if c.groups:
            mx, mean, idx = ref_loss.pairwise_cosine_max(x, y, c.groups)
            assert float((mx - ref["max"]).abs().max()) < 1e-13 and float((mean - ref["mean"]).abs().max()) < 1e-13
            assert torch.equal(idx.to(torch.int32), inp["arg"])
            (mx * inp["dcos"].double()).sum().backward()
        else:
            (cos * inp["dcos"].double()).sum().backward()
        # the reference differentiates at the saved float32 cos / norms the kernel reads: equal to autograd up to their rounding
        dy = ref["dy"] - (inp["dy0"].double() if c.flag_a else 0)
        assert S.row_scaled(dy, y.grad)[0] < 1e-6, S.describe(c)
        if c.flag_b:
            assert S.row_scaled(ref["dx"], x.grad)[0] < 1e-6, S.describe(c)


def test_head_references_against_torch():
    for c in _pick("D", lambda c: c.op == "l2norm", 3):
        inp = S.build(c)
        ref = S.reference(c, inp)
        x = inp["x"].double().requires_grad_(True)
        F.normalize(x, dim=1).backward(inp["dxhat"].double())
        assert float((ref["xhat"] - F.normalize(x.detach(), dim=1)).abs().max()) < 1e-14 and S.row_scaled(ref["dx"], x.grad)[0] < 1e-6
    for c in _pick("D", lambda c: c.op == "infonce" and c.diag_off == 0 and c.rows == c.cols or c.op == "infonce" and c.rows > 1, 3):
        inp = S.build(c)
        ref = S.reference(c, inp)
        s = inp["S"].double().requires_grad_(True)
        tgt = c.diag_off + torch.arange(c.rows)
        ce = F.cross_entropy(s, tgt, reduction="sum")
        assert abs(float(ref["loss"]) - float(inp["loss0"] if c.flag_a else 0) - 0.5 / c.rows * float(ce)) < 1e-9
    for c in _pick("D", lambda c: c.op == "bce", 4):
        inp = S.build(c)
        ref = S.reference(c, inp)
        cos = inp["cos"].double().requires_grad_(True)
        z = cos[:, 0::2] - cos[:, 1::2] if c.flag_a else cos[:, 0::2]
        loss = F.binary_cross_entropy_with_logits(z, inp["labels"][:, :c.cols].double())
        loss.backward()
        assert abs(float(loss) - float(ref["loss"])) < 1e-12 and float((cos.grad - ref["dcos"]).abs().max()) < 1e-15


# ---------------------------------------------------------------------------------------------------------------- E32
def test_e32_table():
    """every entry of E32 is at least what this machine measures and at most twice that: it can neither go stale nor be padded"""
    measured = {}
    for family in ("A", "C", "D"):
        measured.update(S.measure_e32(family))
    print("\n".join(f"{k}: measured {v:.3g}, table {S.E32.get(k)}" for k, v in sorted(measured.items())))
    assert set(measured) == set(S.E32), set(measured) ^ set(S.E32)
    for k, v in measured.items():
        assert v <= S.E32[k] <= 2 * v, f"E32[{k}] = {S.E32[k]:.3g}, measured {v:.3g}"


# ---------------------------------------------------------------------------------------------------------------- power of the sweep
def _sweep(family, kernel, pred=lambda c: True, split=False):
    """run a CPU `kernel(case, inputs) -> outputs` over the family through check(): -> cases it failed on"""
    failed = []
    for c in S.cases(family):
        if not pred(c):
            continue
        inp = S.build(c)
        res = S.check(c, S.reference(c, inp), kernel(c, inp), split)
        if any(not r <= 1.0 for _, r, _ in res):
            failed.append((c, res))
    return failed


def _correct32(c, inp):
    out = S.evaluate(c, inp, F32)
    return {k: v for k, v in out.items() if not k.startswith("mag:")}


@pytest.mark.parametrize("family", FAMILIES)
def test_correct_float32_evaluation_passes_everywhere(family):
    failed = _sweep(family, _correct32)
    assert not failed, "\n".join(S.failures(c, r) for c, r in failed[:5])


def _attn_forward32(c, inp, mask=None, skip_last_tile_max=False, unnormalised_when_first_tile_dead=False):
    x = inp["qkv"]
    mask = inp["mask"] if mask is None else mask
    q, k, v = x.view(c.B, c.L, 3, c.nH, c.dH).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(c.dH)
    live = mask.bool()
    s = torch.where(live[:, None, None, :], s, torch.full_like(s, torch.finfo(F32).min))
    t0 = 64 * ((c.L - 1) // 64)
    m = (s[..., :t0] if skip_last_tile_max and t0 > 0 else s).max(-1, keepdim=True).values
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    if unnormalised_when_first_tile_dead and c.L > 64:
        dead = live.any(1) & ~live[:, :64].any(1)
        p = torch.where(dead[:, None, None, None], e, p)
    return {"probs": p, "ctx": (p @ v).transpose(1, 2).reshape(c.B * c.L, c.nH * c.dH)}


def _fake_attn_suffix(c, inp):
    n = inp["mask"].sum(1, keepdim=True)
    return _attn_forward32(c, inp, mask=(torch.arange(c.L)[None, :] < n).long())


def test_fake_attention_kernels_are_caught():
    assert not _sweep("A", _attn_forward32), "the float32 forward the fakes are variations of must pass"
    caught = _sweep("A", _fake_attn_suffix)
    assert caught and all(c.mask in ("prefix", "holes", "tile", "single", "empty") for c, _ in caught)
    caught = _sweep("A", lambda c, i: _attn_forward32(c, i, skip_last_tile_max=True))
    assert caught and any(c.profile == "std30_outlier" for c, _ in caught), "the row maximum without the last key tile"
    caught = _sweep("A", lambda c, i: _attn_forward32(c, i, unnormalised_when_first_tile_dead=True))
    assert caught and all(c.L > 64 for c, _ in caught), "no renormalisation behind a fully masked first tile"


def _fake_gemm_ignores_ldc(c, inp):
    out = _correct32(c, inp)
    ldc = c.N + c.pad_c
    buf = torch.full((c.M * ldc,), float("nan"))
    buf[:c.M * c.N] = out["out"].reshape(-1)           # rows written N apart
    out["out"] = buf.view(c.M, ldc)[:, :c.N]           # and read ldc apart
    return out


@pytest.mark.parametrize("family", ("B32", "BPL"))
def test_fake_gemm_kernels_are_caught(family):
    drop_tail = lambda c, inp: {k: v for k, v in S._eval_b(c, inp, F32, k_used=c.K - c.K % 32).items() if not k.startswith("mag:")}      # noqa: E731
    caught = {c.index for c, _ in _sweep(family, drop_tail)}
    assert caught == {c.index for c in S.cases(family) if c.K % 32}, "a GEMM without its K tail fails exactly where there is one"
    caught = {c.index for c, _ in _sweep(family, _fake_gemm_ignores_ldc)}
    assert caught and caught == {c.index for c in S.cases(family) if c.pad_c and c.M > 1}


def test_fake_column_kernels_are_caught():
    lost = lambda c, inp: S._eval_c(c, inp, F32, rows_used=c.rows - c.rows % 64)      # noqa: E731
    caught = {c.index for c, _ in _sweep("C", lost)}
    expect = {c.index for c in S.cases("C") if c.rows % 64}
    assert caught and caught <= expect and len(caught) >= 0.9 * len(expect), (len(caught), len(expect))


def _naive_var32(c, inp):
    x = S._seen(None, inp["x"], c.planes, F32)
    mean = x.mean(0)
    scale = c.rows / max(1, c.rows - 1) if c.op == "colstats_unbiased" else 1.0
    return {"mean": mean, "var": ((x * x).mean(0) - mean * mean) * scale}


def test_naive_variance_passes_the_old_metric_and_fails_the_new():
    """E[x^2] - mean^2 in float32 against col_scaled and against today's tensor-wide metric (max |a - b| / max |b| < 2e-5).

    On the generated offset cases (column means up to +-300, deviations 0.1 .. 3.2) the formula loses about mean^2 2^-23, some
    1e-2 absolute: col_scaled rejects every one of them by two to three decades -- but so does today's metric, whose figures
    there are 5e-4 .. 3e-3.  What today's metric cannot see is the same loss where it stays below 2e-5 of the WIDEST column
    while it ruins the narrow ones.  That is shown with the same inputs and their offsets at one tenth (means up to +-30): the
    tensor-wide figure is then 2e-6 .. 2e-5 and passes on most cases, col_scaled still rejects all of them (15 to 450 times its
    bound)."""
    stats = [c for c in S.cases("C") if c.op.startswith("colstats") and c.rows > 1]
    old_pass_new_fail = []
    for c in stats:
        inp = S.build(c)
        ref, got = S.reference(c, inp), _naive_var32(c, inp)
        new = dict((n, r) for n, r, _ in S.check(c, ref, got))["var"]
        assert (new > 1.0) == (c.profile == "offset"), f"{S.describe(c)}: {new:.3g} x bound"
        if c.profile != "offset":
            continue
        inp = dict(inp, x=inp["x"] - 0.9 * inp["x"].mean(0).round())
        ref, got = S.reference(c, inp), _naive_var32(c, inp)
        new = dict((n, r) for n, r, _ in S.check(c, ref, got))["var"]
        old = S.tensor_wide(got["var"], ref["var"])
        print(f"case {c.index}: offsets / 10: tensor-wide {old:.2e}, col_scaled {new:.1f} x bound")
        assert new > 1.0, S.describe(c)
        if old < 2e-5:
            old_pass_new_fail.append(c.index)
    assert len(old_pass_new_fail) >= 3, "the naive variance at small offsets must pass today's metric and fail col_scaled"


def _fake_cosine_overwrites_dx(c, inp):
    out = _correct32(c, inp)
    pc = max(1, 4096 // c.cols)
    if c.flag_b and c.n > pc:
        out["dx"] = S.cosine_backward(c, inp, F32, p_lo=(c.n - 1) // pc * pc)[0]
    return out


def test_fake_cosine_backward_is_caught():
    caught = {c.index for c, _ in _sweep("D", _fake_cosine_overwrites_dx, lambda c: c.op == "cosine")}
    multi = {c.index for c in S.cases("D") if c.op == "cosine" and c.flag_b and S.cosine_chunks(c) > 1}
    assert caught and caught <= multi and len(caught) >= 0.5 * len(multi), (caught, multi)
