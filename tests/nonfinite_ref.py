"""Non-finite propagation cases ("Non-finite values"; include/cxrk.h conventions): every case injects one NaN / +Inf into
a live position of one input, states the float64 CPU reference (the torch operation the entry point's header comment cites, autograd
for backwards) and the device call on the same inputs.  tests/test_nonfinite_host.py checks the reference side alone (the fixtures and
the torch facts of the contract); tests/test_nonfinite_gpu.py runs the device side against it.

A case is built by a function registered in CASES and returns a `Case`:
  ref      {name: float64 tensor}   reference outputs
  expect   {name: bool tensor}      where the contract says the reference is non-finite for a NaN (checked against `ref` on the host)
  loose    {name: bool tensor}      positions the reference multiplies by an exact zero (masked keys, dropped elements): 0 or NaN
  exact    {name: tensor}           integer / bit outputs that must be equal (decision bits at the NaN outputs, argmax, counters)
  tol      {name: float}            fp32-mode tolerance of that output where its family's parity test (tests/test_kernels_gpu.py) uses
                                    another one than `close`'s 2e-5; in split-bf16 mode every tolerance is at least 3e-4, as in `close`
  device   callable(K) -> {name: tensor} with the keys of ref and exact
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from kernel_refs import attention_mask, rnd

DEV = "cuda"
VALUES = {"nan": float("nan"), "inf": float("inf")}
CASES = {}


class Case:
    def __init__(self, ref, device, expect=None, loose=None, exact=None, tol=None):
        self.ref, self.device = ref, device
        self.expect, self.loose, self.exact, self.tol = expect or {}, loose or {}, exact or {}, tol or {}


def case(name, values=("nan", "inf"), **kw):
    """register a case builder; `values`: what is injected (a case whose contract is NaN-only says so)"""
    def deco(fn):
        CASES[name] = (functools.partial(fn, **kw) if kw else fn, values)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def build(name, value):
    """the case `name` with `value` ("nan" / "inf") injected; built once, shared by every test that uses it, never modified"""
    return CASES[name][0](VALUES[value])


def ids():
    """(case, value) pairs of the two test modules"""
    return [(n, v) for n, (_, values) in CASES.items() for v in values]


def inject(t, idx, value):
    """a copy of `t` with `value` at index tuple `idx`"""
    t = t.clone()
    t[idx] = value
    return t


def mask_of(shape, *idx):
    m = torch.zeros(shape, dtype=torch.bool)
    for i in idx:
        m[i] = True
    return m


def nonfinite(t):
    return ~torch.isfinite(t)


def planes_value(t):
    """the value a planes tensor holds for the fp32 tensor t: hi + lo with hi = bf16(t), lo = bf16(t - hi) (include/cxrk.h, "Storage
    formats"); a NaN stays a NaN, an Inf becomes one (lo = Inf - Inf).  References of planes kernels whose family tolerance is below
    the 2^-17 of the storage take their inputs through this, as tests/test_kernels_gpu.py does with `zq`."""
    hi = t.bfloat16().float()
    return hi + (t - hi).bfloat16().float()


def check_mix(c, value):
    """A case that makes everything NaN, or nothing, tests nothing: over all outputs of the case, and for a NaN inside every output for
    which the contract expects a mix, the reference has a non-finite and a finite element.  (An Inf may turn finite again inside one
    output, sigmoid(Inf) = 1 or relu(-Inf) = 0, so for +Inf the outputs are taken together.)"""
    nf = torch.cat([nonfinite(r).reshape(-1) for r in c.ref.values()])
    assert bool(nf.any()) and not bool(nf.all()), f"reference: {int(nf.sum())} of {nf.numel()} non-finite"
    for k, e in c.expect.items():
        if value == "nan" and bool(e.any()) and not bool(e.all()):
            got = nonfinite(c.ref[k])
            assert bool(got.any()) and not bool(got.all()), f"{k}: reference has {int(got.sum())} of {got.numel()} non-finite, the contract expects a mix"


# ------------------------------------------------------------------------------------------------ the two checks
def check_reference(c, value):
    """Host side: the reference has some non-finite and some finite element (a case that makes everything NaN, or nothing, tests
    nothing), and its non-finite elements are the index set the contract states (NaN: exactly; +Inf: inside it, an Inf can turn
    finite again, relu(-Inf) = 0)."""
    check_mix(c, value)
    for k, e in c.expect.items():
        got = nonfinite(c.ref[k])
        assert got.shape == e.shape, (k, got.shape, e.shape)
        lo = c.loose.get(k)
        if lo is not None:
            got, e = got & ~lo, e & ~lo
        if value == "nan":
            assert torch.equal(got, e), f"{k}: reference non-finite at {int(got.sum())} positions, contract {int(e.sum())}, differ at {int((got != e).sum())}"
        else:
            assert not bool((got & ~e).any()), f"{k}: reference non-finite outside the contract's index set"


def check_device(c, out, value, split, report=None):
    """Rules 1 and 2 of the contract on the device outputs `out`.  NaN: reference non-finite => device non-finite, reference finite =>
    device finite and within tolerance (`close` of tests/test_kernels_gpu.py: 2e-5 of the scale of the finite reference elements in
    fp32, 3e-4 in split-bf16; the output's own `tol` where its family's parity test uses another one).  +Inf: the first direction
    only.  The reference side must itself be a mix of non-finite and finite (check_mix)."""
    check_mix(c, value)
    bad = []
    for k, r in c.ref.items():
        d = out[k].detach().double().cpu().reshape(r.shape)
        nf = nonfinite(r)
        lo = c.loose.get(k, torch.zeros_like(nf))
        miss = nf & ~lo & torch.isfinite(d)
        if bool(miss.any()):
            bad.append(f"{k}: {int(miss.sum())} of {int((nf & ~lo).sum())} reference-non-finite elements are finite on the device")
        if value != "nan":
            continue
        fin = ~nf & ~lo
        if not bool(fin.any()):
            continue
        leak = fin & ~torch.isfinite(d)
        if bool(leak.any()):
            bad.append(f"{k}: {int(leak.sum())} reference-finite elements are non-finite on the device")
            continue
        tol = c.tol.get(k, 2e-5)
        if split:
            tol = max(tol, 3e-4)
        scale = r[fin].abs().max().clamp_min(1e-20)
        err = float((d[fin] - r[fin]).abs().max() / scale)
        if report is not None:
            report.append(f"{k}: err {err:.2e} tol {tol:.0e}")
        if not err < tol:
            bad.append(f"{k}: rel-to-max err {err:.3e} (tol {tol})")
    for k, e in c.exact.items():
        g = out[k].detach().cpu().reshape(e.shape)
        if not torch.equal(g.to(e.dtype), e):
            bad.append(f"{k}: {int((g.to(e.dtype) != e).sum())} of {e.numel()} exact values differ")
    assert not bad, "; ".join(bad)


def _d(t):
    return t.contiguous().to(DEV)


def _f(t):
    """fp32 tensor of a Planes / fp32 device result"""
    return t.float() if hasattr(t, "plane") else t


# ------------------------------------------------------------------------------------------------ GEMM
GM, GN, GK = 200, 136, 72            # two row tiles, a ragged column tile, K not a multiple of the k-step
I0, N0, K0 = 131, 133, 70            # second row tile, ragged column tail, last k chunk


def _gemm_inputs(site, value, N=GN):
    x, w, b, r = rnd(GM, GK, scale=0.5), rnd(N, GK, seed=1, scale=0.5), rnd(N, seed=2), rnd(GM, N, seed=3)
    n0 = N - 3
    if site == "a":
        x = inject(x, (I0, K0), value); e = mask_of((GM, N), I0)
    elif site == "w":
        w = inject(w, (n0, K0), value); e = mask_of((GM, N), (slice(None), n0))
    elif site == "bias":
        b = inject(b, (n0,), value); e = mask_of((GM, N), (slice(None), n0))
    else:
        r = inject(r, (I0, n0), value); e = mask_of((GM, N), (I0, n0))
    return x, w, b, r, e


def _pl_gemm_tol(ref, planes):
    """the planes GEMM family is checked at 2e-4 (test_planes_gemm_family), the fp32 one at `close`'s default"""
    return {k: 2e-4 for k in ref} if planes else {}


def _gemm_fwd_ref(x, w, b, r):
    pre = x.double() @ w.double().T + b.double() + r.double()
    return {"none": pre, "relu": F.relu(pre), "gelu": F.gelu(pre), "preact": pre}


def _gemm_fwd(value, site, planes):
    x, w, b, r, e = _gemm_inputs(site, value)
    ref = _gemm_fwd_ref(x, w, b, r)

    def device(K):
        if planes:
            xp, wp, rp = K.split_planes(_d(x)), K.split_planes(_d(w)), K.split_planes(_d(r))
            pre = torch.empty(GM, GN, device=DEV)
            return {"none": K.linear_fwd_pl(xp, wp, bias=_d(b), residual=rp),
                    "relu": K.linear_fwd_pl(xp, wp, bias=_d(b), residual=_d(r), act=K.ACT_RELU, out_planes=True).float(),
                    "gelu": K.linear_fwd_pl(xp, wp, bias=_d(b), residual=rp, act=K.ACT_GELU, preact_out=pre, out_planes=True).float(),
                    "preact": pre}
        pre = torch.empty(GM, GN, device=DEV)
        return {"none": K.linear_fwd(_d(x), _d(w), bias=_d(b), residual=_d(r)),
                "relu": K.linear_fwd(_d(x), _d(w), bias=_d(b), residual=_d(r), act=K.ACT_RELU),
                "gelu": K.linear_fwd(_d(x), _d(w), bias=_d(b), residual=_d(r), act=K.ACT_GELU, preact_out=pre),
                "preact": pre}
    return Case(ref, device, expect={k: e for k in ref}, tol=_pl_gemm_tol(ref, planes))


for _site in ("a", "w", "bias", "res"):
    case(f"gemm_f32_fwd_{_site}", site=_site, planes=False)(_gemm_fwd)
    case(f"gemm_pl_fwd_{_site}", site=_site, planes=True)(_gemm_fwd)


@case("gemm_pl_relu_maskout")
def _gemm_pl_maskout(value):
    """ReLU + decision bits on planes operands; the bit mask exists for N % 64 == 0 only, hence N = 192 (three column tiles).  The bit
    of a NaN output is 0, as NaN > 0 is."""
    N = 192
    x, w, b, r, e = _gemm_inputs("a", value, N=N)
    pre = x.double() @ w.double().T + b.double()
    ref = {"relu": F.relu(pre)}
    nan_out = torch.isnan(ref["relu"])

    def device(K):
        mask = torch.empty(GM, N // 8, dtype=torch.uint8, device=DEV)
        y = K.linear_fwd_pl(K.split_planes(_d(x)), K.split_planes(_d(w)), bias=_d(b), act=K.ACT_RELU, out_planes=True, maskout=mask).float()
        return {"relu": y, "bits_at_nan": K.unpack_mask(mask, N).view(GM, N)[nan_out]}
    return Case(ref, device, expect={"relu": e}, exact={"bits_at_nan": torch.zeros(int(nan_out.sum()), dtype=torch.bool)}, tol={"relu": 2e-4})


def _gelu_grad64(a):
    return 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)


def _gemm_bwd_data(value, planes):
    """dx = dy @ w through every fused backward epilogue, NaN in dy[m0, n0]: row m0 (the ReLU-off positions stay 0: select)"""
    dy, w, aux, add = rnd(GM, GN, seed=4, scale=0.5), rnd(GN, GK, seed=1, scale=0.5), rnd(GM, GK, seed=5), rnd(GM, GK, seed=6)
    dy = inject(dy, (I0, N0), value)
    dx = dy.double() @ w.double()
    on = aux > 0
    ref = {"plain": dx, "relu_mask": torch.where(on, dx, torch.zeros_like(dx)), "gelu_grad": dx * _gelu_grad64(aux.double())}
    row = mask_of((GM, GK), I0)
    expect = {"plain": row, "relu_mask": row & on, "gelu_grad": row}
    if planes:
        ref["residual"] = dx + add.double(); expect["residual"] = row
        ref["accumulate"] = dx + 1.0; expect["accumulate"] = row

    def device(K):
        if planes:
            dyp, wp = K.split_planes(_d(dy)), K.split_planes(_d(w))
            bits = torch.from_numpy(np.packbits(on.numpy(), axis=1, bitorder="little")).to(DEV)
            return {"plain": K.linear_bwd_data_pl(dyp, wp),
                    "relu_mask": K.linear_bwd_data_pl(dyp, wp, maskin=bits, out_planes=True).float(),
                    "gelu_grad": K.linear_bwd_data_pl(dyp, wp, aux=_d(aux), auxmode=K.AUX_GELU_GRAD, out_planes=True).float(),
                    "residual": K.linear_bwd_data_pl(dyp, wp, residual=K.split_planes(_d(add))),
                    "accumulate": K.linear_bwd_data_pl(dyp, wp, out=torch.full((GM, GK), 1.0, device=DEV), accumulate=True)}
        return {"plain": K.linear_bwd_data(_d(dy), _d(w)),
                "relu_mask": K.linear_bwd_data(_d(dy), _d(w), aux=_d(aux), auxmode=K.AUX_RELU_MASK),
                "gelu_grad": K.linear_bwd_data(_d(dy), _d(w), aux=_d(aux), auxmode=K.AUX_GELU_GRAD)}
    return Case(ref, device, expect=expect, tol=_pl_gemm_tol(ref, planes))


case("gemm_f32_bwd_data", planes=False)(_gemm_bwd_data)
case("gemm_pl_bwd_data", planes=True)(_gemm_bwd_data)


def _gemm_bwd_weight(value, planes):
    """dW = dy^T x (split-K, accumulate), NaN in dy[m0, n0]: row n0 of dW only"""
    dy, x, base = rnd(GM, GN, seed=4, scale=0.5), rnd(GM, GK, seed=2, scale=0.5), rnd(GN, GK, seed=7)
    dy = inject(dy, (I0, N0), value)
    dw = dy.double().T @ x.double()
    ref = {"auto": dw, "accumulate": dw + base.double()}
    if not planes:
        ref["splitk3"] = dw
    row = mask_of((GN, GK), N0)

    def device(K):
        if planes:
            dyp, xp = K.split_planes(_d(dy)), K.split_planes(_d(x))
            return {"auto": K.linear_bwd_weight_pl(dyp, xp, torch.zeros(GN, GK, device=DEV)),
                    "accumulate": K.linear_bwd_weight_pl(dyp, xp, _d(base), accumulate=True)}
        return {"auto": K.linear_bwd_weight(_d(dy), _d(x), torch.zeros(GN, GK, device=DEV)),
                "accumulate": K.linear_bwd_weight(_d(dy), _d(x), _d(base), accumulate=True),
                "splitk3": K.gemm(_d(dy), _d(x), torch.empty(GN, GK, device=DEV), GN, GK, GM, True, False, splitk=3)}
    return Case(ref, device, expect={k: row for k in ref}, tol=_pl_gemm_tol(ref, planes))


case("gemm_f32_bwd_weight", planes=False)(_gemm_bwd_weight)
case("gemm_pl_bwd_weight", planes=True)(_gemm_bwd_weight)


@case("gemm_pl_splitk3")
def _gemm_pl_splitk3(value):
    dy, x = inject(rnd(GM, GN, seed=4, scale=0.5), (I0, N0), value), rnd(GM, GK, seed=2, scale=0.5)
    ref = {"splitk3": dy.double().T @ x.double()}

    def device(K):
        return {"splitk3": K.gemm_pl(K.split_planes(_d(dy)), K.split_planes(_d(x)), GN, GK, GM, True, False,
                                     out=torch.empty(GN, GK, device=DEV), splitk=3)}
    return Case(ref, device, expect={"splitk3": mask_of((GN, GK), N0)}, tol={"splitk3": 2e-4})


@case("colsums")
def _colsums(value):
    """stand-alone and fused column sums: a NaN stays in its column"""
    x = inject(rnd(GM, GN, seed=4), (I0, N0), value)
    mean = x.double().nan_to_num(0.0, 0.0, 0.0).mean(0).float()       # a finite mean: colvar's NaN comes from x alone
    dy, w = rnd(GM, GN, seed=8, scale=0.5), inject(rnd(GN, GK, seed=1, scale=0.5), (N0, K0), value)
    dx = dy.double() @ w.double()
    ref = {"colsum": x.double().sum(0), "colsum_pl": x.double().sum(0), "colvar": ((x.double() - mean.double()) ** 2).sum(0),
           "colvar_pl": ((x.double() - mean.double()) ** 2).sum(0), "fused_dx": dx, "fused_colsum": dx.sum(0)}
    col, kcol = mask_of((GN,), N0), mask_of((GK,), K0)

    def device(K):
        xp = K.split_planes(_d(x))
        cs = torch.full((GK,), 3.0, device=DEV)
        dxp = K.linear_bwd_data_pl(K.split_planes(_d(dy)), K.split_planes(_d(w)), out_planes=True, colsum=cs)
        return {"colsum": K.colsum(_d(x), torch.empty(GN, device=DEV)), "colsum_pl": K.colsum(xp, torch.empty(GN, device=DEV)),
                "colvar": K.colvar(_d(x), _d(mean), torch.empty(GN, device=DEV)), "colvar_pl": K.colvar(xp, _d(mean), torch.empty(GN, device=DEV)),
                "fused_dx": dxp.float(), "fused_colsum": cs}
    return Case(ref, device, expect={"colsum": col, "colsum_pl": col, "colvar": col, "colvar_pl": col,
                                     "fused_dx": mask_of((GM, GK), (slice(None), K0)), "fused_colsum": kcol},
                tol={"fused_dx": 2e-4, "fused_colsum": 8e-4})      # the planes GEMM family's 2e-4, and its 4x for the fused sums


# ------------------------------------------------------------------------------------------------ train-mode BatchNorm chain
def _bn_inputs(rows, C):
    g = torch.Generator().manual_seed(rows + C)
    z = torch.randn(rows, C, generator=g) * torch.linspace(0.5, 2.0, C) + torch.linspace(-2.0, 2.0, C)
    res, dy = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return z, res, dy, gamma, beta, rm0, rv0


def _bn_fwd(value, rows, C, planes):
    """colstats -> bn_train_fwd_coeffs (running statistics included) -> bn_apply (ReLU, residual, decision bits); NaN in z[r0, c0]:
    channel c0 only"""
    z, res, _, gamma, beta, rm0, rv0 = _bn_inputs(rows, C)
    r0, c0 = rows - 5, C - 3
    z = inject(z, (r0, c0), value)
    z64 = (planes_value(z) if planes else z).double()      # the values the kernels see
    res = planes_value(res) if planes else res
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = F.relu(F.batch_norm(z64, rm, rv, gamma.double(), beta.double(), training=True, momentum=0.1, eps=1e-5) + res.double())
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    ref = {"mean": mean, "var": var, "scale": gamma.double() * rstd, "shift": beta.double() - mean * gamma.double() * rstd, "rstd": rstd,
           "running_mean": rm, "running_var": rv, "y": y}
    ch = mask_of((C,), c0)
    expect = {k: ch for k in ref if k != "y"}
    expect["y"] = mask_of((rows, C), (slice(None), c0))
    nan_out = torch.isnan(y)

    def device(K):
        wrap = (lambda t: K.split_planes(_d(t))) if planes else _d
        zd = wrap(z)
        mean_d, var_d = K.colstats(zd)
        rmd, rvd = _d(rm0), _d(rv0)
        scale, shift, rstd_d = K.bn_train_fwd_coeffs(mean_d, var_d, _d(gamma), _d(beta), 1e-5, rows, 0.1, rmd, rvd)
        yd, mask = K.bn_apply(zd, scale, shift, residual=wrap(res), relu=True, want_mask=True)
        return {"mean": mean_d, "var": var_d, "scale": scale, "shift": shift, "rstd": rstd_d, "running_mean": rmd, "running_var": rvd,
                "y": _f(yd), "bits_at_nan": K.unpack_mask(mask, C).view(rows, C)[nan_out]}
    return Case(ref, device, expect=expect, exact={"bits_at_nan": torch.zeros(int(nan_out.sum()), dtype=torch.bool)},
                tol={"mean": 1e-6, "y": 3e-5, "running_mean": 2e-6})      # test_train_mode_batchnorm_kernels' own


def _bn_bwd(value, rows, C, planes):
    """colsum -> coldot -> bn_train_bwd_coeffs -> bn_train_dz with finite saved state; NaN in dy[r0, c0]: channel c0 only"""
    z, _, dy, gamma, beta, _, _ = _bn_inputs(rows, C)
    r0, c0 = rows - 5, C - 3
    dy = inject(dy, (r0, c0), value)
    zq, dyq = (planes_value(z), planes_value(dy)) if planes else (z, dy)      # the values the kernels see
    z64 = zq.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.batch_norm(z64, None, None, g64, b64, training=True, eps=1e-5).backward(dyq.double())
    zc = zq.double() - zq.double().mean(0)
    ref = {"sumdy": dyq.double().sum(0), "dot": (dyq.double() * zc).sum(0), "dgamma": g64.grad, "dbeta": b64.grad, "dz": z64.grad}
    ch = mask_of((C,), c0)
    expect = {k: ch for k in ref if k != "dz"}
    expect["dz"] = mask_of((rows, C), (slice(None), c0))

    def device(K):
        wrap = (lambda t: K.split_planes(_d(t))) if planes else _d
        zd, dyd = wrap(z), wrap(dy)
        mean_d, var_d = K.colstats(zd)
        _, _, rstd_d = K.bn_train_fwd_coeffs(mean_d, var_d, _d(gamma), _d(beta), 1e-5, rows, 0.0)
        sumdy = K.colsum(dyd, torch.empty(C, device=DEV))
        dot = K.coldot(dyd, zd, mean_d)
        dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        A, B, Cc = K.bn_train_bwd_coeffs(_d(gamma), mean_d, rstd_d, sumdy, dot, rows, dgam, dbet, False)
        return {"sumdy": sumdy, "dot": dot, "dgamma": dgam, "dbeta": dbet, "dz": _f(K.bn_train_dz(dyd, zd, A, B, Cc))}
    return Case(ref, device, expect=expect, tol={"dgamma": 3e-4, "dz": 1e-4})


for _rows, _C, _pl in ((777, 264, True), (5000, 64, False)):
    case(f"bn_train_fwd_{_rows}x{_C}", rows=_rows, C=_C, planes=_pl)(_bn_fwd)
    case(f"bn_train_bwd_{_rows}x{_C}", rows=_rows, C=_C, planes=_pl)(_bn_bwd)


# ------------------------------------------------------------------------------------------------ pooling, layout, planes format
PH, PW = 13, 11


def _pool_x(C, post_relu):
    x = rnd(2, C, PH, PW, seed=C)
    return F.relu(x) if post_relu else x


def _maxpool_fwd(value, C, planes):
    """3x3 / stride 2 / pad 1 max-pool: torch lets a NaN win wherever it sits in the window.  (3, 3) is the last tap of window (1, 1)
    and the first tap of window (2, 2); (4, 6) is the centre tap of one window."""
    x = inject(inject(_pool_x(C, planes), (0, 1, 3, 3), value), (1, C - 1, 4, 6), value)
    ref = {"y": F.max_pool2d((planes_value(x) if planes else x).double(), 3, 2, 1)}
    Ho, Wo = ref["y"].shape[2:]
    e = torch.zeros(2, C, Ho, Wo, dtype=torch.bool)
    e[0, 1, 1:3, 1:3] = True
    e[1, C - 1, 2, 3] = True

    def device(K):
        xd = _d(x.permute(0, 2, 3, 1))
        y = K.maxpool_fwd_pl(K.split_planes(xd))[0].float() if planes else K.maxpool_fwd(xd)[0]
        return {"y": y.permute(0, 3, 1, 2)}
    return Case(ref, device, expect={"y": e})


def _maxpool_bwd(value, C, planes):
    """NaN in one dy element, finite saved state: only the window's winner receives it (the planes form masks by the stem ReLU
    through the sign of the pooled value: select)"""
    x = planes_value(_pool_x(C, True)) if planes else _pool_x(C, False)
    x64 = x.double().requires_grad_(True)
    y = F.max_pool2d(x64, 3, 2, 1)
    n0, c0, ho, wo = 1, C - 2, 3, 2
    assert float(y.detach()[n0, c0, ho, wo]) > 0
    gy = inject(rnd(*y.shape, seed=3), (n0, c0, ho, wo), value)
    y.backward((planes_value(gy) if planes else gy).double())
    dx = x64.grad
    if planes:
        dx = torch.where(x.double() > 0, dx, torch.zeros_like(dx))
    ref = {"dx": dx}
    win = (x[n0, c0] == y[n0, c0, ho, wo].float()).nonzero()
    assert win.shape[0] == 1
    e = mask_of(tuple(x.shape), (n0, c0, int(win[0, 0]), int(win[0, 1])))

    def device(K):
        xd, gyd = _d(x.permute(0, 2, 3, 1)), _d(gy.permute(0, 2, 3, 1))
        if planes:
            pooled, idx = K.maxpool_fwd_pl(K.split_planes(xd))
            d = K.maxpool_bwd_pl(K.split_planes(gyd), idx, pooled, PH, PW)
        else:
            _, idx = K.maxpool_fwd(xd)
            d = K.maxpool_bwd(gyd, idx, xd, False)
        return {"dx": d.permute(0, 3, 1, 2)}
    return Case(ref, device, expect={"dx": e})


for _C, _pl in ((12, False), (24, True)):
    case(f"maxpool_fwd_C{_C}", C=_C, planes=_pl)(_maxpool_fwd)
    case(f"maxpool_bwd_C{_C}", C=_C, planes=_pl)(_maxpool_bwd)


@case("spatial_mean")
def _spatial_mean(value):
    p = inject(rnd(3, 49, 128), (1, 17, 5), value)
    g = inject(rnd(3, 128, seed=1), (2, 77), value)
    add = rnd(3, 49, 128, seed=2)
    bwd = (g.double() / 49)[:, None, :].expand(3, 49, 128)
    ref = {"fwd": p.double().mean(1), "bwd": bwd, "bwd_pl": bwd + add.double()}
    eb = mask_of((3, 49, 128), (2, slice(None), 77))

    def device(K):
        return {"fwd": K.spatial_mean_fwd(_d(p)), "bwd": K.spatial_mean_bwd(_d(g), 49), "bwd_pl": K.spatial_mean_bwd_pl(_d(g), 49, add=_d(add)).float()}
    return Case(ref, device, expect={"fwd": mask_of((3, 128), (1, 5)), "bwd": eb, "bwd_pl": eb})


@case("layout_and_planes_format")
def _layout(value):
    """NCHW <-> NHWC and fp32 <-> planes: the element stays non-finite, nothing else changes.  (+Inf becomes NaN in planes storage,
    lo = Inf - Inf: the kind is not pinned.)"""
    x = inject(rnd(2, 3, 9, 7), (1, 2, 4, 5), value)
    xn = inject(rnd(2, 9, 7, 8, seed=1), (1, 4, 5, 6), value)
    t = inject(rnd(300, 136), (177, 133), value)
    nhwc = F.pad(x.double().permute(0, 2, 3, 1), (0, 1))
    ref = {"nchw_to_nhwc": nhwc, "nhwc_to_nchw": xn.double().permute(0, 3, 1, 2), "split_merge": t.double(), "split_hi": t.bfloat16().double()}

    def device(K):
        p = K.split_planes(_d(t))
        return {"nchw_to_nhwc": K.nchw_to_nhwc(_d(x), 4), "nhwc_to_nchw": K.nhwc_to_nchw(_d(xn)), "split_merge": p.float(), "split_hi": p.t[0].float()}
    return Case(ref, device, expect={"nchw_to_nhwc": mask_of(nhwc.shape, (1, 4, 5, 2)), "nhwc_to_nchw": mask_of((2, 8, 9, 7), (1, 6, 4, 5)),
                                     "split_merge": mask_of((300, 136), (177, 133)), "split_hi": mask_of((300, 136), (177, 133))},
                tol={"split_hi": 1e-30})     # the hi plane is bf16(x), round to nearest even: exact


# ------------------------------------------------------------------------------------------------ convolution (+ folded eval BatchNorm)
CONV_SHAPES = {   # N, H, W, C, Ko, R, stride, pad
    "1x1": (2, 14, 14, 64, 256, 1, 1, 0), "3x3s2": (2, 15, 15, 64, 128, 3, 2, 1), "halo": (2, 12, 12, 64, 64, 3, 1, 1),
    "stem": (2, 32, 32, 4, 64, 7, 2, 3),
}


def _conv_inputs(cfg):
    N, H, W, C, Ko, R, stride, pad = cfg
    cr = 3 if C == 4 else C
    x = rnd(N, cr, H, W)
    w = rnd(Ko, cr, R, R, seed=1, scale=1.0 / math.sqrt(cr * R * R))
    gamma, beta = 1 + 0.1 * rnd(Ko, seed=2), 0.1 * rnd(Ko, seed=3)
    rm, rv = 0.1 * rnd(Ko, seed=4), 0.5 + rnd(Ko, seed=5).abs()
    return cr, x, w, gamma, beta, rm, rv


def _fold(K, planes, w, gamma, beta, rm, rv, Ko, R, cr, C):
    """(w_scaled, scale, shift, rstd, w_cl) on the device"""
    w_cl = _d(w.permute(0, 2, 3, 1))
    sc, sh, rstd = (torch.empty(Ko, device=DEV) for _ in range(3))
    if planes:
        ws = K.Planes.empty(Ko, R * R * C, device=DEV)
        K.bn_fold_pl(w_cl, _d(gamma), _d(beta), _d(rm), _d(rv), 1e-5, Ko, R * R, cr, C, ws, sc, sh, rstd)
    else:
        ws = torch.empty(Ko, R, R, C, device=DEV)
        K.bn_fold(w_cl, _d(gamma), _d(beta), _d(rm), _d(rv), 1e-5, Ko, R * R, cr, C, ws, sc, sh, rstd)
    return ws, sc, sh, rstd, w_cl


def _conv_fwd(value, shape, planes):
    """conv + folded BN + residual + ReLU (+ decision bits on planes); NaN at one input pixel and channel: exactly its receptive
    field, across all Ko"""
    cfg = CONV_SHAPES[shape]
    N, H, W, C, Ko, R, stride, pad = cfg
    cr, x, w, gamma, beta, rm, rv = _conv_inputs(cfg)
    n0, c0, h0, w0 = 1, cr - 1, 5, 6
    x = inject(x, (n0, c0, h0, w0), value)
    z = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    stem = C == 4
    res = rnd(*z.shape, seed=9)
    y = F.relu(F.batch_norm(z, rm.double(), rv.double(), gamma.double(), beta.double(), training=False, eps=1e-5) + res.double())
    ind = torch.zeros(1, 1, H, W, dtype=torch.float64); ind[0, 0, h0, w0] = 1
    field = F.conv2d(ind, torch.ones(1, 1, R, R, dtype=torch.float64), stride=stride, padding=pad)[0, 0] > 0
    e = torch.zeros_like(y, dtype=torch.bool)
    e[n0, :, field] = True
    ref = {"y": y}
    nan_out = torch.isnan(y.permute(0, 2, 3, 1))
    Ho, Wo = y.shape[2:]

    def device(K):
        ws, sc, sh, rstd, _ = _fold(K, planes and not stem, w, gamma, beta, rm, rv, Ko, R, cr, C)
        resn = _d(res.permute(0, 2, 3, 1))
        if planes:    # the stem reads the fp32 image and fp32 filters (in_planes = 0) and writes planes like every other unit
            xd = K.nchw_to_nhwc(_d(x), C) if stem else K.split_planes(_d(x.permute(0, 2, 3, 1)))
            yd = K.Planes.empty(N, Ho, Wo, Ko, device=DEV)
            mask = torch.empty(N * Ho * Wo, Ko // 8, dtype=torch.uint8, device=DEV)
            K.conv_fwd_pl(xd, ws, sh, K.split_planes(resn), yd, mask, N, H, W, C, Ko, R, R, stride, pad, True)
            return {"y": yd.float().permute(0, 3, 1, 2), "bits_at_nan": K.unpack_mask(mask, Ko).view(N, Ho, Wo, Ko)[nan_out]}
        yd = torch.empty(N, Ho, Wo, Ko, device=DEV)
        K.conv_fwd(K.nchw_to_nhwc(_d(x), C), ws, sh, resn, yd, N, H, W, C, Ko, R, R, stride, pad, True)
        return {"y": yd.permute(0, 3, 1, 2)}
    exact = {"bits_at_nan": torch.zeros(int(nan_out.sum()), dtype=torch.bool)} if planes else {}
    return Case(ref, device, expect={"y": e}, exact=exact, tol={"y": 2e-4} if planes else {})      # planes conv family: 2e-4


def _conv_bwd_data(value, shape, planes):
    """data gradient with residual, ReLU mask (select) and fused column sums; NaN in one dy element"""
    cfg = CONV_SHAPES[shape]
    N, H, W, C, Ko, R, stride, pad = cfg
    cr, x, w, gamma, beta, rm, rv = _conv_inputs(cfg)
    sc64 = gamma.double() / torch.sqrt(rv.double() + 1e-5)
    wsc = w.double() * sc64[:, None, None, None]
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    n0, k0, ho, wo = 1, Ko - 2, 3, 4
    gy = inject(rnd(N, Ko, Ho, Wo, seed=10), (n0, k0, ho, wo), value)
    add = rnd(N, C, H, W, seed=11)
    on = rnd(N, C, H, W, seed=12) > 0
    x64 = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, wsc, stride=stride, padding=pad).backward(gy.double())
    plain = x64.grad
    full = torch.where(on, plain + add.double(), torch.zeros_like(plain))
    ref = {"plain": plain, "res_mask": full, "sums": full.sum(dim=(0, 2, 3))}
    ind = torch.zeros(1, 1, Ho, Wo, dtype=torch.float64); ind[0, 0, ho, wo] = 1
    field = F.conv_transpose2d(ind, torch.ones(1, 1, R, R, dtype=torch.float64), stride=stride, padding=pad,
                               output_padding=(H + 2 * pad - R) % stride)[0, 0] > 0
    e = torch.zeros(N, C, H, W, dtype=torch.bool)
    e[n0, :, field] = True
    relu_src = torch.where(on, torch.ones(N, C, H, W), -torch.ones(N, C, H, W))

    def device(K):
        ws, sc, sh, rstd, _ = _fold(K, planes, w, gamma, beta, rm, rv, Ko, R, cr, C)
        gyn, addn = _d(gy.permute(0, 2, 3, 1)), _d(add.permute(0, 2, 3, 1))
        sums = torch.empty(C, device=DEV)
        if planes:
            gyp = K.split_planes(gyn)
            d0, d1 = K.Planes.empty(N, H, W, C, device=DEV), K.Planes.empty(N, H, W, C, device=DEV)
            bits = torch.from_numpy(np.packbits(on.permute(0, 2, 3, 1).reshape(-1, C).numpy(), axis=1, bitorder="little")).to(DEV)
            K.conv_bwd_data_pl(gyp, ws, None, None, d0, N, H, W, C, Ko, R, R, stride, pad)
            K.conv_bwd_data_pl(gyp, ws, K.split_planes(addn), bits, d1, N, H, W, C, Ko, R, R, stride, pad, sums=sums)
            d0, d1 = d0.float(), d1.float()
        else:
            d0, d1 = torch.empty(N, H, W, C, device=DEV), torch.empty(N, H, W, C, device=DEV)
            K.conv_bwd_data(gyn, ws, None, None, d0, N, H, W, C, Ko, R, R, stride, pad)
            K.conv_bwd_data(gyn, ws, addn, _d(relu_src.permute(0, 2, 3, 1)), d1, N, H, W, C, Ko, R, R, stride, pad, sums=sums)
        return {"plain": d0.permute(0, 3, 1, 2), "res_mask": d1.permute(0, 3, 1, 2), "sums": sums}
    return Case(ref, device, expect={"plain": e, "res_mask": e & on}, tol={k: 3e-4 if planes else 5e-5 for k in ref})


def _conv_bwd_params(value, shape, planes):
    """weight / gamma / beta gradients; NaN in dy[..., k0]: only dW[k0], dgamma[k0], dbeta[k0]"""
    cfg = CONV_SHAPES[shape]
    N, H, W, C, Ko, R, stride, pad = cfg
    cr, x, w, gamma, beta, rm, rv = _conv_inputs(cfg)
    w64, g64, b64 = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    y = F.batch_norm(F.conv2d(x.double(), w64, stride=stride, padding=pad), rm.double(), rv.double(), g64, b64, training=False, eps=1e-5)
    n0, k0, ho, wo = 1, Ko - 2, 3, 4
    gy = inject(rnd(*y.shape, seed=10), (n0, k0, ho, wo), value)
    y.backward(gy.double())
    ref = {"dw": w64.grad, "dgamma": g64.grad, "dbeta": b64.grad}
    stem = C == 4

    def device(K):
        _, sc, sh, rstd, w_cl = _fold(K, False, w, gamma, beta, rm, rv, Ko, R, cr, C)
        gyn = _d(gy.permute(0, 2, 3, 1))
        dw, dg, db = torch.empty(Ko, R, R, cr, device=DEV), torch.empty(Ko, device=DEV), torch.empty(Ko, device=DEV)
        if planes and not stem:
            gyp = K.split_planes(gyn)
            sumdy = K.colsum(gyp.view(-1, Ko), torch.empty(Ko, device=DEV))
            K.conv_bwd_params_pl(K.split_planes(_d(x.permute(0, 2, 3, 1))), gyp, w_cl, sc, rstd, _d(rm), sumdy, dw, dg, db, False,
                                 N, H, W, C, Ko, R, R, stride, pad)
        else:
            sumdy = K.colsum(gyn.view(-1, Ko), torch.empty(Ko, device=DEV))
            K.conv_bwd_params(K.nchw_to_nhwc(_d(x), C), gyn, w_cl, sc, rstd, _d(rm), sumdy, dw, dg, db, False, N, H, W, cr, C, Ko, R, R,
                              stride, pad)
        return {"dw": dw.permute(0, 3, 1, 2), "dgamma": dg, "dbeta": db}
    ch = mask_of((Ko,), k0)
    return Case(ref, device, expect={"dw": mask_of(tuple(w.shape), k0), "dgamma": ch, "dbeta": ch},
                tol={"dw": 3e-4, "dgamma": 2e-2, "dbeta": 3e-4} if planes and not stem else {"dw": 5e-5, "dgamma": 2e-3, "dbeta": 5e-5})


for _shape in CONV_SHAPES:
    for _pl in (False, True):
        _sfx = f"{_shape}_{'pl' if _pl else 'f32'}"
        case(f"conv_fwd_{_sfx}", shape=_shape, planes=_pl)(_conv_fwd)
        if not (_shape == "stem" and _pl):        # the stem's weight gradient is fp32 in both modes
            case(f"conv_bwd_params_{_sfx}", shape=_shape, planes=_pl)(_conv_bwd_params)
        if _shape != "stem":                      # the stem has no data gradient (its input is the image)
            case(f"conv_bwd_data_{_sfx}", shape=_shape, planes=_pl)(_conv_bwd_data)


@case("conv_bwd_data_pl_s2res")
def _conv_s2res(value):
    """the data gradient with the compact stride-2 residual (even pixels only); NaN in one dy element and in one residual element"""
    N, H, W, C, Ko, R = 2, 12, 12, 64, 64, 3
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(N, Ko, H, W, generator=g)
    w1 = torch.randn(Ko, C, R, R, generator=g) * 0.05
    comp = torch.randn(N, C, H // 2, W // 2, generator=g)
    on = torch.rand(N, C, H, W, generator=g) > 0.5
    dy = inject(dy, (1, 5, 3, 4), value)
    comp = inject(comp, (0, 9, 2, 1), value)        # dense pixel (4, 2) of image 0, channel 9
    on[0, 9, 4, 2] = True
    x64 = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w1.double(), padding=1).backward(dy.double())
    dense = torch.zeros(N, C, H, W, dtype=torch.float64)
    dense[:, :, ::2, ::2] = comp.double()
    full = torch.where(on, x64.grad + dense, torch.zeros_like(dense))
    ref = {"dx": full, "sums": full.sum(dim=(0, 2, 3))}
    e = torch.zeros(N, C, H, W, dtype=torch.bool)
    e[1, :, 2:5, 3:6] = True
    e[0, 9, 4, 2] = True

    def device(K):
        bits = torch.from_numpy(np.packbits(on.permute(0, 2, 3, 1).reshape(-1, C).numpy(), axis=1, bitorder="little")).to(DEV)
        dx, sums = K.Planes.empty(N, H, W, C, device=DEV), torch.empty(C, device=DEV)
        K.conv_bwd_data_pl(K.split_planes(_d(dy.permute(0, 2, 3, 1))), K.split_planes(_d(w1.permute(0, 2, 3, 1)).view(Ko, R * R * C)),
                           K.split_planes(_d(comp.permute(0, 2, 3, 1))), bits, dx, N, H, W, C, Ko, R, R, 1, 1, sums, residual_s2=True)
        return {"dx": dx.float().permute(0, 3, 1, 2), "sums": sums}
    return Case(ref, device, expect={"dx": e & on}, tol={"dx": 3e-4, "sums": 3e-4})


# ------------------------------------------------------------------------------------------------ BERT pieces
@case("embed_ln_fwd")
def _embed_ln(value):
    V, H, L, B = 50, 64, 8, 3
    word, pos, typ = rnd(V, H), rnd(16, H, seed=1), rnd(2, H, seed=2)
    g, b = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V - 1, (B, L), generator=torch.Generator().manual_seed(5))
    ids[1, 3] = V - 1                                   # the one token that uses the poisoned row
    word = inject(word, (V - 1, 17), value)
    ref = {"y": F.layer_norm(word.double()[ids] + pos.double()[:L][None] + typ.double()[0], (H,), g.double(), b.double(), 1e-12).view(B * L, H)}
    ref["y_planes"] = ref["y"]
    e = mask_of((B * L, H), 1 * L + 3)

    def device(K):
        a = (_d(ids), _d(word), _d(pos), _d(typ[0]), _d(g), _d(b), 1e-12, L)
        return {"y": K.embed_ln_fwd(*a)[0], "y_planes": K.embed_ln_fwd(*a, out_planes=True)[0].float()}
    return Case(ref, device, expect={"y": e, "y_planes": e})


@case("residual_ln_fwd")
def _ln_fwd(value):
    rows, H = 77, 128
    x, r = inject(rnd(rows, H), (70, 5), value), rnd(rows, H, seed=1)
    g, b = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    s = x.double() + r.double()
    mean = s.mean(1, keepdim=True)
    var = ((s - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-12)
    xhat = (s - mean) * rstd
    y = xhat * g.double() + b.double()
    ref = {"y": y, "y_planes": y, "xhat": xhat, "rstd": rstd[:, 0]}
    row = mask_of((rows, H), 70)

    def device(K):
        y_, xh, rs = K.residual_ln_fwd(_d(x), _d(r), _d(g), _d(b), 1e-12)
        yp, _, _ = K.residual_ln_fwd(_d(x), _d(r), _d(g), _d(b), 1e-12, out_planes=True)
        return {"y": y_, "y_planes": yp.float(), "xhat": xh, "rstd": rs}
    return Case(ref, device, expect={"y": row, "y_planes": row, "xhat": row, "rstd": mask_of((rows,), 70)})


@case("residual_ln_bwd")
def _ln_bwd(value):
    """NaN in dy[r0, h0], finite saved state: row r0 of dx, column h0 of dgamma / dbeta; the fused column sums of dx see row r0 in
    every column"""
    rows, H = 77, 128
    s = (rnd(rows, H) + rnd(rows, H, seed=1)).double().requires_grad_(True)
    g64, b64 = (1 + 0.1 * rnd(H, seed=2)).double().requires_grad_(True), (0.1 * rnd(H, seed=3)).double().requires_grad_(True)
    gy, add = inject(rnd(rows, H, seed=4), (70, 5), value), rnd(rows, H, seed=5)
    F.layer_norm(s, (H,), g64, b64, 1e-12).backward(gy.double())
    dx = s.grad + add.double()
    ref = {"dx": dx, "dx_planes": dx, "dgamma": g64.grad, "dbeta": b64.grad, "dxsum": dx.sum(0)}
    row, col = mask_of((rows, H), 70), mask_of((H,), 5)
    sd = s.detach()
    mean = sd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((sd - mean) ** 2).mean(1, keepdim=True) + 1e-12)
    xhat = ((sd - mean) * rstd).float()

    def device(K):
        dg, db, bs = torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.full((H,), 7.0, device=DEV)
        a = (_d(gy), _d(xhat), _d(rstd[:, 0].float()), _d(g64.detach().float()))
        dxp = K.residual_ln_bwd(*a, dg, db, dx_add=_d(add), out_planes=True, dxsum=bs)
        dg2, db2 = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        return {"dx": K.residual_ln_bwd(*a, dg2, db2, dx_add=_d(add)), "dx_planes": dxp.float(), "dgamma": dg, "dbeta": db, "dxsum": bs}
    return Case(ref, device, expect={"dx": row, "dx_planes": row, "dgamma": col, "dbeta": col, "dxsum": torch.ones(H, dtype=torch.bool)})


AB, AH, AD = 3, 4, 32


def _attn_ref(qkv, mask, L, gc=None):
    x = qkv.double().requires_grad_(True)
    q, k, v = x.view(AB, L, 3, AH, AD).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(AD) + (1.0 - mask[:, None, None, :].double()) * torch.finfo(torch.float32).min
    p = torch.softmax(s, -1)
    ctx = (p @ v).transpose(1, 2).reshape(AB * L, AH * AD)
    if gc is None:
        return ctx.detach(), p.detach()
    ctx.backward(gc.double())
    return x.grad


def _attn_fwd(value, L, site):
    """NaN in q / k / v of a live token of sequence 1, head 2.  Masked keys: the reference's NaN row is NaN there too (softmax of a
    NaN row), the kernel may write its exact 0: loose."""
    qkv = rnd(AB * L, 3 * AH * AD, scale=0.7)
    mask = attention_mask(AB, L, True)
    b0, h0, t0, d0 = 1, 2, 3, 7
    col = {"q": 0, "k": 1, "v": 2}[site] * AH * AD + h0 * AD + d0
    qkv = inject(qkv, (b0 * L + t0, col), value)
    ctx, p = _attn_ref(qkv, mask, L)
    ref = {"ctx": ctx, "ctx_planes": ctx, "probs": p}
    ec, ep = torch.zeros(AB, L, AH, AD, dtype=torch.bool), torch.zeros(AB, AH, L, L, dtype=torch.bool)
    if site == "q":
        ec[b0, t0, h0] = True; ep[b0, h0, t0] = True
    elif site == "k":
        ec[b0, :, h0] = True; ep[b0, h0] = True
    else:
        ec[b0, :, h0, d0] = True
    masked = (mask == 0)[:, None, None, :].expand(AB, AH, L, L)

    def device(K):
        c, pr = K.attn_fwd(_d(qkv), _d(mask), AB, L, AH, AD)
        cp, _ = K.attn_fwd(_d(qkv), _d(mask), AB, L, AH, AD, out_planes=True)
        return {"ctx": c, "ctx_planes": cp.float(), "probs": pr}
    e2 = ec.reshape(AB * L, AH * AD)
    return Case(ref, device, expect={"ctx": e2, "ctx_planes": e2, "probs": ep}, loose={"probs": masked.clone()})


def _attn_bwd(value, L):
    """NaN in dctx[b0, t0, h0, d0], finite qkv / probs: dq row t0, dk every live key, dv column d0 of every live key of that sequence
    and head.  At masked keys the reference multiplies the NaN by a probability that is exactly 0: loose."""
    qkv = rnd(AB * L, 3 * AH * AD, scale=0.7)
    mask = attention_mask(AB, L, True)
    b0, h0, t0, d0 = 1, 2, 3, 7
    gc = inject(rnd(AB * L, AH * AD, seed=2), (b0 * L + t0, h0 * AD + d0), value)
    _, p = _attn_ref(qkv, mask, L)
    dqkv = _attn_ref(qkv, mask, L, gc)
    ref = {"dqkv": dqkv, "dqkv_planes": dqkv}
    e = torch.zeros(AB, L, 3, AH, AD, dtype=torch.bool)
    e[b0, t0, 0, h0] = True; e[b0, :, 1, h0] = True; e[b0, :, 2, h0, d0] = True
    lo = torch.zeros_like(e)
    dead = mask[b0] == 0
    lo[b0, dead, 1, h0] = True; lo[b0, dead, 2, h0] = True
    e, lo = e.reshape(AB * L, 3 * AH * AD), lo.reshape(AB * L, 3 * AH * AD)

    def device(K):
        qd = _d(qkv)
        pr = _d(p.float())
        return {"dqkv": K.attn_bwd(qd, pr, _d(gc), AB, L, AH, AD), "dqkv_planes": K.attn_bwd(qd, pr, _d(gc), AB, L, AH, AD, out_planes=True).float()}
    return Case(ref, device, expect={"dqkv": e, "dqkv_planes": e}, loose={"dqkv": lo, "dqkv_planes": lo}, tol={"dqkv": 5e-5, "dqkv_planes": 5e-5})


for _L in (17, 100):                  # 17: one workgroup per (sequence, head); 100: the tiled kernels
    for _s in ("q", "k", "v"):
        case(f"attn_fwd_L{_L}_{_s}", L=_L, site=_s)(_attn_fwd)
    case(f"attn_bwd_L{_L}", L=_L)(_attn_bwd)


@case("embed_bwd")
def _embed_bwd(value):
    """segmented sums over long id runs: the NaN row of one token reaches only its id's row of dword"""
    T, V, H = 300, 20, 72
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[torch.rand(T, generator=g) < 0.5] = 0
    ids[::32] = 7
    t0 = 155
    ids[t0] = 7                                          # inside the run of id 7, between the runs of ids 6 and 8 in the sorted list
    dx = rnd(T, H, seed=12)
    dx[t0] = value
    base = rnd(V, H, seed=13)
    ref = {"dword": base.double().index_add_(0, ids, dx.double())}

    def device(K):
        out = _d(base)
        K.embed_bwd(_d(ids), _d(dx), out)
        return {"dword": out}
    return Case(ref, device, expect={"dword": mask_of((V, H), 7)})


@case("elementwise_bert")
def _elementwise(value):
    """gelu_bwd, scale_mask (select at the ReLU-off position: a NaN there gives 0) and planes_add_rows"""
    n = 1000
    pre, dy = rnd(n, seed=1), inject(rnd(n, seed=2), (501,), value)
    x, src = rnd(n, seed=3), rnd(n, seed=4)
    src[10], src[20] = 1.0, -1.0
    x = inject(inject(x, (10,), value), (20,), value)
    a = torch.tensor(0.5)
    rows = rnd(16, 128, seed=5)
    rows = inject(rows, (9, 100), value)
    dst = rnd(16, 3 * 128, seed=6)
    added = dst.double().clone()
    added[:, :128] += rows.double()
    ref = {"gelu_bwd": dy.double() * _gelu_grad64(pre.double()),
           "scale_mask": torch.where(src.double() > 0, 2.0 * 0.5 * x.double(), torch.zeros(n, dtype=torch.float64)), "add_rows": added}

    def device(K):
        d = _d(dst)
        K.planes_add_rows(K.split_planes(_d(rows)), d[:, :128])
        return {"gelu_bwd": K.gelu_bwd(_d(dy), _d(pre)), "scale_mask": K.scale_mask(_d(x), _d(src), _d(a), 2.0), "add_rows": d}
    return Case(ref, device, expect={"gelu_bwd": mask_of((n,), 501), "scale_mask": mask_of((n,), 10), "add_rows": mask_of((16, 384), (9, 100))})


# ---- the four dropout entry points at p = 0.2: NaN at a kept position; dropped positions multiply the NaN by an exact 0 (loose)
DROP_P = 0.2


def _keep(site, N, L, C, nH=1):
    import dropout_ref
    return torch.from_numpy(dropout_ref.keep_mask(1234, 3, 1, site, 0, DROP_P, N, L, C, nH))


@case("embed_ln_fwd_drop")
def _embed_ln_drop(value):
    V, H, L, B = 50, 64, 8, 3
    word, pos, typ = rnd(V, H), rnd(16, H, seed=1), rnd(2, H, seed=2)
    g, b = 1 + 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    ids = torch.randint(0, V - 1, (B, L), generator=torch.Generator().manual_seed(5))
    ids[1, 3] = V - 1
    word = inject(word, (V - 1, 17), value)
    keep = _keep(0, B, L, H).view(B * L, H)
    s = 1.0 / (1.0 - float(np.float32(DROP_P)))
    y = F.layer_norm(word.double()[ids] + pos.double()[:L][None] + typ.double()[0], (H,), g.double(), b.double(), 1e-12).view(B * L, H)
    ref = {"y": y * keep.double() * s}

    def device(K):
        return {"y": K.embed_ln_fwd(_d(ids), _d(word), _d(pos), _d(typ[0]), _d(g), _d(b), 1e-12, L, drop=K.Drop(1234, 3, 1, 0, 0, DROP_P))[0]}
    return Case(ref, device, expect={"y": mask_of((B * L, H), 1 * L + 3)}, loose={"y": ~keep})


@case("residual_ln_drop")
def _ln_drop(value):
    """forward: y = LN(keep s x + res), NaN in x at a kept position; backward: NaN in dy[r0, h0] -> dx row r0, dxm = keep s dx"""
    B, L, H = 3, 8, 128
    rows = B * L
    keep = _keep(2, B, L, H).view(rows, H)
    r0 = 13
    h0 = int(keep[r0].nonzero()[0])
    s = 1.0 / (1.0 - float(np.float32(DROP_P)))
    x, r = inject(rnd(rows, H), (r0, h0), value), rnd(rows, H, seed=1)
    g, b = 1 + 0.1 * rnd(H, seed=2), 0.1 * rnd(H, seed=3)
    y = F.layer_norm(torch.where(keep, x.double() * s, torch.zeros(rows, H, dtype=torch.float64)) + r.double(), (H,), g.double(), b.double(), 1e-12)
    # backward on finite inputs
    xf = rnd(rows, H).double().requires_grad_(True)
    rf = r.double().requires_grad_(True)
    g64 = g.double().requires_grad_(True)
    sm = xf * keep.double() * s + rf
    gy = inject(rnd(rows, H, seed=4), (r0, 5), value)
    F.layer_norm(sm, (H,), g64, b.double(), 1e-12).backward(gy.double())
    smd = sm.detach()
    mean = smd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((smd - mean) ** 2).mean(1, keepdim=True) + 1e-12)
    xhat = ((smd - mean) * rstd).float()
    ref = {"y": y, "dsum": rf.grad, "dxm": xf.grad, "dgamma": g64.grad}
    row = mask_of((rows, H), r0)

    def device(K):
        drop = K.Drop(1234, 3, 1, 2, 0, DROP_P)
        yd, _, _ = K.residual_ln_fwd(_d(x), _d(r), _d(g), _d(b), 1e-12, drop=drop, rows_per_seq=L)
        dg, db = torch.empty(H, device=DEV), torch.empty(H, device=DEV)
        dsum, dxm = K.residual_ln_bwd_drop(_d(gy), _d(xhat), _d(rstd[:, 0].float()), _d(g), dg, db, drop, L)
        return {"y": yd, "dsum": dsum, "dxm": dxm, "dgamma": dg}
    return Case(ref, device, expect={"y": row, "dsum": row, "dxm": row, "dgamma": mask_of((H,), 5)}, loose={"dxm": ~keep})


@case("attn_drop")
def _attn_drop(value):
    """forward: NaN in q of a live token -> its context row (every kept key carries it) and its saved probabilities; backward: NaN in
    dctx -> dq row t0, dk of every live key, dv column d0 of the live keys the query kept"""
    L = 17
    keep = _keep(1, AB, L, L, AH)
    s = 1.0 / (1.0 - float(np.float32(DROP_P)))
    fac = keep.double() * s
    mask = attention_mask(AB, L, True)
    b0, h0, t0, d0 = 1, 2, 3, 7
    qkv = rnd(AB * L, 3 * AH * AD, scale=0.7)
    add_mask = (1.0 - mask[:, None, None, :].double()) * torch.finfo(torch.float32).min

    def fwd(xin):
        q, k, v = xin.view(AB, L, 3, AH, AD).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(AD) + add_mask, -1)
        return ((p * fac) @ v).transpose(1, 2).reshape(AB * L, AH * AD), p
    qn = inject(qkv, (b0 * L + t0, h0 * AD + d0), value)
    ctx, p = fwd(qn.double())
    xg = qkv.double().requires_grad_(True)
    cf, pf = fwd(xg)
    gc = inject(rnd(AB * L, AH * AD, seed=2), (b0 * L + t0, h0 * AD + d0), value)
    cf.backward(gc.double())
    ref = {"ctx": ctx, "probs": p, "dqkv": xg.grad}
    ec, ep = torch.zeros(AB, L, AH, AD, dtype=torch.bool), torch.zeros(AB, AH, L, L, dtype=torch.bool)
    ec[b0, t0, h0] = True; ep[b0, h0, t0] = True
    e = torch.zeros(AB, L, 3, AH, AD, dtype=torch.bool)
    e[b0, t0, 0, h0] = True; e[b0, :, 1, h0] = True; e[b0, :, 2, h0, d0] = True
    lo = torch.zeros_like(e)
    dead = mask[b0] == 0
    lo[b0, dead, 1, h0] = True
    lo[b0, dead | ~keep[b0, h0, t0], 2, h0] = True
    masked = (mask == 0)[:, None, None, :].expand(AB, AH, L, L).clone()

    def device(K):
        drop = K.Drop(1234, 3, 1, 1, 0, DROP_P)
        c, pr = K.attn_fwd(_d(qn), _d(mask), AB, L, AH, AD, drop=drop)
        return {"ctx": c, "probs": pr, "dqkv": K.attn_bwd(_d(qkv), _d(pf.detach().float()), _d(gc), AB, L, AH, AD, drop=drop)}
    return Case(ref, device, expect={"ctx": ec.reshape(AB * L, AH * AD), "probs": ep, "dqkv": e.reshape(AB * L, 3 * AH * AD)},
                loose={"probs": masked, "dqkv": lo.reshape(AB * L, 3 * AH * AD)}, tol={"dqkv": 5e-5})


# ------------------------------------------------------------------------------------------------ heads
@case("l2norm")
def _l2norm(value):
    """F.normalize: a NaN element makes its row and the row's norm NaN (the clamp to eps must not hide it)"""
    x = inject(rnd(32, 128), (21, 77), value)
    xf = rnd(32, 128).double().requires_grad_(True)
    d = inject(rnd(32, 128, seed=3), (20, 5), value)
    F.normalize(xf, dim=1).backward(d.double())
    n64 = torch.linalg.norm(x.double(), dim=1).clamp_min(1e-12)
    ref = {"xhat": F.normalize(x.double(), dim=1), "norm": n64, "dx": xf.grad}
    nf = torch.linalg.norm(xf.detach(), dim=1)

    def device(K):
        xh, nm = K.l2norm_fwd(_d(x))
        return {"xhat": xh, "norm": nm, "dx": K.l2norm_bwd(_d(d), _d((xf.detach() / nf[:, None]).float()), _d(nf.float()))}
    return Case(ref, device, expect={"xhat": mask_of((32, 128), 21), "norm": mask_of((32,), 21), "dx": mask_of((32, 128), 20)})


BLOCKS = {   # rows, cols, ld, misaligned base
    "5x13_ld16": (5, 13, 16, False),             # 16-byte body + scalar tail
    "5x13_ld16_unaligned": (5, 13, 16, True),    # scalar path
    "8x1032": (8, 1032, 1032, False),            # vector path, two 1024-column chunks
}


def _block_on_device(S, ld, off1):
    """S [rows, cols] as a view with row stride ld (base one float past a 16-byte boundary when off1) of a zero-filled buffer"""
    rows, cols = S.shape
    buf = torch.zeros(rows * ld + 4, device=DEV)
    v = buf[1 if off1 else 0:][:rows * ld].view(rows, ld)[:, :cols]
    v.copy_(S)
    return v


def _loss_heads(value, block, keyed, scaled):
    """One logits block through row statistics, the in-place gradient transform, the d theta partial sums and logit_scale_grad; the NaN
    / +Inf logit sits at [i0, j0]: lse[i0], the loss, row i0 and column j0 of the gradient, their partial sums, d theta."""
    import multipos_ref
    rows, cols, ld, off1 = BLOCKS[block]
    off = 2
    i0, j0 = rows - 2, cols - 1
    theta = math.log(1 / 0.07) if scaled else 0.0
    sc = math.exp(theta)
    S = rnd(rows, cols, scale=0.3 if scaled else 2.0)
    S = inject(S, (i0, j0), value)
    if keyed:
        kr, kc = torch.arange(rows, dtype=torch.int64) % 3, torch.arange(cols, dtype=torch.int64) % 3
    else:
        kc = torch.arange(cols, dtype=torch.int64)
        kr = kc[off:off + rows].clone()
    X = sc * S.double()
    lse, _, npos = multipos_ref.block_stats(X, kr, kc)
    eq = kr[:, None] == kc[None, :]
    pm = torch.where(eq, X, torch.zeros_like(X)).sum(1) / npos      # the positives are selected, not multiplied by a 0 / 1 mask
    lse_col = torch.logsumexp(X, 0)
    loss = ((lse - pm) * 0.25).sum()
    G = multipos_ref.block_grad(X, kr, kc, npos, lse, lse_col)
    ref = {"lse": lse, "posmean": pm, "loss": loss.reshape(1), "grad": sc * G}
    e = {"lse": mask_of((rows,), i0), "grad": mask_of((rows, cols), i0, (slice(None), j0))}
    nch = (cols + 1023) // 1024
    if scaled:
        GX = F.pad(G * X, (0, nch * 1024 - cols)).view(rows, nch, 1024).sum(2)
        ref["partials"] = GX.reshape(-1)
        ref["dtheta"] = (3.0 * 0.5 * GX.sum()).reshape(1)
        ep = torch.zeros(rows, nch, dtype=torch.bool); ep[i0] = True; ep[:, j0 // 1024] = True
        e["partials"] = ep.reshape(-1)

    def device(K):
        Sd = _block_on_device(S, ld, off1)
        lo = torch.zeros(1, device=DEV)
        th = torch.tensor(theta, device=DEV)
        lr, lc = _d(lse.float()), _d(lse_col.float())
        if scaled and keyed:
            l_, p_, n_ = K.multipos_row_stats_scaled(Sd, _d(kr), _d(kc), th, loss_out=lo, loss_scale=0.25)
            _, part = K.multipos_grad_scaled_inplace(Sd, _d(kr), _d(kc), _d(npos.float()), lr, lc, th)
        elif scaled:
            l_, p_ = K.infonce_row_lse_scaled(Sd, off, th, loss_out=lo, loss_scale=0.25)
            _, part = K.infonce_grad_scaled_inplace(Sd, off, lr, lc, th)
        elif keyed:
            l_, p_, n_ = K.multipos_row_stats(Sd, _d(kr), _d(kc), loss_out=lo, loss_scale=0.25)
            K.multipos_grad_inplace(Sd, _d(kr), _d(kc), _d(npos.float()), lr, lc)
        else:
            l_, p_ = K.infonce_row_lse(Sd, off, loss_out=lo, loss_scale=0.25)
            K.infonce_grad_inplace(Sd, off, lr, lc)
        out = {"lse": l_, "posmean": p_, "loss": lo, "grad": Sd}
        if scaled:
            out["partials"] = part
            out["dtheta"] = K.logit_scale_grad(part, None, torch.tensor(3.0, device=DEV), 0.5, torch.empty(1, device=DEV), False)
        return out
    return Case(ref, device, expect=e)


for _b in BLOCKS:
    for _keyed in (False, True):
        for _scaled in (False, True):
            case(f"{'multipos' if _keyed else 'infonce'}{'_scaled' if _scaled else ''}_{_b}", block=_b, keyed=_keyed, scaled=_scaled)(_loss_heads)


def _cos64(x, y):
    return (x / torch.linalg.norm(x, dim=1, keepdim=True)) @ (y / torch.linalg.norm(y, dim=1, keepdim=True)).T


@case("pairwise_cosine")
def _cosine(value):
    """forward: NaN in one x row and in one y row; backward: NaN in dcos[i0, p0] with finite saved state: dx row i0, dy row p0"""
    B, P, D = 70, 10, 128
    x, y = inject(rnd(B, D), (33, 100), value), inject(rnd(P, D, seed=1), (6, 2), value)
    cos = _cos64(x.double(), y.double())
    xf, yf = rnd(B, D).double().requires_grad_(True), rnd(P, D, seed=1).double().requires_grad_(True)
    cf = _cos64(xf, yf)
    dc = inject(rnd(B, P, seed=2), (33, 6), value)
    cf.backward(dc.double())
    ref = {"cos": cos, "xnorm": torch.linalg.norm(x.double(), dim=1), "ynorm": torch.linalg.norm(y.double(), dim=1), "dx": xf.grad, "dy": yf.grad}

    def device(K):
        c, xn, yn = K.pairwise_cosine_fwd(_d(x), _d(y))
        xd, yd = _d(xf.detach().float()), _d(yf.detach().float())
        cfd, xnf, ynf = K.pairwise_cosine_fwd(xd, yd)
        dx, dy = K.pairwise_cosine_bwd(xd, yd, cfd, _d(dc), xnf, ynf)
        return {"cos": c, "xnorm": xn, "ynorm": yn, "dx": dx, "dy": dy}
    return Case(ref, device, expect={"cos": mask_of((B, P), 33, (slice(None), 6)), "xnorm": mask_of((B,), 33), "ynorm": mask_of((P,), 6),
                                     "dx": mask_of((B, D), 33), "dy": mask_of((P, D), 6)})


@case("pairwise_cosine_max", values=("nan",))
def _cosine_max(value):
    """MAX_EMB head: a NaN cosine wins its group and argmax is its index, as torch.max; a NaN x row makes every group NaN with index 0"""
    B, G, Pg, D = 7, 3, 4, 128
    x, y = inject(rnd(B, D, seed=3), (5, 9), value), inject(rnd(G * Pg, D, seed=4), (1 * Pg + 2, 30), value)
    res = _cos64(x.double(), y.double()).reshape(B, G, Pg)
    mx, idx = torch.max(res, dim=2)
    ref = {"cos": res.reshape(B, G * Pg), "max": mx, "mean": res.mean(2)}
    eg = mask_of((B, G), 5, (slice(None), 1))

    def device(K):
        c, _, _, m, mean, arg = K.pairwise_cosine_max_fwd(_d(x), _d(y), G)
        return {"cos": c, "max": m, "mean": mean, "argmax_at_nan": arg[_d(eg)]}
    return Case(ref, device, expect={"cos": mask_of((B, G * Pg), 5, (slice(None), Pg + 2)), "max": eg, "mean": eg},
                exact={"argmax_at_nan": idx[eg].to(torch.int32)})


@case("bce_eval_group_patch")
def _bce_eval(value):
    B, C, D = 70, 5, 128
    cos = torch.tanh(rnd(B, 2 * C))
    cos = inject(cos, (41, 2 * 3), value)
    labels = (rnd(B, C, seed=2) > 0.5).float()
    c64 = cos.double().requires_grad_(True)
    logits = c64[:, 0::2] - c64[:, 1::2]
    loss = F.binary_cross_entropy_with_logits(logits, labels.double())
    loss.backward()
    e = inject(rnd(10 * 4, D, seed=5), (2 * 4 + 1, 17), value)
    gm = inject(rnd(10, D, seed=6), (3, 20), value)
    pat, txt = inject(rnd(225, D, seed=7), (100, 64), value), rnd(D, seed=8)
    ref = {"logits": logits.detach(), "dcos": c64.grad, "loss": loss.detach().reshape(1), "score": (cos.double()[:, 0::2] + 1) / 2,
           "group_mean": e.double().view(10, 4, D).mean(1), "group_mean_bwd": (gm.double() / 4)[:, None].expand(10, 4, D).reshape(40, D),
           "patch_sim": pat.double() @ txt.double()}
    pred = (cos[:, 0::2] > cos[:, 1::2]).float()

    def device(K):
        lg, dcos, ls = K.bce_posneg_fwd_bwd(_d(cos), _d(labels))
        sc, pr = K.eval_score(_d(cos))
        return {"logits": lg, "dcos": dcos, "loss": ls.reshape(1), "score": sc, "pred": pr, "group_mean": K.group_mean_fwd(_d(e), 10, 4),
                "group_mean_bwd": K.group_mean_bwd(_d(gm), 10, 4), "patch_sim": K.patch_similarity(_d(pat), _d(txt))}
    eb = torch.zeros(10, 4, D, dtype=torch.bool); eb[3, :, 20] = True
    return Case(ref, device, expect={"logits": mask_of((B, C), (41, 3)), "dcos": mask_of((B, 2 * C), (41, 6), (41, 7)), "loss": torch.ones(1, dtype=torch.bool),
                                     "score": mask_of((B, C), (41, 3)), "group_mean": mask_of((10, D), (2, 17)), "group_mean_bwd": eb.reshape(40, D),
                                     "patch_sim": mask_of((225,), 100)}, exact={"pred": pred})


# ------------------------------------------------------------------------------------------------ optimiser
@case("adam_sgd")
def _adam_sgd(value):
    """n = 1027: 256 float4 bodies + a scalar tail of 3; a NaN gradient element changes only its own p / m / v"""
    n = 1027
    p0, m0, v0 = rnd(n), 0.1 * rnd(n, seed=1), 0.01 * rnd(n, seed=2).abs()
    g = inject(inject(rnd(n, seed=3), (5,), value), (1025,), value)
    p = p0.double().clone().requires_grad_(True)
    f32 = lambda v: float(np.float32(v))      # the hyper-parameters as the C ABI passes them (float)
    opt = torch.optim.Adam([p], lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
    p.grad = g.double().clone()
    opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
    opt.step()
    q = p0.double().clone().requires_grad_(True)
    so = torch.optim.SGD([q], lr=f32(0.1))
    q.grad = g.double().clone()
    so.step()
    ref = {"adam_p": p.detach(), "adam_m": opt.state[p]["exp_avg"], "adam_v": opt.state[p]["exp_avg_sq"], "sgd_p": q.detach()}
    e = mask_of((n,), 5, 1025)

    def device(K):
        pd, md, vd, qd = _d(p0), _d(m0), _d(v0), _d(p0)
        K.adam_fused(pd, _d(g), md, vd, 1e-3, 0.9, 0.999, 1e-8, 0.0, 4)
        K.sgd(qd, _d(g), 0.1)
        return {"adam_p": pd, "adam_m": md, "adam_v": vd, "sgd_p": qd}
    return Case(ref, device, expect={k: e for k in ref}, tol={k: 1e-6 for k in ref})


@case("weight_reset", values=("nan",))
def _weight_reset(value):
    """Trainer.myIncremental: torch's min() / max() of |new - old| propagate the NaN, the threshold is NaN, nothing is below it:
    no element is restored.  Values (bit for bit) and the counter equal oracle.ref_step.weight_reset on the same input."""
    from oracle import ref_step
    new, old = inject(rnd(5000, seed=7), (4321,), value), rnd(5000, seed=8)
    out, cnt = ref_step.weight_reset(new, old, 0.3)
    ref = {"values": out.double()}

    def device(K):
        nd = _d(new)
        counters = torch.zeros(2, dtype=torch.int64, device=DEV)
        K.weight_reset(nd, _d(old), 0.3, counters)
        return {"values": nd, "bits": nd.view(torch.int32), "count": counters[:1]}
    return Case(ref, device, expect={"values": mask_of((5000,), 4321)},
                exact={"bits": out.view(torch.int32), "count": torch.tensor([cnt], dtype=torch.int64)}, tol={"values": 1e-30})


# ------------------------------------------------------------------------------------------------ model level (both test modules)
TEXT_CFG = dict(vocab_size=2048, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=32)
POISON_ID, POISON_COL = 2047, 5          # the word-embedding row (and column) that holds the NaN
POISON_PIXEL = (1, 0, 20, 33)            # image 1


def model_images(B=3):
    """(clean, poisoned) [B, 3, 64, 64] batches: one NaN pixel in image 1"""
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    clean = syn.synthetic_images(B, 64, seed=13)
    bad = clean.clone()
    bad[POISON_PIXEL] = float("nan")
    return clean, bad


def model_tokens(B=3):
    """(ids, mask) [B, 16]: the poisoned id is a live token of sequence 1 and of no other"""
    from incremental_multimodal_medical_learning_ii_amd import synthetic as syn
    ids, mask = syn.synthetic_tokens(B, 16, vocab=TEXT_CFG["vocab_size"], seed=8)
    ids[ids == POISON_ID] = 1
    ids[1, 2] = POISON_ID
    mask[1, 2] = 1
    return ids, mask
