"""The memory-contract helper (tests/memguard.py) against fake "kernels" written in torch on CPU tensors: each is wrong in exactly one
way that the helper must report, and the correct one must pass.  Without these the GPU cases built on it
(tests/test_memory_contract_gpu.py) could be green because the detector is broken."""
import types

import pytest
import torch

import memguard as MG

G = 1024        # guard width of these self-tests (the GPU module uses the 4 MiB default)
NP = 4          # partial rows of the fake reduction


def _raw(t: torch.Tensor, offset: int, n: int = 1) -> torch.Tensor:
    """n elements of t's storage starting `offset` elements from t's first element (may lie outside t)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + offset)


def _module():
    """a stand-in for the kernels module: `workspace` is looked up as an attribute at call time; the session buffer starts as NaN"""
    m = types.SimpleNamespace()
    buf = torch.full((1 << 12,), float("nan"))
    m.workspace = lambda nbytes, device: buf
    return m


def fake_colsum(m, x, out, bug=None):
    """out[cols] = a two-stage column sum through workspace partials, as the library's reductions are built"""
    rows, cols = x.shape
    need = NP * cols * 4
    ws = m.workspace(need, x.device)
    if ws.numel() * 4 < need:
        if bug != "ignores_size":
            raise RuntimeError("fake_colsum: workspace too small (cxrk code -2)")
        ws = torch.empty(NP * cols)                             # the bug: carries on regardless of the declared size
    part = _raw(ws, 0, NP * cols).view(NP, cols)
    per = (rows + NP - 1) // NP
    for p in range(NP):
        if bug in ("stale_part", "fmax_part") and p == NP - 1:
            continue                                            # the last partial row is never written, but is read below
        part[p] = x[p * per:(p + 1) * per].sum(0)
    if bug == "ws_plus_4":
        _raw(ws, NP * cols).fill_(0.0)                          # asked for n bytes, writes n + 4
    if bug == "fmax_part":
        acc = part[0].clone()
        for p in range(1, NP):
            acc = torch.fmax(acc, part[p])                      # the NaN-dropping maximum (fmaxf on the device)
        out.copy_(acc)
    else:
        out.copy_(part.sum(0))
    if bug == "before":
        _raw(out, -1).fill_(0.0)
    if bug == "after":
        _raw(out, out.numel()).fill_(0.0)


def fake_scale(m, x, out, bug=None):
    """out[rows, cols] (possibly pitched) = 2 x"""
    if bug == "last_row":
        out[:-1].copy_(2 * x[:-1])
    else:
        out.copy_(2 * x)
    if bug == "padding":
        _raw(out, x.shape[1]).fill_(0.0)                        # first padding column of row 0


def fake_mask(m, x, out, bug=None):
    """out (uint8) = packed sign bits, 8 columns per byte"""
    bits = (x > 0).view(x.shape[0], -1, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, dtype=torch.uint8)).sum(-1).to(torch.uint8)
    if bug == "one_byte":
        out.view(-1)[:-1].copy_(packed.view(-1)[:-1])
    else:
        out.copy_(packed)


X = torch.randn(37, 16, generator=torch.Generator().manual_seed(0))


def _colsum(bug=None, fmax=False, **kw):
    m = _module()
    ref = {"out": X.double().sum(0)}
    if fmax:                         # the buggy maximum is judged on its memory behaviour alone
        ref = None
    return MG.run_contract(lambda o: fake_colsum(m, X, o["out"], bug), {"out": MG.Out((16,))}, ref, 1e-5, module=m, guard_bytes=G, **kw)


def test_correct_kernels_pass():
    _colsum()
    m = _module()
    MG.run_contract(lambda o: fake_scale(m, X, o["y"]), {"y": MG.Out((37, 16), ld=24)}, {"y": 2 * X.double()}, 1e-6, module=m, guard_bytes=G)
    MG.run_contract(lambda o: fake_mask(m, X, o["mask"]), {"mask": MG.Out((37, 2), torch.uint8)}, module=m, guard_bytes=G)
    MG.refuses_short_workspace(lambda o: fake_colsum(m, X, o["out"]), {"out": MG.Out((16,))}, module=m, guard_bytes=G)
    with pytest.raises(AssertionError, match="at least two runs"):
        MG.run_contract(lambda o: fake_mask(m, X, o["mask"]), {"mask": MG.Out((37, 2), torch.uint8)}, module=m, guard_bytes=G, runs=("nan",))


@pytest.mark.parametrize("bug,where", [("before", "FRONT guard"), ("after", "BACK guard")])
def test_store_outside_the_payload_is_reported(bug, where):
    with pytest.raises(AssertionError, match=where):
        _colsum(bug)


def test_store_into_pitch_padding_is_reported():
    m = _module()
    with pytest.raises(AssertionError, match="pitch padding"):
        MG.run_contract(lambda o: fake_scale(m, X, o["y"], "padding"), {"y": MG.Out((37, 16), ld=24)}, module=m, guard_bytes=G)


def test_unwritten_last_row_is_reported():
    m = _module()
    with pytest.raises(AssertionError, match="never written"):
        MG.run_contract(lambda o: fake_scale(m, X, o["y"], "last_row"), {"y": MG.Out((37, 16))}, module=m, guard_bytes=G)


def test_unwritten_mask_byte_is_reported_by_the_two_sentinel_rule():
    m = _module()
    with pytest.raises(AssertionError, match="differs between workspace"):
        MG.run_contract(lambda o: fake_mask(m, X, o["mask"], "one_byte"), {"mask": MG.Out((37, 2), torch.uint8)}, module=m, guard_bytes=G)


def test_stale_workspace_read_is_reported_under_nan():
    with pytest.raises(AssertionError, match="non-finite output"):
        _colsum("stale_part", runs=("nan", "nan"))


def test_fmax_over_stale_workspace_needs_the_alternating_poison():
    _colsum("fmax_part", fmax=True, runs=("session", "nan"))            # NaN alone: swallowed by fmax, nothing to see
    with pytest.raises(AssertionError, match="differs between workspace 'session' and 'alt'"):
        _colsum("fmax_part", fmax=True)                                 # +-1e30 alternating: seen


def test_workspace_overrun_by_four_bytes_is_reported():
    with pytest.raises(AssertionError, match="workspace.*BACK guard"):
        _colsum("ws_plus_4")


def test_wrapper_that_ignores_the_declared_size_is_reported():
    m = _module()
    with pytest.raises(pytest.fail.Exception):
        MG.refuses_short_workspace(lambda o: fake_colsum(m, X, o["out"], "ignores_size"), {"out": MG.Out((16,))}, module=m, guard_bytes=G)


def test_guarded_layout():
    g = MG.Guarded((2, 5, 8), torch.bfloat16, ld=16, gap=24, guard_bytes=G)
    assert g.t.data_ptr() % 256 == 0 and g.t.stride() == (5 * 16 + 24, 16, 1)
    assert int(g.bits().view(-1)[0]) == MG._signed(MG.SENTINEL_BF16, 16)
    with pytest.raises(AssertionError, match="never written"):
        g.check()
    g.t.fill_(1.0)
    g.check()
    _raw(g.t[1], -1).fill_(0.0)                                         # the gap between the planes is guarded too
    with pytest.raises(AssertionError, match="plane gap"):
        g.check()
    assert MG.Guarded((3, 7), guard_bytes=None).guard >= 4 << 20        # default: >= 4 MiB and >= 256 rows
    assert MG.Guarded((1, 8192), guard_bytes=None).guard >= 256 * 8192 * 4
    assert MG.Guarded((1 << 21,), guard_bytes=None).guard == 4 << 20      # a long vector (a workspace) does not scale its guards
    w = MG.WorkspaceRecorder("alt", G)
    t = w(10, "cpu")
    assert t.numel() == 3 and [x > 0 for x in t.tolist()] == [True, False, True] and float(t.abs().min()) > 9e29 and w.requests == [10]
