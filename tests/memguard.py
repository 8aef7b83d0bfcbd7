"""Memory-contract helpers for the kernel tests: guard regions, sentinels, exact-size poisoned workspaces.

Plain torch ops only, so the logic runs on any device (tests/test_memguard_host.py exercises it on the CPU with deliberately
wrong fake kernels).  Nothing here provokes a fault: guards are ordinary memory owned by the test, wide enough that a whole
256-row tile of overrun stays inside them, and the short-workspace check only shrinks the *declared* size.

  Guarded                one allocation = front guard + payload (optionally pitched) + back guard, all sentinel-filled
  exact_workspace        replaces `kernels.workspace` by one that hands out exactly the bytes asked for, poisoned and guarded
  refuses_short_workspace the wrapper must raise CXRK_ERR_WS when the declared workspace size is 0, and must not touch its outputs
  run_contract           ordinary workspace / NaN poison / +-1e30 poison -> bit-identical outputs, guards and padding intact,
                         outputs fully written, values against a float64 reference
"""
from __future__ import annotations

import contextlib
import math
import re
from typing import Callable, Dict, List, Optional

import torch

SENTINEL_F32 = 0x7FC0DEAD          # NaN payloads arithmetic never produces
SENTINEL_BF16 = 0x7FDE
BYTE_SENTINELS = (0xA5, 0x5A)      # integer outputs: "fully written" = identical payloads over two different fills
GUARD_BYTES = 4 << 20
POISONS = ("nan", "alt")

_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.int32: torch.int32,
             torch.int64: torch.int64}


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


def _sentinel_bits(dtype, byte: int) -> int:
    """value of one element of the dtype's integer view that the sentinel fill produces"""
    if dtype == torch.float32:
        return _signed(SENTINEL_F32, 32)
    if dtype == torch.bfloat16:
        return _signed(SENTINEL_BF16, 16)
    if dtype == torch.uint8:
        return byte
    n = torch.empty((), dtype=dtype).element_size()
    return _signed(int.from_bytes(bytes([byte]) * n, "little"), 8 * n)


def poison_fill(t: torch.Tensor, poison: str) -> torch.Tensor:
    """nan: every element NaN.  alt: +1e30 / -1e30 alternating per element: a second poison that no operation can skip.  (The kernels
    themselves keep a NaN that they read -- ReLU, max-pool, clamps and min / max reductions compare instead of calling fmaxf / fminf,
    DESIGN.md 3.1; the row maxima of the softmax / log-sum-exp kernels still skip a NaN operand, it then arrives through the exponent.)"""
    if poison == "nan":
        t.fill_(float("nan"))
    elif poison == "alt":
        t.fill_(1e30)
        t[1::2] = -1e30
    else:
        raise ValueError(f"poison {poison!r}: expected one of {POISONS}")
    return t


class Guarded:
    """A tensor of `shape` inside one backing allocation [front guard | region | back guard].

    The payload `.t` is a view whose first element sits at a 256-byte-aligned address; its rows (last dimension) are `ld >= cols`
    elements apart, and `gap` extra elements separate the slices of the FIRST dimension (the two planes of a split-bf16 tensor
    [2, ...]).  Guards, pitch padding and gaps hold the sentinel; so does the payload until it is written or `load()`ed.
    `must_write=False` (inputs, accumulated outputs) drops the fully-written part of `check()`."""

    def __init__(self, shape, dtype=torch.float32, *, ld: Optional[int] = None, gap: int = 0, device="cpu", guard_bytes: Optional[int] = None,
                 byte_sentinel: int = BYTE_SENTINELS[0], must_write: bool = True, name: str = "tensor"):
        shape = tuple(int(s) for s in shape)
        self.name, self.dtype, self.shape, self.must_write = name, dtype, shape, must_write
        self.isz = torch.empty((), dtype=dtype).element_size()
        cols = shape[-1] if shape else 1
        self.ld = int(ld) if ld is not None else cols
        if self.ld < cols:
            raise ValueError(f"{name}: ld {self.ld} < cols {cols}")
        # contiguous strides over (..., ld), plus `gap` between slices of dim 0
        strides, acc = [], 1
        for i in range(len(shape) - 1, -1, -1):
            strides.append(acc)
            acc = acc * (self.ld if i == len(shape) - 1 else shape[i])
        strides.reverse()
        if gap and len(shape) >= 2:
            strides[0] += int(gap)
        self.strides = tuple(strides)
        numel = math.prod(shape) if shape else 1
        self.region = (sum((s - 1) * st for s, st in zip(shape, strides)) + 1) if numel > 0 else 0
        if guard_bytes is None:
            # 4 MiB, and at least a 256-row tile of a tensor that has rows (a vector's only "row" is the vector itself)
            guard_bytes = max(GUARD_BYTES, 256 * self.ld * self.isz if len(shape) >= 2 else 0)
        self.guard = (int(guard_bytes) + 255) // 256 * 256
        region_bytes = (self.region * self.isz + 255) // 256 * 256
        self.backing = torch.empty(self.guard + region_bytes + self.guard + 256, dtype=torch.uint8, device=device)
        self.off = self.guard + (-(self.backing.data_ptr() + self.guard)) % 256
        self.end = self.off + self.region * self.isz
        self.ibits = _INT_VIEW[dtype]
        self.sent = _sentinel_bits(dtype, byte_sentinel)
        self.byte_sentinel = byte_sentinel
        self._fill_sentinel()
        self.t = torch.as_strided(self._region(dtype), shape, self.strides) if numel > 0 else self._region(dtype)[:0].reshape(shape)
        if numel > 0:
            assert self.t.data_ptr() % 256 == 0
            cov = torch.zeros(self.region, dtype=torch.bool, device=device)
            torch.as_strided(cov, shape, self.strides).fill_(True)
            self.covered = cov
        else:
            self.covered = torch.zeros(0, dtype=torch.bool, device=device)

    def _region(self, dtype):
        return self.backing[self.off:self.end].view(dtype)

    def _fill_sentinel(self):
        if self.dtype in (torch.float32, torch.bfloat16):
            pat = (SENTINEL_F32 if self.dtype == torch.float32 else SENTINEL_BF16).to_bytes(self.isz, "little")
            self.backing.view(-1, self.isz).copy_(torch.tensor(list(pat), dtype=torch.uint8).to(self.backing.device))
        else:
            self.backing.fill_(self.byte_sentinel)
        # guards are compared bytewise against a pristine copy of themselves
        self._front0 = self.backing[:self.off].clone()
        self._back0 = self.backing[self.end:].clone()

    def load(self, src: torch.Tensor) -> "Guarded":
        """copy values in (an input, or the starting value of an accumulated output); drops the fully-written requirement"""
        self.t.copy_(src.to(self.t.device))
        self.must_write = False
        return self

    def data_ptr(self) -> int:
        return self.backing.data_ptr() + self.off

    def bits(self) -> torch.Tensor:
        """payload as a contiguous integer tensor of raw bits"""
        if self.t.numel() == 0:
            return torch.empty(self.shape, dtype=self.ibits, device=self.backing.device)
        return torch.as_strided(self._region(self.ibits), self.shape, self.strides).clone()

    def value(self) -> torch.Tensor:
        """payload as float64 on the CPU; a bf16 [2, ...] planes tensor gives hi + lo"""
        v = self.t.detach().cpu()
        if self.dtype == torch.bfloat16 and len(self.shape) >= 2 and self.shape[0] == 2:
            return v[0].double() + v[1].double()
        return v.double()

    def check(self, written: Optional[bool] = None) -> None:
        """(a) guards untouched, (b) padding / gaps untouched, (c) no sentinel left in a payload that had to be fully written"""
        nm = self.name
        ne = self.backing[:self.off] != self._front0
        if bool(ne.any()):
            bad = ne.nonzero()
            raise AssertionError(f"{nm}: {bad.numel()} byte(s) of the FRONT guard overwritten, nearest {self.off - int(bad.max())} B before the payload")
        ne = self.backing[self.end:] != self._back0
        if bool(ne.any()):
            bad = ne.nonzero()
            raise AssertionError(f"{nm}: {bad.numel()} byte(s) of the BACK guard overwritten, first {int(bad.min())} B past the payload")
        if self.region == 0:
            return
        raw = self._region(self.ibits)
        hit = (raw != self.sent) & ~self.covered
        assert not bool(hit.any()), f"{nm}: {int(hit.sum())} element(s) of pitch padding / plane gap overwritten, first at region offset {int(hit.nonzero()[0])} (ld {self.ld})"
        if self.must_write if written is None else written:
            if self.dtype in (torch.float32, torch.bfloat16):
                left = (raw == self.sent) & self.covered
                assert not bool(left.any()), f"{nm}: {int(left.sum())} payload element(s) never written, first at region offset {int(left.nonzero()[0])} (shape {self.shape}, ld {self.ld})"


class _ShortWs:
    """What `refuses_short_workspace` hands the wrappers: a valid, fully backed address with a declared length of zero."""

    def __init__(self, g: Guarded):
        self.g = g

    def numel(self) -> int:
        return 0

    def data_ptr(self) -> int:
        return self.g.data_ptr()


class WorkspaceRecorder:
    """Stand-in for `kernels.workspace`: every request gets a fresh float32 buffer of exactly ceil(nbytes / 4) elements between guards,
    pre-filled with the poison."""

    def __init__(self, poison: str, guard_bytes: Optional[int] = None, short: bool = False, misalign: bool = False):
        self.poison, self.guard_bytes, self.short, self.misalign = poison, guard_bytes, short, misalign
        self.requests: List[int] = []
        self.bufs: List[Guarded] = []

    def __call__(self, nbytes: int, device):
        n = (int(nbytes) + 3) // 4 + int(self.misalign)
        g = Guarded((n,), torch.float32, device=device, guard_bytes=self.guard_bytes, must_write=False, name=f"workspace[{len(self.bufs)}] of {nbytes} B")
        if n:
            poison_fill(g.t, self.poison)
        self.requests.append(int(nbytes))
        self.bufs.append(g)
        if self.misalign:                # full size, 4 bytes off the 256-byte boundary
            return g.t[1:]
        return _ShortWs(g) if self.short else g.t

    def check(self) -> None:
        for g in self.bufs:
            g.check()


def _kernels_module():
    from incremental_multimodal_medical_learning_ii_amd import kernels
    return kernels


def exact_workspace(monkeypatch, poison: str, module=None, guard_bytes: Optional[int] = None, short: bool = False,
                    misalign: bool = False) -> WorkspaceRecorder:
    """Patch `module.workspace` (default: the package's kernels module, which looks it up as a global at call time)."""
    rec = WorkspaceRecorder(poison, guard_bytes, short, misalign)
    monkeypatch.setattr(module if module is not None else _kernels_module(), "workspace", rec)
    return rec


@contextlib.contextmanager
def _patched(poison, module, guard_bytes, short=False, misalign=False):
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        yield exact_workspace(mp, poison, module, guard_bytes, short, misalign)


class Out:
    """Specification of one output of a guarded call.  `init`: starting value (accumulated outputs, in-place operands): reloaded
    before every run, and the fully-written check does not apply.  `written=False`: the call leaves part of it untouched on purpose."""

    def __init__(self, shape, dtype=torch.float32, *, ld=None, gap=0, init: Optional[torch.Tensor] = None, written: bool = True):
        self.shape, self.dtype, self.ld, self.gap, self.init, self.written = tuple(shape), dtype, ld, gap, init, written

    def make(self, name, device, guard_bytes, byte_sentinel) -> Guarded:
        g = Guarded(self.shape, self.dtype, ld=self.ld, gap=self.gap, device=device, guard_bytes=guard_bytes, byte_sentinel=byte_sentinel,
                    must_write=self.written, name=name)
        if self.init is not None:
            g.load(self.init)
        return g


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref| (the measure of tests/test_kernels_gpu.py's close())"""
    ref = ref.double().cpu()
    got = got.double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-20))


def run_contract(call: Callable[[Dict[str, torch.Tensor]], None], outputs: Dict[str, Out], reference=None, tol=None, *, module=None,
                 device="cpu", guard_bytes: Optional[int] = None, runs=("session", "nan", "alt"), report: Optional[list] = None):
    """Run `call(outs)` (outs: name -> guarded payload view) once through the ordinary workspace and once per poison through an
    exact-size guarded workspace.  Asserts: guards / padding of every output and workspace intact; float outputs fully written;
    all runs bit-identical (which is also what shows an integer output fully written: its fill differs between runs); values
    within `tol` (scalar or name -> bound; relative to the reference's largest magnitude) of `reference` (name -> tensor, float64)."""
    module = module if module is not None else _kernels_module()
    if any(spec.dtype not in (torch.float32, torch.bfloat16) for spec in outputs.values()):
        assert len(runs) >= 2, "an integer output is shown fully written by two fills: at least two runs are needed"
    results = []
    for i, mode in enumerate(runs):
        outs = {n: spec.make(n, device, guard_bytes, BYTE_SENTINELS[0] if i < len(runs) - 1 else BYTE_SENTINELS[1]) for n, spec in outputs.items()}
        views = {n: g.t for n, g in outs.items()}
        if mode == "session":
            call(views)
            rec = None
        else:
            with _patched(mode, module, guard_bytes) as rec:
                call(views)
        for g in outs.values():
            try:
                g.check()
            except AssertionError as e:
                raise AssertionError(f"[workspace: {mode}] {e}") from None
        if rec is not None:
            try:
                rec.check()
            except AssertionError as e:
                raise AssertionError(f"[workspace: {mode}] {e}") from None
        results.append((mode, outs, {n: g.bits() for n, g in outs.items()}))
    m0, outs0, bits0 = results[0]
    for mode, _, bits in results[1:]:
        for n in outputs:
            same = torch.equal(bits0[n], bits[n])
            assert same, (f"{n}: differs between workspace '{m0}' and '{mode}' in {int((bits0[n] != bits[n]).sum())} of {bits[n].numel()} element(s): "
                          f"the call reads memory it did not write, or leaves output unwritten")
    if reference is not None:
        ref = reference(outs0) if callable(reference) else reference
        for n, r in ref.items():
            bound = tol[n] if isinstance(tol, dict) else tol
            err = rel_err(outs0[n].value(), r)
            if report is not None:
                report.append((n, err, bound))
            assert err < bound, f"{n}: rel-to-max err {err:.3e} (tol {bound})"
    return outs0


def _refuses(call, outputs, module, device, guard_bytes, misaligned):
    import pytest
    module = module if module is not None else _kernels_module()
    outs = {n: Out(s.shape, s.dtype, ld=s.ld, gap=s.gap).make(n, device, guard_bytes, BYTE_SENTINELS[0]) for n, s in outputs.items()}
    before = {n: g.backing.clone() for n, g in outs.items()}
    with _patched("nan", module, guard_bytes, short=not misaligned, misalign=misaligned) as rec:
        with pytest.raises((ValueError if misaligned else RuntimeError), match=re.escape("cxrk code -1" if misaligned else "cxrk code -2")):
            call({n: g.t for n, g in outs.items()})
    assert rec.requests and max(rec.requests) > 0, "the call asked for no workspace: nothing was refused"
    for n, g in outs.items():
        assert torch.equal(g.backing, before[n]), f"{n}: written although the workspace was refused"
    rec.check()
    for g in rec.bufs:
        if g.region:
            assert bool(torch.isnan(g.t).all()), "workspace written although it was refused"


def refuses_short_workspace(call: Callable[[Dict[str, torch.Tensor]], None], outputs: Dict[str, Out], *, module=None, device="cpu",
                            guard_bytes: Optional[int] = None) -> None:
    """The same wrapper call with the declared workspace size forced to 0 (the address stays valid and fully backed, so nothing
    can be overrun even if the library did launch): the wrapper must raise from CXRK_ERR_WS (code -2) and leave the outputs alone."""
    _refuses(call, outputs, module, device, guard_bytes, False)


def refuses_misaligned_workspace(call: Callable[[Dict[str, torch.Tensor]], None], outputs: Dict[str, Out], *, module=None, device="cpu",
                                 guard_bytes: Optional[int] = None) -> None:
    """A workspace of the full size, 4 bytes off the 256-byte boundary include/cxrk.h asks for: bad argument (code -1), outputs and
    workspace untouched."""
    _refuses(call, outputs, module, device, guard_bytes, True)
