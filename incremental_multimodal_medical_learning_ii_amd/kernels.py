"""Tensor-level wrappers over the cxrk C-ABI (one Python function per entry point family).

PyTorch is plumbing here: it owns device memory (caching allocator) and the current HIP stream.  Every function
checks that its operands are CUDA(HIP) fp32 tensors laid out as the kernel expects and raises otherwise; nothing
falls back to torch arithmetic.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import check

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
AUX_NONE, AUX_RELU_MASK, AUX_GELU_GRAD, AUX_MASK_BITS = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the GPU (the cxrk path has no CPU fallback), got "
                         f"{type(t).__name__} on {getattr(t, 'device', None)}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def _chk_out(t, shape, name: str, dtype=torch.float32):
    """a caller-provided output (`out=`): fp32 tensor (contiguous columns; rows may be strided) or contiguous Planes of `shape`"""
    if isinstance(t, Planes):
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous Planes of shape {tuple(shape)}, got {tuple(t.shape)}")
        return t
    _chk(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor of shape {tuple(shape)}, got {tuple(t.shape)} strides {t.stride()}")
    return t


def _rowmajor2d(t: torch.Tensor, name: str) -> Tuple[torch.Tensor, int]:
    _chk(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name}: expected 2-D, got shape {tuple(t.shape)}")
    if t.shape[1] != 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


class Planes:
    """A tensor in split-bf16 storage: `t` is a bf16 tensor [2, *shape] — plane 0 = bf16(x), plane 1 = bf16(x - plane 0) — i.e. the
    same 4 bytes per element as fp32, x ~ hi + lo to ~2^-17 relative.  It is the activation / weight format of the encoders in
    split-bf16 mode: the MFMA mainloops load the planes as they are (no conversion work), see csrc/gemm_loaders.h."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        if t.dtype != torch.bfloat16 or t.dim() < 2 or t.shape[0] != 2 or not t.is_cuda:
            raise ValueError(f"Planes: expected a bf16 GPU tensor [2, ...], got {t.dtype} {tuple(t.shape)} on {t.device}")
        self.t = t

    @staticmethod
    def empty(*shape, device) -> "Planes":
        return Planes(torch.empty((2,) + tuple(shape), dtype=torch.bfloat16, device=device))

    @staticmethod
    def zeros(*shape, device) -> "Planes":
        return Planes(torch.zeros((2,) + tuple(shape), dtype=torch.bfloat16, device=device))

    @property
    def shape(self):
        return self.t.shape[1:]

    @property
    def device(self):
        return self.t.device

    @property
    def plane(self) -> int:
        """distance between the hi and the lo plane, in elements"""
        return self.t.stride(0)

    def ptr(self) -> int:
        return self.t.data_ptr()

    def numel(self) -> int:
        return self.t.numel() // 2

    def view(self, *shape) -> "Planes":
        return Planes(self.t.view((2,) + tuple(shape)))

    def rows(self, sl) -> "Planes":
        """row slice / strided row view of a 2-D planes tensor"""
        return Planes(self.t[:, sl])

    def is_contiguous(self) -> bool:
        return self.t[0].is_contiguous()

    def float(self) -> torch.Tensor:
        """fp32 value hi + lo (host-side consumers, tests)"""
        if self.is_contiguous() and self.numel() % 8 == 0:
            out = torch.empty(tuple(self.shape), dtype=torch.float32, device=self.t.device)
            check(_lib.load().cxrk_merge_planes(self.ptr(), self.plane, self.numel(), _p(out), _stream()), "cxrk_merge_planes")
            return out
        return self.t[0].float() + self.t[1].float()


def split_planes(x: torch.Tensor, out: Optional[Planes] = None) -> Planes:
    """fp32 tensor -> its split-bf16 planes (numel % 8 == 0, contiguous)."""
    _chk(x, "split_planes.x")
    x = x.contiguous()
    if out is None:
        out = Planes.empty(*x.shape, device=x.device)
    check(_lib.load().cxrk_split_planes(_p(x), x.numel(), out.ptr(), out.plane, _stream()), "cxrk_split_planes")
    return out


def _pl2d(t: Planes, name: str):
    """(pointer, row stride, plane stride) of a 2-D planes operand with contiguous columns"""
    if not isinstance(t, Planes) or len(t.shape) != 2:
        raise ValueError(f"{name}: expected a 2-D Planes tensor")
    v = t.t
    if v.shape[2] != 1 and v.stride(2) != 1:
        raise ValueError(f"{name}: planes columns must be contiguous")
    return v.data_ptr(), (v.stride(1) if v.shape[1] > 1 else max(v.shape[2], v.stride(1))), v.stride(0)


class LaunchProfiler:
    """Optional per-launch timing of the MFMA GEMM family with HIP events recorded on the launch stream
    (bench.py's `roofline` object).  Off by default; when on, every GEMM / implicit-GEMM entry point is bracketed by two
    events and tagged with its algorithmic FLOPs (2*M*N*K), its algorithmic HBM bytes (every operand and side input read once,
    every output written once) and what the library says it launched (`cxrk_last_launch_label` / `_count` / `_split_bf16`): the
    kernel instantiation under the name rocprofv3 reports (scripts/pmc_summary_key.py), the number of MFMA launches, and the
    mainloop's number format.  Tile choice and kernel names exist in the library only (csrc/gemm_dispatch.h)."""

    PEAK_BF16X3, PEAK_F32, PEAK_HBM = 2500e12 / 3.0, 157.3e12, 8.0e12   # /opt/skills/guides/MI355X_MICROARCH.md (bench.py's constants)

    def __init__(self):
        self.on = False
        self.rows = []  # [key, flops, bytes, start_event, end_event, MFMA launches inside the bracket, split-bf16 mainloop]

    def start(self):
        self.on, self.rows = True, []

    def stop(self):
        self.on = False

    def bracket(self, flops: float, nbytes: float = 0.0):
        """Opens a row in front of a library call; `end` closes it.  None when the profiler is off."""
        if not self.on:
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        row = [None, flops, nbytes, a, b, 0, False]
        self.rows.append(row)
        return row

    def end(self, row):
        """Behind the library call, on the thread that made it (the library's launch record is per thread)."""
        if row is None:
            return
        row[4].record()
        lib = _lib.load()
        row[0], row[5], row[6] = lib.cxrk_last_launch_label().decode(), lib.cxrk_last_launch_count(), bool(lib.cxrk_last_launch_split_bf16())

    def summary(self):
        """{kernel: {"launches", "flops", "bytes", "ms"}} — call after torch.cuda.synchronize()."""
        out = {}
        for key, flops, nbytes, a, b, sub, split in self.rows:
            d = out.setdefault(key, {"launches": 0, "flops": 0.0, "bytes": 0.0, "ms": 0.0, "floor_ms": 0.0})
            d["launches"] += sub
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += a.elapsed_time(b)
            # the launch's own binding roof: max(FLOPs / MFMA peak of its mainloop, algorithmic bytes / HBM peak)
            d["floor_ms"] += 1e3 * max(flops / (self.PEAK_BF16X3 if split else self.PEAK_F32), nbytes / self.PEAK_HBM)
        return out


profiler = LaunchProfiler()


class _Workspace:
    """Grow-on-demand scratch buffer per device and stream; reuse is safe because kernels of one stream run in order."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        # one buffer per (device, stream): the two encoders of the joint step run on two streams
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() * 4 < nbytes:
            n = max(int(nbytes * 1.25) // 4 + 64, 1 << 20)
            buf = torch.empty(n, dtype=torch.float32, device=device)
            self.bufs[key] = buf
        return buf


_ws = _Workspace()


def workspace(nbytes: int, device) -> torch.Tensor:
    return _ws.get(nbytes, device)


# ----------------------------------------------------------------------------------------------------------------
# GEMM family
# ----------------------------------------------------------------------------------------------------------------

def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, trans_a: bool, trans_b: bool,
         bias=None, residual=None, aux=None, auxmode: int = 0, preact_out=None, act: int = 0, alpha: float = 1.0,
         accumulate: bool = False, splitk: int = 1) -> torch.Tensor:
    lib = _lib.load()
    a, lda = _rowmajor2d(a, "gemm.a")
    b, ldb = _rowmajor2d(b, "gemm.b")
    _chk(out, "gemm.out")
    if out.dim() != 2 or out.stride(1) != 1:
        raise ValueError("gemm.out must be a row-major 2-D tensor")
    ldc = out.stride(0)
    ldr = ldaux = ldc2 = 0
    if residual is not None:
        residual, ldr = _rowmajor2d(residual, "gemm.residual")
    if aux is not None:
        aux, ldaux = _rowmajor2d(aux, "gemm.aux")
    if preact_out is not None:
        _chk(preact_out, "gemm.preact_out")
        ldc2 = preact_out.stride(0)
    if bias is not None:
        _chk(bias, "gemm.bias")
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError("gemm.bias must be contiguous with N elements")
    ws = None
    wsb = 0
    if splitk > 1:
        wsb = lib.cxrk_gemm_splitk_ws_bytes(M, N, splitk)
        ws = workspace(wsb, out.device)
        wsb = ws.numel() * 4
    ev = profiler.bracket(2.0 * M * N * K,
                          4.0 * (M * K + N * K + M * N * (1 + (residual is not None) + (aux is not None) + (preact_out is not None)
                                                       + int(bool(accumulate))))) if profiler.on else None
    rc = lib.cxrk_gemm_f32(int(trans_a), int(trans_b), M, N, K, _p(a), lda, _p(b), ldb, _p(out), ldc, _p(bias),
                           _p(residual), ldr, _p(aux), ldaux, auxmode, _p(preact_out), ldc2, act, float(alpha),
                           int(accumulate), int(splitk), _p(ws), wsb, _stream())
    profiler.end(ev)
    check(rc, f"cxrk_gemm_f32(M={M},N={N},K={K},tA={trans_a},tB={trans_b})")
    return out


def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias=None, act: int = 0, residual=None, preact_out=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = act(x[M,K] @ w[N,K]^T + bias + residual)."""
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_fwd: x is [{M},{K}] but w is {tuple(w.shape)}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    return gemm(x, w, out, M, N, K, False, True, bias=bias, residual=residual, preact_out=preact_out, act=act)


def linear_bwd_data(dy: torch.Tensor, w: torch.Tensor, aux=None, auxmode: int = 0, residual=None,
                    out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """dx[M,K] = (dy[M,N] @ w[N,K] + residual) (* mask/gelu'(aux))."""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    return gemm(dy, w, out, M, K, N, False, False, aux=aux, auxmode=auxmode, residual=residual, accumulate=accumulate)


def _wgrad_splitk(n_out: int, n_in: int, rows: int, planes: bool = False) -> int:
    return int(_lib.load().cxrk_gemm_wgrad_splitk(n_out, n_in, rows, int(planes)))


def linear_bwd_weight(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]  (deterministic split-K over M)."""
    M, N = dy.shape
    K = x.shape[1]
    sk = _wgrad_splitk(N, K, M)
    if sk > 1:
        return gemm(dy, x, dw, N, K, M, True, False, accumulate=accumulate, splitk=sk)
    return gemm(dy, x, dw, N, K, M, True, False, accumulate=accumulate)


def gemm_pl(a: Planes, b: Planes, M: int, N: int, K: int, trans_a: bool, trans_b: bool, out=None, bias=None, residual=None,
            aux=None, auxmode: int = 0, maskin=None, maskout=None, preact_out=None, act: int = 0, alpha: float = 1.0,
            accumulate: bool = False, splitk: int = 1, colsum=None, colsum_accumulate: bool = False):
    """The GEMM family on planes operands.  `out`: fp32 tensor or Planes (row-major [M, N]); `residual`: fp32 tensor or Planes;
    `aux` (auxmode 2): fp32 pre-activation for gelu'; `maskin` (auxmode 3) / `maskout` (with ReLU): uint8 bit masks [M, N/8];
    `colsum` ([N], optional, splitk == 1): receives (accumulates) the column sums of the stored output, reduced in the epilogue."""
    lib = _lib.load()
    ap, lda, apl = _pl2d(a, "gemm_pl.a")
    bp, ldb, bpl = _pl2d(b, "gemm_pl.b")
    C = Cp = None
    cpl = 0
    if isinstance(out, Planes):
        Cp, ldc, cpl = _pl2d(out, "gemm_pl.out")
    else:
        _chk(out, "gemm_pl.out")
        if out.dim() != 2 or out.stride(1) != 1:
            raise ValueError("gemm_pl.out must be a row-major 2-D tensor")
        C, ldc = out.data_ptr(), out.stride(0)
    R = Rp = None
    ldr = rpl = 0
    if isinstance(residual, Planes):
        Rp, ldr, rpl = _pl2d(residual, "gemm_pl.residual")
    elif residual is not None:
        residual, ldr = _rowmajor2d(residual, "gemm_pl.residual")
        R = residual.data_ptr()
    ldaux = ldc2 = ldmi = ldmo = 0
    if aux is not None:
        aux, ldaux = _rowmajor2d(aux, "gemm_pl.aux")
    if preact_out is not None:
        _chk(preact_out, "gemm_pl.preact_out")
        ldc2 = preact_out.stride(0)
    if maskin is not None:
        _chk(maskin, "gemm_pl.maskin", torch.uint8)
        ldmi = maskin.stride(0)
    if maskout is not None:
        _chk(maskout, "gemm_pl.maskout", torch.uint8)
        ldmo = maskout.stride(0)
    if bias is not None:
        _chk(bias, "gemm_pl.bias")
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError("gemm_pl.bias must be contiguous with N elements")
    ws, wsb = None, 0
    if splitk > 1:
        wsb = lib.cxrk_gemm_splitk_ws_bytes(M, N, splitk)
        ws = workspace(wsb, a.device)
        wsb = ws.numel() * 4
    elif colsum is not None:
        _chk(colsum, "gemm_pl.colsum")
        if colsum.numel() != N or not colsum.is_contiguous():
            raise ValueError("gemm_pl.colsum must be contiguous with N elements")
        ws = workspace(lib.cxrk_gemm_pl_colsum_ws_bytes(M, N), a.device)
        wsb = ws.numel() * 4
    if colsum is not None and splitk > 1:
        raise ValueError("gemm_pl: fused column sums need splitk == 1")
    ev = profiler.bracket(2.0 * M * N * K,
                          4.0 * (M * K + N * K + M * N * (1 + (residual is not None) + (aux is not None) + (preact_out is not None)
                                                       + int(bool(accumulate)))) + M * N / 8.0 * ((maskin is not None) + (maskout is not None))) if profiler.on else None
    rc = lib.cxrk_gemm_pl(int(trans_a), int(trans_b), M, N, K, ap, lda, apl, bp, ldb, bpl, C, Cp, ldc, cpl, _p(bias), R, Rp, ldr, rpl,
                          _p(aux), ldaux, auxmode, _p(maskin), ldmi, _p(maskout), ldmo, _p(preact_out), ldc2, act, float(alpha),
                          int(accumulate), int(splitk), _p(colsum), int(colsum_accumulate), _p(ws), wsb, _stream())
    profiler.end(ev)
    check(rc, f"cxrk_gemm_pl(M={M},N={N},K={K},tA={trans_a},tB={trans_b})")
    return out


def linear_fwd_pl(x: Planes, w: Planes, bias=None, act: int = 0, residual=None, preact_out=None, out=None, out_planes: bool = False,
                  maskout=None):
    """y[M,N] = act(x[M,K] @ w[N,K]^T + bias + residual); y as fp32 (default) or Planes."""
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear_fwd_pl: x is [{M},{K}] but w is {tuple(w.shape)}")
    if out is None:
        out = Planes.empty(M, N, device=x.device) if out_planes else torch.empty(M, N, dtype=torch.float32, device=x.device)
    return gemm_pl(x, w, M, N, K, False, True, out=out, bias=bias, residual=residual, preact_out=preact_out, act=act, maskout=maskout)


def linear_bwd_data_pl(dy: Planes, w: Planes, aux=None, auxmode: int = 0, maskin=None, residual=None, out=None,
                       out_planes: bool = False, accumulate: bool = False, colsum=None, colsum_accumulate: bool = False):
    """dx[M,K] = (dy[M,N] @ w[N,K] + residual) (* gelu'(aux) | * mask bits); `colsum` ([K], optional) receives the column sums of dx
    (the bias gradient of the layer that produced this layer's input) from the same epilogue."""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = Planes.empty(M, K, device=dy.device) if out_planes else torch.empty(M, K, dtype=torch.float32, device=dy.device)
    if maskin is not None:
        auxmode = AUX_MASK_BITS
    return gemm_pl(dy, w, M, K, N, False, False, out=out, aux=aux, auxmode=auxmode, maskin=maskin, residual=residual, accumulate=accumulate,
                   colsum=colsum, colsum_accumulate=colsum_accumulate)


def linear_bwd_weight_pl(dy: Planes, x: Planes, dw: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]  (deterministic split-K over M); dw fp32."""
    M, N = dy.shape
    K = x.shape[1]
    sk = _wgrad_splitk(N, K, M, planes=True)
    return gemm_pl(dy, x, N, K, M, True, False, out=dw, accumulate=accumulate, splitk=sk if sk > 1 else 1)


def colsum_pl(x: Planes, out: torch.Tensor, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    lib = _lib.load()
    xp, ldx, xpl = _pl2d(x, "colsum_pl.x")
    _chk(out, "colsum_pl.out")
    rows, cols = x.shape
    ws = workspace(lib.cxrk_colsum_ws_bytes(rows, cols), x.device)
    check(lib.cxrk_colsum_pl(xp, ldx, xpl, rows, cols, _p(out), float(alpha), int(accumulate), _p(ws), ws.numel() * 4, _stream()),
          "cxrk_colsum_pl")
    return out


def colsum(x: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    if isinstance(x, Planes):
        return colsum_pl(x, out, alpha, accumulate)
    lib = _lib.load()
    x, ldx = _rowmajor2d(x, "colsum.x")
    _chk(out, "colsum.out")
    rows, cols = x.shape
    wsb = lib.cxrk_colsum_ws_bytes(rows, cols)
    ws = workspace(wsb, x.device)
    check(lib.cxrk_colsum(_p(x), ldx, rows, cols, _p(out), float(alpha), int(accumulate), _p(ws), ws.numel() * 4,
                          _stream()), "cxrk_colsum")
    return out


def colvar(x, mean: torch.Tensor, out: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """out[c] = alpha * sum_r (x[r, c] - mean[c])^2 for a 2-D fp32 tensor or Planes (second pass of a two-pass batch variance)."""
    lib = _lib.load()
    if isinstance(x, Planes):
        xp, ldx, xpl = _pl2d(x, "colvar.x")
        rows, cols = x.shape
    else:
        x, ldx = _rowmajor2d(x, "colvar.x")
        xp, xpl = x.data_ptr(), 0
        rows, cols = x.shape
    _chk(mean, "colvar.mean")
    _chk(out, "colvar.out")
    if mean.numel() != cols or out.numel() != cols or not mean.is_contiguous() or not out.is_contiguous():
        raise ValueError(f"colvar: mean / out must be contiguous with {cols} elements")
    ws = workspace(lib.cxrk_colsum_ws_bytes(rows, cols), out.device)
    check(lib.cxrk_colvar(xp, ldx, xpl, rows, cols, _p(mean), _p(out), float(alpha), _p(ws), ws.numel() * 4, _stream()), "cxrk_colvar")
    return out


# ---- train-mode BatchNorm2d around the convolutions (csrc/bn_train.hip) ------------------------------------------------------------

def _fmt(t, name: str):
    """(pointer, plane stride) of a contiguous fp32 tensor (plane 0) or Planes tensor"""
    if isinstance(t, Planes):
        if not t.is_contiguous():
            raise ValueError(f"{name}: planes tensor must be contiguous")
        return t.ptr(), t.plane
    _chk(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr(), 0


def _vec(t: torch.Tensor, C: int, name: str) -> torch.Tensor:
    _chk(t, name)
    if t.numel() != C or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous vector of {C} elements, got {tuple(t.shape)}")
    return t


def colstats(x, unbiased: bool = False, out=None):
    """(mean[C], var[C]) over the rows of x ([..., C] fp32 or Planes, C % 8 == 0) in one pass; var biased (1 / n) or unbiased (1 / (n - 1)).
    `out`: optional (mean, var) pair to write into."""
    lib = _lib.load()
    C = x.shape[-1]
    rows = x.numel() // C
    xp, xpl = _fmt(x, "colstats.x")
    if out is None:
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        var = torch.empty(C, dtype=torch.float32, device=x.device)
    else:
        mean, var = _vec(out[0], C, "colstats.mean"), _vec(out[1], C, "colstats.var")
    ws = workspace(2 * lib.cxrk_coldot_ws_bytes(rows, C), x.device)
    check(lib.cxrk_colstats(xp, xpl, rows, C, _p(mean), _p(var), 1.0 / max(1, rows - 1) if unbiased else 1.0 / rows, _p(ws), ws.numel() * 4,
                            _stream()), f"cxrk_colstats(rows={rows},C={C})")
    return mean, var


def bn_train_fwd_coeffs(mean, var, gamma, beta, eps: float, n: int, momentum: float = 0.0, rmean=None, rvar=None):
    """(scale, shift, rstd) of a train-mode BatchNorm from its batch statistics (var: biased); updates the running statistics in place
    (r = (1 - momentum) r + momentum stat, unbiased variance) when given."""
    lib = _lib.load()
    C = mean.numel()
    for nme, t in (("mean", mean), ("var", var), ("gamma", gamma), ("beta", beta)):
        _vec(t, C, "bn_train." + nme)
    scale, shift, rstd = (torch.empty(C, dtype=torch.float32, device=mean.device) for _ in range(3))
    if rmean is not None:
        _vec(rmean, C, "bn_train.running_mean")
        _vec(rvar, C, "bn_train.running_var")
    check(lib.cxrk_bn_train_fwd_coeffs(_p(mean), _p(var), _p(gamma), _p(beta), float(eps), int(n), float(momentum), _p(scale), _p(shift),
                                       _p(rstd), _p(rmean), _p(rvar), C, _stream()), "cxrk_bn_train_fwd_coeffs")
    return scale, shift, rstd


def bn_apply(z, scale, shift, residual=None, relu: bool = True, want_mask: bool = False):
    """y = relu?(z * scale + shift + residual?) in z's storage format ([..., C], C % 8 == 0); mask: ReLU decision bits [rows, C / 8]."""
    lib = _lib.load()
    C = z.shape[-1]
    rows = z.numel() // C
    zp, zpl = _fmt(z, "bn_apply.z")
    if isinstance(z, Planes):
        y = Planes.empty(*z.shape, device=z.device)
    else:
        y = torch.empty_like(z)
    yp, ypl = _fmt(y, "bn_apply.y")
    rp, rpl = _fmt(residual, "bn_apply.residual") if residual is not None else (None, 0)
    if residual is not None and tuple(residual.shape) != tuple(z.shape):
        raise ValueError(f"bn_apply: residual {tuple(residual.shape)} vs z {tuple(z.shape)}")
    mask = torch.empty(rows, C // 8, dtype=torch.uint8, device=z.device) if (want_mask and relu) else None
    check(lib.cxrk_bn_apply(zp, zpl, _p(_vec(scale, C, "bn_apply.scale")), _p(_vec(shift, C, "bn_apply.shift")), rp, rpl, yp, ypl, _p(mask),
                            rows, C, int(relu), _stream()), f"cxrk_bn_apply(rows={rows},C={C})")
    return y, mask


def coldot(a, b, bshift=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[c] = sum_rows a[r, c] * (b[r, c] - bshift[c]); a, b: [..., C] fp32 or Planes (formats may differ); bshift: fp32 [C] or None."""
    lib = _lib.load()
    C = a.shape[-1]
    rows = a.numel() // C
    if b.shape[-1] != C or b.numel() != a.numel():
        raise ValueError(f"coldot: {tuple(a.shape)} vs {tuple(b.shape)}")
    ap, apl = _fmt(a, "coldot.a")
    bp, bpl = _fmt(b, "coldot.b")
    out = torch.empty(C, dtype=torch.float32, device=a.device) if out is None else _vec(out, C, "coldot.out")
    ws = workspace(lib.cxrk_coldot_ws_bytes(rows, C), a.device)
    check(lib.cxrk_coldot(ap, apl, bp, bpl, _p(_vec(bshift, C, "coldot.bshift")) if bshift is not None else None, rows, C, _p(out), _p(ws), ws.numel() * 4, _stream()), "cxrk_coldot")
    return out


def bn_train_bwd_coeffs(gamma, mean, rstd, sumdy, dot, n: int, dgamma, dbeta, accumulate: bool):
    """dot = sum dy (z - mean) (coldot(dy, z, mean)); dgamma (+)= rstd dot, dbeta (+)= sumdy; returns (A, B, Cc), dz = A dy + B + Cc z."""
    lib = _lib.load()
    C = gamma.numel()
    for nme, t in (("gamma", gamma), ("mean", mean), ("rstd", rstd), ("sumdy", sumdy), ("dot", dot), ("dgamma", dgamma), ("dbeta", dbeta)):
        _vec(t, C, "bn_train_bwd." + nme)
    A, B, Cc = (torch.empty(C, dtype=torch.float32, device=gamma.device) for _ in range(3))
    check(lib.cxrk_bn_train_bwd_coeffs(_p(gamma), _p(mean), _p(rstd), _p(sumdy), _p(dot), int(n), _p(A), _p(B), _p(Cc), _p(dgamma), _p(dbeta),
                                       int(accumulate), C, _stream()), "cxrk_bn_train_bwd_coeffs")
    return A, B, Cc


def bn_train_dz(dy, z, A, B, Cc):
    """dz = A dy + B + Cc z (per channel), in dy's storage format."""
    lib = _lib.load()
    C = dy.shape[-1]
    rows = dy.numel() // C
    dp, dpl = _fmt(dy, "bn_train_dz.dy")
    zp, zpl = _fmt(z, "bn_train_dz.z")
    if z.numel() != dy.numel():
        raise ValueError(f"bn_train_dz: {tuple(dy.shape)} vs {tuple(z.shape)}")
    dz = Planes.empty(*dy.shape, device=dy.device) if isinstance(dy, Planes) else torch.empty_like(dy)
    op, opl = _fmt(dz, "bn_train_dz.dz")
    check(lib.cxrk_bn_train_dz(dp, dpl, zp, zpl, _p(_vec(A, C, "A")), _p(_vec(B, C, "B")), _p(_vec(Cc, C, "Cc")), op, opl, rows, C, _stream()),
          "cxrk_bn_train_dz")
    return dz


# ----------------------------------------------------------------------------------------------------------------
# image encoder pieces (NHWC)
# ----------------------------------------------------------------------------------------------------------------

def bn_fold(w, gamma, beta, rmean, rvar, eps, Ko, taps, C, Cpad, w_scaled, scale, shift, rstd):
    lib = _lib.load()
    for n, t in (("w", w), ("gamma", gamma), ("beta", beta), ("rmean", rmean), ("rvar", rvar)):
        _chk(t, "bn_fold." + n)
    check(lib.cxrk_bn_fold(_p(w), _p(gamma), _p(beta), _p(rmean), _p(rvar), float(eps), Ko, taps, C, Cpad,
                           _p(w_scaled), _p(scale), _p(shift), _p(rstd), _stream()), "cxrk_bn_fold")


def conv_fwd(x, w_scaled, shift, residual, y, N, H, W, C, Ko, R, S, stride, pad, relu):
    lib = _lib.load()
    ev = None
    if profiler.on:
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        fl = 2.0 * N * Ho * Wo * Ko * R * S * C
        ev = profiler.bracket(fl, 4.0 * (N * H * W * C + Ko * R * S * C + N * Ho * Wo * Ko * (1 + (residual is not None))))
    rc = lib.cxrk_conv_bn_act_fwd(_p(_chk(x, "conv.x")), _p(w_scaled), _p(shift), _p(residual), _p(y), N, H, W, C, Ko,
                                  R, S, stride, pad, int(relu), _stream())
    profiler.end(ev)
    check(rc, f"cxrk_conv_bn_act_fwd(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    return y


def _conv_out(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv_bwd_data(dy, w_scaled, residual, relu_src, dx, N, H, W, C, Ko, R, S, stride, pad, sums=None):
    """dx = (relu_src > 0) * (conv^T(dy, w_scaled) + residual); `sums` ([C], optional) receives the column sums of dx (the BN beta
    gradient of the unit that produced relu_src), reduced in the same epilogue."""
    lib = _lib.load()
    ws = workspace(lib.cxrk_conv_bwd_data_colsum_ws_bytes(N, H, W, C, stride), dy.device) if sums is not None else None
    ev = None
    if profiler.on:  # algorithmic FLOPs of a data gradient = those of the forward conv (stride-2 zero taps are waste)
        Ho, Wo = _conv_out(H, W, R, S, stride, pad)
        fl = 2.0 * N * Ho * Wo * Ko * R * S * C
        ev = profiler.bracket(fl, 4.0 * (N * Ho * Wo * Ko + Ko * R * S * C + N * H * W * C * (1 + (residual is not None) + (relu_src is not None))))
    rc = lib.cxrk_conv_bn_act_bwd_data(_p(_chk(dy, "conv.dy")), _p(w_scaled), _p(residual), _p(relu_src), _p(dx), N, H,
                                       W, C, Ko, R, S, stride, pad, _p(sums), _p(ws), ws.numel() * 4 if ws is not None else 0, _stream())
    profiler.end(ev)
    check(rc, f"cxrk_conv_bn_act_bwd_data(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    return dx


def conv_bwd_params(x, dy, w, scale, rstd, rmean, sumdy, dw, dgamma, dbeta, accumulate, N, H, W, C, Cpad, Ko, R, S, stride, pad):
    """dW = scale * wgrad(x, dy); dbeta = sumdy; dgamma = rstd * (<w, wgrad> - mean * sumdy)  (csrc/conv_wgrad.hip)."""
    lib = _lib.load()
    wsb = lib.cxrk_conv_wgrad_ws_bytes(N, H, W, Cpad, Ko, R, S, stride, pad)
    ws = workspace(wsb, x.device)
    ev = None
    if profiler.on:
        Ho, Wo = _conv_out(H, W, R, S, stride, pad)
        fl = 2.0 * N * Ho * Wo * Ko * R * S * Cpad
        ev = profiler.bracket(fl, 4.0 * (N * H * W * Cpad + N * Ho * Wo * Ko + Ko * R * S * Cpad))
    check(lib.cxrk_conv_bn_act_bwd_params(_p(_chk(x, "conv.x")), _p(_chk(dy, "conv.dy")), _p(w), _p(scale), _p(rstd),
                                          _p(rmean), _p(sumdy), _p(dw), _p(dgamma), _p(dbeta), int(accumulate), N, H, W,
                                          C, Cpad, Ko, R, S, stride, pad, _p(ws), ws.numel() * 4, _stream()),
          f"cxrk_conv_bn_act_bwd_params(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    profiler.end(ev)


# ---- planes storage (split-bf16 mode of the image encoder) -------------------------------------------------------------------

def bn_fold_pl(w, gamma, beta, rmean, rvar, eps, Ko, taps, C, Cpad, w_scaled: Planes, scale, shift, rstd):
    lib = _lib.load()
    for n, t in (("w", w), ("gamma", gamma), ("beta", beta), ("rmean", rmean), ("rvar", rvar)):
        _chk(t, "bn_fold." + n)
    check(lib.cxrk_bn_fold_pl(_p(w), _p(gamma), _p(beta), _p(rmean), _p(rvar), float(eps), Ko, taps, C, Cpad, w_scaled.ptr(),
                              w_scaled.plane, _p(scale), _p(shift), _p(rstd), _stream()), "cxrk_bn_fold_pl")


def conv_fwd_pl(x, w_scaled, shift, residual: Optional[Planes], y: Planes, maskout, N, H, W, C, Ko, R, S, stride, pad, relu):
    """x / w_scaled: both Planes, or both fp32 tensors (the stem); y (and residual) Planes; maskout: uint8 [N*Ho*Wo, Ko/8] or None."""
    lib = _lib.load()
    in_planes = isinstance(x, Planes)
    if in_planes != isinstance(w_scaled, Planes):
        raise ValueError("conv_fwd_pl: x and w_scaled must share the storage format")
    ev = None
    if profiler.on:
        Ho, Wo = _conv_out(H, W, R, S, stride, pad)
        fl = 2.0 * N * Ho * Wo * Ko * R * S * C
        nb = 4.0 * (N * H * W * C + Ko * R * S * C + N * Ho * Wo * Ko * (1 + (residual is not None))) + (N * Ho * Wo * Ko / 8.0 if maskout is not None else 0.0)
        ev = profiler.bracket(fl, nb)
    if maskout is not None:
        _chk(maskout, "conv.maskout", torch.uint8)
    xp, xpl = (x.ptr(), x.plane) if in_planes else (_p(_chk(x, "conv.x")), 0)
    wp, wpl = (w_scaled.ptr(), w_scaled.plane) if in_planes else (_p(_chk(w_scaled, "conv.w")), 0)
    rc = lib.cxrk_conv_bn_act_fwd_pl(xp, xpl, wp, wpl, int(in_planes), _p(shift), residual.ptr() if residual is not None else None,
                                     residual.plane if residual is not None else 0, y.ptr(), y.plane, _p(maskout), N, H, W, C, Ko, R, S,
                                     stride, pad, int(relu), _stream())
    profiler.end(ev)
    check(rc, f"cxrk_conv_bn_act_fwd_pl(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    return y


def conv_bwd_data_pl(dy: Planes, w_scaled: Planes, residual: Optional[Planes], maskin, dx: Planes, N, H, W, C, Ko, R, S, stride, pad,
                     sums=None, residual_s2: bool = False):
    """dx = mask(conv^T(dy, w_scaled) + residual) on planes operands (+ column sums of dx).  residual_s2: `residual` is COMPACT,
    [N, (H+1)//2, (W+1)//2, C] = the identity-branch gradient at the even (h, w) pixels only (what a 1x1 / stride-2 projection
    shortcut's data gradient is: see `conv1x1_s2_bwd_data_compact_pl`); the other pixels receive nothing."""
    lib = _lib.load()
    if residual_s2:
        if residual is None or tuple(residual.shape) != (N, (H + 1) // 2, (W + 1) // 2, C):
            raise ValueError(f"conv_bwd_data_pl: compact residual must be [N, (H+1)//2, (W+1)//2, C], got {None if residual is None else tuple(residual.shape)}")
    ws = workspace(lib.cxrk_conv_bwd_data_colsum_ws_bytes(N, H, W, C, stride), dy.device) if sums is not None else None
    ev = None
    if profiler.on:
        Ho, Wo = _conv_out(H, W, R, S, stride, pad)
        fl = 2.0 * N * Ho * Wo * Ko * R * S * C
        ev = profiler.bracket(fl, 4.0 * (N * Ho * Wo * Ko + Ko * R * S * C + N * H * W * C * (1 + (0.0 if residual is None else 0.25 if residual_s2 else 1.0)))
                              + (N * H * W * C / 8.0 if maskin is not None else 0.0))
    fn = lib.cxrk_conv_bn_act_bwd_data_pl_s2res if residual_s2 else lib.cxrk_conv_bn_act_bwd_data_pl
    rc = fn(dy.ptr(), dy.plane, w_scaled.ptr(), w_scaled.plane, residual.ptr() if residual is not None else None,
                                          residual.plane if residual is not None else 0, _p(maskin), dx.ptr(), dx.plane, N, H, W, C, Ko, R, S,
                                          stride, pad, _p(sums), _p(ws), ws.numel() * 4 if ws is not None else 0, _stream())
    profiler.end(ev)
    check(rc, f"cxrk_conv_bn_act_bwd_data_pl{'_s2res' if residual_s2 else ''}(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    return dx


def conv1x1_s2_bwd_data_compact_pl(dy: Planes, w_scaled: Planes, N, H, W, C, Ko) -> Optional[Planes]:
    """Data gradient of a 1x1 / stride-2 / pad-0 convolution in COMPACT form: only the input pixels with even (h, w) receive
    anything, dx[n, 2a, 2b, :] = dy[n, a, b, :] @ w — a dense [N*Ho*Wo, Ko] x [Ko, C] product, returned as [N, Ho, Wo, C] for
    `conv_bwd_data_pl(..., residual_s2=True)`.  None when the compact tensor is too large for that epilogue's 32-bit offsets
    (the caller then takes the dense form)."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if N * Ho * Wo * C * 2 >= (1 << 31):
        return None
    if tuple(dy.shape) not in ((N, Ho, Wo, Ko), (N * Ho * Wo, Ko)) or tuple(w_scaled.shape) != (Ko, C):
        raise ValueError(f"conv1x1_s2_bwd_data_compact_pl: dy {tuple(dy.shape)}, w {tuple(w_scaled.shape)} for N={N},H={H},W={W},C={C},Ko={Ko}")
    out = Planes.empty(N * Ho * Wo, C, device=dy.device)
    linear_bwd_data_pl(dy.view(N * Ho * Wo, Ko), w_scaled, out=out)
    return out.view(N, Ho, Wo, C)


def conv_bwd_params_pl(x: Planes, dy: Planes, w, scale, rstd, rmean, sumdy, dw, dgamma, dbeta, accumulate, N, H, W, C, Ko, R, S, stride, pad):
    lib = _lib.load()
    ws = workspace(lib.cxrk_conv_wgrad_ws_bytes(N, H, W, C, Ko, R, S, stride, pad), x.device)
    ev = None
    if profiler.on:
        Ho, Wo = _conv_out(H, W, R, S, stride, pad)
        fl = 2.0 * N * Ho * Wo * Ko * R * S * C
        ev = profiler.bracket(fl, 4.0 * (N * H * W * C + N * Ho * Wo * Ko + Ko * R * S * C))
    check(lib.cxrk_conv_bn_act_bwd_params_pl(x.ptr(), x.plane, dy.ptr(), dy.plane, _p(w), _p(scale), _p(rstd), _p(rmean), _p(sumdy),
                                             _p(dw), _p(dgamma), _p(dbeta), int(accumulate), N, H, W, C, Ko, R, S, stride, pad, _p(ws),
                                             ws.numel() * 4, _stream()),
          f"cxrk_conv_bn_act_bwd_params_pl(N={N},H={H},W={W},C={C},Ko={Ko},R={R},s={stride})")
    profiler.end(ev)


def maxpool_fwd_pl(x: Planes):
    lib = _lib.load()
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = Planes.empty(N, Ho, Wo, C, device=x.device)
    idx = torch.empty(N, Ho, Wo, C, dtype=torch.uint8, device=x.device)
    check(lib.cxrk_maxpool_fwd_pl(x.ptr(), x.plane, y.ptr(), y.plane, _p(idx), N, H, W, C, _stream()), "cxrk_maxpool_fwd_pl")
    return y, idx


def maxpool_bwd_pl(dy: Planes, idx, pooled: Planes, H: int, W: int) -> torch.Tensor:
    """fp32 gradient w.r.t. the (post-ReLU) stem output, masked by the stem ReLU through the sign of `pooled`."""
    lib = _lib.load()
    N, _, _, C = pooled.shape
    dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dy.device)
    check(lib.cxrk_maxpool_bwd_pl(dy.ptr(), dy.plane, _p(idx), pooled.ptr(), _p(dx), N, H, W, C, _stream()), "cxrk_maxpool_bwd_pl")
    return dx


def stem_pool_fwd_pl(x, w_scaled, shift, N, H, W, C, Ko, R, S, stride, pad, want_idx: bool = True):
    """Stem convolution + folded BatchNorm + ReLU + 3x3/2/1 max-pool in one kernel (csrc/stem_pool.hip): x fp32 [N,H,W,C], w_scaled
    fp32 -> (pooled Planes [N,Hp,Wp,Ko], winners uint8 [N,Hp,Wp,Ko] or None), bit-identical to `conv_fwd_pl(relu=True)` followed by
    `maxpool_fwd_pl`.  -> None when the library does not fuse this geometry (the caller takes the two calls)."""
    lib = _lib.load()
    Hs, Ws = _conv_out(H, W, R, S, stride, pad)
    Hp, Wp = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    y = Planes.empty(N, Hp, Wp, Ko, device=x.device)
    idx = torch.empty(N, Hp, Wp, Ko, dtype=torch.uint8, device=x.device) if want_idx else None
    ev = None
    if profiler.on:
        ev = profiler.bracket(2.0 * N * Hs * Ws * Ko * R * S * C, 4.0 * (N * H * W * C + Ko * R * S * C + N * Hp * Wp * Ko) + (N * Hp * Wp * Ko if want_idx else 0))
    rc = lib.cxrk_stem_pool_fwd(_p(_chk(x, "stem_pool.x")), _p(_chk(w_scaled, "stem_pool.w")), _p(_chk(shift, "stem_pool.shift")), y.ptr(), y.plane,
                                _p(idx), N, H, W, C, Ko, R, S, stride, pad, _stream())
    profiler.end(ev)
    if rc == -4:    # CXRK_ERR_UNSUPPORTED
        return None
    check(rc, f"cxrk_stem_pool_fwd(N={N},H={H},W={W})")
    return y, idx


def stem_pool_bwd_sums(g: Planes, pooled: Planes) -> torch.Tensor:
    """sums[c] of the tensor `maxpool_bwd_pl(g, idx, pooled, ...)` would write, over its pixels, without that tensor: the sum over the
    pooled pixels of g * [pooled > 0] (every window has one winner).  Deterministic."""
    lib = _lib.load()
    N, Hp, Wp, C = pooled.shape
    if tuple(g.shape) != (N, Hp, Wp, C) or not g.is_contiguous() or not pooled.is_contiguous():
        raise ValueError(f"stem_pool_bwd_sums: g {tuple(g.shape)} and pooled {tuple(pooled.shape)} must be contiguous and of one shape")
    sums = torch.empty(C, dtype=torch.float32, device=g.device)
    part = workspace(lib.cxrk_colsum_ws_bytes(N * Hp * Wp, C), g.device)
    ev = None
    if profiler.on:
        ev = profiler.bracket(2.0 * N * Hp * Wp * C, 6.0 * N * Hp * Wp * C)
    rc = lib.cxrk_stem_pool_bwd_sums(g.ptr(), g.plane, pooled.ptr(), _p(sums), N, Hp, Wp, C, _p(part), part.numel() * 4, _stream())
    profiler.end(ev)
    check(rc, f"cxrk_stem_pool_bwd_sums(N={N},Hp={Hp},Wp={Wp},C={C})")
    return sums


def spatial_mean_bwd_pl(dy: torch.Tensor, Pn: int, add: Optional[torch.Tensor] = None) -> Planes:
    lib = _lib.load()
    N, C = dy.shape
    dx = Planes.empty(N, Pn, C, device=dy.device)
    if add is not None:
        add = _chk(add, "spatial_mean.add").contiguous()
    check(lib.cxrk_spatial_mean_bwd_pl(_p(_chk(dy.contiguous(), "spatial_mean.dy")), _p(add), dx.ptr(), dx.plane, N, Pn, C, _stream()),
          "cxrk_spatial_mean_bwd_pl")
    return dx


def unpack_mask(mask: torch.Tensor, C: int) -> torch.Tensor:
    """ReLU decision bits [rows, C/8] (bit c % 8 of byte c / 8) -> bool [rows, C] on the host (tests only)."""
    m = mask.cpu().reshape(-1, C // 8).to(torch.int32)
    bits = (m.unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1
    return bits.reshape(-1, C).bool()


def nchw_to_nhwc(x: torch.Tensor, cpad: int) -> torch.Tensor:
    lib = _lib.load()
    _chk(x, "nchw_to_nhwc.x")
    x = x.contiguous()
    N, C, H, W = x.shape
    y = torch.empty(N, H, W, cpad, dtype=torch.float32, device=x.device)
    check(lib.cxrk_nchw_to_nhwc(_p(x), _p(y), N, C, H, W, cpad, _stream()), "cxrk_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _chk(x, "nhwc_to_nchw.x")
    N, H, W, C = x.shape
    y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    check(lib.cxrk_nhwc_to_nchw(_p(x), _p(y), N, C, H, W, _stream()), "cxrk_nhwc_to_nchw")
    return y


def _chk_images(x: torch.Tensor, name: str) -> torch.Tensor:
    _chk(x, name)
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise ValueError(f"{name}: expected [N, 3, H, W] or [N, 1, H, W] images, got shape {tuple(x.shape)}")
    if x.requires_grad:
        raise ValueError(f"{name}: the augmentation has no input gradient; pass images that do not require grad")
    return x.contiguous()


def augment_params(x: torch.Tensor, spec, seed: int, counter: int, row_offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Parameter rows [N, 8] (a00 a01 a02 a10 a11 a12 gain bias) of the images `x` under `spec` (augment.AugmentSpec), drawn for
    (seed, counter, row_offset + i): include/cxrk.h, "augment".  The images are read only when spec.contrast != 0 (their means)."""
    lib = _lib.load()
    x = _chk_images(x, "augment_params.x")
    N, C, Hs, Ws = x.shape
    Ho, Wo = spec.size_for(Hs, Ws)
    params = torch.empty(N, 8, dtype=torch.float32, device=x.device) if out is None else _chk_out(out, (N, 8), "augment_params.out")
    check(lib.cxrk_augment_params(_p(x) if spec.contrast != 0 else None, N, C, Hs, Ws, Ho, Wo, spec.rotate_deg, spec.translate, spec.zoom[0],
                                  spec.zoom[1], spec.flip_p, spec.brightness, spec.contrast, int(seed) & (2 ** 64 - 1),
                                  int(counter) & 0xFFFFFFFF, int(row_offset), _p(params), _stream()), "cxrk_augment_params")
    return params


def augment_nhwc(x: torch.Tensor, cpad: int, params: torch.Tensor, out_size=None, clamp01: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, C, Hs, Ws] (C = 3, or 1 replicated to three) sampled through the inverse affine maps `params` (augment_params) ->
    fp32 [N, Ho, Wo, cpad]; the augmenting form of `nchw_to_nhwc`.  `out`: a caller's tensor of that shape (its address is checked
    by the library: 16-byte stores)."""
    lib = _lib.load()
    x = _chk_images(x, "augment_nhwc.x")
    N, C, Hs, Ws = x.shape
    Ho, Wo = (Hs, Ws) if out_size is None else (int(out_size[0]), int(out_size[1]))
    _chk(params, "augment_nhwc.params")
    if tuple(params.shape) != (N, 8) or not params.is_contiguous():
        raise ValueError(f"augment_nhwc.params: expected a contiguous [{N}, 8] tensor, got {tuple(params.shape)}")
    y = torch.empty(N, Ho, Wo, cpad, dtype=torch.float32, device=x.device) if out is None else _chk_out(out, (N, Ho, Wo, cpad), "augment_nhwc.out")
    check(lib.cxrk_augment_nhwc(_p(x), _p(params), _p(y), N, C, Hs, Ws, Ho, Wo, cpad, int(bool(clamp01)), _stream()), "cxrk_augment_nhwc")
    return y


def maxpool_fwd(x: torch.Tensor):
    lib = _lib.load()
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(N, Ho, Wo, C, dtype=torch.float32, device=x.device)
    idx = torch.empty(N, Ho, Wo, C, dtype=torch.uint8, device=x.device)
    check(lib.cxrk_maxpool_fwd(_p(_chk(x, "maxpool.x")), _p(y), _p(idx), N, H, W, C, _stream()), "cxrk_maxpool_fwd")
    return y, idx


def maxpool_bwd(dy, idx, x, relu_mask: bool):
    lib = _lib.load()
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    check(lib.cxrk_maxpool_bwd(_p(_chk(dy, "maxpool.dy")), _p(idx), _p(x), _p(dx), N, H, W, C, int(relu_mask), _stream()),
          "cxrk_maxpool_bwd")
    return dx


def spatial_mean_fwd(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    N, Pn, C = x.shape
    y = torch.empty(N, C, dtype=torch.float32, device=x.device)
    check(lib.cxrk_spatial_mean_fwd(_p(_chk(x, "spatial_mean.x")), _p(y), N, Pn, C, _stream()), "cxrk_spatial_mean_fwd")
    return y


def spatial_mean_bwd(dy: torch.Tensor, Pn: int) -> torch.Tensor:
    lib = _lib.load()
    N, C = dy.shape
    dx = torch.empty(N, Pn, C, dtype=torch.float32, device=dy.device)
    check(lib.cxrk_spatial_mean_bwd(_p(_chk(dy.contiguous(), "spatial_mean.dy")), _p(dx), N, Pn, C, _stream()),
          "cxrk_spatial_mean_bwd")
    return dx


# ----------------------------------------------------------------------------------------------------------------
# text encoder pieces
# ----------------------------------------------------------------------------------------------------------------

def _new_out(rows, cols, device, planes: bool):
    """(tensor-or-Planes, pointer, plane stride) of a fresh [rows, cols] output in the requested storage format"""
    if planes:
        o = Planes.empty(rows, cols, device=device)
        return o, o.ptr(), o.plane
    o = torch.empty(rows, cols, dtype=torch.float32, device=device)
    return o, o.data_ptr(), 0


class Drop(NamedTuple):
    """Dropout descriptor of one site of one call (include/cxrk.h, "dropout"): the keep mask is a pure function of these values and
    of the element's (sequence, token, head, column)."""
    seed: int
    counter: int
    layer: int
    site: int
    row_offset: int
    p: float

    def args(self):
        return (self.seed & (2 ** 64 - 1), self.counter & 0xFFFFFFFF, self.layer, self.site, self.row_offset, float(self.p))


DROP_EMBED, DROP_ATTN_PROBS, DROP_ATTN_OUT, DROP_FFN_OUT = 0, 1, 2, 3


def dropout_mask(drop: Drop, N: int, L: int, C: int, nH: int = 1, device="cuda") -> torch.Tensor:
    """uint8 keep mask [N, nH, L, C] of one site (hidden sites: nH = 1, C = H, i.e. the [N*L, H] activation)."""
    keep = torch.empty(N, nH, L, C, dtype=torch.uint8, device=device)
    check(_lib.load().cxrk_dropout_mask(*drop.args(), N, L, nH, C, _p(keep), _stream()), "cxrk_dropout_mask")
    return keep


def embed_ln_fwd(ids, word, pos, type_row, gamma, beta, eps, L, out_planes: bool = False, drop: Optional[Drop] = None):
    """drop: y = keep * s * LayerNorm(...) (BertEmbeddings.dropout); xhat / rstd stay those of the LayerNorm."""
    lib = _lib.load()
    _chk(ids, "embed.ids", torch.int64)
    ids = ids.contiguous()
    T = ids.numel()
    H = word.shape[1]
    y, yp, ypl = _new_out(T, H, word.device, out_planes)
    xhat = torch.empty(T, H, dtype=torch.float32, device=word.device)
    rstd = torch.empty(T, dtype=torch.float32, device=word.device)
    if drop is not None:
        check(lib.cxrk_embed_ln_fwd_drop(_p(ids), _p(_chk(word, "embed.word")), _p(pos), _p(type_row), _p(gamma), _p(beta),
                                         float(eps), T, L, H, yp, ypl, _p(xhat), _p(rstd), *drop.args(), _stream()),
              "cxrk_embed_ln_fwd_drop")
        return y, xhat, rstd
    check(lib.cxrk_embed_ln_fwd(_p(ids), _p(_chk(word, "embed.word")), _p(pos), _p(type_row), _p(gamma), _p(beta),
                                float(eps), T, L, H, yp, ypl, _p(xhat), _p(rstd), _stream()), "cxrk_embed_ln_fwd")
    return y, xhat, rstd


def residual_ln_fwd(x, res, gamma, beta, eps, save: bool = True, out_planes: bool = False, drop: Optional[Drop] = None,
                    rows_per_seq: int = 1):
    """y = LayerNorm(x + res); with `drop`: y = LayerNorm(keep * s * x + res), `res` fp32 or Planes (rows may be strided, e.g. the
    CLS rows), `rows_per_seq` = rows of x per sequence (L, or 1 for CLS rows)."""
    lib = _lib.load()
    rows, H = x.shape
    y, yp, ypl = _new_out(rows, H, x.device, out_planes)
    xhat = torch.empty_like(x) if save else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save else None
    if drop is not None:
        if res is None:
            raise ValueError("residual_ln_fwd(drop=...): the residual is required")
        if isinstance(res, Planes):
            rp, rld, rpl = _pl2d(res, "ln.res")
        else:
            _chk(res, "ln.res")
            if res.stride(1) != 1:
                raise ValueError("ln.res: columns must be contiguous")
            rp, rld, rpl = res.data_ptr(), res.stride(0), 0
        check(lib.cxrk_residual_ln_fwd_drop(_p(_chk(x, "ln.x")), rp, rpl, rld, _p(gamma), _p(beta), float(eps), rows, H, int(rows_per_seq),
                                            yp, ypl, _p(xhat), _p(rstd), *drop.args(), _stream()), "cxrk_residual_ln_fwd_drop")
        return y, xhat, rstd
    check(lib.cxrk_residual_ln_fwd(_p(_chk(x, "ln.x")), _p(res), _p(gamma), _p(beta), float(eps), rows, H, yp, ypl,
                                   _p(xhat), _p(rstd), _stream()), "cxrk_residual_ln_fwd")
    return y, xhat, rstd


def residual_ln_bwd(dy, xhat, rstd, gamma, dgamma, dbeta, dx_add=None, accumulate: bool = False, out=None, out_planes: bool = False,
                    dxsum=None, dxsum_accumulate: bool = False):
    """LayerNorm backward (+ dx_add); `dxsum` ([H], optional) receives the column sums of the returned gradient in the same pass."""
    lib = _lib.load()
    rows, H = dy.shape
    if out is None:
        dx, dxp, dxpl = _new_out(rows, H, dy.device, out_planes)
    elif isinstance(out, Planes):
        dx, dxp, dxpl = out, out.ptr(), out.plane
    else:
        dx, dxp, dxpl = out, out.data_ptr(), 0
    wsb = lib.cxrk_residual_ln_bwd_ws_bytes(rows, H)
    ws = workspace(wsb, dy.device)
    check(lib.cxrk_residual_ln_bwd(_p(_chk(dy, "ln.dy")), _p(xhat), _p(rstd), _p(gamma), rows, H, _p(dx_add), dxp, dxpl,
                                   _p(dgamma), _p(dbeta), int(accumulate), _p(dxsum), int(dxsum_accumulate), _p(ws), ws.numel() * 4,
                                   _stream()),
          "cxrk_residual_ln_bwd")
    return dx


def residual_ln_bwd_drop(dy, xhat, rstd, gamma, dgamma, dbeta, drop: Drop, rows_per_seq: int, accumulate: bool = False,
                         out_planes: bool = False, dxsum=None, dxsum_accumulate: bool = False, mask_dy: bool = False, out=None):
    """Backward of y = LayerNorm(keep * s * x + res): returns (dsum, dxm) -- dsum = the gradient of the sum (the residual path), dxm =
    keep * s * dsum (the dense output's gradient), both fp32 or both Planes; `dxsum` receives the column sums of dxm.
    mask_dy: backward of y = keep * s * LayerNorm(x) instead (the embeddings): returns (dx, None).
    `out`: optional (dx, dxm) pair to write into (both fp32 or both Planes of one plane stride; dxm None with mask_dy)."""
    lib = _lib.load()
    rows, H = dy.shape
    if out is not None:
        dx, dxm = out
        _chk_out(dx, (rows, H), "ln.out[0]")
        if (dxm is None) != bool(mask_dy):
            raise ValueError("residual_ln_bwd_drop: out = (dx, dxm), dxm None exactly when mask_dy")
        dxp, dxpl = (dx.ptr(), dx.plane) if isinstance(dx, Planes) else (dx.data_ptr(), 0)
        dxmp = None
        if dxm is not None:
            _chk_out(dxm, (rows, H), "ln.out[1]")
            if isinstance(dxm, Planes) != isinstance(dx, Planes) or (isinstance(dxm, Planes) and dxm.plane != dxpl):
                raise ValueError("residual_ln_bwd_drop: dx and dxm must share the storage format and the plane stride")
            dxmp = dxm.ptr() if isinstance(dxm, Planes) else dxm.data_ptr()
    else:
        dx, dxp, dxpl = _new_out(rows, H, dy.device, out_planes)
        dxm, dxmp = (None, None) if mask_dy else _new_out(rows, H, dy.device, out_planes)[:2]
    wsb = lib.cxrk_residual_ln_bwd_ws_bytes(rows, H)
    ws = workspace(wsb, dy.device)
    check(lib.cxrk_residual_ln_bwd_drop(_p(_chk(dy, "ln.dy")), _p(xhat), _p(rstd), _p(gamma), rows, H, int(rows_per_seq),
                                        2 if mask_dy else 1, None, dxp, dxmp, dxpl, _p(dgamma), _p(dbeta), int(accumulate), _p(dxsum),
                                        int(dxsum_accumulate), _p(ws), ws.numel() * 4, *drop.args(), _stream()),
          "cxrk_residual_ln_bwd_drop")
    return dx, dxm


def attn_fwd(qkv, mask, B, L, nH, dH, save_probs: bool = True, out_planes: bool = False, drop: Optional[Drop] = None):
    """drop: ctx = (keep * s o P) V; the saved probs stay undropped."""
    lib = _lib.load()
    ctx, cp, cpl = _new_out(B * L, nH * dH, qkv.device, out_planes)
    probs = torch.empty(B, nH, L, L, dtype=torch.float32, device=qkv.device) if save_probs else None
    if mask is not None:
        _chk(mask, "attn.mask", torch.int64)
    if drop is not None:
        check(lib.cxrk_attn_fwd_drop(_p(_chk(qkv, "attn.qkv")), _p(mask), B, L, nH, dH, cp, cpl, _p(probs), *drop.args(), _stream()),
              f"cxrk_attn_fwd_drop(B={B},L={L},nH={nH},dH={dH})")
        return ctx, probs
    check(lib.cxrk_attn_fwd(_p(_chk(qkv, "attn.qkv")), _p(mask), B, L, nH, dH, cp, cpl, _p(probs), _stream()),
          f"cxrk_attn_fwd(B={B},L={L},nH={nH},dH={dH})")
    return ctx, probs


def attn_bwd(qkv, probs, dctx, B, L, nH, dH, out_planes: bool = False, drop: Optional[Drop] = None, out=None):
    lib = _lib.load()
    if out is None:
        dqkv, dp, dpl = _new_out(qkv.shape[0], qkv.shape[1], qkv.device, out_planes)
    else:
        _chk_out(out, tuple(qkv.shape), "attn.out")
        dqkv, dp, dpl = (out, out.ptr(), out.plane) if isinstance(out, Planes) else (out, out.data_ptr(), 0)
    wsb = lib.cxrk_attn_bwd_ws_bytes(B, L, nH, dH)        # the dS matrix of the tiled form (L > 64); 0 otherwise
    ws = workspace(wsb, qkv.device) if wsb else None
    if drop is not None:
        check(lib.cxrk_attn_bwd_drop(_p(qkv), _p(probs), _p(_chk(dctx, "attn.dctx")), B, L, nH, dH, dp, dpl, _p(ws),
                                     ws.numel() * 4 if ws is not None else 0, *drop.args(), _stream()),
              f"cxrk_attn_bwd_drop(B={B},L={L},nH={nH},dH={dH})")
        return dqkv
    check(lib.cxrk_attn_bwd(_p(qkv), _p(probs), _p(_chk(dctx, "attn.dctx")), B, L, nH, dH, dp, dpl, _p(ws),
                            ws.numel() * 4 if ws is not None else 0, _stream()), f"cxrk_attn_bwd(B={B},L={L},nH={nH},dH={dH})")
    return dqkv


def planes_add_rows(src: Planes, dst: torch.Tensor) -> torch.Tensor:
    """dst[r, :] += src[r, :] for a row-strided fp32 `dst` view (e.g. the CLS rows of a [N, L*H] gradient)."""
    lib = _lib.load()
    rows, cols = src.shape
    if tuple(dst.shape) != (rows, cols) or dst.stride(1) != 1 or not src.is_contiguous():
        raise ValueError("planes_add_rows: shape / layout mismatch")
    check(lib.cxrk_planes_add_rows(src.ptr(), src.plane, rows, cols, _p(_chk(dst, "add_rows.dst")), dst.stride(0), _stream()),
          "cxrk_planes_add_rows")
    return dst


def embed_bwd(ids, dx, dword):
    """dword[ids[t]] += dx[t]; every row is summed in ascending token position (deterministic: csrc/embed.hip)."""
    lib = _lib.load()
    T, H = dx.shape
    ws = workspace(lib.cxrk_embed_bwd_ws_bytes(T, H), dx.device)
    check(lib.cxrk_embed_bwd(_p(ids), _p(_chk(dx.contiguous(), "embed.dx")), T, H, _p(dword), _p(ws), ws.numel() * 4, _stream()),
          "cxrk_embed_bwd")


def gelu_bwd(dy, pre):
    lib = _lib.load()
    dx = torch.empty_like(pre)
    check(lib.cxrk_gelu_bwd(_p(_chk(dy.contiguous(), "gelu.dy")), _p(pre), pre.numel(), _p(dx), _stream()), "cxrk_gelu_bwd")
    return dx


# ----------------------------------------------------------------------------------------------------------------
# heads
# ----------------------------------------------------------------------------------------------------------------

def l2norm_fwd(x: torch.Tensor, eps: float = 1e-12, out: Optional[torch.Tensor] = None):
    """xhat = x / max(|x|, eps) row-wise; `out` may be a column slice of a wider buffer (rows out.stride(0) apart)."""
    lib = _lib.load()
    x = _chk(x, "l2norm.x").contiguous()
    rows, D = x.shape
    xhat = torch.empty_like(x) if out is None else _chk(out, "l2norm.out")
    if tuple(xhat.shape) != (rows, D) or xhat.stride(1) != 1:
        raise ValueError(f"l2norm.out must be [{rows},{D}] with contiguous columns, got {tuple(xhat.shape)} strides {xhat.stride()}")
    norm = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib.cxrk_l2norm_fwd(_p(x), rows, D, float(eps), _p(xhat), xhat.stride(0), _p(norm), _stream()), "cxrk_l2norm_fwd")
    return xhat, norm


def l2norm_bwd(dxhat, xhat, norm):
    lib = _lib.load()
    rows, D = xhat.shape
    if xhat.stride(1) != 1:
        raise ValueError("l2norm_bwd: xhat columns must be contiguous")
    dx = torch.empty(rows, D, dtype=torch.float32, device=xhat.device)
    check(lib.cxrk_l2norm_bwd(_p(_chk(dxhat.contiguous(), "l2norm.dxhat")), _p(xhat), xhat.stride(0), _p(norm), rows, D, _p(dx),
                              _stream()), "cxrk_l2norm_bwd")
    return dx


def infonce_row_lse(S, diag_off, loss_out=None, loss_scale: float = 0.0, loss_accumulate: bool = False):
    lib = _lib.load()
    rows, cols = S.shape
    lse = torch.empty(rows, dtype=torch.float32, device=S.device)
    diag = torch.empty(rows, dtype=torch.float32, device=S.device)
    check(lib.cxrk_infonce_row_lse(_p(_chk(S, "infonce.S")), S.stride(0), rows, cols, diag_off, _p(lse), _p(diag),
                                   _p(loss_out), float(loss_scale), int(loss_accumulate), _stream()),
          "cxrk_infonce_row_lse")
    return lse, diag


def infonce_grad_inplace(S, diag_off, lse_row, lse_col):
    lib = _lib.load()
    rows, cols = S.shape
    check(lib.cxrk_infonce_grad_inplace(_p(S), S.stride(0), rows, cols, diag_off, _p(lse_row), _p(lse_col), _stream()),
          "cxrk_infonce_grad_inplace")
    return S


def _keys(k, n, what):
    _chk(k, what, torch.int64)
    if k.dim() != 1 or k.shape[0] != n or not k.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int64 [{n}] tensor, got shape {tuple(k.shape)}")
    return k


def multipos_row_stats(S, keys_row, keys_col, loss_out=None, loss_scale: float = 0.0, loss_accumulate: bool = False):
    """(lse, posmean, npos) per row of S: the positives of row i are the columns j with keys_col[j] == keys_row[i]."""
    lib = _lib.load()
    rows, cols = S.shape
    lse = torch.empty(rows, dtype=torch.float32, device=S.device)
    posmean = torch.empty(rows, dtype=torch.float32, device=S.device)
    npos = torch.empty(rows, dtype=torch.float32, device=S.device)
    check(lib.cxrk_multipos_row_stats(_p(_chk(S, "multipos.S")), S.stride(0), rows, cols, _p(_keys(keys_row, rows, "multipos.keys_row")),
                                      _p(_keys(keys_col, cols, "multipos.keys_col")), _p(lse), _p(posmean), _p(npos), _p(loss_out),
                                      float(loss_scale), int(loss_accumulate), _stream()),
          "cxrk_multipos_row_stats")
    return lse, posmean, npos


def multipos_grad_inplace(S, keys_row, keys_col, n_row, lse_row, lse_col):
    lib = _lib.load()
    rows, cols = S.shape
    check(lib.cxrk_multipos_grad_inplace(_p(S), S.stride(0), rows, cols, _p(_keys(keys_row, rows, "multipos.keys_row")),
                                         _p(_keys(keys_col, cols, "multipos.keys_col")), _p(n_row), _p(lse_row), _p(lse_col), _stream()),
          "cxrk_multipos_grad_inplace")
    return S


def retrieval_ranks(Q, G, diag_off: int = 0, keys_q=None, keys_g=None):
    """(pos, greater, ties), each [N], of the queries Q [N,D] against the whole gallery G [M,D] without the [N,M] score block
    (include/cxrk.h, "retrieval_ranks").  The positives of row i: column i + diag_off, or, with keys, every column j with
    keys_g[j] == keys_q[i].  pos fp32 = the best positive score; greater / ties int32 = the non-positive columns that beat / equal
    it; both -1 for a row that met a NaN.  Exact fp32 whatever the precision mode.  Rows may be strided (stride(0) >= D)."""
    lib = _lib.load()
    _chk(Q, "retrieval.Q"), _chk(G, "retrieval.G")
    if Q.dim() != 2 or G.dim() != 2 or Q.shape[1] != G.shape[1]:
        raise ValueError(f"retrieval_ranks: expected Q [N,D] and G [M,D], got {tuple(Q.shape)} and {tuple(G.shape)}")
    if G.device != Q.device:
        raise ValueError(f"retrieval_ranks: Q is on {Q.device} but G on {G.device}")
    N, D = Q.shape
    M = G.shape[0]
    if (D > 1 and (Q.stride(1) != 1 or G.stride(1) != 1)) or (N > 1 and Q.stride(0) < D) or (M > 1 and G.stride(0) < D):
        raise ValueError(f"retrieval_ranks: columns must be contiguous and rows at least D apart, got strides {Q.stride()} and {G.stride()}")
    if (keys_q is None) != (keys_g is None):
        raise ValueError("retrieval_ranks: keys_q and keys_g go together (both or neither)")
    if keys_q is not None:
        _keys(keys_q, N, "retrieval.keys_q"), _keys(keys_g, M, "retrieval.keys_g")
    pos = torch.empty(N, dtype=torch.float32, device=Q.device)
    greater = torch.empty(N, dtype=torch.int32, device=Q.device)
    ties = torch.empty(N, dtype=torch.int32, device=Q.device)
    ldq = Q.stride(0) if N > 1 else max(D, Q.stride(0))
    ldg = G.stride(0) if M > 1 else max(D, G.stride(0))
    check(lib.cxrk_retrieval_ranks(_p(Q), ldq, N, _p(G), ldg, M, D, int(diag_off), _p(keys_q), _p(keys_g), _p(pos), _p(greater),
                                   _p(ties), _stream()), "cxrk_retrieval_ranks")
    return pos, greater, ties


TOPK_MAX = 64


def _rows_ld(t, what):
    """row pitch of a [n, w] tensor with contiguous columns and rows at least w apart"""
    n, w = t.shape
    if (w > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < w):
        raise ValueError(f"{what}: columns must be contiguous and rows at least {w} apart, got strides {t.stride()}")
    return t.stride(0) if n > 1 else max(w, t.stride(0))


def topk_neighbours(Q, G, k: int, exclude_off: int = -1):
    """(score fp32 [N,k], index int32 [N,k]): for every row of Q [N,D] the k best rows of G [M,D] by dot product, without the [N,M]
    score block (include/cxrk.h, "topk_neighbours").  Rows are sorted by score descending (NaN first), then index ascending; with
    fewer than k candidates the tail is index -1 / score -inf.  exclude_off >= 0: column i + exclude_off is no candidate of row i.
    Exact fp32 whatever the precision mode, bit-reproducible.  Rows may be strided (stride(0) >= D)."""
    lib = _lib.load()
    _chk(Q, "topk.Q"), _chk(G, "topk.G")
    if Q.dim() != 2 or G.dim() != 2 or Q.shape[1] != G.shape[1] or 0 in Q.shape or 0 in G.shape:
        raise ValueError(f"topk_neighbours: expected non-empty Q [N,D] and G [M,D], got {tuple(Q.shape)} and {tuple(G.shape)}")
    if G.device != Q.device:
        raise ValueError(f"topk_neighbours: Q is on {Q.device} but G on {G.device}")
    N, D = Q.shape
    M = G.shape[0]
    k, exclude_off = int(k), int(exclude_off)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk_neighbours: k must be in [1, {TOPK_MAX}], got {k}")
    if exclude_off < -1 or (exclude_off >= 0 and exclude_off + N > M):
        raise ValueError(f"topk_neighbours: exclude_off {exclude_off} with {N} queries does not fit a gallery of {M} rows")
    ldq, ldg = _rows_ld(Q, "topk.Q"), _rows_ld(G, "topk.G")
    score = torch.empty(N, k, dtype=torch.float32, device=Q.device)
    index = torch.empty(N, k, dtype=torch.int32, device=Q.device)
    ws = workspace(lib.cxrk_topk_neighbours_slab_bytes(N, M, k), Q.device)
    check(lib.cxrk_topk_neighbours(_p(Q), ldq, N, _p(G), ldg, M, D, k, exclude_off, _p(score), _p(index), _p(ws), ws.numel() * 4,
                                   _stream()), "cxrk_topk_neighbours")
    return score, index


def knn_vote(score, index, labels, temperature: float):
    """out [N,C] = the softmax((score - score[:, :1]) / temperature)-weighted mean of labels[index] over the k neighbours of each row
    (include/cxrk.h, "knn_vote").  index -1 slots weigh nothing; a row with a NaN score or no neighbour gives NaN."""
    lib = _lib.load()
    _chk(score, "knn_vote.score"), _chk(index, "knn_vote.index", torch.int32), _chk(labels, "knn_vote.labels")
    if score.dim() != 2 or tuple(index.shape) != tuple(score.shape) or not score.is_contiguous() or not index.is_contiguous() \
            or 0 in score.shape:
        raise ValueError(f"knn_vote: score and index must be contiguous non-empty [N,k] tensors, got {tuple(score.shape)} and "
                         f"{tuple(index.shape)}")
    if labels.dim() != 2 or 0 in labels.shape:
        raise ValueError(f"knn_vote: labels must be a non-empty [M,C] tensor, got {tuple(labels.shape)}")
    if index.device != score.device or labels.device != score.device:
        raise ValueError(f"knn_vote: score is on {score.device}, index on {index.device}, labels on {labels.device}")
    N, k = score.shape
    M, C = labels.shape
    if k > TOPK_MAX:
        raise ValueError(f"knn_vote: k must be in [1, {TOPK_MAX}], got {k}")
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature != float("inf")):
        raise ValueError(f"knn_vote: temperature must be finite and > 0, got {temperature!r}")
    ldl = _rows_ld(labels, "knn_vote.labels")
    out = torch.empty(N, C, dtype=torch.float32, device=score.device)
    check(lib.cxrk_knn_vote(_p(score), _p(index), N, k, _p(labels), ldl, M, C, 1.0 / temperature, _p(out), _stream()), "cxrk_knn_vote")
    return out


def _log_scale(t):
    _chk(t, "log_scale")
    if t.numel() != 1 or t.dim() > 1:
        raise ValueError(f"log_scale must be a 0-d or [1] fp32 tensor, got shape {tuple(t.shape)}")
    return t


def scaled_partials_numel(rows: int, cols: int) -> int:
    """floats of the `partials` output of the two *_grad_scaled_inplace entry points (include/cxrk.h)"""
    return rows * ((cols + 1023) // 1024)


def infonce_row_lse_scaled(C, diag_off, log_scale, loss_out=None, loss_scale: float = 0.0, loss_accumulate: bool = False):
    """`infonce_row_lse` on exp(log_scale) * C; log_scale is a device scalar (no host sync)."""
    lib = _lib.load()
    rows, cols = C.shape
    lse = torch.empty(rows, dtype=torch.float32, device=C.device)
    diag = torch.empty(rows, dtype=torch.float32, device=C.device)
    check(lib.cxrk_infonce_row_lse_scaled(_p(_chk(C, "infonce.C")), C.stride(0), rows, cols, diag_off, _p(_log_scale(log_scale)), _p(lse),
                                          _p(diag), _p(loss_out), float(loss_scale), int(loss_accumulate), _stream()),
          "cxrk_infonce_row_lse_scaled")
    return lse, diag


def infonce_grad_scaled_inplace(C, diag_off, lse_row, lse_col, log_scale):
    """C <- exp(log_scale) * G in place; returns (C, partials [rows * ceil(cols / 1024)] of sum G * S for `logit_scale_grad`)."""
    lib = _lib.load()
    rows, cols = C.shape
    part = torch.empty(scaled_partials_numel(rows, cols), dtype=torch.float32, device=C.device)
    check(lib.cxrk_infonce_grad_scaled_inplace(_p(_chk(C, "infonce.C")), C.stride(0), rows, cols, diag_off, _p(lse_row), _p(lse_col),
                                               _p(_log_scale(log_scale)), _p(part), _stream()),
          "cxrk_infonce_grad_scaled_inplace")
    return C, part


def multipos_row_stats_scaled(C, keys_row, keys_col, log_scale, loss_out=None, loss_scale: float = 0.0, loss_accumulate: bool = False):
    """`multipos_row_stats` on exp(log_scale) * C."""
    lib = _lib.load()
    rows, cols = C.shape
    lse = torch.empty(rows, dtype=torch.float32, device=C.device)
    posmean = torch.empty(rows, dtype=torch.float32, device=C.device)
    npos = torch.empty(rows, dtype=torch.float32, device=C.device)
    check(lib.cxrk_multipos_row_stats_scaled(_p(_chk(C, "multipos.C")), C.stride(0), rows, cols, _p(_keys(keys_row, rows, "multipos.keys_row")),
                                             _p(_keys(keys_col, cols, "multipos.keys_col")), _p(_log_scale(log_scale)), _p(lse), _p(posmean),
                                             _p(npos), _p(loss_out), float(loss_scale), int(loss_accumulate), _stream()),
          "cxrk_multipos_row_stats_scaled")
    return lse, posmean, npos


def multipos_grad_scaled_inplace(C, keys_row, keys_col, n_row, lse_row, lse_col, log_scale):
    """the keyed form of `infonce_grad_scaled_inplace`"""
    lib = _lib.load()
    rows, cols = C.shape
    part = torch.empty(scaled_partials_numel(rows, cols), dtype=torch.float32, device=C.device)
    check(lib.cxrk_multipos_grad_scaled_inplace(_p(_chk(C, "multipos.C")), C.stride(0), rows, cols, _p(_keys(keys_row, rows, "multipos.keys_row")),
                                                _p(_keys(keys_col, cols, "multipos.keys_col")), _p(n_row), _p(lse_row), _p(lse_col),
                                                _p(_log_scale(log_scale)), _p(part), _stream()),
          "cxrk_multipos_grad_scaled_inplace")
    return C, part


def logit_scale_grad(part1, part2, upstream, scale: float, out, accumulate: bool):
    """out[0] (+)= upstream * scale * (sum part1 + sum part2); `upstream` a device scalar, `out` a one-element fp32 tensor."""
    lib = _lib.load()
    _chk(out, "logit_scale_grad.out")
    if out.numel() != 1:
        raise ValueError(f"logit_scale_grad.out must hold one element, got shape {tuple(out.shape)}")
    check(lib.cxrk_logit_scale_grad(_p(_chk(part1, "logit_scale_grad.part1")), part1.numel(), _p(part2), 0 if part2 is None else part2.numel(),
                                    _p(_chk(upstream, "logit_scale_grad.upstream")), float(scale), _p(out), int(accumulate), _stream()),
          "cxrk_logit_scale_grad")
    return out


def sigmoid_partials_numel(rows: int, cols: int) -> int:
    """floats of the `partials` output of `sigmoid_pairs_fwd_bwd_inplace`: three planes of rows * ceil(cols / 1024) (include/cxrk.h)"""
    return 3 * scaled_partials_numel(rows, cols)


def _scalar(t, what):
    _chk(t, what)
    if t.numel() != 1 or t.dim() > 1:
        raise ValueError(f"{what} must be a 0-d or [1] fp32 tensor, got shape {tuple(t.shape)}")
    return t


def sigmoid_pairs_fwd_bwd_inplace(C, diag_off, keys_row, keys_col, log_scale, bias, partials: bool = True):
    """C <- exp(log_scale) * g in place, g the gradient of the pairwise sigmoid loss on x = exp(log_scale) * C + bias (both device
    scalars: no host sync).  Positives: column diag_off + i of row i, or, with keys (both or neither), the columns whose key equals
    the row's.  Returns (C, partials): with `partials` a fresh [3, rows * ceil(cols / 1024)] tensor whose planes sum to the loss
    terms, g * (x - bias) and g (for `sigmoid_pairs_loss` / `logit_scale_grad`); without, None and no sums are formed."""
    lib = _lib.load()
    _chk(C, "sigmoid_pairs.C")
    if C.dim() != 2 or (C.shape[1] > 1 and C.stride(1) != 1):
        raise ValueError(f"sigmoid_pairs.C must be a 2-d block with contiguous columns, got shape {tuple(C.shape)} strides {C.stride()}")
    rows, cols = C.shape
    if (keys_row is None) != (keys_col is None):
        raise ValueError("sigmoid_pairs: keys_row and keys_col go together (both or neither)")
    if keys_row is not None:
        _keys(keys_row, rows, "sigmoid_pairs.keys_row"), _keys(keys_col, cols, "sigmoid_pairs.keys_col")
    part = torch.empty(3, scaled_partials_numel(rows, cols), dtype=torch.float32, device=C.device) if partials else None
    ld = C.stride(0) if rows > 1 else max(cols, C.stride(0))
    check(lib.cxrk_sigmoid_pairs_fwd_bwd_inplace(_p(C), ld, rows, cols, int(diag_off), _p(keys_row), _p(keys_col),
                                                 _p(_scalar(log_scale, "sigmoid_pairs.log_scale")), _p(_scalar(bias, "sigmoid_pairs.bias")),
                                                 _p(part), _stream()),
          "cxrk_sigmoid_pairs_fwd_bwd_inplace")
    return C, part


def sigmoid_pairs_loss(partials, scale: float, out=None, accumulate: bool = False):
    """out[0] (+)= scale * sum(partials), one block, fixed order; `out` a one-element fp32 tensor (a fresh 0-d one when None)."""
    lib = _lib.load()
    _chk(partials, "sigmoid_pairs_loss.partials")
    if not partials.is_contiguous() or partials.numel() < 1:
        raise ValueError("sigmoid_pairs_loss.partials must be contiguous and non-empty")
    if out is None:
        if accumulate:
            raise ValueError("sigmoid_pairs_loss: accumulate needs an `out` to add to")
        out = torch.empty((), dtype=torch.float32, device=partials.device)
    _chk(out, "sigmoid_pairs_loss.out")
    if out.numel() != 1:
        raise ValueError(f"sigmoid_pairs_loss.out must hold one element, got shape {tuple(out.shape)}")
    check(lib.cxrk_sigmoid_pairs_loss(_p(partials), partials.numel(), float(scale), _p(out), int(accumulate), _stream()),
          "cxrk_sigmoid_pairs_loss")
    return out


def _block_pair(S, St, what):
    """the student / teacher logits blocks of the distillation head: two distinct 2-d fp32 blocks of one shape, contiguous columns,
    rows may be strided -> (rows, cols, ld, ldt)"""
    for t, name in ((S, "S"), (St, "St")):
        _chk(t, f"{what}.{name}")
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"{what}.{name} must be a 2-d block with contiguous columns, got shape {tuple(t.shape)} strides {t.stride()}")
    if tuple(S.shape) != tuple(St.shape):
        raise ValueError(f"{what}: the student block is {tuple(S.shape)} but the teacher block {tuple(St.shape)}")
    rows, cols = S.shape
    ld = S.stride(0) if rows > 1 else max(cols, S.stride(0))
    ldt = St.stride(0) if rows > 1 else max(cols, St.stride(0))
    return rows, cols, ld, ldt


def _rowvec(t, n, what):
    _chk(t, what)
    if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous fp32 [{n}] tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


def distill_row_stats(S, St, loss_out=None, loss_scale: float = 0.0, loss_accumulate: bool = False):
    """(lse, lse_t, kl) per row of the student block S and the teacher block St (include/cxrk.h, "distill"): the two log-sum-exps and
    KL(softmax(St_i) || softmax(S_i)); with `loss_out` (one fp32 element) also loss_out (+)= loss_scale * sum(kl), in a fixed order."""
    lib = _lib.load()
    rows, cols, ld, ldt = _block_pair(S, St, "distill_row_stats")
    if loss_out is not None and (_chk(loss_out, "distill_row_stats.loss_out").numel() != 1):
        raise ValueError(f"distill_row_stats.loss_out must hold one element, got shape {tuple(loss_out.shape)}")
    lse = torch.empty(rows, dtype=torch.float32, device=S.device)
    lse_t = torch.empty(rows, dtype=torch.float32, device=S.device)
    kl = torch.empty(rows, dtype=torch.float32, device=S.device)
    check(lib.cxrk_distill_row_stats(_p(S), ld, _p(St), ldt, rows, cols, _p(lse), _p(lse_t), _p(kl), _p(loss_out), float(loss_scale),
                                     int(loss_accumulate), _stream()), "cxrk_distill_row_stats")
    return lse, lse_t, kl


def distill_grad_inplace(S, St, lse_row, lse_col, lse_t_row, lse_t_col):
    """S <- (exp(S - lse_row[i]) - exp(St - lse_t_row[i])) + (exp(S - lse_col[j]) - exp(St - lse_t_col[j])) in place; St is only read."""
    lib = _lib.load()
    rows, cols, ld, ldt = _block_pair(S, St, "distill_grad")
    check(lib.cxrk_distill_grad_inplace(_p(S), ld, _p(St), ldt, rows, cols, _p(_rowvec(lse_row, rows, "distill_grad.lse_row")),
                                        _p(_rowvec(lse_col, cols, "distill_grad.lse_col")),
                                        _p(_rowvec(lse_t_row, rows, "distill_grad.lse_t_row")),
                                        _p(_rowvec(lse_t_col, cols, "distill_grad.lse_t_col")), _stream()), "cxrk_distill_grad_inplace")
    return S


# ---- masked-language-modelling head (include/cxrk.h, "mlm"; csrc/mlm.hip) ---------------------------------------------------------

def mlm_capacity(T: int, p: float) -> int:
    """slots of the compact list of selected tokens for T tokens masked with probability p:
    min(T, roundup128(ceil(p T + 8 sqrt(p (1 - p) T)))), at least 1.  The selected count is at most Binomial(T, p) (pads and special
    tokens are never drawn), so the list overflows only beyond eight standard deviations."""
    import math
    if isinstance(T, bool) or not isinstance(T, int) or T < 1:
        raise ValueError(f"mlm_capacity: the number of tokens must be an integer >= 1, got {T!r}")
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"mlm_capacity: the masking probability must lie in [0, 1], got {p!r}")
    need = math.ceil(p * T + 8.0 * math.sqrt(p * (1.0 - p) * T))
    return max(1, min(T, (need + 127) // 128 * 128))


class MlmMask(NamedTuple):
    """what `mlm_mask_tokens` returns: the ids the encoder reads, the compact list of the selected tokens (`sel` int32 token indices in
    ascending order, `tgt` int32 original ids; -1 behind the kept ones), `stats` = int32 {kept, selected} and `count` = fp32 [1] kept"""
    ids: torch.Tensor
    sel: torch.Tensor
    tgt: torch.Tensor
    stats: torch.Tensor
    count: torch.Tensor


def mlm_mask_tokens(ids, mask, seed: int, counter: int, p: float, vocab_size: int, mask_id: int, special_ids=(), row_offset: int = 0,
                    cap: Optional[int] = None) -> MlmMask:
    """HF DataCollatorForLanguageModeling's masking on the device (include/cxrk.h, "mask_tokens"): one Philox block per token, keyed by
    (seed, counter, row_offset + sequence, token); the selected tokens compacted in token order into `cap` slots (default
    `mlm_capacity`).  Nothing is read back: the counts stay in `stats` on the device."""
    import ctypes
    lib = _lib.load()
    _chk(ids, "mlm_mask.ids", torch.int64)
    if ids.dim() != 2:
        raise ValueError(f"mlm_mask.ids: expected [N, L], got {tuple(ids.shape)}")
    ids = ids.contiguous()
    N, L = ids.shape
    if mask is not None:
        _chk(mask, "mlm_mask.mask", torch.int64)
        if tuple(mask.shape) != (N, L):
            raise ValueError(f"mlm_mask.mask: expected {(N, L)}, got {tuple(mask.shape)}")
        mask = mask.contiguous()
    special = tuple(int(s) for s in special_ids)
    if len(special) > 8:
        raise ValueError(f"mlm_mask: at most 8 special ids, got {len(special)}")
    T = N * L
    cap = mlm_capacity(T, p) if cap is None else int(cap)
    dev = ids.device
    out = MlmMask(torch.empty_like(ids), torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                  torch.empty(2, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.float32, device=dev))
    counts = torch.empty((T + 255) // 256, dtype=torch.int32, device=dev)
    sp = (ctypes.c_long * 8)(*(special + (-1,) * (8 - len(special))))
    check(lib.cxrk_mlm_mask_tokens(_p(ids), _p(mask), N, L, int(row_offset), int(seed) & (2 ** 64 - 1), int(counter) & 0xFFFFFFFF, float(p),
                                   int(vocab_size), int(mask_id), ctypes.cast(sp, ctypes.c_void_p), len(special), cap, _p(out.ids),
                                   _p(out.sel), _p(out.tgt), _p(out.stats), _p(out.count), _p(counts), _stream()), "cxrk_mlm_mask_tokens")
    return out


def _mlm_list(sel, stats, what):
    _chk(sel, f"{what}.sel", torch.int32)
    _chk(stats, f"{what}.stats", torch.int32)
    if sel.dim() != 1 or not sel.is_contiguous() or stats.numel() < 1 or not stats.is_contiguous():
        raise ValueError(f"{what}: sel must be a contiguous int32 vector and stats hold the kept count")
    return sel.shape[0]


def mlm_gather_rows(last, sel, stats, out_planes: bool = False):
    """[cap, H] rows last[sel[r]] for r < kept = stats[0], zero rows behind them; fp32 or Planes."""
    lib = _lib.load()
    cap = _mlm_list(sel, stats, "mlm_gather")
    _chk(last, "mlm_gather.last")
    if last.dim() != 2 or not last.is_contiguous():
        raise ValueError(f"mlm_gather.last: expected a contiguous [T, H] tensor, got {tuple(last.shape)}")
    T, H = last.shape
    out, op, opl = _new_out(cap, H, last.device, out_planes)
    check(lib.cxrk_mlm_gather_rows(_p(last), T, H, _p(sel), _p(stats), cap, op, opl, _stream()), "cxrk_mlm_gather_rows")
    return out


def mlm_scatter_rows(dx, sel, stats, T: int):
    """zeroed [T, H] with row sel[r] = dx[r] for r < kept (plain stores: `sel` lists no token twice)"""
    lib = _lib.load()
    cap = _mlm_list(sel, stats, "mlm_scatter")
    _chk(dx, "mlm_scatter.dx")
    if dx.dim() != 2 or dx.shape[0] != cap or not dx.is_contiguous():
        raise ValueError(f"mlm_scatter.dx: expected a contiguous [{cap}, H] tensor, got {tuple(dx.shape)}")
    H = dx.shape[1]
    dlast = torch.zeros(int(T), H, dtype=torch.float32, device=dx.device)
    check(lib.cxrk_mlm_scatter_rows(_p(dx), _p(sel), _p(stats), cap, int(T), H, _p(dlast), _stream()), "cxrk_mlm_scatter_rows")
    return dlast


def mlm_xent_state(rows: int, device):
    """(state [4, rows, 64], target_logit [rows]) of one vocabulary sweep of `mlm_xent_stats`"""
    return (torch.empty(4, rows, 64, dtype=torch.float32, device=device), torch.zeros(rows, dtype=torch.float32, device=device))


def _mlm_block(S, what):
    _chk(S, f"{what}.S")
    if S.dim() != 2 or (S.shape[1] > 1 and S.stride(1) != 1):
        raise ValueError(f"{what}.S must be a 2-d block with contiguous columns, got shape {tuple(S.shape)} strides {S.stride()}")
    rows, cols = S.shape
    return rows, cols, (S.stride(0) if rows > 1 else max(cols, S.stride(0)))


def mlm_xent_stats(S, v0: int, skip: int, bias, tgt, stats, state, target_logit, first: bool) -> None:
    """fold the logits chunk S [rows, cols] (vocabulary columns v0 .. v0 + cols, the first `skip` not counted; the decoder `bias` [V]
    is added here) into the running per-(row, lane) statistics (include/cxrk.h, "xent_stats")"""
    lib = _lib.load()
    rows, cols, ld = _mlm_block(S, "mlm_xent_stats")
    _chk(bias, "mlm_xent_stats.bias")
    _chk(tgt, "mlm_xent_stats.tgt", torch.int32)
    if not bias.is_contiguous() or bias.numel() < v0 + cols or tgt.numel() != rows or tuple(state.shape) != (4, rows, 64):
        raise ValueError(f"mlm_xent_stats: bias must cover columns {v0}..{v0 + cols}, tgt hold {rows} ids and state be [4, {rows}, 64]")
    check(lib.cxrk_mlm_xent_stats(_p(S), ld, rows, cols, int(skip), int(v0), _p(bias), _p(tgt), _p(stats), _p(_chk(state, "mlm.state")),
                                  _p(_rowvec(target_logit, rows, "mlm.target_logit")), int(bool(first)), _stream()), "cxrk_mlm_xent_stats")


def mlm_xent_finish(state, target_logit, tgt, stats, scale):
    """-> (lse [rows], loss = scale * sum_{r < kept} (lse - target logit) as a 0-d tensor, correct = int32 [1] rows whose argmax is the
    target)"""
    lib = _lib.load()
    rows = state.shape[1]
    dev = state.device
    lse = torch.empty(rows, dtype=torch.float32, device=dev)
    rowloss = torch.empty(rows, dtype=torch.float32, device=dev)
    hit = torch.empty(rows, dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    correct = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.cxrk_mlm_xent_finish(_p(state), _p(target_logit), _p(tgt), _p(stats), rows, _p(_scalar(scale, "mlm_xent_finish.scale")),
                                   _p(lse), _p(rowloss), _p(hit), _p(loss), _p(correct), _stream()), "cxrk_mlm_xent_finish")
    return lse, loss, correct


def mlm_xent_grad(S, v0: int, skip: int, bias, tgt, stats, lse, upstream, scale, alpha: float = 1.0, out: Optional[Planes] = None):
    """the recomputed logits chunk S -> its gradient (include/cxrk.h, "xent_grad"), in place, or as Planes into `out` ([rows, cols]
    view of a planes buffer); rows >= kept and the `skip` columns come out exactly zero"""
    lib = _lib.load()
    rows, cols, ld = _mlm_block(S, "mlm_xent_grad")
    gp, ldg, gpl = (None, 0, 0)
    if out is not None:
        if tuple(out.shape) != (rows, cols):
            raise ValueError(f"mlm_xent_grad.out: expected Planes {(rows, cols)}, got {tuple(out.shape)}")
        gp, ldg, gpl = _pl2d(out, "mlm_xent_grad.out")
    check(lib.cxrk_mlm_xent_grad(_p(S), ld, gp, ldg, gpl, rows, cols, int(skip), int(v0), _p(_chk(bias, "mlm_xent_grad.bias")),
                                 _p(_chk(tgt, "mlm_xent_grad.tgt", torch.int32)), _p(stats), _p(_rowvec(lse, rows, "mlm_xent_grad.lse")),
                                 _p(_scalar(upstream, "mlm_xent_grad.upstream")), _p(_scalar(scale, "mlm_xent_grad.scale")), float(alpha),
                                 _stream()), "cxrk_mlm_xent_grad")
    return S if out is None else out


def clamp_inplace(x, lo: float, hi: float):
    """x <- min(max(x, lo), hi) in place on a dense tensor; a NaN stays a NaN."""
    lib = _lib.load()
    _chk(x, "clamp.x")
    if not x.is_contiguous():
        raise ValueError("clamp.x must be contiguous")
    check(lib.cxrk_clamp_inplace(_p(x), x.numel(), float(lo), float(hi), _stream()), "cxrk_clamp_inplace")
    return x


def pairwise_cosine_fwd(x, y):
    lib = _lib.load()
    x = _chk(x, "cosine.x").contiguous()
    y = _chk(y, "cosine.y").contiguous()
    B, D = x.shape
    Pn = y.shape[0]
    if y.shape[1] != D:
        raise ValueError(f"pairwise_cosine: x is [{B},{D}] but y is {tuple(y.shape)}")
    cosv = torch.empty(B, Pn, dtype=torch.float32, device=x.device)
    xn = torch.empty(B, dtype=torch.float32, device=x.device)
    yn = torch.empty(Pn, dtype=torch.float32, device=x.device)
    check(lib.cxrk_pairwise_cosine_fwd(_p(x), _p(y), B, Pn, D, _p(cosv), _p(xn), _p(yn), _stream()),
          "cxrk_pairwise_cosine_fwd")
    return cosv, xn, yn


def pairwise_cosine_bwd(x, y, cosv, dcos, xn, yn, need_dx: bool = True, out=None, accumulate_dy: bool = False):
    """`out`: optional (dx, dy) pair to write into (dx None with need_dx=False); accumulate_dy: dy += instead of dy =."""
    lib = _lib.load()
    B, D = x.shape
    Pn = y.shape[0]
    if out is None:
        dx = torch.empty_like(x) if need_dx else None
        dy = torch.empty_like(y)
    else:
        dx, dy = out
        if (dx is None) != (not need_dx):
            raise ValueError("pairwise_cosine: out = (dx, dy), dx None exactly when need_dx is False")
        if dx is not None:
            _chk_out(dx, (B, D), "cosine.out[0]")
        _chk_out(dy, (Pn, D), "cosine.out[1]")
    wsb = lib.cxrk_pairwise_cosine_bwd_ws_bytes(B, Pn, D)
    ws = workspace(wsb, x.device)
    check(lib.cxrk_pairwise_cosine_bwd(_p(x), _p(y), _p(cosv), _p(_chk(dcos.contiguous(), "cosine.dcos")), _p(xn), _p(yn),
                                       B, Pn, D, _p(dx), _p(dy), int(accumulate_dy), _p(ws), ws.numel() * 4, _stream()),
          "cxrk_pairwise_cosine_bwd")
    return dx, dy


def pairwise_cosine_max_fwd(x, y, groups: int):
    """x [B,D], y [groups*Pg, D] -> cos [B,groups*Pg], max / mean over each group's prompts [B,groups], winner index (int32)."""
    lib = _lib.load()
    x = _chk(x, "cosine.x").contiguous()
    y = _chk(y, "cosine.y").contiguous()
    B, D = x.shape
    Pn = y.shape[0]
    if y.shape[1] != D or groups <= 0 or Pn % groups:
        raise ValueError(f"pairwise_cosine_max: x is [{B},{D}], y is {tuple(y.shape)}, groups = {groups}")
    f = dict(dtype=torch.float32, device=x.device)
    cosv, xn, yn = torch.empty(B, Pn, **f), torch.empty(B, **f), torch.empty(Pn, **f)
    mx, mean = torch.empty(B, groups, **f), torch.empty(B, groups, **f)
    arg = torch.empty(B, groups, dtype=torch.int32, device=x.device)
    check(lib.cxrk_pairwise_cosine_max_fwd(_p(x), _p(y), B, groups, Pn // groups, D, _p(cosv), _p(xn), _p(yn), _p(mx), _p(mean),
                                           _p(arg), _stream()), "cxrk_pairwise_cosine_max_fwd")
    return cosv, xn, yn, mx, mean, arg


def pairwise_cosine_max_bwd(x, y, cosv, dmax, arg, xn, yn, need_dx: bool = True, out=None, accumulate_dy: bool = False):
    lib = _lib.load()
    B, D = x.shape
    Pn = y.shape[0]
    G = arg.shape[1]
    if out is None:
        dx = torch.empty_like(x) if need_dx else None
        dy = torch.empty_like(y)
    else:
        dx, dy = out
        if (dx is None) != (not need_dx):
            raise ValueError("pairwise_cosine: out = (dx, dy), dx None exactly when need_dx is False")
        if dx is not None:
            _chk_out(dx, (B, D), "cosine.out[0]")
        _chk_out(dy, (Pn, D), "cosine.out[1]")
    ws = workspace(lib.cxrk_pairwise_cosine_bwd_ws_bytes(B, Pn, D), x.device)
    check(lib.cxrk_pairwise_cosine_max_bwd(_p(x), _p(y), _p(cosv), _p(_chk(dmax.contiguous(), "cosine.dmax")), _p(arg), _p(xn), _p(yn),
                                           B, G, Pn // G, D, _p(dx), _p(dy), int(accumulate_dy), _p(ws), ws.numel() * 4, _stream()),
          "cxrk_pairwise_cosine_max_bwd")
    return dx, dy


def patch_similarity(patches, text):
    """patches [R,D] fp32, text [D] -> [R]: <patch_r, text> (vlp/inference_engine.py:104)."""
    lib = _lib.load()
    patches = _chk(patches, "patch_similarity.patches").contiguous()
    text = _chk(text, "patch_similarity.text").contiguous().reshape(-1)
    R, D = patches.shape
    if text.numel() != D:
        raise ValueError(f"patch_similarity: patches are [{R},{D}] but the text embedding has {text.numel()} features")
    out = torch.empty(R, dtype=torch.float32, device=patches.device)
    check(lib.cxrk_patch_similarity(_p(patches), _p(text), R, D, _p(out), _stream()), "cxrk_patch_similarity")
    return out


def bce_posneg_fwd_bwd(cosv, labels, diff: bool = True, need_grad: bool = True, out=None):
    """cos [B,2C] (2c = pos, 2c+1 = neg), labels [B,C] view (stride(1)==1) -> logits [B,C], dcos [B,2C], loss []
    `out`: optional (logits, dcos, loss) triple to write into (dcos None with need_grad=False)."""
    lib = _lib.load()
    B, C2 = cosv.shape
    C = C2 // 2
    _chk(labels, "bce.labels")
    if labels.dim() == 1:
        labels = labels.unsqueeze(1)
    if labels.shape[1] > 1 and labels.stride(1) != 1:
        labels = labels.contiguous()
    if out is None:
        logits = torch.empty(B, C, dtype=torch.float32, device=cosv.device)
        dcos = torch.empty_like(cosv) if need_grad else None
        loss = torch.empty((), dtype=torch.float32, device=cosv.device)
    else:
        logits, dcos, loss = out
        if (dcos is None) != (not need_grad):
            raise ValueError("bce: out = (logits, dcos, loss), dcos None exactly when need_grad is False")
        _chk_out(logits, (B, C), "bce.out[0]")
        if dcos is not None:
            _chk_out(dcos, (B, C2), "bce.out[1]")
        _chk_out(loss, (), "bce.out[2]")
    ws = workspace(lib.cxrk_bce_posneg_ws_bytes(), cosv.device)
    check(lib.cxrk_bce_posneg_fwd_bwd(_p(_chk(cosv, "bce.cos")), _p(labels), B, C, labels.stride(0), int(diff), _p(logits),
                                      _p(dcos), _p(loss), _p(ws), ws.numel() * 4, _stream()), "cxrk_bce_posneg_fwd_bwd")
    return logits, dcos, loss


def eval_score(cosv, pred_diff: bool = False):
    lib = _lib.load()
    B, C2 = cosv.shape
    C = C2 // 2
    score = torch.empty(B, C, dtype=torch.float32, device=cosv.device)
    pred = torch.empty(B, C, dtype=torch.float32, device=cosv.device)
    check(lib.cxrk_eval_score(_p(_chk(cosv, "eval.cos")), B, C, int(pred_diff), _p(score), _p(pred), _stream()),
          "cxrk_eval_score")
    return score, pred


def scale_mask(x, mask_src=None, alpha_dev=None, alpha: float = 1.0, out=None):
    """out = alpha * (*alpha_dev) * x * (mask_src > 0); alpha_dev is a 0-d device tensor (no host sync)."""
    lib = _lib.load()
    x = _chk(x, "scale_mask.x").contiguous()
    if out is None:
        out = torch.empty_like(x)
    check(lib.cxrk_scale_mask(_p(x), _p(mask_src), _p(alpha_dev), float(alpha), x.numel(), _p(out), _stream()),
          "cxrk_scale_mask")
    return out


def group_mean_fwd(x, G, n):
    lib = _lib.load()
    D = x.shape[-1]
    out = torch.empty(G, D, dtype=torch.float32, device=x.device)
    check(lib.cxrk_group_mean_fwd(_p(_chk(x.contiguous(), "group_mean.x")), G, n, D, _p(out), _stream()), "cxrk_group_mean_fwd")
    return out


def group_mean_bwd(dout, G, n):
    lib = _lib.load()
    D = dout.shape[-1]
    din = torch.empty(G * n, D, dtype=torch.float32, device=dout.device)
    check(lib.cxrk_group_mean_bwd(_p(_chk(dout.contiguous(), "group_mean.dout")), G, n, D, _p(din), _stream()),
          "cxrk_group_mean_bwd")
    return din


# ----------------------------------------------------------------------------------------------------------------
# optimiser / continual learning
# ----------------------------------------------------------------------------------------------------------------

def adam_fused(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale: float = 1.0):
    lib = _lib.load()
    n = p.numel()
    for nme, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, "adam." + nme)
        if not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"adam.{nme}: must be contiguous with {n} elements")
    check(lib.cxrk_adam_fused(_p(p), _p(g), _p(m), _p(v), n, float(lr), float(beta1), float(beta2), float(eps),
                              float(weight_decay), int(step), float(grad_scale), _stream()), "cxrk_adam_fused")


def flat_nparts(n: int) -> int:
    """number of blocks, and of fp32 partial sums per sum, of a reduction over a flat buffer of n elements (`grad_sqnorm`,
    `ewc_penalty`, `agem_dots`): a function of n alone (csrc/flat_buffers.h)"""
    return _lib.load().cxrk_grad_sqnorm_partials_bytes(int(n)) // 4


grad_sqnorm_nparts = ewc_penalty_nparts = agem_dots_nparts = flat_nparts


def _partials_out(out: Optional[torch.Tensor], name: str, k: int, device):
    """where a flat reduction writes its k partial sums: `out`, else the stream's workspace -> (buffer, its bytes); the sums are
    its first k floats once the call has accepted it"""
    if out is None:
        ws = workspace(4 * k, device)
    else:
        ws = _chk(out, name + ".out")
        if not out.is_contiguous():
            raise ValueError(name + ".out: must be contiguous")
    return ws, ws.numel() * 4


def grad_sqnorm(g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-block partial sums of g[i]^2 over a flat fp32 buffer -> [nparts] (in `out`, else in the stream's workspace: valid until the
    next wrapper call on this stream, which is `adamw_clipped`).  Bit-reproducible; g is not modified."""
    lib = _lib.load()
    _chk(g, "grad_sqnorm.g")
    if g.dim() != 1 or not g.is_contiguous() or g.numel() == 0:
        raise ValueError("grad_sqnorm.g: expected a non-empty contiguous 1-D buffer")
    n = g.numel()
    k = flat_nparts(n)
    ws, ws_bytes = _partials_out(out, "grad_sqnorm", k, g.device)
    check(lib.cxrk_grad_sqnorm(_p(g), n, _p(ws), ws_bytes, _stream()), "cxrk_grad_sqnorm")
    return ws[:k]


def adamw_clipped(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale: float = 1.0, max_norm: float = 0.0,
                  decay_mask: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None,
                  stats: Optional[torch.Tensor] = None):
    """AdamW with decoupled, masked weight decay and global-norm clipping in one launch (include/cxrk.h, "adamw_clipped").
    `partials` = what `grad_sqnorm(g)` returned (None with max_norm <= 0: no clipping); `decay_mask`: uint8 [ceil(n / 4)], one byte
    per aligned group of four elements (None: everything decays); `stats`: 2 floats <- (norm before clipping, coefficient)."""
    lib = _lib.load()
    n = p.numel()
    for nme, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, "adamw." + nme)
        if not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"adamw.{nme}: must be contiguous with {n} elements")
    if decay_mask is not None:
        _chk(decay_mask, "adamw.decay_mask", torch.uint8)
        if not decay_mask.is_contiguous() or decay_mask.numel() != (n + 3) // 4:
            raise ValueError(f"adamw.decay_mask: must be contiguous with ceil({n} / 4) = {(n + 3) // 4} bytes")
    if partials is not None:
        _chk(partials, "adamw.partials")
        if not partials.is_contiguous():
            raise ValueError("adamw.partials: must be contiguous")
    if stats is not None:
        _chk(stats, "adamw.stats")
        if not stats.is_contiguous() or stats.numel() != 2:
            raise ValueError("adamw.stats: must be 2 contiguous floats")
    check(lib.cxrk_adamw_clipped(_p(p), _p(g), _p(m), _p(v), _p(decay_mask), n, float(lr), float(beta1), float(beta2), float(eps),
                                 float(weight_decay), int(step), float(grad_scale), float(max_norm), _p(partials),
                                 0 if partials is None else partials.numel() * 4, _p(stats), _stream()), "cxrk_adamw_clipped")


def _flat(t: torch.Tensor, name: str, n: Optional[int] = None) -> torch.Tensor:
    """a non-empty contiguous 1-D fp32 GPU buffer (of n elements)"""
    _chk(t, name)
    if t.dim() != 1 or not t.is_contiguous() or t.numel() == 0 or (n is not None and t.numel() != n):
        raise ValueError(f"{name}: expected a non-empty contiguous 1-D buffer" + (f" of {n} elements" if n is not None else ""))
    return t


def fisher_accumulate(acc: torch.Tensor, g: torch.Tensor, w: float = 1.0) -> None:
    """acc += w * g^2 over flat fp32 buffers, in place (include/cxrk.h, "fisher_accumulate"); g is not modified."""
    lib = _lib.load()
    _flat(acc, "fisher_accumulate.acc")
    _flat(g, "fisher_accumulate.g", acc.numel())
    check(lib.cxrk_fisher_accumulate(_p(acc), _p(g), acc.numel(), float(w), _stream()), "cxrk_fisher_accumulate")


def ewc_consolidate(F: Optional[torch.Tensor], acc: Optional[torch.Tensor], anchor: torch.Tensor, p: torch.Tensor,
                    gamma: float = 1.0, scale: float = 1.0) -> None:
    """One pass: F = gamma * F + scale * acc and anchor = p (include/cxrk.h, "ewc_consolidate").  acc = None (identity Fisher): only the
    anchor is written, and F must be None too."""
    lib = _lib.load()
    n = _flat(anchor, "ewc_consolidate.anchor").numel()
    _flat(p, "ewc_consolidate.p", n)
    for nme, t in (("F", F), ("acc", acc)):
        if t is not None:
            _flat(t, "ewc_consolidate." + nme, n)
    check(lib.cxrk_ewc_consolidate(_p(F), _p(acc), _p(anchor), _p(p), n, float(gamma), float(scale), _stream()), "cxrk_ewc_consolidate")


def ewc_penalty(g: torch.Tensor, p: torch.Tensor, anchor: torch.Tensor, F: Optional[torch.Tensor], strength: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g += strength * F * (p - anchor) in place, and the per-block partial sums of F * (p - anchor)^2 -> [nparts] (in `out`, else in
    the stream's workspace: valid until the next wrapper call on this stream).  F = None: F = 1 everywhere (L2-SP).  The penalty is
    strength / 2 * the sum of the partials.  Bit-reproducible; p, anchor and F are not modified."""
    lib = _lib.load()
    n = _flat(g, "ewc_penalty.g").numel()
    _flat(p, "ewc_penalty.p", n)
    _flat(anchor, "ewc_penalty.anchor", n)
    if F is not None:
        _flat(F, "ewc_penalty.F", n)
    k = flat_nparts(n)
    ws, ws_bytes = _partials_out(out, "ewc_penalty", k, g.device)
    check(lib.cxrk_ewc_penalty(_p(g), _p(p), _p(anchor), _p(F), n, float(strength), _p(ws), ws_bytes, _stream()), "cxrk_ewc_penalty")
    return ws[:k]


def agem_dots(g: torch.Tensor, gref: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-block partial sums of g * gref -> [:nparts] and of gref * gref -> [nparts:] of a [2 * nparts] buffer (in `out`, else in the
    stream's workspace: valid until the next wrapper call on this stream, which is `agem_project`).  Bit-reproducible; neither
    buffer is modified."""
    lib = _lib.load()
    n = _flat(g, "agem_dots.g").numel()
    _flat(gref, "agem_dots.gref", n)
    k = 2 * flat_nparts(n)
    ws, ws_bytes = _partials_out(out, "agem_dots", k, g.device)
    check(lib.cxrk_agem_dots(_p(g), _p(gref), n, _p(ws), ws_bytes, _stream()), "cxrk_agem_dots")
    return ws[:k]


def agem_project(g: torch.Tensor, gref: torch.Tensor, partials: torch.Tensor, stats: torch.Tensor) -> None:
    """A-GEM's projection in place (include/cxrk.h, "agem_project"): with dot and rr re-derived from `partials` = what
    `agem_dots(g, gref)` returned, g -= (dot / rr) * gref iff !(dot >= 0); otherwise g is not touched.  `stats`: 4 floats <-
    (dot, rr, coef, running count of projected calls, incremented on the device).  gref is not modified."""
    lib = _lib.load()
    n = _flat(g, "agem_project.g").numel()
    _flat(gref, "agem_project.gref", n)
    _chk(partials, "agem_project.partials")
    if not partials.is_contiguous() or partials.numel() != 2 * flat_nparts(n):
        raise ValueError(f"agem_project.partials: must be the {2 * flat_nparts(n)} contiguous floats of agem_dots for {n} elements")
    _chk(stats, "agem_project.stats")
    if not stats.is_contiguous() or stats.numel() != 4:
        raise ValueError("agem_project.stats: must be 4 contiguous floats")
    check(lib.cxrk_agem_project(_p(g), _p(gref), n, _p(partials), _p(stats), _stream()), "cxrk_agem_project")


def ema_update(avg: torch.Tensor, p: torch.Tensor, decay: float) -> None:
    """avg += (1 - decay) * (p - avg) over flat fp32 buffers, in place (include/cxrk.h, "ema_update"): p == avg and decay == 1 leave
    avg as it is bit for bit; p is not modified.  `decay` in [0, 1] is a host float argument of the launch."""
    lib = _lib.load()
    n = _flat(avg, "ema_update.avg").numel()
    _flat(p, "ema_update.p", n)
    check(lib.cxrk_ema_update(_p(avg), _p(p), n, float(decay), _stream()), "cxrk_ema_update")


def flat_swap(a: torch.Tensor, b: torch.Tensor) -> None:
    """exchange two flat fp32 buffers exactly, in place and in one launch (include/cxrk.h, "flat_swap"); they must not overlap"""
    lib = _lib.load()
    n = _flat(a, "flat_swap.a").numel()
    _flat(b, "flat_swap.b", n)
    check(lib.cxrk_flat_swap(_p(a), _p(b), n, _stream()), "cxrk_flat_swap")


def sgd(p, g, lr, weight_decay: float = 0.0, grad_scale: float = 1.0):
    lib = _lib.load()
    check(lib.cxrk_sgd(_p(_chk(p, "sgd.p")), _p(_chk(g, "sgd.g")), p.numel(), float(lr), float(weight_decay),
                       float(grad_scale), _stream()), "cxrk_sgd")


def weight_reset(pnew, pold, threshold, counters):
    """In place: restore entries of pnew whose |pnew-pold| < min + thr*(max-min); counters[0] += #restored (uint64)."""
    lib = _lib.load()
    ws = workspace(lib.cxrk_weight_reset_ws_bytes(), pnew.device)
    check(lib.cxrk_weight_reset(_p(_chk(pnew, "reset.new")), _p(_chk(pold, "reset.old")), pnew.numel(), float(threshold),
                                _p(counters), _p(ws), ws.numel() * 4, _stream()), "cxrk_weight_reset")
