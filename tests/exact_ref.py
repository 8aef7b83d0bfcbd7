"""Bit-exact reference for the split-bf16 ("planes") arithmetic of DESIGN.md section 3, in torch on the CPU (float64).

A planes tensor is two bf16 planes, `hi` and `lo`; the kernels never require `lo` to be the canonical remainder of `hi`.  Fed
INDEPENDENT small-integer planes, a contraction

    sum_k  a_hi b_hi + a_hi b_lo + a_lo b_hi          (three terms: `a_lo b_lo` is dropped)

is an integer that fp32 holds exactly whatever the summation order, tile shape or split-K, provided the sum of the absolute
values of all terms stays below 2^24 (times the common granularity of the terms): every partial sum is then an exactly
representable fp32 number.  `guard_exact` asserts that condition; it is a condition of the test's validity, not a tolerance.
A kernel that ever adds the fourth term changes `three_term` and DESIGN section 3 together.

Planes are compared as raw int16 bit patterns (`plane_bits`), so the sign of a zero and the rounding direction count.
"""
import torch

EXACT_LIMIT = float(1 << 24)


# ---------------------------------------------------------------------------------------------------------------- canonical split
def canonical_planes(y32: torch.Tensor):
    """(hi, lo) bf16 of an fp32 tensor: hi = bf16(y), lo = bf16(y - hi), both round-to-nearest-even; y - hi in fp32 (exact: the
    remainder of a 24-bit value against its 8-bit rounding has at most 16 significant bits)."""
    assert y32.dtype == torch.float32
    hi = y32.bfloat16()
    lo = (y32 - hi.float()).bfloat16()
    return hi, lo


def plane_bits(t: torch.Tensor) -> torch.Tensor:
    """raw 16-bit patterns of a bf16 tensor (on the CPU)"""
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16)


def to_f32_exact(v64: torch.Tensor) -> torch.Tensor:
    """float64 -> fp32, asserting that nothing is lost (the expected value of an exact probe is an fp32 number)"""
    v32 = v64.float()
    assert torch.equal(v32.double(), v64), "expected value is not an fp32 number: the probe's shape or value range is wrong"
    return v32


# ---------------------------------------------------------------------------------------------------------------- generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_tensor(*shape, amax: int, seed: int, zero_frac: float = 0.25) -> torch.Tensor:
    """float64 integers in [-amax, amax] with about `zero_frac` exact zeros on top of the uniform draw"""
    g = _gen(seed)
    v = torch.randint(-amax, amax + 1, shape, generator=g).double()
    v[torch.rand(shape, generator=g) < zero_frac] = 0.0
    return v


def int_planes(*shape, seed: int, amax_hi: int = 7, amax_lo: int = 3):
    """(hi, lo) float64 integer planes drawn INDEPENDENTLY of each other (lo is not the remainder of anything); every value is a
    bf16 number (|v| <= 256)."""
    assert amax_hi <= 256 and amax_lo <= 256
    return int_tensor(*shape, amax=amax_hi, seed=2 * seed + 1), int_tensor(*shape, amax=amax_lo, seed=2 * seed + 2)


def int_f32(*shape, seed: int, amax: int = 7) -> torch.Tensor:
    """float64 integers, |v| <= amax <= 256: bf16 numbers, so an on-the-fly split gives hi = v, lo = 0 and the three-term and
    the exact-fp32 product coincide"""
    assert amax <= 256
    return int_tensor(*shape, amax=amax, seed=seed)


def pq_values(*shape, seed: int, s: int = 8, pmin: int = 8, pmax: int = 15, qmax: int = 3, zero_frac: float = 0.2):
    """Values for the paths that split fp32 operands on the fly: x = 2^s p + q with |p| in [pmin, pmax], |q| <= qmax (and some
    exact zeros, p = q = 0), chosen so that bf16(x) == 2^s p and x - hi == q exactly: asserted here against `canonical_planes`.
    -> (x, hi, lo) float64."""
    g = _gen(seed)
    p = torch.randint(pmin, pmax + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    q = torch.randint(-qmax, qmax + 1, shape, generator=g).double()
    z = torch.rand(shape, generator=g) < zero_frac
    p[z] = 0.0
    q[z] = 0.0
    x = p * float(1 << s) + q
    hi, lo = canonical_planes(to_f32_exact(x))
    assert torch.equal(hi.double(), p * float(1 << s)), "pq_values: bf16(x) != 2^s p (q reaches half an ulp of hi)"
    assert torch.equal(lo.double(), q), "pq_values: x - hi != q"
    return x, hi.double(), lo.double()


# ---------------------------------------------------------------------------------------------------------------- exactness guard
def guard_exact(abs_sum: torch.Tensor, granularity: float = 1.0, what: str = ""):
    """`abs_sum`: per output element, the sum over the reduction of the absolute values of ALL terms that are added (and of any
    epilogue addend).  Below 2^24 granules every partial sum, in any order, is an fp32 number."""
    worst = float(abs_sum.max()) / granularity if abs_sum.numel() else 0.0
    assert worst < EXACT_LIMIT, f"{what}: sum of |terms| = {worst:.4g} granules >= 2^24: this shape / value range cannot be exact in fp32"


# ---------------------------------------------------------------------------------------------------------------- expected values
def plane_terms(a_hi, a_lo, b_hi, b_lo, contract):
    """the four plane products of a bilinear `contract(a, b)` (float64 in, float64 out)"""
    return {"hh": contract(a_hi, b_hi), "hl": contract(a_hi, b_lo), "lh": contract(a_lo, b_hi), "ll": contract(a_lo, b_lo)}


def three_term(terms):
    """a_hi b_hi + a_hi b_lo + a_lo b_hi, explicitly WITHOUT a_lo b_lo"""
    return terms["hh"] + terms["hl"] + terms["lh"]


def guard_terms(a_hi, a_lo, b_hi, b_lo, contract, extra=None, granularity: float = 1.0, what: str = ""):
    """guard for a three-term contraction (+ `extra`: |epilogue addends|, same shape as the output)"""
    t = plane_terms(a_hi.abs(), a_lo.abs(), b_hi.abs(), b_lo.abs(), contract)
    s = three_term(t)
    if extra is not None:
        s = s + extra
    guard_exact(s, granularity, what)


# ---------------------------------------------------------------------------------------------------------------- comparison
def _first_diff(ne: torch.Tensor):
    idx = ne.nonzero()[0].tolist()
    return tuple(idx)


def diagnose(got64: torch.Tensor, exp64: torch.Tensor, terms=None) -> str:
    """first wrong element, and which plane term its error equals (if `terms` is given)"""
    ne = got64 != exp64
    if not bool(ne.any()):
        return "equal as values: only the sign of a zero differs"
    pos = _first_diff(ne)
    g, e = float(got64[pos]), float(exp64[pos])
    msg = f"{int(ne.sum())} of {ne.numel()} wrong, first at {pos}: got {g!r}, expected {e!r}"
    if terms is not None:
        d = g - e
        hints = []
        for name in ("hh", "hl", "lh"):
            t = float(terms[name][pos])
            if t != 0.0 and d == -t:
                hints.append(f"term {name} is missing")
        t = float(terms["ll"][pos])
        if t != 0.0 and d == t:
            hints.append("term ll (lo*lo) was added")
        msg += " (" + ("; ".join(hints) if hints else f"error {d!r} matches no single term: hh {float(terms['hh'][pos])!r} "
                       f"hl {float(terms['hl'][pos])!r} lh {float(terms['lh'][pos])!r} ll {float(terms['ll'][pos])!r}") + ")"
    return msg


def assert_exact(got: torch.Tensor, exp64: torch.Tensor, what: str = "", terms=None):
    """fp32 result against the exact float64 expectation: torch.equal, no tolerance.  On failure: first wrong index and the term."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32, (what, got.dtype)
    exp32 = to_f32_exact(exp64.reshape(got.shape))
    if not torch.equal(got, exp32):
        raise AssertionError(f"{what}: " + diagnose(got.double(), exp32.double(), None if terms is None else
                                                    {k: v.reshape(got.shape) for k, v in terms.items()}))


def assert_planes_exact(got_planes: torch.Tensor, exp64: torch.Tensor, what: str = "", terms=None):
    """bf16 [2, ...] planes tensor against canonical_planes(expected), as int16 bit patterns"""
    t = got_planes.detach().cpu()
    assert t.dtype == torch.bfloat16 and t.shape[0] == 2, (what, t.dtype, tuple(t.shape))
    exp32 = to_f32_exact(exp64.reshape(t.shape[1:]))
    assert_planes_bits(t[0], t[1], exp32, what, terms)


def assert_planes_bits(hi: torch.Tensor, lo: torch.Tensor, y32: torch.Tensor, what: str = "", terms=None):
    """(hi, lo) bf16 against canonical_planes(y32) bit for bit"""
    ehi, elo = canonical_planes(y32.detach().cpu())
    for name, g, e in (("hi", hi, ehi), ("lo", lo, elo)):
        gb, eb = plane_bits(g), plane_bits(e.reshape(g.shape))
        if not torch.equal(gb, eb):
            ne = gb != eb
            pos = _first_diff(ne)
            msg = (f"{what}: {name} plane: {int(ne.sum())} of {ne.numel()} bit patterns wrong, first at {pos}: got "
                   f"0x{int(gb[pos]) & 0xffff:04x} ({float(g.detach().cpu()[pos])!r}), expected 0x{int(eb[pos]) & 0xffff:04x} "
                   f"({float(e.reshape(g.shape)[pos])!r}) for value {float(y32.detach().cpu().reshape(g.shape)[pos])!r}")
            if terms is not None:
                v = (hi.detach().cpu().double() + lo.detach().cpu().double())
                msg += "; as a value: " + diagnose(v, y32.detach().cpu().double().reshape(v.shape),
                                                   {k: t.reshape(v.shape) for k, t in terms.items()})
            raise AssertionError(msg)


def assert_two_roundings(hi: torch.Tensor, lo: torch.Tensor, y32: torch.Tensor, what: str = ""):
    """The fallback for a planes writer whose fp32 form is not the same instruction sequence (so the planes need not be the
    canonical split of THAT fp32 number): both statements follow from two round-to-nearest roundings at unit roundoff 2^-8, neither
    is measured.
      1. |hi + lo - y| <= 2^-16 |y| elementwise.
      2. hi is a bf16 number nearest to hi + lo.  That is hi == bf16(hi + lo), except where lo rounded UP to exactly half an ulp of
         an odd hi: hi + lo is then a tie which round-to-nearest-even gives to the other neighbour.  The canonical split itself
         produces such pairs (about one element in a thousand: test_exact_planes_host.py), so they are accepted: a tie, checked
         exactly in float64."""
    hi, lo = hi.detach().cpu(), lo.detach().cpu()
    v = hi.double() + lo.double()
    y = y32.detach().cpu().double().reshape(v.shape)
    bad = (v - y).abs() > 2.0 ** -16 * y.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements beyond 2^-16 |y|, first at {_first_diff(bad)}"
    r = v.float().bfloat16()
    nearest = (plane_bits(r) == plane_bits(hi)) | ((v - hi.double()).abs() == (v - r.double()).abs())
    assert bool(nearest.all()), f"{what}: hi is not a nearest bf16 of hi + lo at {_first_diff(~nearest)} ({int((~nearest).sum())} elements)"


def close_rel_to_max(a: torch.Tensor, b: torch.Tensor) -> float:
    """the metric of `close()` in tests/test_kernels_gpu.py: max |a - b| / max |b|"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


CLOSE_TOL_SPLIT = 3e-4     # what `close()` allows under split_bf16


# ---------------------------------------------------------------------------------------------------------------- rounding probes
BF16_MAX = float.fromhex("0x1.fep127")          # largest finite bf16 = (2 - 2^-7) 2^127


def rounding_probe_values() -> torch.Tensor:
    """fp32 values that pin the two roundings of a planes writer (a multiple of 8 of them):
    ties of hi (integers with exactly 9 significant bits, kept bit even and odd), values of more than 16 bits (lo itself rounds,
    ties of lo included), negatives, +0 and -0, a value whose lo is subnormal in bf16, the largest finite bf16."""
    v = []
    for m in (257, 259, 261, 263, 385, 387, 509, 511):             # 9 significant bits: exact ties of hi, both parities
        v += [float(m), -float(m), float(m) * 2.0 ** -12, float(m) * 2.0 ** 40]
    for m in (65537, 65539, 98305, 131071, 16777215, 8388609, 12345677, 1234567):   # > 16 bits: lo rounds
        v += [float(m), -float(m), float(m) * 2.0 ** -20]
    # ties of lo: hi = 256 (even), remainder with exactly 9 significant bits
    for m in (257, 259, 383, 385):
        v += [256.0 + m * 2.0 ** -9, -(256.0 + m * 2.0 ** -9)]
    v += [0.0, -0.0, 1.0, -1.0, 3.0, 0.1, -0.1, 1e-3, 1e10, -7e-5]
    # lo subnormal in bf16 (exact; and a tie between two subnormals: 8.5 units of 2^-133 -> 8)
    v += [2.0 ** -120 + 2.0 ** -130, -(2.0 ** -120 + 2.0 ** -130), 2.0 ** -120 + 3 * 2.0 ** -131, 2.0 ** -120 + 2.0 ** -130 + 2.0 ** -134]
    v += [BF16_MAX, -BF16_MAX, BF16_MAX * (1 - 2.0 ** -10), 2.0 ** 127]
    while len(v) % 8:
        v.append(float(len(v)))
    return torch.tensor(v, dtype=torch.float64).float()


def top_of_range_values() -> torch.Tensor:
    """fp32 values of at most 16 significant bits at the top of the bf16 range, the largest finite bf16 included: hi is finite
    and hi + lo == x exactly (8 of them, both signs)"""
    v = [BF16_MAX, BF16_MAX - 2.0 ** 112, BF16_MAX - 2.0 ** 119, 2.0 ** 127 + 2.0 ** 112]
    return torch.tensor(v + [-x for x in v], dtype=torch.float64).float()


def above_range_values() -> torch.Tensor:
    """finite fp32 values at and above the bf16 rounding threshold (2 - 2^-8) 2^127 ~ 3.39e38: hi rounds to Inf (8 of them)"""
    thr = (2.0 - 2.0 ** -8) * 2.0 ** 127
    v = [thr, thr + 2.0 ** 104, 3.4e38, float(torch.finfo(torch.float32).max)]
    return torch.tensor(v + [-x for x in v], dtype=torch.float64).float()


# ---------------------------------------------------------------------------------------------------------------- fake (wrong) kernels
# Plain-torch stand-ins for faults the exact probes must reject (tests/test_exact_planes_host.py).  GEMM fakes take float64 planes
# a [M, K] and b [N, K] (the NT form) and return float64 [M, N] as an fp32 tensor would hold it.
def gemm_nt(a, b):
    return a @ b.T


def fake_gemm_correct(a_hi, a_lo, b_hi, b_lo):
    return three_term(plane_terms(a_hi, a_lo, b_hi, b_lo, gemm_nt))


def fake_gemm_drop_cross_term(a_hi, a_lo, b_hi, b_lo):
    t = plane_terms(a_hi, a_lo, b_hi, b_lo, gemm_nt)
    return t["hh"] + t["hl"]


def fake_gemm_adds_lolo(a_hi, a_lo, b_hi, b_lo):
    t = plane_terms(a_hi, a_lo, b_hi, b_lo, gemm_nt)
    return three_term(t) + t["ll"]


def fake_gemm_lo_ignored_in_k_tail(a_hi, a_lo, b_hi, b_lo, tail: int = 8, operands: str = "b"):
    """one loader's K tail: the lo plane of operand b (the weights; `operands` = "a", "b" or "ab") reads as zero in the last 8 k"""
    a_lo, b_lo = a_lo.clone(), b_lo.clone()
    if "a" in operands:
        a_lo[:, -tail:] = 0
    if "b" in operands:
        b_lo[:, -tail:] = 0
    return fake_gemm_correct(a_hi, a_lo, b_hi, b_lo)


def fake_gemm_lo_from_hi_plane_in_one_block(a_hi, a_lo, b_hi, b_lo, col0: int = 32, width: int = 32):
    """a wrong plane offset for one 32-column block of the output: b's lo rows are read from b's hi plane"""
    b_lo = b_lo.clone()
    b_lo[col0:col0 + width] = b_hi[col0:col0 + width]
    return fake_gemm_correct(a_hi, a_lo, b_hi, b_lo)


def _bf16_truncate(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32)


def fake_split_truncates(x32):
    hi = _bf16_truncate(x32)
    lo = _bf16_truncate(x32 - hi)
    return hi.bfloat16(), lo.bfloat16()


def _bf16_ties_away(x32):
    """round to nearest, ties away from zero: add half an ulp to the magnitude bits, truncate (finite, non-overflowing inputs)"""
    u = x32.contiguous().view(torch.int32)
    return ((u + 0x8000) & -65536).view(torch.float32)


def fake_split_ties_away(x32):
    hi = _bf16_ties_away(x32)
    lo = _bf16_ties_away(x32 - hi)
    return hi.bfloat16(), lo.bfloat16()


def fake_split_lo_from_unrounded(x32):
    """hi is rounded correctly, but lo is the remainder against the UNROUNDED (truncated) upper half of x"""
    hi = x32.bfloat16()
    lo = (x32 - _bf16_truncate(x32)).bfloat16()
    return hi, lo
