"""The exact split-bf16 probes of tests/exact_ref.py, checked without a GPU: the generators' own conditions, and deliberately
wrong fake kernels (plain torch) that the compare functions of tests/test_exact_planes_gpu.py must reject, next to the
demonstration that the tolerance of `close()` in tests/test_kernels_gpu.py (3e-4 of the output maximum under split_bf16) accepts one of them."""
import pytest
import torch

import exact_ref as X

GEMM_SHAPES = [(33, 64, 8), (200, 136, 72), (300, 264, 520)]


def _planes_case(M, N, Kd, seed=0):
    a_hi, a_lo = X.int_planes(M, Kd, seed=seed)
    b_hi, b_lo = X.int_planes(N, Kd, seed=seed + 1)
    X.guard_terms(a_hi, a_lo, b_hi, b_lo, X.gemm_nt, what=f"gemm {M}x{N}x{Kd}")
    return a_hi, a_lo, b_hi, b_lo


# ---------------------------------------------------------------------------------------------------------------- generators
def test_integer_planes_are_independent_bf16_numbers_with_zeros():
    hi, lo = X.int_planes(300, 136, seed=3)
    for p in (hi, lo):
        assert torch.equal(p, p.round()) and torch.equal(p.bfloat16().double(), p)
        assert 0.1 < float((p == 0).double().mean()) < 0.6
    # lo is not the remainder of hi: most elements carry a lo far above half an ulp of their hi
    assert float(((lo != 0) & (hi != 0)).double().mean()) > 0.3
    assert not torch.equal(*X.int_planes(8, 8, seed=1)[:1], *X.int_planes(8, 8, seed=2)[:1])


def test_pq_values_split_exactly():
    x, hi, lo = X.pq_values(64, 40, seed=5)
    assert torch.equal(hi + lo, x)
    assert float(lo.abs().max()) == 3 and float((x == 0).double().mean()) > 0.05
    ehi, elo = X.canonical_planes(x.float())
    assert torch.equal(ehi.double(), hi) and torch.equal(elo.double(), lo)
    with pytest.raises(AssertionError):        # q reaching half an ulp of hi: the generator refuses
        X.pq_values(64, 40, seed=5, s=4, pmin=8, pmax=15, qmax=3)


def test_guard_refuses_a_shape_that_cannot_be_exact():
    X.guard_exact(torch.tensor([2.0 ** 24 - 1]))
    with pytest.raises(AssertionError):
        X.guard_exact(torch.tensor([2.0 ** 24]))
    a_hi, a_lo = X.int_planes(4, 1 << 16, seed=1, amax_hi=256, amax_lo=256)
    a_hi[:], a_lo[:] = 256.0, 256.0
    with pytest.raises(AssertionError):
        X.guard_terms(a_hi, a_lo, a_hi, a_lo, X.gemm_nt)
    X.guard_exact(torch.tensor([2.0 ** 30]), granularity=256.0)          # the granularity is part of the condition


def test_expected_value_has_three_terms():
    a_hi, a_lo, b_hi, b_lo = _planes_case(33, 64, 8)
    t = X.plane_terms(a_hi, a_lo, b_hi, b_lo, X.gemm_nt)
    full = (a_hi + a_lo) @ (b_hi + b_lo).T
    assert torch.equal(X.three_term(t), full - t["ll"]) and float(t["ll"].abs().max()) > 0


def test_canonical_planes_round_to_nearest_even_twice():
    v = X.rounding_probe_values()
    assert v.numel() % 8 == 0
    hi, lo = X.canonical_planes(v)
    # ties of hi go to the even neighbour
    assert float(hi[v == 257.0]) == 256.0 and float(hi[v == 259.0]) == 260.0 and float(hi[v == -257.0]) == -256.0
    assert float(lo[v == 257.0]) == 1.0 and float(lo[v == 259.0]) == -1.0
    # -0.0 keeps its sign in hi; lo of any exactly representable value is +0
    z = (v == 0) & (torch.signbit(v))
    assert int(X.plane_bits(hi)[z]) == -32768 and int(X.plane_bits(lo)[z]) == 0
    # more than 16 bits: hi + lo differs from v by at most 2^-16 |v| (two roundings at unit roundoff 2^-8)
    # (where lo is a normal bf16 number: a subnormal lo rounds to an absolute 2^-134)
    err = (hi.double() + lo.double() - v.double()).abs()
    normal = v.abs() > 2.0 ** -100
    assert bool((err <= 2.0 ** -16 * v.double().abs())[normal].all()) and float(err.max()) > 0
    assert bool((err <= 2.0 ** -134)[~normal].all())
    # a bf16-subnormal lo survives
    s = v == torch.tensor(2.0 ** -120 + 2.0 ** -130, dtype=torch.float64).float()
    assert float(lo[s]) == 2.0 ** -130
    t = X.top_of_range_values()
    thi, tlo = X.canonical_planes(t)
    assert bool(torch.isfinite(thi.float()).all()) and torch.equal(thi.double() + tlo.double(), t.double())
    ahi, alo = X.canonical_planes(X.above_range_values())
    assert bool(torch.isinf(ahi.float()).all()) and bool(torch.isnan(ahi.float() + alo.float()).all())


# ---------------------------------------------------------------------------------------------------------------- fakes: contractions
def test_correct_fake_passes():
    for shape in GEMM_SHAPES:
        a_hi, a_lo, b_hi, b_lo = _planes_case(*shape)
        t = X.plane_terms(a_hi, a_lo, b_hi, b_lo, X.gemm_nt)
        out = X.fake_gemm_correct(a_hi, a_lo, b_hi, b_lo).float()
        X.assert_exact(out, X.three_term(t), "correct", t)
        X.assert_planes_exact(torch.stack(X.canonical_planes(out)), X.three_term(t), "correct -> planes", t)


@pytest.mark.parametrize("shape", GEMM_SHAPES)
@pytest.mark.parametrize("fake,hint", [
    (X.fake_gemm_drop_cross_term, "term lh is missing"),
    (X.fake_gemm_adds_lolo, "term ll (lo*lo) was added"),
    (X.fake_gemm_lo_ignored_in_k_tail, "wrong"),
    (X.fake_gemm_lo_from_hi_plane_in_one_block, "wrong"),
])
def test_wrong_contractions_are_rejected(shape, fake, hint):
    a_hi, a_lo, b_hi, b_lo = _planes_case(*shape)
    t = X.plane_terms(a_hi, a_lo, b_hi, b_lo, X.gemm_nt)
    out = fake(a_hi, a_lo, b_hi, b_lo).float()
    with pytest.raises(AssertionError, match="first at") as e:
        X.assert_exact(out, X.three_term(t), fake.__name__, t)
    assert hint in str(e.value), str(e.value)
    with pytest.raises(AssertionError, match="first at"):
        X.assert_planes_exact(torch.stack(X.canonical_planes(out)), X.three_term(t), fake.__name__, t)


def test_term_isolation_names_the_fault():
    """With only one pair of planes non-zero, the expected value is one term (or exactly 0 for lo x lo)."""
    a_hi, a_lo, b_hi, b_lo = _planes_case(200, 136, 72)
    z_a, z_b = torch.zeros_like(a_hi), torch.zeros_like(b_hi)
    t = X.plane_terms(z_a, a_lo, z_b, b_lo, X.gemm_nt)              # (lo_a, lo_b) with hi = 0
    assert float(X.three_term(t).abs().max()) == 0.0
    X.assert_exact(X.fake_gemm_correct(z_a, a_lo, z_b, b_lo).float(), X.three_term(t), "lo x lo", t)
    with pytest.raises(AssertionError, match="lo\\*lo"):
        X.assert_exact(X.fake_gemm_adds_lolo(z_a, a_lo, z_b, b_lo).float(), X.three_term(t), "lo x lo", t)
    t = X.plane_terms(z_a, a_lo, b_hi, z_b, X.gemm_nt)              # (lo_a, hi_b): exactly lh
    with pytest.raises(AssertionError, match="term lh is missing"):
        X.assert_exact(X.fake_gemm_drop_cross_term(z_a, a_lo, b_hi, z_b).float(), X.three_term(t), "lh", t)


# ---------------------------------------------------------------------------------------------------------------- fakes: planes writers
def test_correct_split_passes():
    v = X.rounding_probe_values()
    X.assert_planes_bits(*X.canonical_planes(v), v, "canonical")


@pytest.mark.parametrize("fake", [X.fake_split_truncates, X.fake_split_ties_away, X.fake_split_lo_from_unrounded])
def test_wrong_splits_are_rejected(fake):
    v = X.rounding_probe_values()
    hi, lo = fake(v)
    assert bool(torch.isfinite(hi.float()).all())
    with pytest.raises(AssertionError, match="bit patterns wrong"):
        X.assert_planes_bits(hi, lo, v, fake.__name__)
    if fake is not X.fake_split_lo_from_unrounded:
        # the two rounding-mode faults stay within 4 times the two-rounding bound: a 3e-4 tolerance sees nothing of them
        err = (hi.double() + lo.double() - v.double()).abs()
        assert bool((err <= 2.0 ** -14 * v.double().abs())[v.abs() > 2.0 ** -100].all())


def test_two_roundings_fallback():
    """the derived fallback accepts the canonical split of a nearby fp32 value (the last place of the fp32 form may differ) and
    rejects the faults; `hi == bf16(hi + lo)` alone is NOT a property of the canonical split: lo can round up to half an ulp of hi"""
    y = torch.randn(100000, generator=torch.Generator().manual_seed(0))
    hi, lo = X.canonical_planes(y)
    naive = X.plane_bits((hi.double() + lo.double()).float().bfloat16()) == X.plane_bits(hi)
    assert 0 < int((~naive).sum()) < y.numel() // 200
    X.assert_two_roundings(hi, lo, y, "canonical")
    X.assert_two_roundings(hi, lo, torch.nextafter(y, torch.zeros_like(y)), "canonical split of the neighbouring fp32 value")
    for fake in (X.fake_split_truncates, X.fake_split_lo_from_unrounded):
        with pytest.raises(AssertionError):
            X.assert_two_roundings(*fake(y), y, fake.__name__)
    # hi one bf16 step too far, lo making up for it: the sum is still within 2^-16 (on the elements kept), hi is not a nearest
    hi2 = (X.plane_bits(hi) + 1).view(torch.bfloat16)
    lo2 = (y - hi2.float()).bfloat16()
    keep = ((hi2.double() + lo2.double() - y.double()).abs() <= 2.0 ** -16 * y.double().abs()) & (y.abs() > 1e-3)
    assert int(keep.sum()) > 1000
    with pytest.raises(AssertionError, match="nearest"):
        X.assert_two_roundings(hi2[keep], lo2[keep], y[keep], "hi one step off")


def test_ties_away_differs_only_on_ties():
    v = torch.tensor([258.0, 1.0, 3.140625, -0.0, 1000.0, 0.0, 6.0, 7.0])      # exactly representable values, no ties
    hi, lo = X.fake_split_ties_away(v)
    X.assert_planes_bits(hi, lo, v, "no ties")


# ---------------------------------------------------------------------------------------------------------------- the gap
def _rnd(*shape, seed=0, scale=1.0):
    """`rnd` of tests/test_kernels_gpu.py"""
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def test_close_tolerance_accepts_the_k_tail_fault():
    """(M, N, K) = (1024, 128, 768) with the very inputs of test_planes_gemm_family (`rnd` at scale 0.5, canonical planes) and
    its reference (x @ w.T in fp32): a kernel whose weight loader ignores the lo plane in the last 8 of the 768 k values has a
    rel-to-max error of 2.4e-4 and passes `close()` at 3e-4 (the same fault in the activation loader: 3.4e-4, in both: 4.3e-4;
    the scheme's own error: 4.7e-6); a whole dropped cross term (1.6e-3) does not pass.  On integer planes the same fault is
    rejected by the exact compare: test_wrong_contractions_are_rejected."""
    M, N, Kd = 1024, 128, 768
    x, w = _rnd(M, Kd, scale=0.5), _rnd(N, Kd, seed=1, scale=0.5)
    (a_hi, a_lo), (b_hi, b_lo) = ([p.double() for p in X.canonical_planes(t)] for t in (x, w))
    ref = x @ w.T
    good = X.close_rel_to_max(X.fake_gemm_correct(a_hi, a_lo, b_hi, b_lo), ref)
    tail = {ops: X.close_rel_to_max(X.fake_gemm_lo_ignored_in_k_tail(a_hi, a_lo, b_hi, b_lo, operands=ops), ref) for ops in ("b", "a", "ab")}
    dropped = X.close_rel_to_max(X.fake_gemm_drop_cross_term(a_hi, a_lo, b_hi, b_lo), ref)
    print(f"rel-to-max error: correct scheme {good:.3e}; lo ignored in the last 8 of K: {tail}; cross term dropped {dropped:.3e}")
    assert good < 1e-5
    assert good * 10 < tail["b"] < X.CLOSE_TOL_SPLIT, "the K-tail fault is 50 times the scheme's own error and still passes close()"
    assert dropped > X.CLOSE_TOL_SPLIT
