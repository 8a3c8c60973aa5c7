"""CPU model of the inputs of tests/test_gpu_fexp_direct.py (tests/fexp_direct_cases.py): for every case,
walk the chain the final-exponentiation kernels run (csrc/fexp_q.hip k_fexp_q, csrc/fexp_pl.hip
k_fexp1) with the oracle's Fp12 arithmetic and assert the regime the case claims.

The chain: easy part g = f^((p^6 - 1)(p^2 + 1)), then five pow-by-x on the bases
    g,  t = g^(x-1),  a = t^(x-1),  b = a^x,  c = b^x                      (d = c^x)
with the result g^3 (a^(p^2) conj(a))^p (b^(p^2) conj(b)) c^p d.  Each pow-by-x runs 57 compressed
squarings of (b0, b1, c0, c1) = coefficients (1, 4, 2, 5) and decompresses the snapshots after 16, 48
and 57 of them with the denominators D = 2 (b0 c0 - xi b1 c1); the product of the three being zero
sends the element to the Granger-Scott square-and-multiply ladder.  A case is 'fallback' when all
three are zero in all five bases, normal when none is in any: nothing in between is admitted, so the
device test's cases reach exactly the branches claimed here.
"""
import pytest

import fexp_direct_cases as C
from oracle import bls12_381 as B
from test_fexp_algebra import comp_sqr, decompress

SNAPS = (16, 48, 57)


def easy_part(f):
    t = B.f12_mul(B.f12_conj(f), B.f12_inv(f))
    return B.f12_mul(B.f12_frob(B.f12_frob(t)), t)


def pow_x(g):
    return B.f12_conj(B.f12_pow(g, B.X_ABS))  # x = -|x|, on the cyclotomic subgroup


def frob2(x):
    return B.f12_frob(B.f12_frob(x))


def chain(f):
    """The five bases and the result, as fexp_q.hip's loop forms them."""
    g = easy_part(list(f))
    t = B.f12_mul(pow_x(g), B.f12_conj(g))
    a = B.f12_mul(pow_x(t), B.f12_conj(t))
    b = pow_x(a)
    c = pow_x(b)
    d = pow_x(c)
    r = B.f12_mul(B.f12_sqr(g), g)
    r = B.f12_mul(B.f12_frob(B.f12_mul(frob2(a), B.f12_conj(a))), r)
    r = B.f12_mul(B.f12_mul(frob2(b), B.f12_conj(b)), r)
    r = B.f12_mul(B.f12_frob(c), r)
    r = B.f12_mul(d, r)
    return [g, t, a, b, c], r


def denominators(base):
    """D after 16, 48 and 57 compressed squarings, and the compressed states there."""
    st = (base[1], base[4], base[2], base[5])
    ds, sts = [], []
    for k in range(1, 58):
        st = comp_sqr(*st)
        if k in SNAPS:
            b0, b1, c0, c1 = st
            ds.append(B.f2_muls(B.f2_sub(B.f2_mul(b0, c0), B.f2_mul_xi(B.f2_mul(b1, c1))), 2))
            sts.append(st)
    return ds, sts


def walk(case):
    """(easy part, per-base regime list, chain result) of one non-zero case."""
    bases, r = chain(case.f)
    regimes = []
    for base in bases:
        ds, sts = denominators(base)
        zeros = [B.f2_is_zero(d) for d in ds]
        assert all(zeros) or not any(zeros), (case.name, zeros)  # nothing in between
        if not zeros[0]:  # the decompression the normal path relies on
            assert decompress(*sts[0]) == B.f12_pow(base, 1 << 16), case.name
        regimes.append(C.FALLBACK if zeros[0] else "normal")
    return bases[0], regimes, r


@pytest.fixture(scope="module")
def walked():
    return {c.name: walk(c) for c in C.cases() if c.kind != C.ZERO_KIND}


def test_every_case_reaches_the_regime_it_claims(walked):
    one = B.f12_one()
    for c in C.cases():
        if c.kind == C.ZERO_KIND:
            assert c.f == C.ZERO and C.expected(c.f) == (C.ZERO_GT, False)
            continue
        g, regimes, r = walked[c.name]
        gt, is_one = C.expected(c.f)
        assert B.gt_to_bytes(r) == gt, c.name  # the kernels' chain is the oracle's final_exp
        if c.kind == C.FALLBACK:
            assert g == one and regimes == [C.FALLBACK] * 5 and is_one and gt == C.ONE_GT, c.name
        else:
            assert g != one and regimes == ["normal"] * 5, c.name
            assert is_one == (c.kind == C.RTH), c.name
            assert (gt == C.ONE_GT) == (c.kind == C.RTH), c.name


def test_support_patterns_split_17_to_46(walked):
    """The elements the easy part kills form the group Fp4* Fp6* (order (p^4 - 1)(p^4 + p^2 + 1), W in it);
    a coordinate subspace lies in it only as W^j Fp4 ({j, j + 3}: 3 patterns) or inside W^j Fp6 (the 7
    non-empty subsets of {0, 2, 4} and of {1, 3, 5}: 14 patterns, the 6 singletons W^j Fp2 among them)."""
    sup = [c for c in C.cases() if c.family == "supports" and c.name.count("_") == 0]
    assert sorted(C.support_of(c.f) for c in sup) == sorted(
        tuple(k for k in range(6) if m >> k & 1) for m in range(1, 64))
    fb = [c for c in sup if walked[c.name][1] == [C.FALLBACK] * 5]
    nm = [c for c in sup if walked[c.name][1] == ["normal"] * 5]
    assert (len(fb), len(nm)) == (17, 46)
    # the fallback supports are exactly those inside W^j times a proper subfield
    assert all(C.support_in_subfield_coset(C.support_of(c.f)) for c in fb)
    assert not any(C.support_in_subfield_coset(C.support_of(c.f)) for c in nm)
    for c in C.cases():
        if c.family in ("units", "subfield", "one"):
            assert c.kind == C.FALLBACK and walked[c.name][1] == [C.FALLBACK] * 5, c.name


def test_families_are_what_they_say():
    cs = C.cases()
    assert len({c.f for c in cs}) <= 115  # the oracle's final_exp runs once per distinct input
    for c in cs:
        assert all(0 <= v < C.P for co in c.f for v in co)
    units = [c for c in cs if c.family == "units"]
    assert len(units) == 24 and len({c.f for c in units}) == 24
    for c in units:
        halves = [v for co in c.f for v in co]
        assert sorted(halves)[:11] == [0] * 11 and max(halves) in (1, C.P - 1)
    for tag, v in (("pm1", C.P - 1), ("ones", 1)):
        var = [c for c in cs if c.name.endswith("_" + tag) and c.family == "supports"]
        assert {c.kind for c in var} == {C.FALLBACK, C.GENERIC}
        assert all(co in (C.F2Z, (v, v)) for c in var for co in c.f)
    assert C.support_of(C.by_name("sub_fp4").f) == (0, 3) and C.support_of(C.by_name("sub_fp6").f) == (0, 2, 4)
    assert C.by_name("sub_fp").f[0][1] == 0 and C.by_name("one").f == C.ONE


def test_scaling_by_fp_leaves_the_gt_unchanged():
    base = C.by_name("scale_base")
    scaled = [c for c in C.cases() if c.same_as == "scale_base"]
    assert len(scaled) == 3
    for c in scaled:
        assert c.f != base.f and C.expected(c.f) == C.expected(base.f), c.name
        k = c.f[0][0] * pow(base.f[0][0], -1, C.P) % C.P
        assert tuple(B.f2_muls(x, k) for x in base.f) == c.f
    assert C.expected(base.f)[0] != C.ONE_GT


def test_rth_powers_end_at_one_through_the_normal_path(walked):
    rth = C.of_kind(C.RTH)
    assert len(rth) >= 2
    for c in rth:
        g, regimes, r = walked[c.name]
        assert regimes == ["normal"] * 5 and g != B.f12_one() and r == B.f12_one()
        assert len(C.support_of(c.f)) == 6  # dense


def test_every_regime_is_populated():
    """A condition on the inputs: the device test draws from each kind, and from sparse, non-trivial
    fallback values (not only f = 1)."""
    for kind in C.KINDS:
        assert C.of_kind(kind), kind
    fb = C.of_kind(C.FALLBACK)
    assert sum(1 for c in fb if c.f != C.ONE) >= 40
    assert any(len(C.support_of(c.f)) == 3 for c in fb) and any(len(C.support_of(c.f)) == 2 for c in fb)
    assert sum(1 for c in C.of_kind(C.GENERIC) if len(C.support_of(c.f)) < 6) >= 40


def test_encoder_round_trips():
    fs = [c.f for c in C.cases()]
    assert C.decode(C.encode(fs), len(fs)) == fs
    assert C.decode(C.encode(fs[:1]), 1) == fs[:1]
    w = C.encode([C.ONE, C.ZERO, C.by_name("generic0").f])
    assert w.shape == (3 * C.F12_WORDS,)
    # word w of Fp slot k of element i at (k * 12 + w) * n + i; one = R in slot 0, zero elsewhere
    assert [int(w[(0 * 12 + j) * 3 + 0]) for j in range(12)] == [(C.R_STORE >> (32 * j)) & 0xFFFFFFFF for j in range(12)]
    assert all(int(w[(k * 12 + j) * 3 + 0]) == 0 for k in range(1, 12) for j in range(12))
    assert all(int(w[(k * 12 + j) * 3 + 1]) == 0 for k in range(12) for j in range(12))
    # slots follow the AMCL order a.a, a.b, b.a, b.b, c.a, c.b = W^0, W^3, W^1, W^4, W^2, W^5
    g = C.by_name("generic0").f
    for s, k in enumerate(B.AMCL_SLOT_TO_W):
        for h in range(2):
            v = sum(int(w[((2 * s + h) * 12 + j) * 3 + 2]) << (32 * j) for j in range(12))
            assert v == g[k][h] * C.R_STORE % C.P
