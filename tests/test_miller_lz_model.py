"""CPU checks of the inputs and expectations of tests/test_gpu_miller_lz_direct.py
(tests/miller_lz_cases.py): conditions on what the device test feeds the pair-lane Miller loops and on
what it expects back, not on the device.

* the R' and storage encodings round-trip and land at the documented words of the prep;
* every expectation formula (two-pair SigG2 / SigG1, twin, quad) obeys bilinearity on the last two of the
  16 pairs: e(a P, Q) = e(P, a Q) = e(P, Q)^a, also for the constant's pair alone;
* the flag rotation reaches every (flag word, pair position, real point or garbage) combination in both
  halves of the first 128-element block of the largest launches, and every computed pair is a real one;
* the tail positions at each listed n are the ones the cases module's docstring claims;
* the twist points of the qcheck tests have the orders their names say;
* the launches built for one property (inverse couples, exchanged credentials) have the expectations
  the device test relies on.
"""
import numpy as np
import pytest

import fexp_direct_cases as C
import miller_lz_cases as M
import miller_wide_cases as W
from oracle import bls12_381 as B
from oracle import subgroup as S


def _value(words, r_inv):
    v = sum(int(x) << (32 * k) for k, x in enumerate(words))
    assert v < B.P
    return v * r_inv % B.P


def test_encodings_round_trip():
    assert M.R_LAZY == pow(2, 392, B.P) and C.R_STORE == pow(2, 406, B.P)
    for p, q in W.pairs() + ((M.gtilde1(), M.gtilde2()),):
        pw, qw, sw = M.p_words(p), M.q_words(q), M.p_store_words(p)
        assert (M.lazy_value(pw[:12]), M.lazy_value(pw[12:])) == p
        assert (_value(sw[:12], C.R_STORE_INV), _value(sw[12:], C.R_STORE_INV)) == p
        got = [_value(qw[12 * k:12 * k + 12], C.R_STORE_INV) for k in range(4)]
        assert ((got[0], got[1]), (got[2], got[3])) == q
    for v in (0, 1, B.P - 1):
        assert M.lazy_value(M._words(v, M.R_LAZY)) == v
    assert not B.G1.on_curve(M.OFFCURVE_P) and not B.G2.on_curve(M.OFFCURVE_Q)
    assert B.G1.on_curve(M.gtilde1()) and M.gtilde1() != B.G1.gen
    assert B.G2.on_curve(M.gtilde2()) and M.gtilde2() not in (B.G2.gen, M.gtilde2(1))


@pytest.mark.parametrize("kind", M.KINDS)
def test_prep_word_positions(kind):
    """Word w of Fp slot s of element i at (s * 12 + w) * pstride + i; what no slot owns holds the fill."""
    n = 5
    creds = M.layout(kind, n)
    m = M.elements_in(kind, n)
    for pstride, fill in ((m, 0), (m + 5, 0xFFFFFFFF)):
        a = M.encode_prep(kind, creds, pstride, fill)
        assert a.shape == (M.PREP_SLOTS * 12 * pstride,)
        owned = np.zeros(a.shape, dtype=bool)
        for e, pos, slot, sides in M.cells(kind, creds):
            assert slot.kind == M.REAL and e < m
            if "q" in sides:
                for k, v in enumerate(slot.q[0] + slot.q[1]):
                    idx = [((M.S_Q[pos] + k) * 12 + w) * pstride + e for w in range(12)]
                    assert _value(a[idx], C.R_STORE_INV) == v
                    owned[idx] = True
            if "p" in sides:
                for k, v in enumerate(slot.p):
                    idx = [((M.S_P[pos] + k) * 12 + w) * pstride + e for w in range(12)]
                    assert M.lazy_value(a[idx]) == v
                    owned[idx] = True
        assert (a[~owned] == fill).all()
        per_elem = {"g2": 48 + 24 + 48, "g1": 48 + 24 + 24}.get(kind)
        assert int(owned.sum()) == (n * per_elem if per_elem else n * 72)
    assert list(M.flags_of(creds)) == [0] * n
    assert (M.S_Q, M.S_P) == ((W.S_Q1, 4), (W.S_P1, 11))


def test_plain_block_holds_the_sixteen_pairs():
    for kind in M.KINDS:
        creds = M.layout(kind, M.PLAIN[kind] + 3)
        assert [cr[-1] for cr in creds[:M.PLAIN[kind]]] == [0] * M.PLAIN[kind]
        assert [(cr[0].p, cr[0].q) for cr in creds[:M.NPAIR]] == list(W.pairs())
        assert M.PLAIN[kind] >= 8 * M.NP[kind]  # the 8 recorded elements are plain


@pytest.mark.parametrize("kind", M.KINDS)
def test_expectations_obey_bilinearity(oc, kind):
    creds, rel = M.bilinear_launch(kind)
    gts = M.expected(oc, kind, creds)
    assert len(gts) == M.outputs(kind, len(creds)) and len(rel) == (2 if M.NP[kind] == 1 else 1)
    for a, b, base in rel:
        assert gts[a] != gts[base] and M.ONE_GT not in (gts[a], gts[base])
        if b is not None:
            assert gts[a] == gts[b]
        assert B.gt_to_bytes(B.f12_pow(list(B.gt_from_bytes(gts[base])), W.A)) == gts[a]
    # a product formula: the plain block's first element is the product of its pairs' own pairings
    plain = M.layout(kind, 4)
    pr = W.pairs()
    e = [B.gt_from_bytes(M.pairing_gt(oc, *pr[t])) for t in range(4)]
    if kind == "g2":
        want = B.f12_mul(list(e[0]), list(B.gt_from_bytes(M.pairing_gt(oc, M.gtilde1(), M.second(0)[1]))))
    elif kind == "g1":
        want = B.f12_mul(list(e[0]), list(B.gt_from_bytes(M.pairing_gt(oc, M.second(0)[0], M.gtilde2()))))
    else:
        want = list(e[0])
        for t in range(1, M.NP[kind]):
            want = B.f12_mul(want, list(e[t]))
    assert M.expected(oc, kind, plain)[0] == B.gt_to_bytes(want)


def test_oracle_pairing_is_the_python_pairing(oc):
    p, q = W.pairs()[0]
    assert M.pairing_gt(oc, p, q) == W.gt_of_pair(0)


@pytest.mark.parametrize("kind", M.KINDS)
def test_flag_rotation_reaches_every_combination(kind):
    npos = M.NP[kind]
    for n in M.SIZES[kind][-3:]:
        creds = M.layout(kind, n)
        M.computed_pairs(kind, creds, "g")  # asserts that no computed pair lies over garbage
        assert M.coverage(kind, creds, 0, n) >= M.full_coverage(kind), n
    creds = M.layout(kind, M.SIZES[kind][-1])
    half = M.BLOCK_PAIRS // 2
    for lo in (0, half):
        assert M.coverage(kind, creds, lo, lo + half) >= M.full_coverage(kind), (kind, lo)
    # every kind of garbage occurs, and a wave (32 elements) past the plain block mixes skipped and computed pairs
    assert {cr[0].kind for cr in creds} == {M.REAL} | set(M.GARBAGE)
    first = M.PLAIN[kind] // npos
    for lo in range(first, M.BLOCK_PAIRS, 32):
        fl = [cr[-1] for c, cr in enumerate(creds) if lo <= c // npos < lo + 32]
        skipped = [any(M.skips2(f)) if npos == 1 else M.skips1(f) for f in fl]
        assert any(skipped) and not all(skipped), (kind, lo)
    # the words named as not skipping do not skip
    assert [f for f in M.FLAGS2 if not any(M.skips2(f))] == [0, 8, 32, 0x28, 0xFFFFFFE8]
    assert [f for f in M.FLAGS2 if M.skips2(f) == (True, False)] == [1, 4, 5, 0x80000001]
    assert [f for f in M.FLAGS2 if M.skips2(f) == (False, True)] == [2, 16, 18]
    assert [f for f in M.FLAGS2 if M.skips2(f) == (True, True)] == [3, 20, 23]
    assert [f for f in M.FLAGS1 if M.skips1(f)] == [1, 4, 5]


def test_tail_positions():
    for kind in ("g2", "g1"):
        assert all(M.absent(kind, n) == [] for n in M.SIZES[kind])
    for kind in ("twin", "quad"):
        for n in M.SIZES[kind]:
            m = M.elements_in(kind, n)
            assert m == (n + 1) // 2 and M.outputs(kind, n) == (n + M.NP[kind] - 1) // M.NP[kind]
            owned = {(e, pos) for e, pos, _, _ in M.cells(kind, M.layout(kind, n))}
            every = {(e, pos) for e in range(m) for pos in (0, 1)}
            assert set(M.absent(kind, n)) == every - owned
            assert M.absent(kind, n) == ([((n - 1) // 2, 1)] if n % 2 else [])
            # the quad loop's absent credentials: those inside the prep are exactly these
            if kind == "quad":
                gone = [(c // 2, c & 1) for c in range(n, 4 * M.outputs(kind, n))]
                assert [g for g in gone if g[0] < m] == M.absent(kind, n)
    assert [n for n in M.SIZES["twin"] if n % 2] == [1, 3, 255, 257]
    assert [n % 4 for n in M.SIZES["quad"]] == [1, 2, 3, 0, 1, 3, 0, 1]


def test_twist_points_have_the_orders_their_names_say():
    tw = M.twist_points()
    assert list(tw) == ["T13", "T23", "kG+T13", "random"]
    assert [tw[k][1] for k in tw] == [13, 23, 13 * B.R, None]
    for name, (q, order) in tw.items():
        assert B.G2.on_curve(q) and B.G2.mul_any(q, B.R) is not None, name  # outside G2
        assert not S.in_g2_endo(q), name
        if order is None:
            assert B.G2.mul_any(q, S.H2 * B.R) is None
            continue
        assert B.G2.mul_any(q, order) is None, name
        for ell in (13, 23, B.R):
            if order % ell == 0:
                assert B.G2.mul_any(q, order // ell) is not None, (name, ell)
    for kind, where in M.TWIST_WHERE.items():  # every pair position, and the last credential of an odd launch
        n = len(M.twist_launch(kind, 0, tw["T23"][0]))
        assert n % 2 == 1 and where[-1] == n - 1
        assert {c % M.NP[kind] for c in where} == set(range(M.NP[kind]))
        for c in where:
            creds = M.twist_launch(kind, c, tw["T23"][0], 4)
            assert [cr[-1] for cr in creds] == [4 if k == c else 0 for k in range(n)]
            assert [cr[0].q == tw["T23"][0] for cr in creds] == [k == c for k in range(n)]


@pytest.mark.parametrize("kind", ["twin", "quad"])
def test_property_launches(oc, kind):
    npos = M.NP[kind]
    n = 4 * npos
    inv = M.inverse_launch(kind, n)
    assert M.expected(oc, kind, inv) == [M.ONE_GT] * 4
    single = M.expected(oc, kind, M.inverse_launch(kind, n, single=True))
    assert M.ONE_GT not in single and len(set(single)) == 4
    for size in (3 * npos, M.BLOCK_PAIRS * npos + 4):
        creds = M.layout(kind, size)
        swapped, (ea, eb) = M.exchange(kind, creds)
        assert ea != eb and sorted(map(repr, swapped)) == sorted(map(repr, creds))
        if size > M.BLOCK_PAIRS * npos:
            assert ea == M.BLOCK_PAIRS - 1 or ea < M.BLOCK_PAIRS <= eb
        g0, g1 = M.expected(oc, kind, creds), M.expected(oc, kind, swapped)
        assert [e for e in range(len(g0)) if g0[e] != g1[e]] == [ea, eb]
