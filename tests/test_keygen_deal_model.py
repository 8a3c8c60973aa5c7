"""CPU tests of the keygen cases (tests/keygen_deal_cases.py): what the GPU tests compare the device with
must itself be a keygen.  Every dealt share passes oracle.keygen.verify_share, the first t shares
reconstruct the secret, the Lagrange combination of the first t verkeys is g~ * secret (the reference's
check_reconstructed_keys, keygen.rs:231-297), every edge case reaches the branch it is named for, and the
combine cases satisfy the DVSS contract (keygen.rs:169-205).

verify_share costs t + 2 point multiplications of the pure-Python oracle a share.  At (33, 40, 1) that is
2,800 of them for the 80 shares (about a minute), so there the ids 1, 2, t and total of both polynomials are
checked; at every other shape every share is."""
import pytest

import keygen_deal_cases as KC
from oracle import bls12_381 as B
from oracle import coconut_ref as C
from oracle import keygen as K

R = B.R


def _ids_to_check(shape):
    t, total, _ = shape
    return range(1, total + 1) if t < 33 else sorted({1, 2, t, total})


@pytest.mark.parametrize("shape", KC.SHAPES, ids=str)
def test_dealt_shares_verify_and_reconstruct(shape):
    t, total, q = shape
    g, h, _ = KC.bases()
    case = KC.pedersen_case(shape, 3 if shape in KC.M3_SHAPES else 1)
    v = case["vals"]
    for k in range(case["m"]):
        for p in range(q + 1):
            comm = v["comm"][(k * (q + 1) + p) * t:(k * (q + 1) + p + 1) * t]
            s = {i: (v["x"][k][i - 1], v["xt"][k][i - 1]) if p == 0 else (v["y"][k][i - 1][p - 1], v["yt"][k][i - 1][p - 1])
                 for i in range(1, total + 1)}
            for i in _ids_to_check(shape):
                assert K.verify_share(t, i, s[i], comm, g, h), (k, p, i)
            if k == 0 and p == 0:
                assert not K.verify_share(t, 1, ((s[1][0] + 1) % R, s[1][1]), comm, g, h)
            sec, sec_t = case["secrets"][k][p]
            assert C.reconstruct_secret(t, {i: s[i][0] for i in range(1, total + 1)}) == sec
            assert C.reconstruct_secret(t, {i: s[i][1] for i in range(1, total + 1)}) == sec_t
            # the rebuilt coefficients are the ones pedersen_deal drew
            o = (k * (q + 1) + p) * t
            assert (case["cf"][o], case["ct"][o]) == (sec, sec_t)
    # the restatement the edge cases rely on gives pedersen_deal's values
    assert KC.restate_deal(t, total, q, case["m"], case["cf"], case["ct"], g, h) == v


@pytest.mark.parametrize("shape", KC.SHAPES, ids=str)
def test_shamir_shares_reconstruct(shape):
    t, total, q = shape
    case = KC.shamir_case(shape)
    v = case["vals"]
    for p in range(q + 1):
        s = {i: v["x"][0][i - 1] if p == 0 else v["y"][0][i - 1][p - 1] for i in range(1, total + 1)}
        assert C.reconstruct_secret(t, s) == case["secrets"][0][p][0] == case["cf"][p * t]
    assert KC.restate_deal(t, total, q, 1, case["cf"], None, None, None) == v


@pytest.mark.parametrize("mode", sorted(KC.MODES))
@pytest.mark.parametrize("shape", KC.SHAPES, ids=str)
def test_reconstructed_verkeys(mode, shape):
    """check_reconstructed_keys: sum_i l_i(0) X~_i == g~ * secret over the first t signers, for x and every y."""
    t, total, q = shape
    case = KC.shamir_case(shape)
    curve, _, dec, ob = KC.oth(mode)
    gt = KC.bases()[2][mode]
    X, Y = KC.verkeys(mode, case["vals"])
    ids = set(range(1, t + 1))
    lag = {i: C.lagrange_basis_at_0(ids, i) for i in ids}
    for p in range(q + 1):
        pts = [dec(X[(i - 1) * ob:i * ob]) if p == 0 else dec(Y[((i - 1) * q + p - 1) * ob:((i - 1) * q + p) * ob])
               for i in sorted(ids)]
        assert curve.msm(pts, [lag[i] for i in sorted(ids)]) == curve.mul(gt, case["secrets"][0][p][0]), p


def test_edge_scalar_cases_reach_their_branches():
    g, h, _ = KC.bases()
    case = KC.edge_unit_case()
    v, names = case["vals"], case["names"]
    assert len(names) == case["m"] and len(set(KC.EDGE_BITS)) > 90
    by = dict(zip(names, range(case["m"])))
    # scalars >= r are reduced: r is zero, r + 1 is one
    assert v["x"][by["f=%#x" % R]] == [0] and v["x"][by["f=%#x" % (R + 1)]] == [1]
    assert v["x"][by["f=%#x" % ((1 << 384) - 1)]] == [((1 << 384) - 1) % R]
    assert v["comm"][by["f=%#x" % R]] == B.G1.mul(h, case["ct"][by["f=%#x" % R]])
    # the zero patterns: identity commitment only when both coefficients vanish
    assert v["comm"][by["all_zero"]] is None and v["x"][by["all_zero"]] == [0]
    assert v["comm"][by["f_zero"]] == B.G1.mul(h, 5) and v["comm"][by["ft_zero"]] == B.G1.mul(g, 7)
    # a boundary bit is alone in its window on one side and in the next window on the other
    for wb in (8, 13):
        for k in range(1, 256 // wb):
            lo, hi = wb * k - 1, wb * k
            assert lo in KC.EDGE_BITS and hi in KC.EDGE_BITS and lo // wb == k - 1 and hi // wb == k
    # every verkey scalar of the batch is its f_0 mod r
    assert [row[0] for row in v["x"]] == [c % R for c in case["cf"]]
    pc = KC.edge_poly_case()
    pv = pc["vals"]
    assert pv["x"][2] == [0, 0, 0] and pv["xt"][2] == [0, 0, 0] and pv["comm"][12:15] == [None] * 3
    assert all(c is not None for c in pv["comm"][15:18]) and [r[0] for r in pv["y"][2]] == [0, 0, 0]
    assert KC.poly([c % R for c in pc["cf"][:3]], 2) == pv["x"][0][1]


def test_related_base_cases_double_cancel_and_restart():
    g = KC.bases()[0]
    for name, h, case, want in KC.related_cases():
        for k, (a, b) in enumerate(zip(case["cf"], case["ct"])):
            ev, acc = KC.window_trace([(g, a), (h, b)], 8)
            assert ev == want[k], (name, k, ev)
            assert acc == case["vals"]["comm"][k]
    doubles, cancels = KC.related_cases()
    assert doubles[2]["vals"]["comm"][0] == B.G1.mul(g, 2 * KC.RELATED_V)
    assert cancels[2]["vals"]["comm"][0] is None
    assert cancels[2]["vals"]["comm"][1] == B.G1.mul(g, -KC.RELATED_U % R)


@pytest.mark.parametrize("mode", sorted(KC.MODES))
def test_bad_base_cases_drop_exactly_the_bad_term(mode):
    cases = KC.bad_base_cases(mode)
    assert len(cases) == (12 if mode == "G2" else 11)
    gtb, gb, hb = KC.base_bytes(mode)
    g, h, gts = KC.bases()
    cf, ct = KC.bad_base_inputs()
    good = KC.pack(KC.restate_deal(2, 2, 1, 1, cf, ct, g, h), mode, gts[mode])
    ob = KC.oth(mode)[3]
    ident = KC.oth(mode)[1](None)
    for name, sgt, sg, sh, exp in cases:
        assert [sgt != gtb, sg != gb, sh != hb].count(True) == 1, name
        assert (exp["x"], exp["y"], exp["xt"], exp["yt"]) == (good["x"], good["y"], good["xt"], good["yt"])
        if name.endswith("coord_ge_p"):
            assert exp == good, name
        elif name.startswith("g_tilde"):
            assert exp["comm"] == good["comm"] and exp["X"] == ident * 2 and exp["Y"] == ident * 2, name
        else:
            assert exp["X"] == good["X"] and exp["comm"] != good["comm"], name
            other = h if name.startswith("g_") else g
            sc = ct if name.startswith("g_") else cf
            assert exp["comm"][:97] == B.g1_to_bytes(B.G1.mul(other, sc[0])), name
    assert len(ident) == ob


def test_combine_cases_satisfy_the_dvss_contract():
    cases = {c[0]: c for c in KC.combine_cases()}
    g, h, _ = KC.bases()
    # d = 5 dealers at (3, 5, 1): share = sum of the dealers' shares, secret = sum of their secrets,
    # commitments = the dealers' sums; the combined shares verify against the combined commitments
    _, m, d, (t, total, q), ins, exp = cases["d5_dealers"]
    big = KC.pedersen_case((3, 5, 1), 5)
    for p in range(q + 1):
        secret = sum(big["secrets"][k][p][0] for k in range(d)) % R
        shares = {i: (exp["xi"][i - 1] if p == 0 else exp["yi"][(i - 1) * q + p - 1]) for i in range(1, total + 1)}
        for i in shares:
            own = [big["vals"]["x"][k][i - 1] if p == 0 else big["vals"]["y"][k][i - 1][p - 1] for k in range(d)]
            assert shares[i] == sum(own) % R
        assert C.reconstruct_secret(t, shares) == secret
        comm = [B.g1_from_bytes(exp["comm"][(p * t + i) * 97:(p * t + i + 1) * 97]) for i in range(t)]
        for i in range(t):
            acc = None
            for k in range(d):
                acc = B.G1.add(acc, big["vals"]["comm"][(k * (q + 1) + p) * t + i])
            assert comm[i] == acc
        bl = exp["xt"] if p == 0 else exp["yt"]
        for i in (1, total):
            o = (i - 1) if p == 0 else (i - 1) * q + p - 1
            assert K.verify_share(t, i, (shares[i], int.from_bytes(bl[o * 48:(o + 1) * 48], "big")), comm, g, h)
    # the branches of the point sum
    name, _, _, _, ins, exp = cases["d1_identity_map"]
    assert all(exp[k] == ins[k] for k in ("x", "y", "xt", "yt", "comm"))
    _, _, _, _, ins, exp = cases["two_equal_dealers"]
    first = B.g1_from_bytes(ins["comm"][:97])
    assert ins["comm"][:388] == ins["comm"][388:] and B.g1_from_bytes(exp["comm"][:97]) == B.G1.dbl(first)
    _, _, _, _, ins, exp = cases["two_opposite_dealers"]
    assert exp["comm"] == KC.G1_ID * 4 and exp["xi"] == [0, 0] and exp["yi"] == [0, 0] and exp["xt"] == bytes(96)
    _, _, _, _, ins, exp = cases["three_dealers_two_opposite"]
    assert exp["comm"] == ins["comm"][2 * 388:] and exp["x"] == ins["x"][2 * 96:]
    _, _, _, _, ins, exp = cases["identity_and_undecodable_commitments"]
    assert [B.g1_from_bytes(ins["comm"][388 + i * 97:388 + (i + 1) * 97]) is None for i in range(4)] == [True] * 3 + [False]
    assert exp["comm"][:3 * 97] == ins["comm"][:3 * 97] and exp["comm"][3 * 97:] != ins["comm"][3 * 97:388]
    _, _, _, _, ins, exp = cases["shares_ge_r"]
    assert int.from_bytes(ins["x"][:48], "big") >= R and int.from_bytes(exp["x"][:48], "big") < R
    assert exp["xi"] == cases["identity_and_undecodable_commitments"][5]["xi"]
    _, m, d, _, ins, exp = cases["two_groups"]
    assert (m, d) == (2, 2) and exp["xi"][:2] == cases["shares_ge_r"][5]["xi"] and len(exp["xi"]) == 4
