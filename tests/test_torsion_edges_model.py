"""CPU test of the small-order inputs themselves (tests/torsion_edges.py, tests/golden/torsion.json): a
condition on the INPUTS that tests/test_gpu_torsion_edges.py feeds the device, not on the device.

* every fixture point has the order it carries, by the definition; the two order-13 points are
  independent; every one is on the curve and outside the subgroup by both the definition and the
  endomorphism tests the device runs; gcd(h2, p - x) = 1, which is what makes the psi test sound;
* the walks reach what the device test relies on: order 13 meets add-to-inverse, three doublings at the
  identity and add-at-identity in the Miller chain and in the psi ladder; orders 23, 299 and the mixed
  points meet nothing; G1 order 3 meets all four events in [x^2] P, order 11 meets add-of-equal.
  UNREACHABLE BY CONSTRUCTION: add-of-equal on the twist (and in G1 outside orders 3 and 11 of the
  fixture): T = Q before an addition needs (k - 1) Q = O for a pre-addition prefix k of |x|, and
  gcd(h2 r, k - 1) = 1 for every such k (asserted here, with the same for k + 1 restricted to 13: the only
  add-to-inverse is the order-13 one).  A whole window 2^(wbits w) B of a table is never the identity for a
  base of odd order (2 is a unit): that branch of k_table_fill is reached by an identity base alone;
* the model's T follows the walk: (0 : Y : 0) after the add-to-inverse, (0, 0, 0) from the add-at-identity on;
* the C oracle and the projective Python model agree byte for byte on GT for every G2 fixture point
  against a fixed G1 point and for every G1 fixture point against a fixed G2 point; for order 13 the Miller
  value is zero and GT is 576 zero bytes;
* the table walk: at widths 8 and 10 the fixture's orders put identity entries first in a run, strictly
  inside one and last in one, and reach the acc = +P, acc = -P and acc = O branches of jac_add_aff;
  whatever the model says is reachable for an order is reached by the runs the device builds (all of them).
"""
import math

import pytest

import torsion_edges as T
from oracle import bls12_381 as B
from oracle import subgroup as S

FX = T.fixture()
G2_ORDERS = {n: r["order"] for n, r in FX["G2"].items()}
G1_ORDERS = {n: r["order"] for n, r in FX["G1"].items()}


def _pt(group, name):
    b = FX[group][name]["point"]
    return B.g1_from_bytes(b) if group == "G1" else B.g2_from_bytes(b)


def test_fixture_names():
    assert list(FX["G2"]) == ["T13", "T13b", "T23", "T13+T23", "kG+T13", "k2G+T13", "-T13"]
    assert list(FX["G1"]) == ["T3", "-T3", "T11", "kG+T11", "kG+T3"]
    assert FX["G1"]["T3"]["point"] == b"\x04" + bytes(48) + (2).to_bytes(48, "big")
    assert FX["G1"]["-T3"]["point"] == b"\x04" + bytes(48) + (B.P - 2).to_bytes(48, "big")
    assert [G2_ORDERS[n] for n in FX["G2"]] == [13, 13, 23, 299, 13 * B.R, 13 * B.R, 13]
    assert [G1_ORDERS[n] for n in FX["G1"]] == [3, 3, 11, 11 * B.R, 3 * B.R]


@pytest.mark.parametrize("group,name", [(g, n) for g in ("G1", "G2") for n in FX[g]])
def test_fixture_orders_and_status(group, name):
    curve = B.G1 if group == "G1" else B.G2
    P, m = _pt(group, name), FX[group][name]["order"]
    assert P is not None and curve.on_curve(P)
    assert curve.mul_any(P, m) is None
    for ell in (3, 11, 13, 23, B.R):
        if m % ell == 0:
            assert curve.mul_any(P, m // ell) is not None, ell
    # status 1: on the curve, outside the subgroup, by the definition and by the device's test
    assert not S.in_subgroup_def(curve, P)
    assert not (S.in_g1_endo(P) if group == "G1" else S.in_g2_endo(P))
    k = FX[group][name]["k"]
    if k is not None:  # the mixed points are what their names say
        tors = _pt(group, {"kG+T13": "T13", "k2G+T13": "T13", "kG+T11": "T11", "kG+T3": "T3"}[name])
        assert curve.add(curve.mul(curve.gen, k), tors) == P


def test_order13_points_independent_and_related():
    a, b = _pt("G2", "T13"), _pt("G2", "T13b")
    assert b not in [B.G2.mul_any(a, k) for k in range(13)]
    assert _pt("G2", "-T13") == B.G2.neg(a)
    assert _pt("G2", "T13+T23") == B.G2.add(a, _pt("G2", "T23"))


def test_cofactors():
    assert S.H2 % 13 ** 2 == 0 and S.H2 % 23 ** 2 == 0 and S.H1 % 3 == 0 and S.H1 % 11 ** 2 == 0
    assert S.H1 == (T.X_ABS + 1) ** 2 // 3
    # psi acts on the twist with psi^2 - t psi + p = 0; on a point with psi(Q) = [x] Q the order divides
    # a combination that gcd(h2, p - x) = 1 confines to r (eprint 2021/1130 section 4)
    assert math.gcd(S.H2, B.P + T.X_ABS) == 1  # p - x, x = -|x|


def _kinds(ev):
    return [e for _, _, e in ev]


def test_miller_and_psi_walks_reach_the_branches():
    want13 = ["add-to-inverse", "double-at-identity", "double-at-identity", "double-at-identity", "add-at-identity"]
    mil = T.miller_events(13)
    assert _kinds(mil) == want13
    assert [b for b, _, _ in mil] == [60, 59, 58, 57, 57]  # bits of |x| below the top one, 62 first
    psi = T.psi_events(13)
    assert _kinds(psi)[:5] == want13 and set(want13) <= set(_kinds(psi))
    for m in (23, 299, 13 * B.R):
        assert T.miller_events(m) == [] and T.psi_events(m) == [], m
    assert T.X_ABS % 23 == 8


def test_unreachable_by_construction():
    """UNREACHABLE BY CONSTRUCTION: add-of-equal on the twist."""
    pre = T.add_prefixes(T.X_ABS)
    assert len(pre) == 5  # |x| has Hamming weight 6
    for k in pre:
        assert math.gcd(S.H2 * B.R, k - 1) == 1, k  # (the issue's 2k - 1 with k the prefix before the doubling)
    # add-to-inverse and the identity need (k + 1) Q = O or k Q = O: 13 alone among the twist's orders
    for k in pre:
        assert math.gcd(S.H2 * B.R, k + 1) in (1, 13) and math.gcd(S.H2 * B.R, k) in (1, 13), k
    for m in G2_ORDERS.values():
        assert "add-of-equal" not in _kinds(T.miller_events(m)) + _kinds(T.psi_events(m))
    # a table window 2^(wbits w) B keeps the order of B
    for m in (3, 11, 13, 23):
        for wbits in (8, 10):
            nwin = (256 + wbits - 1) // wbits
            assert all(pow(2, wbits * w, m) for w in range(nwin))
            assert not any(T.window_is_identity(wbits, w, m) for w in range(nwin))
            # the whole-window branch is an identity base's (inf[j]): tests/test_gpu_torsion_edges.py puts one
            # next to the small-order bases of every table it builds
            assert all(T.window_is_identity(wbits, w, m, base_inf=True) for w in range(nwin))


def test_phi_walk_reaches_the_branches():
    assert set(_kinds(T.phi_events(3))) == set(T.EVENTS)
    assert "add-of-equal" in _kinds(T.phi_events(11))
    for m in (11 * B.R, 3 * B.R):
        assert T.phi_events(m) == []


def test_model_T_follows_the_walk():
    Q, Pt = _pt("G2", "T13"), B.G1.mul(B.G1.gen, 7)
    tr = []
    f = T.miller(Q, Pt, tr)
    z = B.F2_ZERO
    # steps: dbl add | dbl | dbl add(-> O) | dbl dbl dbl add(-> (0, 0, 0))
    assert tr[4][0] == z and tr[4][2] == z and tr[4][1] != z  # (0 : Y : 0)
    for k in (5, 6, 7):
        assert tr[k][0] == z and tr[k][2] == z and tr[k][1] != z
    assert all(t == (z, z, z) for t in tr[8:])
    assert all(c == z for c in f)  # the Miller value is zero
    # curve_pl.h miller_t_in_subgroup on that T: X = psi_x Z and Y = -psi_y Z hold (0 = 0), so its Z != 0
    # clause alone keeps the order-13 point out of the subgroup
    ps, (X, Y, Z) = S.psi(Q), tr[-1]
    assert B.f2_mul(ps[0], Z) == X and B.f2_neg(B.f2_mul(ps[1], Z)) == Y and Z == z
    # order 23 and a mixed point: T stays a finite point and ends as [|x|] Q
    for name in ("T23", "kG+T13"):
        Q, tr = _pt("G2", name), []
        T.miller(Q, Pt, tr)
        assert all(t[2] != z for t in tr)
        X, Y, Z = tr[-1]
        zi = B.f2_inv(Z)
        assert (B.f2_mul(X, zi), B.f2_mul(Y, zi)) == B.G2.mul_any(Q, T.X_ABS)


def test_model_agrees_with_affine_oracle_on_the_subgroup():
    Pt, Q = B.G1.mul(B.G1.gen, 5), B.G2.mul(B.G2.gen, 9)
    assert B.gt_to_bytes(T.final_exp(T.miller(Q, Pt))) == B.gt_to_bytes(B.pairing(Pt, Q))


@pytest.mark.parametrize("name", list(FX["G2"]))
def test_oracle_and_model_agree_on_gt_g2(oc, name):
    Pt = B.G1.mul(B.G1.gen, 0xC0C0)
    gt = T.gt_bytes([(Pt, _pt("G2", name))])
    assert T.oc_pairing(oc, B.g1_to_bytes(Pt), FX["G2"][name]["point"]) == gt
    if G2_ORDERS[name] == 13:
        assert gt == bytes(576)
    else:
        assert any(gt) and gt != B.gt_to_bytes(B.f12_one())


@pytest.mark.parametrize("name", list(FX["G1"]))
def test_oracle_and_model_agree_on_gt_g1(oc, name):
    Q = B.G2.mul(B.G2.gen, 0xC0C0)
    gt = T.gt_bytes([(_pt("G1", name), Q)])
    assert T.oc_pairing(oc, FX["G1"][name]["point"], B.g2_to_bytes(Q)) == gt
    if G1_ORDERS[name] % B.R:  # e(T, Q) has order dividing gcd(m, r) = 1
        assert gt == B.gt_to_bytes(B.f12_one())


def test_oracle_verify_rejects_order13_sigma(oc):
    """oc_verify_batch with sigma_1 = T13 and, separately, sigma_2 = T13: verdict 0 and 576 zero bytes."""
    from conftest import golden
    d = golden("verify_g2_q6.json")
    c = next(c for c in d["creds"] if c["kind"] == "valid")
    h = bytes.fromhex
    Y = b"".join(h(y) for y in d["vk"]["Y"])
    msgs = b"".join(h(m) for m in c["msgs"])
    t13 = FX["G2"]["T13"]["point"]
    for s1, s2 in ((t13, h(c["sigma2"])), (h(c["sigma1"]), t13)):
        v, gt = T.oracle_verify(oc, 0, 1, d["q"], s1, s2, msgs, h(d["vk"]["X"]), Y, h(d["g_tilde"]), 0, 1)
        assert v == [0] and gt == bytes(576)


@pytest.mark.parametrize("wbits", [8, 10])
def test_table_walk_positions_and_branches(wbits):
    pos = {m: T.table_positions(wbits, m) for m in (3, 11, 13, 23)}
    runs = ((1 << wbits) - 1 + T.FILL_RUN - 1) // T.FILL_RUN
    for m, p in pos.items():  # the model against the arithmetic: entry d is the identity iff m | d
        got = sorted(r * T.FILL_RUN + 1 + i for k in p for r, i in p[k])
        assert got == [d for d in range(1, 1 << wbits) if d % m == 0], (wbits, m)
    # the G1 bases (3, 11) and the G2 bases (13, 23) each reach all three positions at this width
    # (UNREACHABLE BY CONSTRUCTION: 'last' for the twist's orders at 8 bits: a run ends at d = 32 k, k <= 7, or
    # at d = 255 = 3 * 5 * 17, and neither 13 nor 23 divides any of those; at 10 bits d = 416 = 32 * 13 does it)
    last = [32 * k for k in range(1, (1 << wbits) // 32)] + [(1 << wbits) - 1]
    for group in ((3, 11), (13, 23)):
        for k in ("first", "inside", "last"):
            reachable = k != "last" or any(d % m == 0 for d in last for m in group)
            assert any(pos[m][k] for m in group) == reachable, (wbits, group, k)
            assert reachable or (wbits, group) == (8, (13, 23))
    assert pos[3]["first"][0] == (1, 0) and pos[3]["last"][0] == (2, 31)  # d = 33 and d = 96
    assert pos[13]["first"][0] == (2, 0)  # d = 65
    if wbits == 10:
        assert (12, 31) in pos[13]["last"]  # d = 416
    else:
        assert pos[13]["last"] == [] and pos[3]["last"][-1] == (7, 30)  # the short last run ends at d = 255
    # the branches of jac_add_aff: whatever an order can reach over all runs, the build (all runs) reaches
    for m in (3, 11, 13, 23):
        tot = {k: 0 for k in ("add-of-equal", "add-to-inverse", "add-at-identity")}
        dbl0 = 0
        for run in range(runs):
            t = T.table_events(wbits, run, m)
            for k in tot:
                tot[k] += t["adds"][k]
            dbl0 += t["dbl_at_identity"]
        assert all(tot.values()), (wbits, m, tot)
        assert dbl0 >= runs  # every run's double-and-add starts by doubling the identity
    # a run that starts ON an identity entry: the first entry's Z is zero and the run goes on from it
    t = T.table_events(wbits, 1, 3)
    assert t["d0"] == 33 and t["identity"][0] == 0 and t["adds"]["add-at-identity"] >= 1
