"""CPU test of the variable-base Straus edge cases themselves (tests/straus_edges.py): a condition on the
INPUTS that tests/test_gpu_straus_edges.py feeds the device, not on the device.

* recode_w4's restatement recomposes every edge scalar; the digits lie in [-7, 8] (so |d| <= 8; -8 cannot
  occur) and d[64] = 0, d[63] <= 7 for every canonical scalar: the 65th window is dead for reduced input,
  and d[63] = 8 needs a raw value >= r (RAW_ONLY), which no caller lets through;
* cck_msm_straus's choice of G restated, and what it gives for the t the device test uses;
* every named case reaches its branch in the layout it names, the model's sum equals the constructed one;
* per layout the union of the cases reaches all five chain branches, all five join branches (the
  one-chain layouts lane and pair have no join), a mid-walk round of skipped doublings, and in the table
  build of the G1 layouts the exceptional branches of an order-3 base.  UNREACHABLE BY CONSTRUCTION: the
  table build in the G2 layouts (pair, wide8, pairsG) takes the general branch alone, since k P = O, P or -P
  for k in 2 .. 8 needs a point of order below 13 and the twist has none; its order-13 base is in every G2
  case list all the same (straus_edges docstring), and its rows are asserted present;
* the oracle agrees with the constructed expectations: verdicts, aggregated points, the order-3 and the
  order-13 point.
"""
import ctypes
import random

import pytest

import straus_edges as S
from conftest import host_threads
from fixed_edges import CHAIN, G1_IDENTITY, G2_IDENTITY, JOIN, R, be48, gen_mul

MODES = (0, 1)
ORDER3 = {"to-identity", "from-identity", "doubling"}


def _recompose(d):
    return sum(v << (4 * w) if v >= 0 else -((-v) << (4 * w)) for w, v in enumerate(d))


def test_recode_w4_recomposes_every_edge_scalar():
    rng = random.Random(5)
    for m in S.edge_scalars() + [rng.randrange(R) for _ in range(2000)]:
        d = S.digits(m)
        assert len(d) == 65 and _recompose(d) == m % R, hex(m)
        assert all(-7 <= v <= 8 for v in d), hex(m)
        assert d[64] == 0 and d[63] <= 7, hex(m)  # canonical input: the 65th window is dead
    for raw in S.RAW_ONLY:  # a top nibble of 7 with an incoming carry: only above r
        d = S.recode_w4(raw)
        assert raw >= R and d[63] == 8 and d[64] == 0 and _recompose(d) == raw
    assert S.recode_w4((1 << 256) - 1)[64] == 1  # the 65th digit is live for raw values only
    # the named edges are what they claim
    assert S.digits(8)[:2] == [8, 0] and S.digits(9)[:2] == [-7, 1] and S.digits(16)[:2] == [0, 1]
    assert S.digits(int("F" * 63, 16)) == [-1] + [0] * 62 + [1, 0]  # a carry through 63 windows
    assert S.digits(int("8" * 63, 16)) == [8] * 63 + [0, 0]
    assert S.digits(int("6" + "F" * 63, 16))[63] == 7 and S.digits(R - 1)[63] == 7
    for w in (0, 31):
        assert S.digits(8 << (4 * w))[w] == 8 and S.digits(9 << (4 * w))[w:w + 2] == [-7, 1]
    assert S.digits(R) == [0] * 65 and S.digits(R + 5)[0] == 5


def test_pairs_per_task_rule():
    want = {1: 4, 2: 4, 3: 4, 5: 5, 17: 9, 33: 11}
    for t in S.AGG_T:
        assert S.straus_pairs(t) == want[t]
        for ntask in range(1, 65):
            for cus in (32, 64, 256, 304):
                assert S.straus_pairs_launch(t, ntask, cus) == S.straus_pairs(t), (t, ntask, cus)
    gs = {t: S.straus_pairs(t) for t in S.AGG_T}
    assert any(g & (g - 1) for g in gs.values())  # a G that is no power of two
    assert any(g > t for t, g in gs.items())  # idle pairs
    assert any(t > g for t, g in gs.items())  # two bases on one pair


def _all_traces():
    """(layout, name, trace, expected, reach for that layout) for every case of every caller."""
    for mode in MODES:
        for q in S.VERIFY_Q:
            for c in S.verify_cases(mode, q):
                for lay in S.VERIFY_LAYOUTS[mode]:
                    yield (lay, f"verify{mode}/q{q}/{c['name']}", S.trace(lay, c["logs"], c["msgs"], c["xlog"]),
                           S.expected(c["logs"], c["msgs"], c["xlog"]), [(w, b) for l, w, b in c["reach"] if l == lay])
    for lay in ("lanes16", "pairsG"):
        for t in S.AGG_T:
            for r in S.agg_rows(lay, t):
                yield (lay, f"agg/t{t}/{r['name']}", S.trace(lay, r["logs"][:t], r["scalars"]),
                       S.expected(r["logs"][:t], r["scalars"]), r["reach"])
    for mode in MODES:
        lay = S.SIG_LAYOUT[mode]
        for k in S.BLIND_K:
            for call in S.blind_sets(mode, k):
                for rq in call["requests"]:
                    for which, last in (("a", 0), ("b", rq["e"])):
                        sc = call["y"][:k] + [last]
                        yield (lay, f"blind{mode}/k{k}/{rq['name']}/{which}", S.trace(lay, rq[which]["logs"], sc),
                               S.expected(rq[which]["logs"], sc), rq[which]["reach"])


@pytest.fixture(scope="module")
def traces():
    return list(_all_traces())


def test_named_cases_reach_their_branches(traces):
    named = {lay: 0 for lay in S.LAYOUTS}
    for lay, name, tr, want, reach in traces:
        assert tr["final"] == want, (lay, name)
        assert lay in S.HAS_JOIN or not tr["join"]
        for where, branch in reach:
            assert branch in tr[where], (lay, name, where, branch, tr[where])
            named[lay] += 1
    # the named list did not silently shrink
    assert all(named[lay] >= 12 for lay in ("lane", "pair", "wide16", "wide8")), named
    assert all(named[lay] >= 60 for lay in ("lanes16", "pairsG")), named


def test_every_branch_is_reached_in_every_layout(traces):
    for layout in S.LAYOUTS:
        chain, jn, build, wk = set(), set(), set(), set()
        for lay, _, tr, _, _ in traces:
            if lay == layout:
                chain |= set(tr["chain"])
                jn |= set(tr["join"])
                build |= set(tr["build"])
                wk |= set(tr["walk"])
        assert chain == set(CHAIN), (layout, sorted(set(CHAIN) - chain))
        assert wk == {S.WALK}, layout
        if layout in S.HAS_JOIN:
            assert jn == set(JOIN), (layout, sorted(set(JOIN) - jn))
        if layout in S.G1_LAYOUTS:
            assert ORDER3 | {"general"} <= build, (layout, build)
        else:
            assert build == {"general"}, (layout, build)  # unreachable by construction (module docstring)


def test_order3_table_build():
    """T, 2T, [3T = O], 4T = T, 5T = 2T by DOUBLING, [6T = O], 7T = T, 8T = 2T by doubling."""
    want = ["to-identity", "from-identity", "doubling", "to-identity", "from-identity", "doubling"]
    assert S.table_build(S.T3) == want and S.table_build(2 * S.T3) == want
    assert S.table_build(S.sub(12345)) == ["general"] * 6 and S.table_build(0) == []
    assert [d * S.T3 % S.M == 0 for d in range(1, 9)] == [False, False, True, False, False, True, False, False]


def test_oracle_on_the_order3_point(oc):
    for k, want in ((3, G1_IDENTITY), (6, G1_IDENTITY), (5, S.G1_ORDER3_NEG), (1, S.G1_ORDER3), (2, S.G1_ORDER3_NEG),
                    (4, S.G1_ORDER3)):
        assert S.msm(oc, 1, S.G1_ORDER3, [k]) == want, k
    assert S.point_bytes(oc, 1, [S.T3, 2 * S.T3, 0]) == S.G1_ORDER3 + S.G1_ORDER3_NEG + G1_IDENTITY
    mixed = S.point_bytes(oc, 1, [S.sub(7) + S.T3])
    assert S.msm(oc, 1, mixed, [3]) == gen_mul(oc, 1, [21])


def test_order13_table_build_and_rows():
    """An order-13 base: 2 T .. 8 T all by the general branch (unreachable by construction: module docstring),
    and every G2 case list holds the order-13 rows next to the G1 lists' order-3 ones."""
    assert S.table_build(S.T13) == ["general"] * 6 and S.table_build(12 * S.T13) == ["general"] * 6
    assert all(d * S.T13 % S.M for d in range(1, 9)) and 13 * S.T13 % S.M == 0 and 3 * S.T3 % S.M == 0
    assert S.T13 % R == 0 and S.T13 % 3 == 0 and S.T13 % 13 == 1 and S.T3 % 13 == 0 and S.GEN % 39 == 0
    for lay in S.LAYOUTS:
        ell = 3 if lay in S.G1_LAYOUTS else 13
        names = {c["name"] for c in S.msm_cases(lay, [5, 6, R - 1, 77, 12345], 1, with_x=True)}
        assert {f"order{ell}_first", f"order{ell}_neg_last", f"all_order{ell}", f"x_order{ell}"} <= names, (lay, names)
        other = {3: 13, 13: 3}[ell]  # the other group's small order
        assert not any(f"order{other}" in n for n in names)
    for mode in MODES:
        for q in S.VERIFY_Q:
            ell = 3 if mode == 0 else 13
            assert sum(f"order{ell}" in c["name"] for c in S.verify_cases(mode, q)) >= 8


def test_oracle_on_the_order13_point(oc):
    t13 = S.g2_order13()
    assert S.msm(oc, 2, t13, [13]) == G2_IDENTITY and S.msm(oc, 2, t13, [26]) == G2_IDENTITY
    assert S.msm(oc, 2, t13, [14]) == t13 and S.msm(oc, 2, t13, [1]) == t13
    assert S.point_bytes(oc, 2, [S.T13, 0]) == t13 + G2_IDENTITY
    assert S.point_bytes(oc, 2, [12 * S.T13]) == S.msm(oc, 2, t13, [12])
    mixed = S.point_bytes(oc, 2, [S.sub(7) + S.T13])
    assert S.msm(oc, 2, mixed, [13]) == gen_mul(oc, 2, [91])


def test_lagrange_matches_the_oracle(oc):
    for t in S.AGG_T:
        for ids in S.id_sets(t):
            out = ctypes.create_string_buffer(48 * t)
            oc.oc_lagrange(ctypes.c_size_t(t), (ctypes.c_uint64 * t)(*ids[:t]), out)
            assert out.raw == b"".join(be48(v) for v in S.lagrange(ids[:t])), (t, ids)
    assert S.lagrange([1, 2]) == [2, R - 1]


@pytest.mark.parametrize("q", S.VERIFY_Q)
@pytest.mark.parametrize("mode", MODES)
def test_verify_verdicts_by_construction_match_the_oracle(oc, mode, q):
    b = S.verify_batch_inputs(oc, mode, q)
    v, gts = S.oracle_verify(oc, mode, q, b, host_threads())
    assert v == b["expect"], [(n, a, e) for n, a, e in zip(b["names"], v, b["expect"]) if a != e]
    gt = [gts[576 * i:576 * (i + 1)] for i in range(b["n"])]
    one = {gt[i] for i, e in enumerate(b["expect"]) if e}
    assert len(one) == 1
    for i in range(0, b["n"], 2):  # a twin off by G is rejected with another GT (which pins the MSM's point)
        assert gt[i + 1] != gt[i] and gt[i + 1] not in one, b["names"][i]


@pytest.mark.parametrize("t", S.AGG_T)
@pytest.mark.parametrize("mode", MODES)
def test_aggregates_by_construction_match_the_oracle(oc, mode, t):
    sg, og = (2, 1) if mode == 0 else (1, 2)
    sb, ob = (192, 97) if mode == 0 else (97, 192)
    rows = S.agg_rows(S.SIG_LAYOUT[mode], t)
    _, pts = S.agg_inputs(oc, sg, rows)
    for i, r in enumerate(rows):
        row = pts[i * (t + 1) * sb:(i + 1) * (t + 1) * sb]
        o1, o2 = S.oracle_sig_aggregate(oc, mode, t, r["ids"], row, row)
        assert o1 == row[:sb]
        assert o2 == S.point_bytes(oc, sg, [S.expected(r["logs"][:t], r["scalars"])]), (mode, t, r["name"])
    rows = S.vkagg_rows(mode, t)
    assert 3 * len(rows) <= 64
    _, X, Y = S.vkagg_inputs(oc, mode, rows)
    for i, r in enumerate(rows):
        oX, oY = S.oracle_vk_aggregate(oc, mode, t, 2, r["ids"], X[i * (t + 1) * ob:(i + 1) * (t + 1) * ob],
                                       Y[i * (t + 1) * 2 * ob:(i + 1) * (t + 1) * 2 * ob])
        want = [S.expected(col[:t], r["scalars"]) for col in (r["X"]["logs"], r["Y0"], r["Y1"]["logs"])]
        assert oX + oY == S.point_bytes(oc, og, want), (mode, t, r["name"])


@pytest.mark.parametrize("k", S.BLIND_K)
@pytest.mark.parametrize("mode", MODES)
def test_blind_sums_by_construction_match_the_oracle(oc, mode, k):
    """With the stand-in for h (HLOG G) the oracle's MSM is the model's sum; one request has e = 0."""
    sg = 2 if mode == 0 else 1
    for call in S.blind_sets(mode, k):
        assert [rq["e"] for rq in call["requests"]].count(0) == 1
        for rq in call["requests"]:
            assert rq["e"] == (call["x"] + call["y"][k] * rq["known"]) % R
            for which, last in (("a", 0), ("b", rq["e"])):
                c, sc = rq[which], call["y"][:k] + [last]
                assert c["logs"][k] == S.sub(S.HLOG)
                got = S.msm(oc, sg, S.point_bytes(oc, sg, c["logs"], c["off"]), sc)
                assert got == S.point_bytes(oc, sg, [S.expected(c["logs"], sc)]), (mode, k, rq["name"], which)
