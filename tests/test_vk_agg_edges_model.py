"""CPU checks of tests/vk_agg_edges.py: the rows reach the branches they are named for, the coverage the
device test (tests/test_gpu_vk_agg_edges.py) relies on is complete, the coefficient edges have the digits they
claim, the steering means what it says (the oracle's Verkey::aggregate of the encoded keys is the point the
discrete logarithms give), and every build's tables stay within the size bound."""
import pytest

import straus_edges as S
import vk_agg_edges as V
from fixed_edges import CHAIN, JOIN, R, ft_digit, limbs, nwin

MODES = (0, 1)


def _traces(mode, wbits):
    for r in V.rows(mode, wbits):
        for j in range(r["q"] + 1):
            yield r, j, V.trace(mode, wbits, r["coef"], [l[j] for l in r["logs"]])


@pytest.mark.parametrize("wbits", V.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_rows_reach_their_branches(mode, wbits):
    for r in V.rows(mode, wbits):
        for j, kind, where, branch in r["reach"]:
            tr = V.trace(mode, wbits, r["coef"], [l[j] for l in r["logs"]])
            assert branch in tr[kind][where], (mode, wbits, r["name"], j, kind, where, branch)
    for r, j, tr in _traces(mode, wbits):  # the model's sum is the point the logarithms give
        assert tr["final"] == V.expected(r["coef"], [l[j] for l in r["logs"]]), (mode, wbits, r["name"], j)


def _coverage(mode, wbits):
    chain = set()
    joins = {m: set() for m in V.DISTS[mode]}
    for _, _, tr in _traces(mode, wbits):
        chain |= {b for part in tr["chain"] for b in part}
        for m in V.DISTS[mode]:
            joins[m] |= set(tr["join"][m])
    return chain, joins


@pytest.mark.parametrize("wbits", V.FULL)
@pytest.mark.parametrize("mode", MODES)
def test_full_widths_reach_every_branch_at_every_distance(mode, wbits):
    chain, joins = _coverage(mode, wbits)
    assert chain == set(CHAIN), (mode, wbits, set(CHAIN) - chain)
    for m in V.DISTS[mode]:
        assert joins[m] == set(JOIN), (mode, wbits, m, set(JOIN) - joins[m])


@pytest.mark.parametrize("wbits", V.REDUCED)
@pytest.mark.parametrize("mode", MODES)
def test_reduced_widths_reach_the_steered_branches(mode, wbits):
    """The reduced list: every chain branch, and a steered doubling or cancellation at every distance (next to
    the general and identity joins the coefficient rows give)."""
    chain, joins = _coverage(mode, wbits)
    assert chain == set(CHAIN), (mode, wbits, set(CHAIN) - chain)
    for m in V.DISTS[mode]:
        assert {"left-identity", "right-identity", "general"} <= joins[m], (mode, wbits, m, joins[m])
        assert joins[m] & {"doubling", "to-identity"}, (mode, wbits, m, joins[m])
    assert {"doubling", "to-identity"} <= set().union(*joins.values())


@pytest.mark.parametrize("wbits", V.FULL)
def test_chain_steering_hits_first_middle_and_last_windows(wbits):
    """At the full widths the doubling / cancellation sits at the second issuer's first, a middle and the last
    non-zero window, and after a cancellation at the last window the part's third issuer starts afresh."""
    for mode in MODES:
        seen = set()
        for r in V.rows(mode, wbits):
            if not r["name"].startswith("chain/"):
                continue
            where = r["name"].split("/")[1]
            npart, k2 = V.NPART[mode], V.NPART[mode]
            for j in range(r["q"] + 1):
                log = V.trace(mode, wbits, r["coef"], [l[j] for l in r["logs"]])["chain"][0]
                first = sum(1 for w in range(nwin(wbits)) if V.digit_plain(r["coef"][0], w, wbits))
                nz2 = sum(1 for w in range(nwin(wbits)) if V.digit_plain(r["coef"][k2], w, wbits))
                at = {"first": 0, "middle": nz2 // 2, "last": nz2 - 1}[where]
                assert log[first + at] in ("doubling", "to-identity"), (mode, wbits, r["name"], j)
                seen.add((where, log[first + at]))
                if where == "last" and log[first + at] == "to-identity":
                    assert r["t"] > 2 * npart and log[first + nz2] == "from-identity"
        assert seen == {(w, b) for w in ("first", "middle", "last") for b in ("doubling", "to-identity")}, (mode, seen)


@pytest.mark.parametrize("wbits", V.WIDTHS)
def test_coefficient_edges_have_their_digits(wbits):
    n, ones = nwin(wbits), (1 << wbits) - 1
    claimed = 0
    for r in V.rows(0, wbits):
        for k, v in r["claim"]:
            assert r["coef"][k] == v % R, (wbits, r["name"], k)
            assert [ft_digit(limbs(v % R), w, wbits) for w in range(n)] == [V.digit_plain(v % R, w, wbits) for w in range(n)]
            claimed += 1
    assert claimed > 6 * len(V.boundary_bits(wbits))
    rows = {r["name"]: r for r in V.rows(0, wbits)}
    straddles = 0
    for s in V.boundary_bits(wbits):
        w, b = divmod(s, wbits)
        dg = [ft_digit(limbs(rows[f"coef/pow2_{s}"]["coef"][0]), x, wbits) for x in range(n)]
        assert dg == [(1 << b) if x == w else 0 for x in range(n)], (wbits, s)  # one bit beside the boundary
        dg = [ft_digit(limbs(rows[f"coef/ones_{s}"]["coef"][0]), x, wbits) for x in range(n)]
        assert dg == [ones if x < w else ((1 << b) - 1 if x == w else 0) for x in range(n)], (wbits, s)
        assert dg[0] == (ones if s >= wbits else (1 << s) - 1)  # s >= wbits: the last entry of a window
        o = w * wbits  # the window of bit s straddles two 32-bit limbs: ft_digit's generic branch
        straddles += (o & 31) + wbits > 32 and (o >> 5) + 1 < 8
    assert (straddles > 0) == (wbits in (10, 12, 13)), (wbits, straddles)
    # r - x: the short top window holds r's top bits
    top = ft_digit(limbs(R - 1), n - 1, wbits)
    assert top == (R - 1) >> (wbits * (n - 1)) and ft_digit(limbs(rows["coef/r_minus_1"]["coef"][0]), n - 1, wbits) == top
    # bits above 64 and high id words
    assert all(c >> 64 for c in rows[f"coef/three_{V.boundary_bits(wbits)[-1]}"]["coef"][::2])
    assert max(rows["coef/high_words"]["ids"]) == (1 << 64) - 1
    # id 0 at every position of the first t: each part, and a part's second round
    assert [r["coef"] for name, r in rows.items() if name.startswith("coef/id0_at_")] == \
        [[int(k == p) for k in range(V.NPART[0] + 1)] for p in range(V.NPART[0] + 1)]


@pytest.mark.parametrize("wbits", V.FULL)
@pytest.mark.parametrize("mode", MODES)
def test_small_order_key_meets_empty_entries(mode, wbits):
    """The small-order key (order 3 in G1, 13 in G2) has digits on identity multiples: entries stored empty and
    skipped, at the non-byte widths too; its other digits meet T and -T again and again."""
    r = next(r for r in V.rows(mode, wbits) if r["name"] == "enc/small_order")
    tors = r["logs"][1][0]
    assert tors and tors % R == 0
    dg = [V.digit_plain(r["coef"][1], w, wbits) for w in range(nwin(wbits))]
    assert any(d and d * pow(2, wbits * w, S.M) * tors % S.M == 0 for w, d in enumerate(dg)), (mode, wbits, dg)
    assert V.trace(mode, wbits, r["coef"], [l[0] for l in r["logs"]])["chain"][1]


@pytest.mark.parametrize("wbits", V.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_builds_fit_and_hold_every_row_once(mode, wbits):
    bs = V.builds(mode, wbits)
    names = [r["name"] for b in bs for r in b["rows"]]
    assert sorted(names) == sorted(r["name"] for r in V.rows(mode, wbits)) and len(set(names)) == len(names)
    own = [i for r in V.rows(mode, wbits) if not r["pool"] for i in r["ids"]]
    assert len(own) == len(set(own))  # a steered row owns its issuers
    for b in bs:
        nb = len(b["ids"]) * (b["q"] + 1)
        assert b["bytes"] == nb * nwin(wbits) * ((1 << wbits) - 1) * (96 if mode == 0 else 192) <= 1 << 30
        assert not set(V.UNKNOWN) & set(b["ids"])
        assert b["ids"] != sorted(b["ids"]) or len(b["ids"]) == 1  # cc_set_issuers has to sort them
        for r in b["rows"]:
            assert set(r["ids"]) <= set(b["ids"])
    assert any(len(b["ids"]) == 1 for b in bs)  # n_iss = 1
    if wbits == 16:
        assert max(len(b["ids"]) for b in bs) <= (10 if mode == 0 else 5)
    if wbits in V.FULL:
        assert {b["q"] for b in bs} == {0, 1, 5}
        assert {r["t"] for r in V.rows(mode, wbits)} >= {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33}
        lo, hi = min(i for b in bs for i in b["ids"]), max(i for b in bs for i in b["ids"])
        assert (lo, hi) == (0, (1 << 64) - 1)  # rows at the first and the last id of their tables


@pytest.mark.parametrize("wbits", V.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_steering_agrees_with_the_oracle(oc, mode, wbits):
    """sum l_k x_k as a point (oc_gen_mul, oc_msm for a small-order part) is the oracle's oc_verkey_aggregate of
    the encoded keys, for every row and column, the undecodable and the >= p encodings included."""
    og, ob = (1, 97) if mode == 0 else (2, 192)
    for b in V.builds(mode, wbits):
        for r in b["rows"]:
            wX, wY = V.oracle_row(oc, b, r)
            got = wX + wY
            want = S.point_bytes(oc, og, [V.expected(r["coef"], [l[j] for l in r["logs"]]) for j in range(b["q"] + 1)])
            assert got == want, (mode, wbits, r["name"])
            assert len(got) == ob * (b["q"] + 1)
