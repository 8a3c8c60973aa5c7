"""CPU test of the fixed-base edge cases themselves (tests/fixed_edges.py): a condition on the INPUTS that
tests/test_gpu_fixed_edges.py feeds the device, not on the device.

The model in fixed_edges restates, in discrete-log space, the order in which each prep kernel adds its
table entries (ft_digit; k_prep_sigg2_pair's window halves and their jac_add; the one-wave kernels' term
t = j nwin + w to group t mod NG and the jg_group_sum / jl_group_sum butterflies; the PoK preps' role
split and lane rotation) and names the branch of the group law every addition takes.  Here:

* every case named for a branch reaches it in the layout it is meant for, at every width and mode;
* per width, mode and layout the union of the cases reaches all five chain branches (fresh, general,
  doubling, to-identity, from-identity) and all five join branches (left-identity, right-identity,
  general, doubling, to-identity); k_prep_sigg1_pair has one chain and no join;
* the model's sum equals x + sum m_j y_j for every case (the model adds what the kernel must add);
* the verdicts known by construction equal the C oracle's: the whole list at 16 bits, the related-base
  cases at every width; the PoK lists against oc_pok_verify;
* ft_digit's restatement recomposes every edge scalar at every width 8 .. 22.
"""
import pytest

import fixed_edges as F
from conftest import host_threads

MODES = (0, 1)
GENERIC = ("zero", "one", "r_minus_1", "small", "bit_", "bits_three", "ones_", "near_r", "noncanon_")


def _sets(wbits, mode, cache={}):
    if (wbits, mode) not in cache:
        cache[wbits, mode] = F.verify_sets(wbits, mode)
    return cache[wbits, mode]


def _layouts(mode):
    """(layout, has a join)"""
    return (("pair", mode == 0), ("wide", True))


@pytest.mark.parametrize("wbits", range(8, 23))
def test_ft_digit_recomposes_every_edge_scalar(wbits):
    n = F.nwin(wbits)
    for m in F.edge_scalars(wbits):
        d = F.digits(m, wbits)
        assert len(d) == n and all(0 <= v < (1 << wbits) for v in d), (wbits, hex(m))
        assert sum(v << (wbits * w) for w, v in enumerate(d)) == m % F.R, (wbits, hex(m))
    # the named edges are what they claim: an all-ones digit is the window's last entry (index 2^wbits - 2)
    ones = (1 << wbits) - 1
    assert F.digits(ones << (wbits * (n // 2)), wbits)[n // 2] == ones
    top = (F.R - 1) >> (wbits * (n - 1))
    assert F.digits(F.R - 1, wbits)[n - 1] == top and F.digits(top << (wbits * (n - 1)), wbits)[n - 1] == top


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wbits", F.WIDTHS)
def test_named_cases_reach_their_branches(wbits, mode):
    named = 0
    for vk, cases in _sets(wbits, mode):
        for c in cases:
            for layout, has_join in _layouts(mode):
                t = F.trace_verify(vk, c["msgs"], layout)
                assert t["final"] == vk["gk"] * F.scalar_of(vk, c["msgs"]) % F.R, (vk["name"], c["name"], layout)
                assert has_join or not t["join"]
                for lay, where, branch in c["reach"]:
                    if lay == layout:
                        assert branch in t[where], (vk["name"], c["name"], layout, where, branch, t[where])
                        named += 1
    assert named >= (30 if mode == 0 else 15)  # the named list did not silently shrink (SigG1: no pair join)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wbits", F.WIDTHS)
def test_every_branch_is_reached_in_every_layout(wbits, mode):
    for layout, has_join in _layouts(mode):
        chain, jn = set(), set()
        for vk, cases in _sets(wbits, mode):
            for c in cases:
                t = F.trace_verify(vk, c["msgs"], layout)
                chain |= set(t["chain"])
                jn |= set(t["join"])
        assert chain == set(F.CHAIN), (layout, sorted(set(F.CHAIN) - chain))
        if has_join:
            assert jn == set(F.JOIN), (layout, sorted(set(F.JOIN) - jn))


def test_related_bases_are_what_the_model_assumes():
    """entry (1, w, d) = sign entry (0, w + a, d) and entry (2, w, d) = -entry (0, w, d) as multiples of
    the generator, for every verkey; X~ = Y~_0 / identity where the verkey says so."""
    for wbits in F.WIDTHS:
        for mode in MODES:
            for vk, _ in _sets(wbits, mode):
                n, a, y = F.nwin(wbits), vk["a"], vk["y"]
                for w in range(n):
                    if 0 <= w + a < n:
                        assert F.entry(y[1], w, 5, wbits) == vk["sign"] * F.entry(y[0], w + a, 5, wbits) % F.R
                    assert (F.entry(y[2], w, 5, wbits) + F.entry(y[0], w, 5, wbits)) % F.R == 0
                assert vk["x"] == {"y0": y[0], "inf": 0}.get(vk["xkind"], vk["x"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wbits", F.WIDTHS)
def test_verdicts_by_construction_match_the_oracle(oc, wbits, mode):
    """16 bits: every case; the other widths: the related-base cases (the generic ones differ only in
    where their digits fall, which the oracle does not see)."""
    for vk, cases in _sets(wbits, mode):
        if wbits != 16:
            cases = [c for c in cases if not c["name"].startswith(GENERIC)]
        vkb = F.verkey_bytes(oc, vk)
        b = F.verify_batch_inputs(oc, vk, cases)
        v, gts = F.oracle_verify(oc, vk, vkb, b, host_threads())
        assert v == b["expect"], [(n, a, e) for n, a, e in zip(b["names"], v, b["expect"]) if a != e]
        # a valid credential's GT is one: all the valid ones share it, no twin off by G does (that twin's
        # GT is what pins the MSM's point on the device)
        one = {gts[576 * i:576 * (i + 1)] for i, e in enumerate(b["expect"]) if e}
        assert len(one) <= 1
        assert all(gts[576 * i:576 * (i + 1)] not in one for i, nm in enumerate(b["names"]) if nm.endswith("/off_by_g"))


POK_SETS = ([1, 4], [], list(range(F.POK_Q)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("wbits", F.POK_WIDTHS)
def test_pok_cases_reach_their_branches(wbits, mode):
    vk = F.make_pok_verkey(wbits, mode)
    lay = "split" if mode == 0 else "pair"
    chain, wide_chain, wide_join = set(), set(), set()
    for rev in POK_SETS:
        cases = {c["name"]: c for c in F.make_pok_cases(vk, rev)}
        tr = {k: F.trace_pok(vk, c, rev, lay) for k, c in cases.items()}
        for c in cases.values():
            chain |= set(tr[c["name"]]["chain"])
            tw = F.trace_pok(vk, c, rev, "wide")
            wide_chain |= set(tw["chain"])
            wide_join |= set(tw["join"])
        assert tr["resp_zero"]["roles"] == (0, 0) and not tr["resp_zero"]["chain"]
        if len(rev) == F.POK_Q:
            continue  # no hidden response: the Schnorr sum is g~'s term alone
        hsum = lambda c: sum(vk["gk"] * vk["y"][i] * (v % F.R)  # noqa: E731
                             for i, v in zip([i for i in range(F.POK_Q) if i not in rev], c["resp"][1:])) % F.R
        g0 = lambda c: vk["gk"] * (c["resp"][0] % F.R) % F.R  # noqa: E731
        assert g0(cases["roleA_zero"]) == 0 and hsum(cases["roleA_zero"]) != 0
        assert g0(cases["roleB_zero"]) != 0 and hsum(cases["roleB_zero"]) == 0
        assert g0(cases["roles_equal"]) == hsum(cases["roles_equal"]) != 0
        assert (g0(cases["roles_opposite"]) + hsum(cases["roles_opposite"])) % F.R == 0 != g0(cases["roles_opposite"])
        if mode == 0:  # k_prep_pok_split with split = 0: role A is g~'s term, role B every hidden response
            assert F.pok_split(F.POK_Q, len(rev), wbits) == 0
            assert tr["roleA_zero"]["join"] == ["left-identity"] and tr["roleB_zero"]["join"] == ["right-identity"]
            assert tr["roles_equal"]["join"] == ["doubling"] and tr["roles_opposite"]["join"] == ["to-identity"]
            assert tr["roles_equal"]["roles"] == (g0(cases["roles_equal"]), hsum(cases["roles_equal"]))
        else:  # k_prep_pok_g1pl: one chain; opposite shares end it at the identity
            assert tr["roles_opposite"]["chain"][-1] == "to-identity" and tr["roles_opposite"]["roles"][0] == 0
        assert {"to-identity", "from-identity"} <= set(tr["chain_cancel"]["chain"])
        assert "doubling" in tr["chain_doubling"]["chain"]
        if rev:  # {1, 4}: the two equal terms on lanes of one parity meet before -T's lane joins them
            assert "doubling" in F.trace_pok(vk, cases["lanes_equal"], rev, "wide")["join"]
        if rev:
            assert "to-identity" in tr["jprime_identity"]["jchain"]  # J' ends at the identity
    # this mode's many-proof layout (k_prep_pok_split / k_prep_pok_g1pl): all five chain branches
    assert chain == set(F.CHAIN), sorted(set(F.CHAIN) - chain)
    # the one-block layout: all five branches of the lanes' butterfly.  Its chains are short (nwin <= 32
    # windows a response over 64 lanes or 32 pairs: a lane holds at most one term of a response), and two
    # related terms share a lane only if (s - s') nwin = w' - w mod L, which q = 6 with y_2 = -y_0 and
    # y_3 = 4^wbits y_0 does not give at every width; there the exceptional steps are the butterfly's.
    assert {"fresh", "general"} <= wide_chain
    assert wide_join == set(F.JOIN), sorted(set(F.JOIN) - wide_join)


@pytest.mark.parametrize("mode", MODES)
def test_pok_verdicts_by_construction_match_the_oracle(oc, mode):
    """Valid by construction with CHOSEN responses (T = sum rho_k B_k + c J): accepted unless J' is the
    identity (sigma'_2 is then the identity); a response off by one or sigma'_2 off by G: rejected.  The
    oracle leaves a GT exactly where it reaches the pairing."""
    vk = F.make_pok_verkey(14, mode)
    vkb = F.verkey_bytes(oc, vk)
    for rev in POK_SETS:
        b = F.pok_batch_inputs(oc, vk, F.make_pok_cases(vk, rev), rev)
        for name, (v, gt) in zip(b["names"], F.oracle_pok(oc, vk, vkb, b)):
            case, kind = name.split("/")
            assert v == int(kind == "valid" and case != "jprime_identity"), name
            assert (gt is None) == (kind == "resp_off_by_1" or (case == "jprime_identity" and kind == "valid")), name


def test_fixed_base_mul_expectations_are_well_defined(oc):
    """The oracle's k B for the edge scalars: identity for k = 0 and k = r and for the identity / off-curve
    bases, B for k = 1 and r + 1, and -B = (r - 1) B."""
    for group in (1, 2):
        eb = 97 if group == 1 else 192
        ident = F.G1_IDENTITY if group == 1 else F.G2_IDENTITY
        ks = F.fbm_scalars()
        for name, base in F.fbm_bases(oc, group):
            out = F.oracle_mul(oc, group, base, ks)
            pt = {k: out[eb * i:eb * (i + 1)] for i, k in enumerate(ks)}
            assert pt[0] == ident and pt[F.R] == ident
            if name in ("identity", "off_curve"):
                assert all(v == ident for v in pt.values()), name
            else:
                assert pt[1] == base == pt[F.R + 1] and pt[F.R - 1] not in (base, ident)
