"""CPU test of the issuer-side edge cases themselves (tests/issuer_edges.py, tests/golden/
hash_to_curve_edges.json): conditions on the INPUTS that tests/test_gpu_issuer_edges.py feeds the device, not
on the device.

* every named request and share reaches, in the model of the ladder (issuer_edges.ladder), the branch it is
  named for, and the model's verdict equals the C oracle's for the same check;
* for every case the C-oracle expectation (oc_msm over the encodings sent) equals the verdict the
  construction intends and the Python oracle's sigreq_proof_verify / verify_share on the decoded inputs
  (the whole lists in the tests marked slow; unmarked: one request of every case family per mode, every
  share at t <= 5);
* per group mode the union of the request cases reaches every branch of issuer_edges.BRANCHES in each of
  the four check kinds, and the union of the share cases reaches every one both among the g / h entries
  and among the C_k entries;
* the encodings are what their names say: off-curve and bad-prefix forms decode to the identity, shifted
  coordinates are >= p and decode to the same point, the scalars of the flipped-bit cases have 48
  different bytes, the sub-batches fill one request, exactly 64 lanes, and a block boundary inside a
  request;
* every record of hash_to_curve_edges.json is what the traced mapit of oracle/hash_to_curve.py gives now,
  the traced walk ends at the untraced functions' points, and every class of make_golden.H2C_CLASSES and
  every length of H2C_LENGTHS is present.

UNREACHABLE BY CONSTRUCTION: a base of order 2 (a doubling that lands on the identity, jac_dbl of a point
with y = 0): both curves' orders h1 r and h2 r are odd, so neither has such a point.  Among the g / h
entries of k_vss_verify the 'skipped' base is h alone (an identity g takes the same branch and is not
built).
"""
import collections
import hashlib
import os
import re
import sys

import pytest

import issuer_edges as E
from conftest import GOLDEN, golden
from fixed_edges import P, R

sys.path.insert(0, GOLDEN)
MODES = ("G2", "G1")


def _env(oc, mode):
    return E.Env(oc, 2 if mode == "G2" else 1)


def _family(name):
    """A request's case family: its name without the check kind and the index."""
    return re.sub(r"_(sk|comm|ct1|ct2|\d+)$", "", name)


# ---------------------------------------------------------------- request proofs
@pytest.mark.parametrize("mode", MODES)
def test_request_cases_reach_their_branches(oc, mode):
    env = _env(oc, mode)
    union = collections.defaultdict(set)
    named = 0
    for call in E.sigreq_calls(oc, mode):
        for req in call["reqs"]:
            want = collections.defaultdict(set)
            for kind, b in req["reach"]:
                want[kind].add(b)
            exp = E.expect_checks(env, call, req)
            for kind in want:
                got = set()
                for key in (k for k in exp if k[0] == kind):
                    tr = E.trace_check(env, call, req, key)
                    assert int(tr["ok"]) == exp[key], (call["name"], req["name"], key)
                    got |= {b for _, b in tr["log"]} | {"final:" + tr["final"]}
                assert want[kind] <= got, (call["name"], req["name"], kind, want[kind] - got)
                union[kind] |= got
                named += 1
    assert named > 40
    for kind in E.KINDS:
        assert set(E.BRANCHES) <= union[kind], (kind, set(E.BRANCHES) - union[kind])
        assert {"final:skipped", "final:doubling", "final:to-identity"} <= union[kind], kind


@pytest.mark.parametrize("mode", MODES)
def test_request_expectations_are_the_intended_ones(oc, mode):
    """The C oracle's verdict is the construction's for every request; accepting and rejecting requests
    are both present in every call and in both orders the device test runs."""
    env = _env(oc, mode)
    calls = E.sigreq_calls(oc, mode)
    assert [(c["q"], c["k"]) for c in calls[:len(E.SHAPES)]] == list(E.SHAPES)
    for call in calls:
        exp = [E.expect_request(env, call, r) for r in call["reqs"]]
        assert exp == [r["intent"] for r in call["reqs"]], call["name"]
        assert 0 < sum(exp) < len(exp), call["name"]
        assert len({r["name"] for r in call["reqs"]}) == len(call["reqs"])
        perm = E.permutation(len(exp))
        assert sorted(perm) == list(range(len(exp))) and perm != sorted(perm)
        assert all(n <= len(exp) for n in call["slices"])
    # the sub-batches: one request; exactly one block of k_sigreq_checks; a request across two blocks
    byshape = {(c["q"], c["k"]): c for c in calls[:len(E.SHAPES)]}
    for (q, k), c in byshape.items():
        lanes = [n * (2 + 2 * k) for n in c["slices"]]
        assert 1 in c["slices"] and (64 in lanes or k in (2, 17)), (q, k, lanes)
    for k in (2, 17):
        assert 64 % (2 + 2 * k) != 0  # 6 and 36 lanes a request: one straddles lanes 63 / 64
    assert all(len(c["reqs"]) == 11 for c in calls[len(E.SHAPES):])  # 66 lanes with k = 2


def _python_agrees(env, call, reqs):
    for req in reqs:
        assert E.python_verdict(env, call, req) == E.expect_request(env, call, req) == req["intent"], \
            (call["name"], req["name"])


@pytest.mark.parametrize("mode", MODES)
def test_python_oracle_agrees_on_every_request_family(oc, mode):
    env = _env(oc, mode)
    calls = E.sigreq_calls(oc, mode)
    call = next(c for c in calls if (c["q"], c["k"]) == (3, 1))
    first = {}
    for req in call["reqs"]:
        first.setdefault(_family(req["name"]), req)
    every = {_family(r["name"]) for c in calls[:len(E.SHAPES)] for r in c["reqs"]}
    assert every == set(first), every ^ set(first)  # k = 1 has a request of every family
    _python_agrees(env, call, first.values())
    for c in calls[len(E.SHAPES):]:  # the per-call bases: the call's own request
        _python_agrees(env, c, c["reqs"][-1:])


@pytest.mark.slow
@pytest.mark.parametrize("mode", MODES)
def test_python_oracle_agrees_on_every_request(oc, mode):
    env = _env(oc, mode)
    for call in E.sigreq_calls(oc, mode):
        _python_agrees(env, call, call["reqs"])


@pytest.mark.parametrize("mode", MODES)
def test_request_encodings_are_what_they_claim(oc, mode):
    env = _env(oc, mode)
    calls = E.sigreq_calls(oc, mode)
    main = next(c for c in calls if c["name"] == "q6k2")
    by = {r["name"]: r for r in main["reqs"]}
    for nm, form in env.identity_forms(__import__("random").Random(1)):
        assert env.dec(form) is None and env.canon(form) == env.identity, nm
        assert env.dec(by[f"pk_{nm}"]["pk"]) is None and env.dec(by[f"commitment_{nm}"]["commitment"]) is None
        assert env.dec(by[f"c1_{nm}"]["cts"][1][0]) is None and env.dec(by[f"c2_{nm}"]["cts"][0][1]) is None
        if nm != "identity":  # a finite point with one thing wrong, not the identity's own encoding
            assert by[f"pk_{nm}"]["pk"] != env.identity
        # compute_h hashed the re-encoded commitment: the identity's canonical bytes
        from oracle import issuance as I
        r0 = by[f"commitment_{nm}"]
        assert r0["h"] == env.enc(I.compute_h(env.grp, None, [m % R for m in r0["known"]]))
    for j in (1, "max"):
        for pt in [by[f"pk_coords_plus_{j}p"]["pk"]] + by[f"ct_coords_plus_{j}p"]["cts"][0]:
            body = pt[1:] if env.group == 1 else pt
            co = [int.from_bytes(body[o:o + 48], "big") for o in range(0, len(body), 48)]
            assert all(v >= P for v in co) and env.dec(pt) is not None and env.canon(pt) != pt
            if j == "max":
                assert all(v + P >= 1 << 384 for v in co)
    tor = E.torsion_fixture()["G1" if env.group == 1 else "G2"]
    for nm, order in (("T3", 3), ("-T3", 3)) if env.group == 1 else (("T13", 13), ("-T13", 13)):
        pt = env.dec(by[f"pk_{nm}"]["pk"])
        assert pt is not None and env.curve.mul_any(pt, order) is None and tor[nm]["order"] == order
    for kind in E.KINDS:
        for nm in (f"flip_response_{kind}", f"flip_T_{kind}", f"flip_challenge_{kind}"):
            r0 = by[nm]
            sc = [r0["r_sk"], r0["chal"]] + r0["r_comm"] + r0["r1"] + r0["r2a"]
            assert sum(len(set(E.be48(v))) == 48 for v in sc) >= len(sc) - 1, nm  # but the flipped one
            assert sum(E.expect_checks(env, main, r0).values()) == len(E.expect_checks(env, main, r0)) - 1, nm
    assert all(len(set(E.be48(v))) == 48 for v in by["valid_distinct_bytes"]["r_comm"])
    # the combine rule alone: every Schnorr check of these holds
    for i in (0, 1):
        for nm, same in ((f"combine_v_and_v_plus_r_{i}", 1), (f"combine_v_plus_r_and_v_{i}", 1),
                         (f"combine_v_and_v_plus_1_{i}", 0)):
            r0 = by[nm]
            assert all(E.expect_checks(env, main, r0).values()), nm
            assert r0["r_comm"][i] != r0["r2b"][i] and (r0["r_comm"][i] % R == r0["r2b"][i] % R) == bool(same)
    # an identity sum accepts exactly when T decodes to the identity
    for nm in ("scalars_all_zero", "scalars_all_r", "zero_sum_off_curve_T"):
        assert all(t == env.identity for t in (env.canon(t) for t in by[nm]["T"].values())), nm
    wide = next(c for c in calls if c["k"] == 17)
    assert {"combine_v_and_v_plus_1_0", "combine_v_and_v_plus_1_16"} <= {r["name"] for r in wide["reqs"]}


# ---------------------------------------------------------------- VSS shares
VSS_CALLS = [(t, "rand") for t in E.VSS_T] + [(3, h) for h in E.VSS_H[1:]]


def test_share_cases_reach_their_branches_and_oracles_agree(oc):
    env = E.Env(oc, 1)
    union = collections.defaultdict(set)
    for t, hk in VSS_CALLS:
        call = E.vss_call(oc, t, hk)
        assert len(call["sets"]) >= 3 and all(len(s) == t for s in call["sets"])
        for c in call["cases"]:
            exp = E.expect_share(env, call, c)
            assert exp == c["intent"], (t, hk, c["name"])
            if t <= 5:
                assert E.python_share(env, call, c) == exp, (t, hk, c["name"])
            if c["reach"] or t <= 3:
                tr = E.trace_share(env, call, c)
                assert int(tr["ok"]) == exp, (t, hk, c["name"])
                assert set(c["reach"]) <= set(tr["log"]), (t, hk, c["name"], set(c["reach"]) - set(tr["log"]))
                for tag, b in tr["log"]:
                    union[tag].add(b)
            nm = c["name"].split("/")[1]
            if nm.startswith("valid"):
                assert exp == 1, (t, hk, c["name"])
            elif hk == "rand" and not nm.startswith("zero_share") and not (t == 1 and nm.startswith("wrongid")):
                assert exp == 0, (t, hk, c["name"])  # (a constant polynomial's share is valid under any id)
        names = {c["name"].split("/")[1].split("_id_")[0] for c in call["cases"]}
        assert {"s_plus_1", "st_plus_1", "negated", "wrongid", "other_set", "valid"} <= names
        assert {c["id"] for c in call["cases"]} == set(E.VSS_IDS)
        # shares of different sets next to each other, the last share on the last set, in both orders
        for n in E.VSS_SIZES:
            for order in (0, 1):
                b = E.vss_batch(call, n, order)
                assert len(b) == n and b[-1]["set"] == len(call["sets"]) - 1
                assert n < 3 or any(x["set"] != y["set"] for x, y in zip(b, b[1:]))
        assert [c["name"] for c in E.vss_batch(call, 130)] != [c["name"] for c in E.vss_batch(call, 130, 1)]
    for tag in ("gh", "C"):
        assert set(E.BRANCHES) <= union[tag], (tag, set(E.BRANCHES) - union[tag])


def test_share_encodings_are_what_they_claim(oc):
    env = E.Env(oc, 1)
    call = E.vss_call(oc, 5, "rand")
    by = {c["name"]: c for c in call["cases"]}
    assert (by["r_and_r_plus_1/valid"]["s"], by["r_and_r_plus_1/valid"]["st"]) == (R, R + 1)
    assert by["max/valid"]["s"] == by["max/valid"]["st"] == (1 << 384) - 1
    assert (by["both_zero/valid"]["s"], by["both_zero/valid"]["st"]) == (0, 0)
    assert by["s_zero/valid"]["s"] == 0 != by["s_zero/valid"]["st"]
    assert by["st_zero/valid"]["st"] == 0 != by["st_zero/valid"]["s"]
    assert by["r_minus_1/valid"]["s"] == by["r_minus_1/valid"]["st"] == R - 1
    # id^k wraps mod r from k = 4 on for the largest id
    assert ((1 << 64) - 1) ** 3 < R < ((1 << 64) - 1) ** 4
    rel = call["sets"][1]
    assert rel[1] == rel[0] and rel[2] == env.neg(rel[0]) and rel[3] == env.identity
    assert env.dec(rel[4]) is None and rel[4] != env.identity
    gs = call["sets"][2]
    assert gs[0] == call["g"] and gs[1] == env.neg(call["g"])
    for hk, want in (("identity", env.identity), ("eq_g", None), ("neg_g", None)):
        c2 = E.vss_call(oc, 3, hk)
        assert c2["h"] == (want or (c2["g"] if hk == "eq_g" else env.neg(c2["g"])))
    off = E.vss_call(oc, 3, "off_curve")
    assert env.dec(off["h"]) is None and off["h"] != env.identity


@pytest.mark.slow
def test_python_oracle_agrees_on_the_shares_at_t33(oc):
    env = E.Env(oc, 1)
    call = E.vss_call(oc, 33, "rand")
    for c in call["cases"]:
        assert E.python_share(env, call, c) == E.expect_share(env, call, c), c["name"]


# ---------------------------------------------------------------- compute_h's inputs
@pytest.mark.parametrize("mode", MODES)
def test_compute_h_inputs_are_non_canonical_as_named(oc, mode):
    import random
    env = _env(oc, mode)
    rows = E.compute_h_inputs(env, 6, 2, random.Random(3))
    by = {nm: (cm, kn) for nm, cm, kn in rows}
    assert env.canon(by["canonical"][0]) == by["canonical"][0] and all(m < R for m in by["canonical"][1])
    for nm, (cm, kn) in by.items():
        if nm.startswith("commitment_"):
            assert env.canon(cm) != cm or nm == "commitment_identity", nm
            assert (env.dec(cm) is None) == ("coords" not in nm), nm
        if nm.startswith("known_"):
            assert all(m >= R or m == 0 or "edges" in nm for m in kn) and any(m >= R for m in kn), nm
    assert all(m + R >= 1 << 384 for m in by["known_plus_max_r"][1])
    assert {(1 << 384) - 1, R, 0} <= set(by["known_edges"][1])


# ---------------------------------------------------------------- hash-to-curve by branch
def test_hash_to_curve_edges_fixture_is_current_and_complete():
    import make_golden as M
    from oracle import bls12_381 as B
    from oracle import hash_to_curve as H
    d = golden("hash_to_curve_edges.json")["messages"]
    assert os.path.getsize(os.path.join(GOLDEN, "hash_to_curve_edges.json")) < 64 << 10
    seen = set()
    for rec in d:
        m = bytes.fromhex(rec["msg"])
        tr, g1, g2 = H.mapit_trace(m)
        assert tr == rec["trace"], rec["classes"]
        assert hashlib.shake_256(m).hexdigest(48) == rec["shake256_48"] == H.hash_msg(m).hex()
        assert int(rec["shake256_48"], 16) // P == tr["reductions"]
        assert B.g1_to_bytes(g1).hex() == rec["g1"] == B.g1_to_bytes(H.g1_from_msg_hash(m)).hex()
        assert B.g2_to_bytes(g2).hex() == rec["g2"] == B.g2_to_bytes(H.g2_from_msg_hash(m)).hex()
        assert not tr["wrapped"] and "halves" not in tr["g2_rejects"] and tr["g2_root"] in ("first", "second")
        mine = M.h2c_classes(tr)
        assert {c for c in rec["classes"] if not c.startswith("length_")} <= mine
        seen |= mine | set(rec["classes"])
    assert set(M.H2C_CLASSES) <= seen, set(M.H2C_CLASSES) - seen
    lens = [len(r["msg"]) // 2 for r in d]
    assert set(M.H2C_LENGTHS) <= set(lens) and {f"length_{n}" for n in M.H2C_LENGTHS} <= seen
    assert len(set(lens)) == len(lens) and max(lens) == 1000  # all of distinct lengths
    assert 9 * P < 1 << 384 < 10 * P  # nine subtractions are the most
    for word in ("x^3 + b = 0", "wrapping past p - 1", "zero Fp2 argument", "identity after cofactor clearing",
                 "4096 failed tries"):
        assert word in M.make_hash_to_curve_edges.__doc__, word
