"""GPU tests of the issuer's and the dealer's rows at the edges (the cases of tests/issuer_edges.py and
tests/golden/hash_to_curve_edges.json, whose branch coverage tests/test_issuer_edges_model.py asserts on
the CPU):

* cc_sigreq_verify_batch (issue.hip k_sigreq_checks, k_sigreq_combine) in both group modes at (q, k) =
  (3, 0), (3, 1), (3, 3), (6, 2), (18, 17) and with g or an h_j special per call: responses and challenge
  at 0, 1, r - 1, r, r + 1, 2^384 - 1, bit 254 alone; T as the identity, off-curve, with a bad prefix,
  negated, finite against an identity sum; related bases that make the ladder double, cancel and restart in
  every check kind; bases that decode to the identity; coordinates >= p; small-order ElGamal keys; the
  response-equality rule alone; one flipped bit per field with scalars of 48 different bytes (in SigG1
  every scalar of the record sits at an odd offset).  Each list runs whole, in a second fixed order, and
  as sub-batches of one request, exactly 64 lanes and one more; verdicts against the C oracle's sums;
* cc_vss_verify_batch (k_vss_verify) at t = 1, 2, 3, 5, 33, ids 0 .. 2^64 - 1, shares 0, r - 1, r, r + 1,
  2^384 - 1, identity / related g and h, identity / repeated / opposite / off-curve commitments, invalid
  shares, nine interleaved commitment sets, batches of 1, 64, 65 and 130 in two orders, under a SIG_G2 and
  a SIG_G1 context, and its argument checks;
* cc_hash_msg and cc_hash_to_curve on messages chosen by mapit's branches and by length, more than one
  block of lanes with neighbours of different lengths at unaligned offsets, byte for byte;
* compute_h's input canonicalisation (k_h_input_canon) through cc_blind_sign_batch: off-curve, identity,
  bad-prefix and >= p commitments, known messages >= r.
"""
import random

import pytest

import issuer_edges as E
from conftest import golden
from fixed_edges import R, be48

pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
SPECIAL = ["g_identity", "g_off_curve", "g_bad_prefix", "h1_identity", "h1_off_curve", "h1_bad_prefix", "h1_eq_h0",
           "h1_eq_neg_h0", "h0_eq_g"]


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _env(oc, mode):
    return E.Env(oc, 2 if mode == "G2" else 1)


def _call_names(mode):  # (a G2 encoding has no prefix byte: SigG1 alone has the bad-prefix calls)
    return [f"q{q}k{k}" for q, k in E.SHAPES] + [s for s in SPECIAL if mode == "G1" or "bad_prefix" not in s]


@pytest.mark.parametrize("mode,name", [(m, n) for m in ("G2", "G1") for n in _call_names(m)])
def test_request_proof_edges(oc, ctxs, mode, name):
    from coconut import sigreq_verify_batch
    env = _env(oc, mode)
    calls = {c["name"]: c for c in E.sigreq_calls(oc, mode)}
    assert set(calls) == set(_call_names(mode))
    call = calls[name]
    reqs = call["reqs"]
    want = [E.expect_request(env, call, r) for r in reqs]
    assert want == [r["intent"] for r in reqs]
    got = list(sigreq_verify_batch(ctxs[mode], *E.call_args(call, reqs)))
    assert got == want, [(r["name"], g, w) for r, g, w in zip(reqs, got, want) if g != w]
    perm = E.permutation(len(reqs))
    got = list(sigreq_verify_batch(ctxs[mode], *E.call_args(call, [reqs[i] for i in perm])))
    assert got == [want[i] for i in perm], [(reqs[i]["name"], g) for i, g in zip(perm, got) if g != want[i]]
    for n in call["slices"]:  # one request, one full block of lanes, a block and a request more
        got = list(sigreq_verify_batch(ctxs[mode], *E.call_args(call, reqs[:n])))
        assert got == want[:n], (n, [(r["name"], g) for r, g, w in zip(reqs, got, want) if g != w])


VSS_CALLS = [(t, "rand") for t in E.VSS_T] + [(3, h) for h in E.VSS_H[1:]]


@pytest.mark.parametrize("t,hkind", VSS_CALLS)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_vss_share_edges(oc, ctxs, mode, t, hkind):
    from coconut import vss_verify_batch
    env = E.Env(oc, 1)  # the row is G1 under either context
    call = E.vss_call(oc, t, hkind)
    want = {c["name"]: E.expect_share(env, call, c) for c in call["cases"]}
    assert all(want[c["name"]] == c["intent"] for c in call["cases"])
    assert 0 < sum(want.values()) < len(want)
    for n in E.VSS_SIZES:
        for order in (0, 1):
            if order and n == 1:
                continue
            batch = E.vss_batch(call, n, order)
            got = list(vss_verify_batch(ctxs[mode], *E.vss_args(call, batch)))
            exp = [want[c["name"]] for c in batch]
            bad = [(i, c["name"], g) for i, (c, g, w) in enumerate(zip(batch, got, exp)) if g != w]
            assert not bad, (n, order, bad)


def test_vss_argument_checks(oc, ctxs):
    from coconut import CoconutError, vss_verify_batch
    call = E.vss_call(oc, 3, "rand")
    batch = E.vss_batch(call, 5)
    t, g, h, sets, set_of, ids, shares = E.vss_args(call, batch)
    for bad in ((0, g, h, [[] for _ in sets], set_of, ids, shares),
                (t, g, h, sets, [len(sets)] + set_of[1:], ids, shares),
                (t, g, h, sets, set_of[:-1] + [0xFFFFFFFF], ids, shares)):
        with pytest.raises(CoconutError) as e:
            vss_verify_batch(ctxs["G2"], *bad)
        assert e.value.code == -4  # CC_ERR_DECODE
    assert list(vss_verify_batch(ctxs["G2"], t, g, h, sets, set_of, ids, shares)) == [c["intent"] for c in batch]


# ---------------------------------------------------------------- hash-to-curve by branch
def _hash_list():
    """The fixture's messages three times over in three orders: more than 64 lanes, every message next to
    ones of other lengths, offsets of every residue."""
    d = golden("hash_to_curve_edges.json")["messages"]
    rng = random.Random(17)
    second, third = list(d), list(d)
    rng.shuffle(second)
    rng.shuffle(third)
    out = d + second + third + d[:7]
    assert len(out) > 64 and all(a["msg"] != b["msg"] for a, b in zip(out, out[1:]))
    offs, o = set(), 0
    for r in out:
        offs.add(o % 8)
        o += len(r["msg"]) // 2
    assert offs == set(range(8))
    return out


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_hash_to_curve_every_branch_and_length(ctxs, mode):
    from coconut import hash_msg, hash_to_curve
    recs = _hash_list()
    msgs = [bytes.fromhex(r["msg"]) for r in recs]
    got = hash_msg(ctxs[mode], msgs)
    assert [g.hex() for g in got] == [r["shake256_48"] for r in recs]
    for group, key in ((1, "g1"), (2, "g2")):
        got = hash_to_curve(ctxs[mode], group, msgs)
        bad = [(i, r["classes"]) for i, (g, r) in enumerate(zip(got, recs)) if g.hex() != r[key]]
        assert not bad, (key, bad)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_compute_h_canonicalises_its_inputs(oc, ctxs, mode):
    """Every row gives the h of the oracle's compute_h on the decoded commitment and the reduced messages,
    and the c~1, c~2 of its canonical form (oc_msm with that h)."""
    from coconut import blind_sign_batch
    from oracle import issuance as I
    env = _env(oc, mode)
    q, k = 6, 2
    rng = random.Random(40 + MODES[mode])
    rows = E.compute_h_inputs(env, q, k, rng)
    x, y = rng.randrange(R), [rng.randrange(R) for _ in range(q)]
    cts = [[(env.rand_pt(rng), env.rand_pt(rng)) for _ in range(k)] for _ in rows]
    enc = lambda ms: [be48(m) for m in ms]  # noqa: E731
    hs, c1s, c2s = blind_sign_batch(ctxs[mode], q, k, [cm for _, cm, _ in rows], [enc(kn) for _, _, kn in rows], cts,
                                    be48(x), enc(y))
    canon = [(env.canon(cm), [m % R for m in kn]) for _, cm, kn in rows]
    hs0, c1s0, c2s0 = blind_sign_batch(ctxs[mode], q, k, [cm for cm, _ in canon], [enc(kn) for _, kn in canon], cts,
                                       be48(x), enc(y))
    for i, (nm, cm, kn) in enumerate(rows):
        h = env.enc(I.compute_h(env.grp, env.dec(cm), [m % R for m in kn]))
        e = (x + sum(y[k + j] * (m % R) for j, m in enumerate(kn))) % R
        c1 = env.msm([a for a, _ in cts[i]], y[:k])
        c2 = env.msm([b for _, b in cts[i]] + [h], y[:k] + [e])
        assert (hs[i], c1s[i], c2s[i]) == (h, c1, c2), nm
        assert (hs0[i], c1s0[i], c2s0[i]) == (h, c1, c2), nm
