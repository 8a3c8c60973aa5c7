"""GPU tests of the variable-base windowed Straus MSMs at edge scalars and exceptional sums (the cases of
tests/straus_edges.py, whose branch coverage tests/test_straus_edges_model.py asserts on the CPU).  Every
comparison is byte equality with the C oracle.

* Signature::verify with a verkey per credential, q = 3 and q = 18 (more than 16 and than 8: lane groups of
  the one-wave prep hold two bases), both modes: every case as a valid credential and as its twin with
  sigma_2 off by G (whose GT bytes pin the MSM's point), as one small batch (k_prep_sig*_var_wide), as single
  credentials, and tiled by repetition just past kPrepWideMax (capi_verify.cpp: the per-verkey prep becomes
  k_prep_sigg2_var / k_prep_sigg1_var), kFexpWideMax and kWideMax (the batch Miller loop);
* Signature::aggregate for t in {1, 2, 3, 5, 17, 33} with t + 1 entries a row (the unused one present),
  <= 64 rows a call, Lagrange scalars 2 and r - 1 among them; an all-identity row gives the identity;
* cc_verkey_aggregate_batch with q = 2: X~ and Y~_1 take different steered rows (l_div = q, pt_jstride);
* cc_blind_sign_batch with k = 2 and k = 17 hidden messages, issuer scalars from the edge list, related
  ciphertext bases, one request with e = 0: c~1, c~2 against oc_msm with the call's own h;
* the G1 order-3 base (0, +-2) wherever G1 is the variable base: a verkey component and X~ in SigG2, an
  aggregated sigma_2 and a ciphertext in SigG1 (it is part of every G1 case list).  The aggregation and
  blind-signing outputs are the points themselves, so they pin the order-3 part of the sum.  The verify
  outputs cannot: e(P, T) = 1 for a point T of order 3, so a wrong multiple of T in pr changes neither
  verdict nor GT; there the order-3 cases show only that the rest of the sum is unharmed;
* the G2 order-13 base T13 (tests/golden/torsion.json) wherever G2 is the variable base: a verkey component
  and X~ in SigG1, an aggregated sigma_2 and a ciphertext in SigG2.  Here verify does pin the small-order
  part: pr is the Miller loop's Q side, a pr of order 13 r is rejected by the oracle and its GT bytes depend
  on the order-13 part of the sum.

What the file notices, measured on an MI355X with one branch changed at a time (never committed), BEFORE the
G2 case lists gained their order-13 rows; the counts were not measured again with those rows: the
doubling / to-identity choice flipped in the window walk's mixed addition of straus_g2lz_pair fails 7 of
these tests (verify, both aggregates, blind signing), in straus_g1lz_lane's 2 (verify), in the table build
of k_msm_straus<Fp, 16> 12 (every order-3 row).  Two changes it cannot notice, by the arithmetic: the same
flip in straus_g1lz_lane's table build (reached by order-3 bases alone, whose part the pairing drops), and
swapped operands in k_msm_straus_g2lz_g's join (the sum is the same point and the output is affine).
"""
import sys

import pytest

import straus_edges as S
from conftest import ROOT, host_threads
from fixed_edges import G1_IDENTITY, G2_IDENTITY, be48, gen_mul

sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
WIDE_MAX, FEXP_WIDE_MAX, PREP_WIDE_MAX = 4096, 2048, 1024  # slots.h kWideMax, kFexpWideMax, kPrepWideMax


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _tile(data, item, n):
    k = len(data) // item
    return (data * ((n + k - 1) // k))[:n * item]


def _first_diff(got, want, item, n):
    """Index of the first of n items of `got` that differs from `want` repeated, or -1."""
    k = len(want) // item
    for lo in range(0, n, k):
        m = min(k, n - lo)
        if got[lo * item:(lo + m) * item] != want[:m * item]:
            return next(lo + i for i in range(m) if got[(lo + i) * item:(lo + i + 1) * item] != want[i * item:(i + 1) * item])
    return -1


@pytest.mark.parametrize("q", S.VERIFY_Q)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_pervk_verify_edge_cases(ctxs, oc, mode, q):
    from coconut import verify_batch
    m, ctx = MODES[mode], ctxs[mode]
    sb, ob = (192, 97) if m == 0 else (97, 192)
    b = S.verify_batch_inputs(oc, m, q)
    want_v, want_gt = S.oracle_verify(oc, m, q, b, host_threads())
    assert want_v == b["expect"]  # the oracle agrees with the construction
    n = b["n"]
    assert n <= PREP_WIDE_MAX
    ctx.set_params(b["g"])

    def run(lo, hi):
        return verify_batch(ctx, hi - lo, q, b["s1"][lo * sb:hi * sb], b["s2"][lo * sb:hi * sb],
                            b["msgs"][lo * q * 48:hi * q * 48],
                            vk=(b["X"][lo * ob:hi * ob], b["Y"][lo * q * ob:hi * q * ob]), want_gt=True)
    v, gt = run(0, n)  # a small batch: the one-wave prep
    for i, name in enumerate(b["names"]):
        assert v[i] == want_v[i], (mode, q, name)
        assert gt[576 * i:576 * (i + 1)] == want_gt[576 * i:576 * (i + 1)], (mode, q, name)
    for i in sorted(set(range(0, n, 9)) | {n - 2, n - 1}):  # single credentials
        v1, g1 = run(i, i + 1)
        assert v1[0] == want_v[i] and g1 == want_gt[576 * i:576 * (i + 1)], (mode, q, b["names"][i])
    # tiled: the lane / lane-pair Straus prep, then the lane-pair final exponentiation, then the batch Miller loop
    for N in (PREP_WIDE_MAX + 1, FEXP_WIDE_MAX + 1, WIDE_MAX + 8):
        vN, gN = verify_batch(ctx, N, q, _tile(b["s1"], sb, N), _tile(b["s2"], sb, N), _tile(b["msgs"], q * 48, N),
                              vk=(_tile(b["X"], ob, N), _tile(b["Y"], q * ob, N)), want_gt=True)
        i = _first_diff(vN.tobytes(), bytes(want_v), 1, N)
        assert i < 0, (mode, q, N, i, b["names"][i % n])
        i = _first_diff(gN, want_gt, 576, N)
        assert i < 0, (mode, q, N, i, b["names"][i % n])


@pytest.mark.parametrize("t", S.AGG_T)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_signature_aggregate_edge_rows(ctxs, oc, mode, t):
    from coconut import signature_aggregate_batch
    m, ctx = MODES[mode], ctxs[mode]
    sg, sb = (2, 192) if m == 0 else (1, 97)
    rows = S.agg_rows(S.SIG_LAYOUT[m], t)
    n, L = len(rows), t + 1
    assert n <= 64
    ids, pts = S.agg_inputs(oc, sg, rows)
    want = [S.oracle_sig_aggregate(oc, m, t, r["ids"], pts[i * L * sb:(i + 1) * L * sb], pts[i * L * sb:(i + 1) * L * sb])
            for i, r in enumerate(rows)]
    ident = G2_IDENTITY if sg == 2 else G1_IDENTITY
    assert any(w[1] == ident for w in want)  # the identity encoding is among the expectations
    o1, o2 = signature_aggregate_batch(ctx, n, L, t, ids, pts, pts)
    for i, r in enumerate(rows):
        assert o1[i * sb:(i + 1) * sb] == want[i][0], (mode, t, r["name"])
        assert o2[i * sb:(i + 1) * sb] == want[i][1], (mode, t, r["name"])
    for i in range(0, n, 5):  # single rows
        a1, a2 = signature_aggregate_batch(ctx, 1, L, t, [rows[i]["ids"]], pts[i * L * sb:(i + 1) * L * sb],
                                           pts[i * L * sb:(i + 1) * L * sb])
        assert (a1, a2) == want[i], (mode, t, rows[i]["name"])


@pytest.mark.parametrize("t", S.AGG_T)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_verkey_aggregate_edge_rows(ctxs, oc, mode, t):
    from coconut import verkey_aggregate_batch
    m, ctx = MODES[mode], ctxs[mode]
    ob = 97 if m == 0 else 192
    rows = S.vkagg_rows(m, t)
    n, L, q = len(rows), t + 1, 2
    assert n * (q + 1) <= 64
    ids, X, Y = S.vkagg_inputs(oc, m, rows)
    oX, oY = verkey_aggregate_batch(ctx, n, L, t, q, ids, X, Y)
    for i, r in enumerate(rows):
        wX, wY = S.oracle_vk_aggregate(oc, m, t, q, r["ids"], X[i * L * ob:(i + 1) * L * ob],
                                       Y[i * L * q * ob:(i + 1) * L * q * ob])
        assert oX[i * ob:(i + 1) * ob] == wX, (mode, t, r["name"], "X")
        assert oY[i * q * ob:(i + 1) * q * ob] == wY, (mode, t, r["name"], "Y", r["Y1"]["name"])


@pytest.mark.parametrize("k", S.BLIND_K)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_blind_sign_edge_requests(ctxs, oc, mode, k):
    from coconut import blind_sign_batch
    m, ctx = MODES[mode], ctxs[mode]
    sg, sb = (2, 192) if m == 0 else (1, 97)
    q = k + 1
    for ci, call in enumerate(S.blind_sets(m, k)):
        rq = call["requests"]
        n = len(rq)
        assert 2 * n <= 64
        cm = gen_mul(oc, sg, [1000 * ci + r + 7 for r in range(n)])
        A = [S.point_bytes(oc, sg, r["a"]["logs"][:k], r["a"]["off"]) for r in rq]
        B = [S.point_bytes(oc, sg, r["b"]["logs"][:k], r["b"]["off"]) for r in rq]
        cts = [[(A[r][i * sb:(i + 1) * sb], B[r][i * sb:(i + 1) * sb]) for i in range(k)] for r in range(n)]
        hs, c1, c2 = blind_sign_batch(ctx, q, k, [cm[r * sb:(r + 1) * sb] for r in range(n)],
                                      [[be48(r["known"])] for r in rq], cts, be48(call["x"]), [be48(v) for v in call["y"]])
        assert len(set(hs)) == n  # every request its own h
        for r in range(n):
            w1 = S.msm(oc, sg, A[r] + hs[r], call["y"][:k] + [0])
            w2 = S.msm(oc, sg, B[r] + hs[r], call["y"][:k] + [rq[r]["e"]])
            assert c1[r] == w1, (mode, k, ci, rq[r]["name"], "c1")
            assert c2[r] == w2, (mode, k, ci, rq[r]["name"], "c2")
