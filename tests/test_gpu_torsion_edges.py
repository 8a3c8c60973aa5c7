"""GPU tests with curve points of small order outside G1 / G2 (tests/golden/torsion.json; the walks that say
which exceptional steps they reach are asserted on the CPU by tests/test_torsion_edges_model.py).  Every
comparison is byte equality with the C oracle, which tests/test_torsion_edges_model.py pins against an
independent projective Python model on the same points.

(a) Signature::verify, SigG2 (sigma is the Miller loop's Q side): sigma_1 / sigma_2 of order 13 (the loop's T
    meets lambda = 0, three doublings at (0 : Y : 0) and ends (0, 0, 0): a zero Miller value, whose final
    exponentiation has to give 576 zero bytes through the Fp12 inversion of zero, the compressed squarings'
    zero-denominator fallback and the quad-shared inversion beside valid neighbours), of order 23, 299 and
    13 r (no event: a non-trivial GT, bit-exact).  Batches of 16 (k_miller_wide2 + k_fexp1), 136
    (k_miller_wide + k_fexp1), 2,056 (k_miller_wide + the quad-lane final exponentiation) and 4,104
    (pair-lane k_miller + quad-lane), at neighbouring credentials, the ends of a quad, the ends of 128-credential
    blocks and the end of the batch; one single credential.
(b) SigG1 (Q side: pr and g~): a verkey of multiples of T13 with pr of order 13 and pr = O, one small-order
    component among honest ones, g~ = T13 (zero precomputed lines); shared verkey (G2 tables) and one
    verkey per credential through cc_verify_batch_pervk_device at q = 3 and 18 (the Straus layouts).
(c) PoK verify at q = 6: sigma'_1 of small order; J a small-order point and J + a small-order point, with
    the commitment recomputed so that the Schnorr relation holds and the pairing over J' is reached (GT
    byte-exact; in SigG2 J + T is accepted per proof); per proof and through the RLC form, whose fall-back
    word then can only come from the subgroup tests.
(d) cc_subgroup_check gives status 1 for every fixture point at lanes 0, 63 and 64; the RLC form rejects
    a batch holding one and falls back to the per-credential verdicts.
(e) fixed-base tables over small-order bases at widths 8 and 10 (identity entries inside k_table_fill's
    runs), digits on identity entries, on P and on -P, a partial sum that returns to the identity;
    cc_fixed_base_mul and the issuer table with small-order bases.
"""
import ctypes
import random
import sys

import numpy as np
import pytest

import torsion_edges as T
from conftest import ROOT, golden, host_threads
from fixed_edges import G1_GENERATOR, G2_GENERATOR, R, be48, gen_mul  # noqa: F401

sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
WIDE_MAX, FEXP_WIDE_MAX = 4096, 2048  # slots.h kWideMax, kFexpWideMax
# <= 128 credentials: k_miller_wide2 (miller_wide.hip: kWide2Max = 256 pairs); <= kFexpWideMax: k_fexp1, above it the
# quad-lane final exponentiation; above kWideMax the pair-lane k_miller
SIZES = (16, 136, FEXP_WIDE_MAX + 8, WIDE_MAX + 8)
FX = T.fixture()
ZERO_GT = bytes(576)
ORDER13 = ("T13,valid", "valid,T13", "T13,T13b")  # the cases whose Miller value is zero


def g2(name):
    return FX["G2"][name]["point"]


def g1(name):
    return FX["G1"][name]["point"]


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def valid_g2(ctxs):
    """One valid SigG2 batch of the largest size (bench.make_verify_batch); smaller sizes take its head."""
    import bench
    return bench.make_verify_batch(ctxs["G2"], 0, SIZES[-1], 6, seed=4242, bad_every=0)


def _put(buf, i, item, val):
    assert len(val) == item
    buf[i * item:(i + 1) * item] = val


def _check(names, v, gt, want_v, want_gt):
    assert len(gt) == len(want_gt)
    for i, name in names.items():
        assert v[i] == want_v[i], (i, name)
        assert gt[576 * i:576 * (i + 1)] == want_gt[576 * i:576 * (i + 1)], (i, name)
    if list(v) != list(want_v) or gt != want_gt:  # the untouched credentials
        bad = next(i for i in range(len(want_v)) if v[i] != want_v[i] or gt[576 * i:576 * (i + 1)] != want_gt[576 * i:576 * (i + 1)])
        raise AssertionError(("untouched credential changed", bad))


# ---------------------------------------------------------------- (a) SigG2: sigma of small order
def _sigma_cases(oc):
    t23x2 = T.oracle_msm(oc, 2, g2("T23"), [2])
    return [("T13,valid", g2("T13"), None), ("valid,T13", None, g2("T13")), ("T13,T13b", g2("T13"), g2("T13b")),
            ("T23,valid", g2("T23"), None), ("T23,2T23", g2("T23"), t23x2), ("kG+T13,valid", g2("kG+T13"), None),
            ("T13+T23,valid", g2("T13+T23"), None)]


def _positions(n):
    """[(credential, case)]: neighbours (2k, 2k + 1), the ends (4k, 4k + 3) of a quad whose middle stays valid,
    the ends of 128-credential blocks, the end of the batch."""
    if n < 128:
        return [(2, 0), (3, 0), (4, 1), (7, 1), (0, 2), (n - 1, 3), (8, 4), (11, 5), (12, 6), (13, 4)]
    pos = []
    for c in range(7):
        base = 16 * (c + 1)
        pos += [(base + 2, c), (base + 3, c), (base + 4, c), (base + 7, c)]
    edges = [0, 127, 128, n - 1]
    if n > 256:
        last = n // 128 * 128
        edges += [255, 256, last - 128, last - 1, last]
    off = n % 7
    return pos + [(e, (k + off) % 7) for k, e in enumerate(edges)]


@pytest.mark.parametrize("n", SIZES)
def test_verify_sigg2_small_order_sigma(ctxs, oc, valid_g2, n):
    from coconut import verify_batch
    ctx, b, q, sb = ctxs["G2"], valid_g2, 6, 192
    cases = _sigma_cases(oc)
    s1, s2 = bytearray(b["s1"][:n * sb]), bytearray(b["s2"][:n * sb])
    names = {}
    for i, c in _positions(n):
        assert i not in names and 0 <= i < n
        name, a1, a2 = cases[c]
        names[i] = name
        if a1:
            _put(s1, i, sb, a1)
        if a2:
            _put(s2, i, sb, a2)
    assert {nm for nm in names.values()} == {c[0] for c in cases}
    s1, s2, msgs = bytes(s1), bytes(s2), b["msgs"][:n * q * 48]
    # the oracle on the first 16 credentials and on the quad of every touched one (the verkey is shared, so a
    # credential's result does not depend on its neighbours); every other one is valid: verdict 1, GT one
    sel = sorted(set(range(16)) | {j for i in names for j in range(i // 4 * 4, min(n, i // 4 * 4 + 4))})
    take = lambda data, item: b"".join(data[i * item:(i + 1) * item] for i in sel)  # noqa: E731
    sv, sgt = T.oracle_verify(oc, 0, len(sel), q, take(s1, sb), take(s2, sb), take(msgs, q * 48), b["X"], b["Y"],
                              b["g_tilde"], 0, host_threads())
    one = sgt[576:2 * 576]
    assert 1 not in names and sv[1] == 1 and one[47] == 1 and not any(one[:47]) and not any(one[48:])
    want_v, want_gt = [1] * n, bytearray(one * n)
    for k, i in enumerate(sel):  # a touched credential is rejected, order 13 gives the zero GT; the rest stay valid
        want_v[i] = sv[k]
        want_gt[576 * i:576 * (i + 1)] = sgt[576 * k:576 * (k + 1)]
        if i in names:
            assert sv[k] == 0, names[i]
            assert (sgt[576 * k:576 * (k + 1)] == ZERO_GT) == (names[i] in ORDER13), names[i]
        else:
            assert sv[k] == 1 and sgt[576 * k:576 * (k + 1)] == one
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    v, gt = verify_batch(ctx, n, q, s1, s2, msgs, want_gt=True)
    _check(names, v, gt, want_v, bytes(want_gt))


def test_verify_sigg2_single_credential_order13(ctxs, oc, valid_g2):
    from coconut import verify_batch
    ctx, b, q = ctxs["G2"], valid_g2, 6
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    for s1, s2 in ((g2("T13"), b["s2"][:192]), (b["s1"][:192], g2("-T13"))):
        want_v, want_gt = T.oracle_verify(oc, 0, 1, q, s1, s2, b["msgs"][:q * 48], b["X"], b["Y"], b["g_tilde"], 0, 1)
        assert want_v == [0] and want_gt == ZERO_GT
        v, gt = verify_batch(ctx, 1, q, s1, s2, b["msgs"][:q * 48], want_gt=True)
        assert list(v) == [0] and gt == ZERO_GT


# ---------------------------------------------------------------- (b) SigG1: pr and g~ of small order
def _g1_sigmas(oc, n, seed):
    rng = random.Random(seed)
    return (gen_mul(oc, 1, [rng.randrange(1, R) for _ in range(n)]), gen_mul(oc, 1, [rng.randrange(1, R) for _ in range(n)]))


def _sigg1_verkeys(oc, q):
    """[(name, X~, Y~ (q points), g~, messages of credential i)] over the G2 fixture points."""
    rng = random.Random(77 + q)
    honest = gen_mul(oc, 2, [rng.randrange(1, R) for _ in range(q + 2)])
    hX, hY, hg = honest[:192], honest[192:192 * (q + 1)], honest[192 * (q + 1):]
    a = [rng.randrange(1, 13) for _ in range(q)]
    a[q // 2] = 0  # one component the identity (a_j = 0 mod 13)
    t13 = g2("T13")
    yt = b"".join(T.oracle_msm(oc, 2, t13, [13 * rng.randrange(1 << 200) + aj]) for aj in a)

    def msgs_for(residue):
        """pr = (1 + sum m_j a_j) T13 has the given residue mod 13: the last message with a_j != 0 adjusts it"""
        def f(i):
            r2 = random.Random(1000 * q + i)
            m = [r2.randrange(R) for _ in range(q)]
            j = max(k for k in range(q) if a[k])
            rest = 1 + sum(mk * ak for k, (mk, ak) in enumerate(zip(m, a)) if k != j)
            m[j] %= R - 13  # stays below r after the adjustment: a value >= r would be reduced and lose its residue
            m[j] = m[j] - m[j] % 13 + (residue - rest) * pow(a[j], -1, 13) % 13
            assert 0 <= m[j] < R and (1 + sum(mk * ak for mk, ak in zip(m, a))) % 13 == residue
            return m
        return f

    def rnd(i):
        r2 = random.Random(2000 * q + i)
        return [r2.randrange(R) for _ in range(q)]

    mixed = bytearray(hY)
    mixed[192:384] = t13
    return [("pr_order13", t13, yt, hg, msgs_for(1 + (q % 11))), ("pr_identity", t13, yt, hg, msgs_for(0)),
            ("one_component_T13", hX, bytes(mixed), hg, rnd), ("gtilde_T13", hX, hY, t13, rnd)]


@pytest.mark.parametrize("n", [16, WIDE_MAX + 8])
def test_verify_sigg1_small_order_verkey_and_gtilde(ctxs, oc, n):
    from coconut import verify_batch
    ctx, q = ctxs["G1"], 6
    n0 = min(n, 72)  # the oracle on n0 distinct credentials; the larger batch repeats them
    s1, s2 = _g1_sigmas(oc, n0, 5 + n)
    s1 = bytearray(s1)
    _put(s1, n0 - 2, 97, T.G1_IDENTITY)  # the oracle's identity rule beside the small-order Q side
    s1 = bytes(s1)
    rep = (n + n0 - 1) // n0
    for name, X, Y, g, mf in _sigg1_verkeys(oc, q):
        msgs = b"".join(be48(m) for i in range(n0) for m in mf(i))
        want_v, want_gt = T.oracle_verify(oc, 1, n0, q, s1, s2, msgs, X, Y, g, 0, host_threads())
        assert not any(want_v)
        if name == "pr_order13":  # a zero Miller value from pr's side (but for the identity sigma_1: that pair is one)
            assert want_gt[:576] == ZERO_GT
        ctx.set_params(g)
        ctx.set_verkey(X, Y)
        v, gt = verify_batch(ctx, n, q, (s1 * rep)[:n * 97], (s2 * rep)[:n * 97], (msgs * rep)[:n * q * 48], want_gt=True)
        assert not v.any(), name
        for i in range(n):
            assert gt[576 * i:576 * (i + 1)] == want_gt[576 * (i % n0):576 * (i % n0 + 1)], (name, i)


@pytest.mark.parametrize("q", [3, 18])
def test_verify_sigg1_pervk_small_order_bases(ctxs, oc, q):
    """The same verkeys as one verkey per credential (cc_verify_batch_pervk_device): the first small-order
    G2 bases in the variable-base Straus layouts (k_prep_sigg1_var_wide; tiled past kPrepWideMax the
    lane-pair form)."""
    import torch
    from coconut import _lib
    ctx = ctxs["G1"]
    vks = _sigg1_verkeys(oc, q)
    dev = torch.device("cuda", 0)
    to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    honest_g, t13 = vks[0][3], g2("T13")
    assert {vk[3] for vk in vks} == {honest_g, t13}
    # g~ is the context's, so one call per g~: the honest g~ at both sizes, g~ = T13 at n = 16
    for n, gs in ((16, [honest_g, t13]), (1032, [honest_g])):
        for g in gs:
            use = [vk for vk in vks if vk[3] == g]
            pick = [use[i % len(use)] for i in range(n)]
            s1, s2 = _g1_sigmas(oc, n, 9 + n + q)
            msgs = b"".join(be48(m) for i in range(n) for m in pick[i][4](i))
            X, Y = b"".join(p[1] for p in pick), b"".join(p[2] for p in pick)
            want_v, want_gt = T.oracle_verify(oc, 1, n, q, s1, s2, msgs, X, Y, g, 1, host_threads())
            ctx.set_params(g)
            v = torch.zeros(n, dtype=torch.uint8, device=dev)
            gt = torch.zeros(n * 576, dtype=torch.uint8, device=dev)
            D = [to(x) for x in (s1, s2, msgs, X, Y)]
            torch.cuda.synchronize()
            assert _lib.lib.cc_verify_batch_pervk_device(ctx.h, n, q, *[P(x) for x in D], P(v), P(gt), None) == 0
            torch.cuda.synchronize()
            v, gt = v.cpu().numpy(), bytes(gt.cpu().numpy())
            assert list(v) == want_v, (n, [p[0] for p in use])
            for i in range(n):
                assert gt[576 * i:576 * (i + 1)] == want_gt[576 * i:576 * (i + 1)], (n, i, pick[i][0])


# ---------------------------------------------------------------- (c) PoK
def _oracle_pok(oc, d, b):
    mode = b["mode"]
    sb, ob = (192, 97) if mode == 0 else (97, 192)
    r, nr, q = len(b["revealed"]), b["nresp"], b["q"]
    idx = (ctypes.c_uint64 * max(r, 1))(*b["revealed"])
    h = bytes.fromhex
    X, Y, g = h(d["vk"]["X"]), b"".join(h(y) for y in d["vk"]["Y"]), h(d["g_tilde"])
    out = []
    for i in range(b["n"]):
        gt = ctypes.create_string_buffer(576)
        v = oc.oc_pok_verify(mode, ctypes.c_size_t(q), ctypes.c_size_t(r), b["s1"][i * sb:(i + 1) * sb],
                             b["s2"][i * sb:(i + 1) * sb], b["J"][i * ob:(i + 1) * ob], b["T"][i * ob:(i + 1) * ob],
                             b["resp"][i * nr * 48:(i + 1) * nr * 48], ctypes.c_size_t(nr), b["chal"][48 * i:48 * (i + 1)],
                             idx, b["rev"][i * r * 48:(i + 1) * r * 48], X, Y, g, gt)
        out.append((v, gt.raw))
    return out


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_pok_small_order_sigma_and_J(ctxs, oc, mode):
    from test_gpu_pok_rlc import _decide, _fix_batch, _host, _load
    from coconut import pok_verify_batch
    d = golden(f"pok_{mode.lower()}_q6.json")
    ctx = ctxs[mode]
    _load(ctx, d)
    valid = [p for p in d["proofs"] if p["kind"] == "valid"]
    base = _fix_batch(d, [valid[i % len(valid)] for i in range(8)])
    sb, ob = (192, 97) if MODES[mode] == 0 else (97, 192)
    if mode == "G2":
        sig = [g2("T13"), g2("T23")]
        Js = [g1("T3"), g1("T11")]
    else:
        sig = [g1("T3"), g1("T11")]  # (the Miller loop's P side: cofactor-blind)
        Js = [g2("T13"), g2("T23")]
    og, nr, q = (1 if MODES[mode] == 0 else 2), base["nresp"], base["q"]
    h = bytes.fromhex
    hidden = [i for i in range(q) if i not in base["revealed"]]
    schnorr_bases = h(d["g_tilde"]) + b"".join(h(d["vk"]["Y"][i]) for i in hidden)
    num = lambda x: int.from_bytes(x, "big")  # noqa: E731

    s1 = bytearray(base["s1"])
    _put(s1, 1, sb, sig[0])
    _put(s1, 4, sb, sig[1])
    b1 = dict(base, s1=bytes(s1))
    # J replaced by a small-order point (proofs 2, 7) and J + a small-order point (3, 5); the commitment is
    # recomputed, T = sum rho_k B_k + c J, so the Schnorr relation HOLDS for the new J: the oracle reaches the
    # pairing over J' = X~ + J + ..., its GT bytes pin the device's, and nothing but J's subgroup test (flag bit 6
    # of pok_rlc.hip; bit 3 is the Schnorr check) can raise the partial's fall-back word
    J, Tc = bytearray(base["J"]), bytearray(base["T"])
    for i, newJ in ((2, Js[0]), (7, Js[1]), (3, T.oracle_msm(oc, og, base["J"][3 * ob:4 * ob] + Js[0], [1, 1])),
                    (5, T.oracle_msm(oc, og, base["J"][5 * ob:6 * ob] + Js[1], [1, 1]))):
        _put(J, i, ob, newJ)
        sc = [num(base["resp"][(i * nr + k) * 48:(i * nr + k + 1) * 48]) for k in range(nr)]
        _put(Tc, i, ob, T.oracle_msm(oc, og, schnorr_bases + newJ, sc + [num(base["chal"][48 * i:48 * (i + 1)])]))
    b2 = dict(base, J=bytes(J), T=bytes(Tc))
    for tag, b, touched in (("sigma1", b1, (1, 4)), ("J", b2, (2, 3, 5, 7))):
        want = _oracle_pok(oc, d, b)
        assert [w[0] for i, w in enumerate(want) if i not in touched] == [1] * (8 - len(touched))
        # every proof's Schnorr relation holds (sigma'_1 is no part of it), so the oracle reached every pairing:
        # a GT of 576 zero bytes below is a computed one, not a proof rejected before the pairing
        if tag == "sigma1":
            assert all(any(wgt) for i, (_, wgt) in enumerate(want) if not (mode == "G2" and i == 1))
            if mode == "G2":
                assert want[1] == (0, ZERO_GT) and want[4][0] == 0
        elif mode == "G2":  # e(sigma, T) = 1 for a G1 point T of order 3 or 11: J + T is accepted per proof, T alone not
            assert [want[i][0] for i in touched] == [0, 1, 1, 0] and all(any(w[1]) for w in want)
        else:  # J' of order 13 r / 23 r on the Miller loop's Q side: no event, a non-trivial GT, rejected
            assert [want[i][0] for i in touched] == [0, 0, 0, 0] and all(any(w[1]) for w in want)
        v, gt = pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], b["s1"], b["s2"], b["J"], b["T"], b["resp"],
                                 b["chal"], b["rev"], want_gt=True)
        for i, (wv, wgt) in enumerate(want):
            assert v[i] == wv, (mode, tag, i)
            assert gt[576 * i:576 * (i + 1)] == wgt, (mode, tag, i)
        vr = _host(ctx, b, True)
        assert list(vr) == [w[0] for w in want], (mode, tag)
        accept, flag, _ = _decide(ctx, b)
        assert not accept, (mode, tag)
        # the partial's fall-back word (0 / 1: the OR over the batch of rlc.hip's sigma flags and pok_rlc.hip's
        # bits 3 and 6).  Every Schnorr relation holds here, so bit 3 is out: the word can only come from the
        # subgroup tests (the Miller loop's T for a G2 sigma'_1, the phi test for a G1 one, J's test)
        assert flag == 1, (mode, tag)
    if mode == "G2":
        # the forgery path itself: only J + T, every per-proof verdict 1 and the weighted product one; the
        # RLC form must still refuse to accept, and only J's subgroup test can make it
        keep = [0, 3, 5, 6]
        cut = lambda k, item: b"".join(b2[k][i * item:(i + 1) * item] for i in keep)  # noqa: E731
        r = len(base["revealed"])
        b3 = dict(base, n=len(keep), s1=cut("s1", sb), s2=cut("s2", sb), J=cut("J", ob), T=cut("T", ob),
                  resp=cut("resp", nr * 48), chal=cut("chal", 48), rev=cut("rev", r * 48))
        assert _host(ctx, b3, False).all()
        accept, flag, _ = _decide(ctx, b3)
        assert flag == 1 and not accept
        assert _host(ctx, b3, True).all()
        honest = lambda k, item: b"".join(base[k][i * item:(i + 1) * item] for i in keep)  # noqa: E731
        accept, flag, _ = _decide(ctx, dict(b3, J=honest("J", ob), T=honest("T", ob)))
        assert accept and flag == 0  # (the same proofs with their own J and T are accepted)


# ---------------------------------------------------------------- (d) subgroup status and the RLC form
@pytest.mark.parametrize("group", [1, 2])
def test_subgroup_check_small_order_points(ctxs, oc, group):
    from coconut import subgroup_check
    eb = 97 if group == 1 else 192
    good = gen_mul(oc, group, [random.Random(3).randrange(1, R) + i for i in range(130)])
    for name, rec in FX["G1" if group == 1 else "G2"].items():
        pts = bytearray(good)
        for lane in (0, 63, 64):
            _put(pts, lane, eb, rec["point"])
        st = subgroup_check(ctxs["G2"], group, bytes(pts))
        assert [int(s) for s in st] == [1 if i in (0, 63, 64) else 2 for i in range(130)], name


@pytest.mark.parametrize("n", [8, 260])
def test_rlc_rejects_small_order_sigma(ctxs, oc, valid_g2, n):
    import torch
    from coconut import verify_batch
    from coconut.dist import PARTIAL_FLAG, DeviceEngine
    ctx, b, q, sb = ctxs["G2"], valid_g2, 6, 192
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    msgs = b["msgs"][:n * q * 48]
    dev = torch.device("cuda", 0)
    to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    assert verify_batch(ctx, n, q, b["s1"][:n * sb], b["s2"][:n * sb], msgs, rlc=True).all()
    for k, (name, a1, a2) in enumerate([c for c in _sigma_cases(oc) if c[0] in ("T13,valid", "valid,T13", "T23,valid",
                                                                                "kG+T13,valid")]):
        i = (5 + 67 * k) % n
        s1, s2 = bytearray(b["s1"][:n * sb]), bytearray(b["s2"][:n * sb])
        if a1:
            _put(s1, i, sb, a1)
        if a2:
            _put(s2, i, sb, a2)
        s1, s2 = bytes(s1), bytes(s2)
        per = verify_batch(ctx, n, q, s1, s2, msgs)
        want_v, _ = T.oracle_verify(oc, 0, n, q, s1, s2, msgs, b["X"], b["Y"], b["g_tilde"], 0, host_threads())
        assert want_v == [int(j != i) for j in range(n)] and [int(x) for x in per] == want_v, name
        assert np.array_equal(verify_batch(ctx, n, q, s1, s2, msgs, rlc=True), per), name
        e = DeviceEngine(ctx, n, q, to(s1), to(s2), to(msgs), seed=bytes(range(32)))
        part = e.partial().clone()
        torch.cuda.synchronize()
        assert not e.finish(part.reshape(1, -1), 1), name
        if a1:  # the Miller-T subgroup test, not only the zero product, caught the point
            assert int(part[PARTIAL_FLAG].item()) != 0, name


# ---------------------------------------------------------------- (e) fixed-base tables over small-order bases
def _digit_msgs(wbits, m):
    """Scalars whose table digits (fixed_edges.ft_digit) land on identity entries (d = 0 mod m), on P
    (d = 1 mod m), on -P (d = -1 mod m); partial sums that return to the identity mid-chain; 0 and r - 1."""
    def D(w, d):
        return d << (wbits * w)
    big = (1 << wbits) - 1
    top_m = big - big % m  # the largest identity digit
    out = [0, R - 1, m, D(0, m) | D(1, 2 * m) | D(3, top_m), 1, m + 1, D(0, 1) | D(2, top_m + 1 if top_m + 1 <= big else 1),
           m - 1, D(0, m - 1) | D(1, 2 * m - 1), D(0, 1) | D(1, m - 1) | D(2, 1), D(0, m - 1) | D(1, 1) | D(4, 2),
           D(0, 32) | D(1, 33) | D(2, 64) | D(3, 65) | D(4, 96)]  # the ends of k_table_fill's runs
    import fixed_edges as F
    assert all(d % m == 0 for d in F.digits(out[3], wbits)) and F.digits(out[3], wbits)[3] == top_m
    assert F.digits(out[9], wbits)[:3] == [1, m - 1, 1]  # P, then to the identity, then on from it
    for d in F.digits(out[3], wbits)[:4]:  # the table-walk model calls these entries the identity
        if d:
            assert (d - 1) % T.FILL_RUN in T.table_events(wbits, (d - 1) // T.FILL_RUN, m)["identity"], (wbits, m, d)
    for d in (1, m + 1, m - 1, 2 * m - 1, 32, 33, 64, 65, 96):  # and these not
        assert (d - 1) % T.FILL_RUN not in T.table_events(wbits, (d - 1) // T.FILL_RUN, m)["identity"] or d % m == 0
    return out


def _table_verify(ctx, oc, mode, bits, X, Y, g, q, pats):
    """Credentials (random sigma) whose first two messages run through `pats`, at n = 16 (the one-wave prep)
    and tiled to kWideMax + 8 (the lane-pair prep): verdicts and GT against the oracle."""
    from coconut import verify_batch
    sg, sb = (2, 192) if mode == 0 else (1, 97)
    ctx.set_table_bits(bits, 0)
    ctx.set_params(g)
    ctx.set_verkey(X, Y)
    assert ctx.table_bits()[0] == bits
    rng = random.Random(bits + mode)
    n = max(16, len(pats[0]))
    rows = []
    for i in range(n):
        m = [rng.randrange(R) for _ in range(q)]
        m[0], m[1] = pats[0][i % len(pats[0])], pats[1][(i + i // len(pats[1])) % len(pats[1])]
        rows.append(b"".join(be48(v) for v in m))
    msgs = b"".join(rows)
    s1 = gen_mul(oc, sg, [rng.randrange(1, R) for _ in range(n)])
    s2 = gen_mul(oc, sg, [rng.randrange(1, R) for _ in range(n)])
    want_v, want_gt = T.oracle_verify(oc, mode, n, q, s1, s2, msgs, X, Y, g, 0, host_threads())
    for N in (n, WIDE_MAX + 8):
        rep = (N + n - 1) // n
        v, gt = verify_batch(ctx, N, q, (s1 * rep)[:N * sb], (s2 * rep)[:N * sb], (msgs * rep)[:N * q * 48], want_gt=True)
        for i in range(N):
            assert v[i] == want_v[i % n], (bits, N, i)
            assert gt[576 * i:576 * (i + 1)] == want_gt[576 * (i % n):576 * (i % n + 1)], (bits, N, i)


@pytest.mark.parametrize("bits", [8, 10])
def test_tables_sigg2_small_order_g1_bases(oc, valid_g2, bits):
    import coconut
    b, q = valid_g2, 6
    ctx = coconut.Context(0, coconut.GroupMode(0))
    try:
        # an identity component next to the small-order ones: k_table_pow2's inf[j], whole windows of (0, 0)
        Y = g1("T3") + g1("T11") + T.G1_IDENTITY + b["Y"][3 * 97:]
        pats = (_digit_msgs(bits, 3), _digit_msgs(bits, 11))
        _table_verify(ctx, oc, 0, bits, b["X"], Y, b["g_tilde"], q, pats)
        # X~ = -T3: with m_0 = 1 (the entry T3) the chain that starts from X~ returns to the identity at once
        _table_verify(ctx, oc, 0, bits, g1("-T3"), Y, b["g_tilde"], q, pats)
    finally:
        ctx.close()


@pytest.mark.parametrize("bits", [8, 10])
def test_tables_sigg1_small_order_g2_bases(oc, bits):
    import coconut
    q = 6
    ctx = coconut.Context(0, coconut.GroupMode(1))
    try:
        honest = gen_mul(oc, 2, [random.Random(31).randrange(1, R) + i for i in range(q + 1)])
        Y = g2("T23") + g2("T13b") + T.G2_IDENTITY + honest[3 * 192:q * 192]  # (an identity component: inf[j])
        pats = (_digit_msgs(bits, 23), _digit_msgs(bits, 13))
        _table_verify(ctx, oc, 1, bits, g2("T13"), Y, honest[q * 192:], q, pats)
        # X~ = -T13, Y~_0 = T13: with m_0 = 1 the chain that starts from X~ returns to the identity at once
        Y = g2("T13") + g2("T23") + T.G2_IDENTITY + honest[3 * 192:q * 192]
        _table_verify(ctx, oc, 1, bits, g2("-T13"), Y, honest[q * 192:], q, (pats[1], pats[0]))
    finally:
        ctx.close()


@pytest.mark.parametrize("group,name", [(1, "T3"), (1, "T11"), (2, "T13"), (2, "T23")])
def test_fixed_base_mul_small_order_base(ctxs, oc, group, name):
    import coconut
    from oracle import bls12_381 as B
    rec = FX["G1" if group == 1 else "G2"][name]
    m, eb = rec["order"], 97 if group == 1 else 192
    curve, dec, enc = (B.G1, B.g1_from_bytes, B.g1_to_bytes) if group == 1 else (B.G2, B.g2_from_bytes, B.g2_to_bytes)
    rng = random.Random(m)
    ks = [0, 1, m - 1, m, m + 1, R - 1] + [rng.randrange(R) for _ in range(64)]
    got = coconut.fixed_base_mul(ctxs["G2"], group, rec["point"], b"".join(be48(k) for k in ks))
    mult = [curve.mul_any(dec(rec["point"]), j) for j in range(m)]  # k P = (k mod m) P
    for i, k in enumerate(ks):
        want = enc(mult[k % m])
        assert T.oracle_msm(oc, group, rec["point"], [k]) == want  # the C oracle agrees
        assert got[eb * i:eb * (i + 1)] == want, (name, hex(k))


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_issuer_table_small_order_keys(oc, mode):
    import coconut
    m = MODES[mode]
    og, ob = (1, 97) if m == 0 else (2, 192)
    q, ids = 2, [1, 2, 3, 4]
    honest = gen_mul(oc, og, [random.Random(8 + m).randrange(1, R) + i for i in range(4 * (q + 1))])
    keys = [(honest[3 * i * ob:(3 * i + 1) * ob], honest[(3 * i + 1) * ob:(3 * i + 3) * ob]) for i in range(4)]
    keys[1] = (g1("T3"), g1("T11") + g1("-T3")) if m == 0 else (g2("T13"), g2("T23") + g2("T13b"))
    ctx = coconut.Context(0, coconut.GroupMode(m))
    try:
        ctx.set_table_bits(0, 8)
        ctx.set_issuers(ids, b"".join(k[0] for k in keys), b"".join(k[1] for k in keys), q)
        assert ctx.table_bits()[1] == 8
        for t, rows in ((2, [[1, 2], [2, 3], [2, 1], [4, 2], [3, 4]]), (3, [[1, 2, 3], [2, 3, 4], [4, 2, 1], [1, 3, 4]])):
            oX, oY = coconut.verkey_aggregate_ids(ctx, len(rows), t, t, rows)
            for i, row in enumerate(rows):
                X = b"".join(keys[j - 1][0] for j in row)
                Y = b"".join(keys[j - 1][1] for j in row)
                ox, oy = ctypes.create_string_buffer(ob), ctypes.create_string_buffer(ob * q)
                assert oc.oc_verkey_aggregate(m, ctypes.c_size_t(t), ctypes.c_size_t(t), ctypes.c_size_t(q),
                                              (ctypes.c_uint64 * t)(*row), X, Y, ox, oy) == 0
                assert oX[i * ob:(i + 1) * ob] == ox.raw, (mode, t, row)
                assert oY[i * q * ob:(i + 1) * q * ob] == oy.raw, (mode, t, row)
    finally:
        ctx.close()
