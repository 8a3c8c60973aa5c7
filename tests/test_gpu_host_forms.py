"""GPU tests of the host forms' staging (csrc/devbuf.h HostForm, capi_*.cpp):
cc_subgroup_check, cc_hash_to_curve, cc_hash_msg, cc_fixed_base_mul, cc_blind_sign_batch,
cc_sigreq_verify_batch and cc_vss_verify_batch keep their staging buffers as locals that are freed on
return.  Each is called on ONE context at n = 1, at n = 3 (every buffer is allocated anew and larger) and at
n = 1 again, in both group modes, and every output is compared byte for byte with the oracle's fixtures
(tests/golden/host_forms.json: q = 2, k = 1, t = 2, the smallest shapes with a hidden and a known message;
hash_to_curve.json and subgroup.json as the codec tests use them).  An ownership mistake — a buffer handed out of
compute_h_batch by reference, a moved-from buffer, a buffer freed under a queued copy — shows as wrong
bytes or a fault here.  A refused call (documented error code) must leave the context usable.

The verify, aggregation and PoK verify forms (cc_verify_batch with a shared verkey, one verkey per credential
and rlc = 1; cc_signature_aggregate_batch, cc_verkey_aggregate_batch, cc_verkey_aggregate_ids;
cc_pok_verify_batch, cc_pok_verify_batch_rlc, cc_pok_verify_batch_pervk) stage through the context's own
buffers, which grow at n = 3 and are reused at n = 1: the same three calls over cuts of verify_*_q6.json,
aggregate_*.json (t = 3) and pok_*_q6.json, and over proofs of tests/pok_pervk_cases.py.  Each RLC form runs over
a cut that all verifies (the whole-batch check accepts: one sequence) and over one holding a refused element
(the per-element sequence follows)."""
import ctypes

import numpy as np
import pytest

import pok_pervk_cases as C
from conftest import golden, host_threads
from test_gpu_parity import MODES

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 1)  # grow, then shrink back: the second call reallocates every staging buffer


def _b(h):
    return bytes.fromhex(h)


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def fx():
    return golden("host_forms.json")


def _blind_sign(ctx, case, rq):
    from coconut import blind_sign_batch
    return blind_sign_batch(ctx, case["q"], case["k"], [_b(r["commitment"]) for r in rq],
                            [[_b(m) for m in r["known"]] for r in rq],
                            [[(_b(a), _b(b)) for a, b in r["ciphertexts"]] for r in rq], _b(case["x"]),
                            [_b(v) for v in case["y"]])


def _check_blind_sign(ctx, case, rq):
    hs, c1s, c2s = _blind_sign(ctx, case, rq)
    for r, h, c1, c2 in zip(rq, hs, c1s, c2s):
        assert (h.hex(), c1.hex(), c2.hex()) == (r["h"], r["c1"], r["c2"]), r["kind"]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_codec_forms_at_growing_batch(ctxs, mode):
    from coconut import hash_msg, hash_to_curve, subgroup_check
    ctx = ctxs[mode]
    msgs = golden("hash_to_curve.json")["messages"]
    sub = golden("subgroup.json")
    for i, n in enumerate(SIZES):
        rows = msgs[-n:] if i < 2 else msgs[:n]  # the longest messages; at the end the empty one (no upload)
        data = [_b(r["msg"]) for r in rows]
        assert [d.hex() for d in hash_msg(ctx, data)] == [r["shake256_48"] for r in rows], n
        for group, key in ((1, "g1"), (2, "g2")):
            assert [p.hex() for p in hash_to_curve(ctx, group, data)] == [r[key] for r in rows], (n, group)
            pts = sub[f"G{group}"][:n]
            st = subgroup_check(ctx, group, b"".join(_b(p["point"]) for p in pts))
            assert list(st) == [p["status"] for p in pts], (n, group)


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_mul_at_growing_batch(ctxs, fx, mode, group):
    from coconut import fixed_base_mul
    key = "g1" if group == 1 else "g2"
    kg, eb = fx["keygen"], 97 if group == 1 else 192
    for n in SIZES:
        rows = kg[f"derive_{key}"][:n]
        out = fixed_base_mul(ctxs[mode], group, _b(kg[f"g_tilde_{key}"]), b"".join(_b(r["x"]) for r in rows))
        assert [out[i * eb:(i + 1) * eb].hex() for i in range(n)] == [r["alpha"] for r in rows], n


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_issuance_forms_at_growing_batch(ctxs, fx, mode):
    from coconut import sigreq_verify_batch
    ctx, case = ctxs[mode], fx["issuance"][mode]
    assert (case["q"], case["k"]) == (2, 1)
    assert {r["verdict"] for r in case["requests"]} == {0, 1}
    for n in SIZES:
        rq = case["requests"][-n:] if n == 1 else case["requests"][:n]  # n = 1: a refused proof
        _check_blind_sign(ctx, case, rq)
        v = sigreq_verify_batch(ctx, 2, 1, _b(case["g"]), [_b(x) for x in case["h"]][:1],
                                [_b(r["commitment"]) for r in rq], [[_b(m) for m in r["known"]] for r in rq],
                                [[(_b(a), _b(b)) for a, b in r["ciphertexts"]] for r in rq], [_b(r["pk"]) for r in rq],
                                [_b(r["proof"]) for r in rq], [_b(r["chal"]) for r in rq])
        assert list(v) == [r["verdict"] for r in rq], n


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_vss_verify_at_growing_batch(ctxs, fx, mode):
    from coconut import vss_verify_batch
    kg = fx["keygen"]
    assert kg["t"] == 2 and {c["ok"] for c in kg["checks"]} == {0, 1}
    sets = [[_b(c) for c in s] for s in kg["commitments"]]
    for n in SIZES:
        ch = kg["checks"][-n:]  # the last check is a refused share
        v = vss_verify_batch(ctxs[mode], 2, _b(kg["g"]), _b(kg["h"]), sets, [c["set"] for c in ch], [c["id"] for c in ch],
                             [(_b(c["s"]), _b(c["s_t"])) for c in ch])
        assert list(v) == [c["ok"] for c in ch], n


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_refused_calls_leave_the_context_usable(ctxs, fx, mode):
    from coconut import CoconutError, CoconutErrorKind, blind_sign_batch, hash_to_curve
    from coconut._lib import lib
    ctx, case = ctxs[mode], fx["issuance"][mode]
    sb = ctx.mode.sig_bytes
    # cc_hash_to_curve: offsets[0] != 0 is CC_ERR_DECODE
    rows = golden("hash_to_curve.json")["messages"][:2]
    data = np.frombuffer(b"".join(_b(r["msg"]) for r in rows) + b"\0", dtype=np.uint8)
    offs = np.array([1, 1, 1], dtype=np.uint64)
    out = np.zeros(2 * sb, dtype=np.uint8)
    rc = lib.cc_hash_to_curve(ctx.h, 2 if sb == 192 else 1, 2, ctypes.c_void_p(data.ctypes.data),
                              ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    assert rc == CoconutErrorKind.Decode.value
    for group, key in ((1, "g1"), (2, "g2")):
        assert [p.hex() for p in hash_to_curve(ctx, group, [_b(r["msg"]) for r in rows])] == [r[key] for r in rows]
    # cc_blind_sign_batch: k > q is CC_ERR_LEN (hidden + known == y.len() in the reference)
    r = case["requests"][0]
    with pytest.raises(CoconutError) as e:
        blind_sign_batch(ctx, 1, 2, [_b(r["commitment"])], [[]], [[tuple(_b(c) for c in r["ciphertexts"][0])] * 2],
                         _b(case["x"]), [_b(case["y"][0])])
    assert e.value.kind == CoconutErrorKind.UnsupportedNoOfMessages
    _check_blind_sign(ctx, case, case["requests"])


# ---------------------------------------------------------------- verify, aggregation and PoK verify forms
def _cat(hexes):
    return b"".join(_b(h) for h in hexes)


def _bind(ctx, d):
    ctx.set_params(_b(d["g_tilde"]))
    if "vk" in d:
        ctx.set_verkey(_b(d["vk"]["X"]), [_b(y) for y in d["vk"]["Y"]])


def _rows(out, n):
    w = len(out) // n
    return [out[i * w:(i + 1) * w].hex() for i in range(n)]


def _check_gt(gts, rows):
    for i, r in enumerate(rows):
        if r["gt"] is not None:
            assert gts[576 * i:576 * (i + 1)].hex() == r["gt"], (i, r["kind"])


def _verify(ctx, d, cr, **kw):
    from coconut import verify_batch
    vk = (_cat(c["vk"]["X"] for c in cr), _cat(y for c in cr for y in c["vk"]["Y"])) if "vk" in cr[0] else None
    return verify_batch(ctx, len(cr), d["q"], _cat(c["sigma1"] for c in cr), _cat(c["sigma2"] for c in cr),
                        _cat(m for c in cr for m in c["msgs"]), vk=vk, **kw)


# indices into the verify fixtures' credentials, sizes 1, 3, 1: all valid / with a refused one (1: sigma2_plus_g,
# 4: msg_plus_1)
VERIFY_ACCEPT = ((0,), (0, 2, 3), (2,))
VERIFY_MIXED = ((1,), (0, 1, 2), (4,))


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("pervk", [False, True], ids=["shared", "pervk"])
def test_verify_at_growing_batch(ctxs, mode, pervk):
    d = golden(f"verify_{mode.lower()}_q6{'_pervk' if pervk else ''}.json")
    ctx = ctxs[mode]
    _bind(ctx, d)
    for idx in VERIFY_MIXED + VERIFY_ACCEPT[:1]:
        cr = [d["creds"][i] for i in idx]
        assert [c["verdict"] for c in cr] == [int(i not in (1, 4)) for i in idx]
        v, gts = _verify(ctx, d, cr, want_gt=True)
        assert list(v) == [c["verdict"] for c in cr], idx
        _check_gt(gts, cr)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_verify_rlc_accept_and_fallback(ctxs, mode):
    d = golden(f"verify_{mode.lower()}_q6.json")
    ctx = ctxs[mode]
    _bind(ctx, d)
    for idx in VERIFY_ACCEPT + VERIFY_MIXED:  # the whole-batch check accepts / rejects and falls back
        cr = [d["creds"][i] for i in idx]
        assert list(_verify(ctx, d, cr, rlc=True)) == [c["verdict"] for c in cr], idx
    from test_gpu_rlc_fold_direct import rlc_engine_accepts
    for idx in VERIFY_ACCEPT:  # the RLC check itself accepts them (fixed seed, no fallback behind it)
        cr = [d["creds"][i] for i in idx]
        assert rlc_engine_accepts(ctx, len(cr), d["q"], _cat(c["sigma1"] for c in cr), _cat(c["sigma2"] for c in cr),
                                  _cat(m for c in cr for m in c["msgs"])) is True, idx
    # the plain form right behind the RLC's two sequences, on the same staging buffers
    cr = d["creds"][:3]
    v, gts = _verify(ctx, d, cr, want_gt=True)
    assert list(v) == [c["verdict"] for c in cr]
    _check_gt(gts, cr)


AGG_SETS = ((0,), (0, 1, 2), (4,))  # cases of len = t = 3 ids; the last one repeats an id


def _aggregate_all(ctx, d, cs):
    """The three aggregation host forms over the cases cs, against the fixture's outputs."""
    from coconut import signature_aggregate_batch, verkey_aggregate_batch, verkey_aggregate_ids
    n, t, q, ids = len(cs), d["threshold"], d["q"], [c["ids"] for c in cs]
    o1, o2 = signature_aggregate_batch(ctx, n, 3, t, ids, _cat(s for c in cs for s in c["sigma1"]),
                                       _cat(s for c in cs for s in c["sigma2"]))
    assert (_rows(o1, n), _rows(o2, n)) == ([c["out_sigma1"] for c in cs], [c["out_sigma2"] for c in cs])
    want = ([c["out_X"] for c in cs], ["".join(c["out_Y"]) for c in cs])
    oX, oY = verkey_aggregate_batch(ctx, n, 3, t, q, ids, _cat(x for c in cs for x in c["X"]),
                                    _cat(y for c in cs for row in c["Y"] for y in row))
    assert (_rows(oX, n), _rows(oY, n)) == want
    oX, oY = verkey_aggregate_ids(ctx, n, 3, t, ids)
    assert (_rows(oX, n), _rows(oY, n)) == want


def _set_issuers(ctx, d):
    table = {i: (x, ys) for c in d["cases"] for i, x, ys in zip(c["ids"], c["X"], c["Y"])}
    ids = sorted(table)
    ctx.set_issuers(ids, _cat(table[i][0] for i in ids), _cat(y for i in ids for y in table[i][1]), d["q"])


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_aggregation_forms_at_growing_batch(ctxs, mode):
    d = golden(f"aggregate_{mode.lower()}.json")
    assert d["threshold"] == 3
    ctx = ctxs[mode]
    _set_issuers(ctx, d)
    for idx in AGG_SETS:
        cs = [d["cases"][i] for i in idx]
        assert all(len(c["ids"]) == 3 for c in cs)
        _aggregate_all(ctx, d, cs)


def _pok(ctx, d, pr, nresp=None, **kw):
    from coconut import pok_verify_batch
    nr = len(pr[0]["responses"])
    pad = b"\0" * (48 * len(pr) * ((nresp or nr) - nr))  # a wrong response count still gets a buffer of its size
    return pok_verify_batch(ctx, len(pr), d["q"], d["revealed"], nresp or nr, _cat(p["sigma1"] for p in pr),
                            _cat(p["sigma2"] for p in pr), _cat(p["J"] for p in pr), _cat(p["T"] for p in pr),
                            _cat(x for p in pr for x in p["responses"]) + pad, _cat(p["chal"] for p in pr),
                            _cat(m for p in pr for m in p["revealed_msgs"]), **kw)


# indices into the PoK fixtures' proofs: all valid / with a refused one (2: bad_chal, 4: bad_response)
POK_ACCEPT = ((0,), (0, 1, 7), (1,))
POK_MIXED = ((2,), (0, 2, 7), (4,))


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_pok_verify_forms_at_growing_batch(ctxs, mode):
    d = golden(f"pok_{mode.lower()}_q6.json")
    ctx = ctxs[mode]
    _bind(ctx, d)
    for idx in POK_MIXED + POK_ACCEPT:
        pr = [d["proofs"][i] for i in idx]
        assert [p["verdict"] for p in pr] == [int(i not in (2, 4)) for i in idx]
        v, gts = _pok(ctx, d, pr, want_gt=True)
        assert list(v) == [p["verdict"] for p in pr], idx
        _check_gt(gts, pr)
        assert list(_pok(ctx, d, pr, rlc=True)) == [p["verdict"] for p in pr], idx  # accepts / falls back


def _pok_pervk(ctx, b, nresp=None):
    from coconut import pok_verify_batch
    nr = nresp or b["nresp"]
    return pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], nr, b["s1"], b["s2"], b["J"], b["T"],
                            b["resp"] + b"\0" * (48 * b["n"] * (nr - b["nresp"])), b["chal"], b["rev"], want_gt=True,
                            vk=(b["X"], b["Y"]))


@pytest.fixture(scope="module")
def pervk_proofs(oc):
    """Per mode: four proofs under their own verkeys (the last one refused: a response off by 5) and the oracle's
    (verdict, GT) of each."""
    out = {}
    for mode, m in MODES.items():
        b = C.distinct_batch(C.oracle_mul(oc, host_threads()), m, 4, 6, (5, 2), seed=4100 + m)
        assert b["expect"] == [1, 1, 1, 0]
        out[mode] = (b, C.oracle_pok(oc, b, threads=host_threads()))
    return out


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_pok_verify_pervk_at_growing_batch(ctxs, pervk_proofs, mode):
    b, want = pervk_proofs[mode]
    ctx = ctxs[mode]
    ctx.set_params(b["g"])
    for idx in ((0,), (0, 1, 2), (3,)):
        cut = C.take(b, list(idx))
        v, gts = _pok_pervk(ctx, cut)
        assert list(v) == cut["expect"] == [want[i][0] for i in idx], idx
        for k, i in enumerate(idx):
            if want[i][1] is not None:
                assert gts[576 * k:576 * (k + 1)] == want[i][1], i


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_refused_verify_aggregate_and_pok_calls_leave_the_context_usable(ctxs, pervk_proofs, mode):
    """One documented refusal per form, then a correct call of the same form on the same context."""
    from coconut import CoconutError, CoconutErrorKind, signature_aggregate_batch, verkey_aggregate_batch, \
        verkey_aggregate_ids, verify_batch
    ctx = ctxs[mode]

    def refused(kind, f, *a, **kw):
        with pytest.raises(CoconutError) as e:
            f(*a, **kw)
        assert e.value.kind == kind

    # cc_verify_batch, shared verkey, with and without rlc: q != the verkey's q is CC_ERR_LEN
    d = golden(f"verify_{mode.lower()}_q6.json")
    _bind(ctx, d)
    cr = d["creds"][:3]
    for rlc in (False, True):
        refused(CoconutErrorKind.UnsupportedNoOfMessages, verify_batch, ctx, 3, 5, _cat(c["sigma1"] for c in cr),
                _cat(c["sigma2"] for c in cr), _cat(m for c in cr for m in c["msgs"][:5]), rlc=rlc)
        assert list(_verify(ctx, d, cr, rlc=rlc)) == [c["verdict"] for c in cr]
    # the aggregation forms: len < t is CC_ERR_THRESHOLD
    d = golden(f"aggregate_{mode.lower()}.json")
    _set_issuers(ctx, d)
    c = d["cases"][0]
    two = lambda k: _cat(c[k][:2])  # noqa: E731
    refused(CoconutErrorKind.Threshold, signature_aggregate_batch, ctx, 1, 2, 3, [c["ids"][:2]], two("sigma1"),
            two("sigma2"))
    refused(CoconutErrorKind.Threshold, verkey_aggregate_batch, ctx, 1, 2, 3, d["q"], [c["ids"][:2]], two("X"),
            _cat(y for row in c["Y"][:2] for y in row))
    refused(CoconutErrorKind.Threshold, verkey_aggregate_ids, ctx, 1, 2, 3, [c["ids"][:2]])
    _aggregate_all(ctx, d, [c])
    # the PoK forms: nresp != q - r + 1 is CC_ERR_BASES_EXPS
    d = golden(f"pok_{mode.lower()}_q6.json")
    _bind(ctx, d)
    pr = d["proofs"][:3]
    for rlc in (False, True):
        refused(CoconutErrorKind.UnequalNoOfBasesExponents, _pok, ctx, d, pr, nresp=6, rlc=rlc)
        assert list(_pok(ctx, d, pr, rlc=rlc)) == [p["verdict"] for p in pr]
    b, want = pervk_proofs[mode]
    ctx.set_params(b["g"])
    refused(CoconutErrorKind.UnequalNoOfBasesExponents, _pok_pervk, ctx, b, nresp=6)
    assert list(_pok_pervk(ctx, b)[0]) == b["expect"]
