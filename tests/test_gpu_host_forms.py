"""GPU tests of the older host forms' staging (csrc/devbuf.h HostForm, capi.cpp):
cc_subgroup_check, cc_hash_to_curve, cc_hash_msg, cc_fixed_base_mul, cc_blind_sign_batch,
cc_sigreq_verify_batch and cc_vss_verify_batch keep their staging buffers as locals that are freed on
return.  Each is called on ONE context at n = 1, at n = 3 (every buffer is allocated anew and larger) and at
n = 1 again, in both group modes, and every output is compared byte for byte with the oracle's fixtures
(tests/golden/host_forms.json: q = 2, k = 1, t = 2, the smallest shapes with a hidden and a known message;
hash_to_curve.json and subgroup.json as the codec tests use them).  An ownership mistake — a buffer handed out of
compute_h_batch by reference, a moved-from buffer, a buffer freed under a queued copy — shows as wrong
bytes or a fault here.  A refused call (documented error code) must leave the context usable."""
import ctypes

import numpy as np
import pytest

from conftest import golden
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
