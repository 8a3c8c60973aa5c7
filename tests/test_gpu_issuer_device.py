"""GPU tests of the issuer's device forms (csrc/issue_dev.hip, capi_issuer.cpp): cc_sigreq_verify_batch_device and
cc_blind_sign_batch_device against the host forms they mirror, the C oracle and the intended verdicts, in
both group modes, on caller streams.  Inputs: tests/issuer_edges.py (every call of the host form's edge
suite) and tests/issuer_device_cases.py (the exceptional steps of the device form's own window schedule;
tests/test_issuer_device_model.py asserts their branch coverage on the CPU).  8-bit request tables unless a
test says otherwise."""
import ctypes
import random

import pytest

import issuer_device_cases as D
import issuer_edges as E
from fixed_edges import R, be48

pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
OK, ERR_LEN, ERR_DECODE, ERR_STATE = 0, -1, -4, -7
SPECIAL = ["g_identity", "g_off_curve", "g_bad_prefix", "h1_identity", "h1_off_curve", "h1_bad_prefix", "h1_eq_h0",
           "h1_eq_neg_h0", "h0_eq_g"]


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


def _env(oc, mode):
    return E.Env(oc, 2 if mode == "G2" else 1)


def _call_names(mode):  # (a G2 encoding has no prefix byte: SigG1 alone has the bad-prefix calls)
    return [f"q{q}k{k}" for q, k in E.SHAPES] + [s for s in SPECIAL if mode == "G1" or "bad_prefix" not in s]


def _to(b):
    import torch
    return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8)[:len(b)].to(torch.device("cuda", 0))


def _dev_args(call, reqs):
    """The request tensors of the device forms: commitment, known, ciphertexts, ElGamal keys, proofs, challenges."""
    _q, _k, _g, _h, cm, kn, cts, pks, proofs, chals = E.call_args(call, reqs)
    return [_to(b"".join(cm)), _to(b"".join(m for row in kn for m in row)),
            _to(b"".join(a + b for row in cts for a, b in row)), _to(b"".join(pks)), _to(b"".join(proofs)),
            _to(b"".join(chals))]


def _verify_dev(ctx, stream, call, reqs, want_h=False):
    import coconut
    import torch
    args = _dev_args(call, reqs)
    stream.wait_stream(torch.cuda.current_stream())  # the uploads
    out = coconut.sigreq_verify_batch_device(ctx, len(reqs), call["q"], call["k"], *args, want_h=want_h, stream=stream)
    stream.synchronize()
    if want_h:
        return [int(x) for x in out[0].cpu()], bytes(out[1].cpu().numpy())
    return [int(x) for x in out.cpu()]


def _parity(oc, ctx, stream, mode, call, bits=8, host=True):
    """Device verdicts == the C oracle's == the intended ones == the host form's, for the whole list, the list
    in a second order and every sub-batch of the call."""
    from coconut import sigreq_verify_batch
    env = _env(oc, mode)
    reqs = call["reqs"]
    want = [E.expect_request(env, call, r) for r in reqs]
    assert want == [r["intent"] for r in reqs]
    ctx.set_request_params(call["g"], call["hvec"], bits)
    got = _verify_dev(ctx, stream, call, reqs)
    assert got == want, [(r["name"], g, w) for r, g, w in zip(reqs, got, want) if g != w]
    if host:
        assert list(sigreq_verify_batch(ctx, *E.call_args(call, reqs))) == want
    perm = E.permutation(len(reqs))
    got = _verify_dev(ctx, stream, call, [reqs[i] for i in perm])
    assert got == [want[i] for i in perm], [(reqs[i]["name"], g) for i, g in zip(perm, got) if g != want[i]]
    for n in call["slices"]:
        got = _verify_dev(ctx, stream, call, reqs[:n])
        assert got == want[:n], (n, [(r["name"], g) for r, g, w in zip(reqs, got, want) if g != w])


@pytest.mark.parametrize("mode,name", [(m, n) for m in ("G2", "G1") for n in _call_names(m)])
def test_verdict_parity_at_the_edges(oc, ctxs, stream, mode, name):
    calls = {c["name"]: c for c in E.sigreq_calls(oc, mode)}
    assert set(calls) == set(_call_names(mode))
    _parity(oc, ctxs[mode], stream, mode, calls[name])


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("bits", [8, 13, 16])
def test_table_widths(oc, ctxs, stream, mode, bits):
    call = next(c for c in E.sigreq_calls(oc, mode) if c["name"] == "q6k2")
    _parity(oc, ctxs[mode], stream, mode, dict(call, slices=()), bits, host=False)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_the_device_forms_own_exceptional_steps(oc, ctxs, stream, mode):
    """issuer_device_cases: recoding edges, related variable bases, F = +-S1, identity T, small-order points."""
    _parity(oc, ctxs[mode], stream, mode, D.device_call(oc, mode))


def _sign_inputs(env, q, k, n, rng, rows=None):
    """n requests for blind signing: commitments and known messages (rows: E.compute_h_inputs first), ciphertext
    halves with identity and off-curve ones among them."""
    rows = list(rows or [])
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    while len(rows) < n:
        rows.append((f"rand{len(rows)}", env.rand_pt(rng), [fr() for _ in range(q - k)]))
    rows = rows[:n]
    forms = [f for _, f in env.identity_forms(rng)]
    cts = []
    for i in range(n):
        row = [[env.rand_pt(rng), env.rand_pt(rng)] for _ in range(k)]
        if k and i % 3 == 1:
            row[i % k][i % 2] = forms[i % len(forms)]
        cts.append([tuple(p) for p in row])
    return rows, cts


def _sign_dev(ctx, stream, q, k, rows, cts, x, y, h=None):
    import coconut
    import torch
    cm = _to(b"".join(c for _, c, _ in rows))
    kn = _to(b"".join(be48(m) for _, _, ms in rows for m in ms))
    ct = _to(b"".join(a + b for row in cts for a, b in row))
    stream.wait_stream(torch.cuda.current_stream())
    out = coconut.blind_sign_batch_device(ctx, len(rows), q, k, cm, kn, ct, be48(x), [be48(v) for v in y], h=h,
                                          stream=stream)
    stream.synchronize()
    return [bytes(o.cpu().numpy()) for o in out]


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("q,k", [(3, 0), (3, 3), (6, 2), (18, 17)])
def test_sign_parity(oc, ctxs, stream, mode, q, k):
    """The host form's bytes at n = 1 and n = 65, with h hashed by the call and with the h the verify wrote; x = 0
    and some y_i = 0 in the second key."""
    from coconut import blind_sign_batch
    env, ctx = _env(oc, mode), ctxs[mode]
    rng = random.Random(600 + 10 * q + k + MODES[mode])
    g, hvec = E._params(env, q, 610 + q + MODES[mode])
    ctx.set_request_params(g, hvec, 8)
    sb = env.sb
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    keys = [(rng.randrange(R), [rng.randrange(R) for _ in range(q)]),
            (0, [0 if j % 2 == 0 else rng.randrange(R) for j in range(q)])]
    for n in (1, 65):
        rows, cts = _sign_inputs(env, q, k, n, rng, E.compute_h_inputs(env, q, k, rng) if (q, k) == (6, 2) else None)
        # any proof bytes will do for the verify that supplies h: h does not depend on them
        import torch
        args = [_to(b"".join(c for _, c, _ in rows)), _to(b"".join(be48(m) for _, _, ms in rows for m in ms)),
                _to(b"".join(a + b for row in cts for a, b in row)), _to(b"".join(env.rand_pt(rng) for _ in range(n))),
                _to(bytes(n * pb)), _to(bytes(n * 48))]
        import coconut
        stream.wait_stream(torch.cuda.current_stream())
        _v, hdev = coconut.sigreq_verify_batch_device(ctx, n, q, k, *args, want_h=True, stream=stream)
        stream.synchronize()
        for x, y in keys:
            want = blind_sign_batch(ctx, q, k, [c for _, c, _ in rows], [[be48(m) for m in ms] for _, _, ms in rows], cts,
                                    be48(x), [be48(v) for v in y])
            want = [b"".join(w) for w in want]
            assert bytes(hdev.cpu().numpy()) == want[0], (n, "the verify's h")
            assert _sign_dev(ctx, stream, q, k, rows, cts, x, y) == want, (n, "h hashed by the call")
            assert _sign_dev(ctx, stream, q, k, rows, cts, x, y, h=hdev) == want, (n, "h from the verify")


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_out_h(oc, ctxs, stream, mode):
    """d_out_h is blind_sign_batch's h on compute_h's edge rows (off-curve, identity, >= p commitments, known
    messages >= r), for accepted and rejected requests alike."""
    from coconut import blind_sign_batch
    env, ctx = _env(oc, mode), ctxs[mode]
    call = next(c for c in E.sigreq_calls(oc, mode) if c["name"] == "q6k2")
    ctx.set_request_params(call["g"], call["hvec"], 8)
    reqs = call["reqs"]
    want_v = [r["intent"] for r in reqs]
    assert 0 in want_v and 1 in want_v
    got_v, h = _verify_dev(ctx, stream, call, reqs, want_h=True)
    assert got_v == want_v
    q, k = call["q"], call["k"]
    x, y = be48(5), [be48(7 + j) for j in range(q)]
    _q, _k, _g, _h, cm, kn, cts, _pk, _pr, _ch = E.call_args(call, reqs)
    hs, _c1, _c2 = blind_sign_batch(ctx, q, k, cm, kn, cts, x, y)
    assert h == b"".join(hs)
    assert h == b"".join(r["h"] for r in reqs)  # the oracle's compute_h of the decoded inputs
    # compute_h's edge rows under proofs that are all refused (zero records)
    rng = random.Random(71 + MODES[mode])
    rows = E.compute_h_inputs(env, q, k, rng)
    n, sb = len(rows), env.sb
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    cts = [[(env.rand_pt(rng), env.rand_pt(rng)) for _ in range(k)] for _ in rows]
    import coconut
    import torch
    args = [_to(b"".join(c for _, c, _ in rows)), _to(b"".join(be48(m) for _, _, ms in rows for m in ms)),
            _to(b"".join(a + b for row in cts for a, b in row)), _to(b"".join(env.rand_pt(rng) for _ in rows)),
            _to(bytes([1]) * (n * pb)), _to(bytes([2]) * (n * 48))]
    stream.wait_stream(torch.cuda.current_stream())
    v, h = coconut.sigreq_verify_batch_device(ctx, n, q, k, *args, want_h=True, stream=stream)
    stream.synchronize()
    assert not v.cpu().any()
    hs, _c1, _c2 = blind_sign_batch(ctx, q, k, [c for _, c, _ in rows], [[be48(m) for m in ms] for _, _, ms in rows],
                                    cts, x, y)
    assert bytes(h.cpu().numpy()) == b"".join(hs)


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("corrupt", [False, True])
def test_whole_flow_resident(oc, ctxs, stream, mode, corrupt):
    """new -> init -> challenge -> gen_proof -> device verify -> device sign with the verify's h -> unblind_batch
    -> verify_batch accepts; q = 6, k = 3, n = 65.  corrupt: one response byte of request 32 flipped; its verdict
    is 0, its neighbours' 1."""
    import coconut
    import torch
    ctx = ctxs[mode]
    sg = 2 if mode == "G2" else 1
    env, oth = E.Env(oc, sg), E.Env(oc, 3 - sg)
    rng = random.Random(900 + MODES[mode])
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    q, k, n = 6, 3, 65
    sb = ctx.mode.sig_bytes
    g, hvec = E._params(env, q, 901 + MODES[mode])
    g_tilde = oth.rand_pt(rng)
    x, y = fr(), [fr() for _ in range(q)]
    ctx.set_request_params(g, hvec, 8)
    sks = [fr() for _ in range(n)]
    msgs = b"".join(be48(fr()) for _ in range(n * q))
    skb = b"".join(be48(s) for s in sks)
    pk = coconut.fixed_base_mul(ctx, sg, g, skb)
    cm, h, ct, rand = coconut.sigreq_new_batch(ctx, n, q, k, msgs, pk)
    init, blind = coconut.sigreq_pok_init_batch(ctx, n, q, k, h, pk)
    chal = coconut.sigreq_challenge_batch(ctx, n, k, g, hvec, h, pk, init)
    rec = coconut.sigreq_pok_gen_proof_batch(ctx, n, q, k, msgs, rand, blind, skb, chal, init)
    pb = len(rec) // n
    if corrupt:
        bad = bytearray(rec)
        bad[32 * pb + sb + 47] ^= 1  # r_sk of request 32
        rec = bytes(bad)
    known = b"".join(msgs[(i * q + k) * 48:(i + 1) * q * 48] for i in range(n))
    d = [_to(v) for v in (cm, known, ct, pk, rec, chal)]
    stream.wait_stream(torch.cuda.current_stream())
    v, hd = coconut.sigreq_verify_batch_device(ctx, n, q, k, *d, want_h=True, stream=stream)
    ho, c1, c2 = coconut.blind_sign_batch_device(ctx, n, q, k, None, d[1], d[2], be48(x), [be48(t) for t in y], h=hd,
                                                 stream=stream)
    stream.synchronize()
    v = [int(t) for t in v.cpu()]
    assert v == [0 if corrupt and i == 32 else 1 for i in range(n)]
    assert bytes(hd.cpu().numpy()) == h == bytes(ho.cpu().numpy())
    cut = lambda t: [bytes(t.cpu().numpy())[i * sb:(i + 1) * sb] for i in range(n)]  # noqa: E731
    s2 = coconut.unblind_batch(ctx, cut(c1), cut(c2), [be48(s) for s in sks])
    ctx.set_params(g_tilde)
    ctx.set_verkey(oth.msm([g_tilde], [x]), [oth.msm([g_tilde], [t]) for t in y])
    ok = coconut.verify_batch(ctx, n, q, h, b"".join(s2), msgs)
    assert [int(t) for t in ok] == [1] * n


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_argument_checks(oc, ctxs, mode):
    """The header's checks in its order, before the n = 0 shortcut."""
    import coconut
    from coconut._lib import lib
    env, ctx = _env(oc, mode), ctxs[mode]
    q = 4
    g, hvec = E._params(env, q, 991)
    ctx.set_request_params(g, hvec, 8)
    N = None
    one = ctypes.create_string_buffer(64 * (q + 1))
    B = ctypes.cast(one, ctypes.c_void_p)

    def ver(n, q_, k, p=N, hh=ctx.h, known=0, cts=0, out_h=N):
        return lib.cc_sigreq_verify_batch_device(hh, n, q_, k, p, p if known == 0 else known, p if cts == 0 else cts, p,
                                                 p, p, p, out_h, N)

    def sign(n, q_, k, p=N, hh=ctx.h, x=B, y=B, cm=0, h=N):
        return lib.cc_blind_sign_batch_device(hh, n, q_, k, p if cm == 0 else cm, p, p, h, x, y, p, p, p, N)

    for f in (ver, sign):
        assert f(0, q, 2) == OK                            # n = 0 with NULLs
        assert f(1, q, 2) == ERR_DECODE                    # NULL buffers with n > 0
        assert f(0, q, q + 1) == ERR_LEN                   # k > q
        assert f((1 << 26) + 1, q, 2, B) == ERR_DECODE     # before anything is read or launched
        assert f(0, q, 2, hh=N) == ERR_DECODE and f(1, q, 2, B, hh=N) == ERR_DECODE
    assert ver(0, q + 1, 2) == ERR_LEN and ver(1, q + 1, 2, B) == ERR_LEN   # q != the params' q
    assert sign(0, q + 1, 2) == OK                         # signing holds no params to compare with
    assert sign(0, 4097, 2) == ERR_DECODE                  # q > CC_MAX_Q
    assert sign(0, 4096, 4097) == ERR_LEN
    assert sign(0, q, 2, x=N) == ERR_DECODE and sign(0, q, 2, y=N) == ERR_DECODE
    assert sign(0, 0, 0, y=N) == OK
    bare = coconut.Context(0, coconut.GroupMode(MODES[mode]))  # no request params
    try:
        assert ver(0, q, 2, hh=bare.h) == ERR_STATE and ver(1, q, 2, B, hh=bare.h) == ERR_STATE
        assert ver(1, q, 2, hh=bare.h) == ERR_DECODE       # the NULL check comes first
        assert sign(0, q, 2, hh=bare.h) == OK              # signing needs no request params
    finally:
        bare.close()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_optional_buffers_and_n_zero(oc, ctxs, stream, mode):
    """k = 0: the ciphertexts may be NULL; q = k: known may be NULL; with h given the commitments may be NULL;
    n = 0 returns empty tensors."""
    import coconut
    import torch
    env, ctx = _env(oc, mode), ctxs[mode]
    for name in ("q3k0", "q3k3"):
        call = next(c for c in E.sigreq_calls(oc, mode) if c["name"] == name)
        ctx.set_request_params(call["g"], call["hvec"], 8)
        reqs = call["reqs"][:5]
        a = _dev_args(call, reqs)
        if call["k"] == 0:
            a[2] = None
        else:
            a[1] = None
        stream.wait_stream(torch.cuda.current_stream())
        v, h = coconut.sigreq_verify_batch_device(ctx, 5, call["q"], call["k"], *a, want_h=True, stream=stream)
        outs = coconut.blind_sign_batch_device(ctx, 5, call["q"], call["k"], None, a[1], a[2], be48(3),
                                               [be48(9)] * call["q"], h=h, stream=stream)
        stream.synchronize()
        assert [int(t) for t in v.cpu()] == [r["intent"] for r in reqs]
        _q, _k, _g, _h, cm, kn, cts, _pk, _pr, _ch = E.call_args(call, reqs)
        want = coconut.blind_sign_batch(ctx, call["q"], call["k"], cm, kn, cts, be48(3), [be48(9)] * call["q"])
        assert [bytes(o.cpu().numpy()) for o in outs] == [b"".join(w) for w in want]
    e = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert coconut.sigreq_verify_batch_device(ctx, 0, 3, 3, e, e, e, e, e, e).numel() == 0
    assert all(o.numel() == 0 for o in coconut.blind_sign_batch_device(ctx, 0, 3, 3, e, e, e, be48(1), [be48(1)] * 3))
