"""GPU tests of the holder side of issuance (csrc/sigreq_prove.hip): cc_set_request_params,
cc_sigreq_new_batch, cc_sigreq_pok_init_batch, cc_sigreq_pok_gen_proof_batch and their *_device forms,
byte for byte against oracle/issuance.py (signature_request_new / compute_h / sigreq_pok_init /
sigreq_gen_proof), in both group modes.  Small forced tables (8-bit unless a test says otherwise), never
the memory-chosen width.  Inputs and oracle expectations: tests/sigreq_prove_cases.py (the CPU model
check of the same inputs: tests/test_sigreq_prove_abi.py)."""
import ctypes

import pytest

import sigreq_prove_cases as K
from test_gpu_parity import MODES
from test_gpu_reference_flows import Flow, _fr, check_signing_on_random_msgs

pytestmark = pytest.mark.gpu

R = K.R
OK, ERR_LEN, ERR_DECODE, ERR_HIP, ERR_STATE = 0, -1, -4, -5, -7


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _prove(ctx, w, k, rows, bits=8):
    """new + init + gen_proof through the host forms -> dict of byte strings (n rows each)."""
    import coconut
    ctx.set_request_params(w.g_enc, w.h_enc, bits)
    n, q = len(rows), w.q
    a = K.inputs(w, k, rows)
    cm, h, ct, rand_back = coconut.sigreq_new_batch(ctx, n, q, k, a["msgs"], a["pk"], a["rand"])
    assert rand_back == a["rand"]
    init, blind_back = coconut.sigreq_pok_init_batch(ctx, n, q, k, h, a["pk"], a["blind"])
    assert blind_back == a["blind"]
    rec = coconut.sigreq_pok_gen_proof_batch(ctx, n, q, k, a["msgs"], a["rand"], a["blind"], a["sk"], a["chal"], init)
    return dict(a, commitment=cm, h=h, cts=ct, init=init, record=rec)


def _check_bytes(ctx, got, k, rows):
    sb = ctx.mode.sig_bytes
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    for i, r in enumerate(rows):
        w = r["want"]
        assert got["commitment"][i * sb:(i + 1) * sb] == w["commitment"], ("commitment", r["name"])
        assert got["h"][i * sb:(i + 1) * sb] == w["h"], ("h", r["name"])
        assert got["cts"][i * k * 2 * sb:(i + 1) * k * 2 * sb] == w["cts"], ("ciphertexts", r["name"])
        assert got["init"][i * pb:(i + 1) * pb] == w["init"], ("init", r["name"])
        assert got["record"][i * pb:(i + 1) * pb] == w["record"], ("gen_proof", r["name"])


def _verify(ctx, w, k, got, n, record=None):
    import coconut
    sb = ctx.mode.sig_bytes
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    q = w.q
    cut = lambda b, s: [b[i * s:(i + 1) * s] for i in range(n)]  # noqa: E731
    msgs = cut(got["msgs"], q * 48)
    known = [[_fr(int.from_bytes(m[48 * j:48 * j + 48], "big")) for j in range(k, q)] for m in msgs]
    cts = [[(c[2 * j * sb:(2 * j + 1) * sb], c[(2 * j + 1) * sb:(2 * j + 2) * sb]) for j in range(k)]
           for c in cut(got["cts"], k * 2 * sb)]
    chal = [_fr(int.from_bytes(c, "big")) for c in cut(got["chal"], 48)]
    return coconut.sigreq_verify_batch(ctx, q, k, w.g_enc, w.h_enc, cut(got["commitment"], sb), known, cts,
                                       cut(got["pk"], sb), cut(got["record"] if record is None else record, pb), chal)


def _batch(ctx, w, k, rows, bits=8):
    import coconut
    got = _prove(ctx, w, k, rows, bits)
    _check_bytes(ctx, got, k, rows)
    n = len(rows)
    tb = coconut.sigreq_pok_to_bytes_batch(ctx, n, k, w.g_enc, w.h_enc, got["h"], got["pk"], got["init"])
    for i, r in enumerate(rows):
        assert tb[i] == r["want"]["to_bytes"], r["name"]
    v = _verify(ctx, w, k, got, n)
    assert [int(x) for x in v] == [int(r["valid"]) for r in rows], [r["name"] for r in rows]
    return got


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_shapes_against_the_oracle(ctxs, mode):
    """(q, k) = (3, 0), (3, 1), (4, 2), (3, 3), (6, 5): commitment, h, ciphertexts, the proof record after
    init and after gen_proof and to_bytes equal the oracle's for the same draws; the verifier accepts."""
    seen = []
    for _name, w, k, rows in K.expected(mode, "shapes"):
        _batch(ctxs[mode], w, k, rows)
        seen.append((w.q, k))
    assert tuple(seen) == K.SHAPES


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_edges(ctxs, mode):
    """The edge scalars and related bases of sigreq_prove_cases.edge_batches: bytes from the oracle, the
    verifier's verdict as the oracle's."""
    seen = 0
    for _name, w, k, rows in K.expected(mode, "edges"):
        _batch(ctxs[mode], w, k, rows)
        seen += len(rows)
    assert seen == 15


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("bits", [13, 16])
def test_table_widths(ctxs, mode, bits):
    """The edge-scalar batch and the (6, 5) shape over 13-bit (ft_digit's generic path) and 16-bit tables:
    the oracle's bytes again, so the same as over the 8-bit tables of the tests above."""
    ctx = ctxs[mode]
    name, w, k, rows = K.expected(mode, "edges")[0]
    assert name == "edge scalars"
    _batch(ctx, w, k, rows, bits)
    _name, w, k, rows = K.expected(mode, "shapes")[-1]
    _batch(ctx, w, k, rows, bits)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_auto_width_and_rebuild(ctxs, mode):
    """table_bits = 0 on a fresh context picks a width by memory; the bytes do not depend on it."""
    import coconut
    _name, w, k, rows = K.expected(mode, "shapes")[2]
    ctx = coconut.Context(0, coconut.GroupMode(MODES[mode]))
    try:
        _batch(ctx, w, k, rows, 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_block_boundaries(ctxs, mode):
    """n one more than a block of each kernel (64, 128 and 256 requests or tasks a block), and n k one more
    than a block where tasks are per (request, i): k = 3 with n = 43 (n k = 129), 65, 129 and 257; k = 1
    with n = 65, 129 and 257 (n k = n).  The distinct rows repeat, so the oracle computes each once."""
    ctx = ctxs[mode]
    name, w, k, rows = K.expected(mode, "edges")[0]
    assert name == "edge scalars" and k == 3 and len(rows) == 5
    for n in (43, 65, 129, 257):
        many = [rows[(3 * i) % 5] for i in range(n)]  # row n - 1, alone in its block, varies with n
        got = _prove(ctx, w, 3, many)
        _check_bytes(ctx, got, 3, many)
        assert _verify(ctx, w, 3, got, n).all()
    _name, w, k, rows = K.expected(mode, "shapes")[1]
    assert (w.q, k) == (3, 1)
    for n in (65, 129, 257):
        many = [rows[(i // 64 + i) % 2] for i in range(n)]
        got = _prove(ctx, w, 1, many)
        _check_bytes(ctx, got, 1, many)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_known_message_above_r_hashes_as_its_reduced_value(ctxs, mode):
    import coconut
    ctx = ctxs[mode]
    batch = [b for b in K.expected(mode, "edges") if b[0] == "known m>=r"][0]
    _name, w, k, rows = batch
    r = rows[0]
    assert k == 0 and r["msgs"][0] >= R
    ctx.set_request_params(w.g_enc, w.h_enc, 8)
    a = K.inputs(w, k, rows)
    reduced = b"".join(K.fr(m) for m in r["msgs"])
    assert reduced != a["msgs"]
    one = coconut.sigreq_new_batch(ctx, 1, w.q, 0, a["msgs"], b"", a["rand"])
    two = coconut.sigreq_new_batch(ctx, 1, w.q, 0, reduced, b"", a["rand"])
    assert one[:3] == two[:3] and one[1] == r["want"]["h"] and one[2] == b""
    # the same with one hidden message: m_1, m_2 known
    one = coconut.sigreq_new_batch(ctx, 1, w.q, 1, a["msgs"][48:] + a["msgs"][:48], a["pk"], a["rand"] + bytes(48))
    two = coconut.sigreq_new_batch(ctx, 1, w.q, 1, reduced[48:] + reduced[:48], a["pk"], a["rand"] + bytes(48))
    assert one[:3] == two[:3]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_device_forms(ctxs, mode):
    """The *_device forms on a caller stream give the host forms' bytes."""
    import torch
    from coconut._lib import lib
    ctx = ctxs[mode]
    _name, w, k, rows = K.expected(mode, "shapes")[2]  # q = 4, k = 2
    q, n = w.q, len(rows)
    host = _prove(ctx, w, k, rows)
    sb = ctx.mode.sig_bytes
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    dev = torch.device("cuda", 0)
    to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    D = {key: to(host[key]) for key in ("msgs", "pk", "rand", "blind", "sk", "chal")}
    o = [torch.zeros(n * s, dtype=torch.uint8, device=dev) for s in (sb, sb, k * 2 * sb)]
    pr = torch.full((n * pb,), 0xAB, dtype=torch.uint8, device=dev)  # init zeroes the response fields itself
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    sp = ctypes.c_void_p(st.cuda_stream)
    assert lib.cc_sigreq_new_batch_device(ctx.h, n, q, k, P(D["msgs"]), P(D["pk"]), P(D["rand"]), P(o[0]), P(o[1]),
                                          P(o[2]), sp) == OK
    assert lib.cc_sigreq_pok_init_batch_device(ctx.h, n, q, k, P(o[1]), P(D["pk"]), P(D["blind"]), P(pr), sp) == OK
    st.synchronize()
    assert bytes(pr.cpu().numpy()) == host["init"]
    assert lib.cc_sigreq_pok_gen_proof_batch_device(ctx.h, n, q, k, P(D["msgs"]), P(D["rand"]), P(D["blind"]),
                                                    P(D["sk"]), P(D["chal"]), P(pr), sp) == OK
    st.synchronize()
    for key, t in zip(("commitment", "h", "cts", "record"), o + [pr]):
        assert bytes(t.cpu().numpy()) == host[key], key


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_errors(ctxs, mode):
    """Every check of the header's list, in its order and before the n = 0 shortcut."""
    import coconut
    from coconut._lib import lib
    ctx = ctxs[mode]
    _name, w, _k, _rows = K.expected(mode, "shapes")[2]  # q = 4
    ctx.set_request_params(w.g_enc, w.h_enc, 8)
    h, q, N = ctx.h, w.q, None
    one = ctypes.create_string_buffer(8)
    B = ctypes.cast(one, ctypes.c_void_p)

    def new(n, q_, k, p=N, hh=h, ct=0):
        c = p if ct == 0 else ct
        return (lib.cc_sigreq_new_batch(hh, n, q_, k, p, p, p, p, p, c),
                lib.cc_sigreq_new_batch_device(hh, n, q_, k, p, p, p, p, p, c, N))

    def init(n, q_, k, p=N, hh=h):
        return (lib.cc_sigreq_pok_init_batch(hh, n, q_, k, p, p, p, p),
                lib.cc_sigreq_pok_init_batch_device(hh, n, q_, k, p, p, p, p, N))

    def gen(n, q_, k, p=N, hh=h):
        return (lib.cc_sigreq_pok_gen_proof_batch(hh, n, q_, k, p, p, p, p, p, p),
                lib.cc_sigreq_pok_gen_proof_batch_device(hh, n, q_, k, p, p, p, p, p, p, N))

    both = lambda v: (v, v)  # noqa: E731
    for f in (new, init, gen):
        assert f(0, q, 2) == both(OK)                      # n = 0 with NULLs
        assert f(1, q, 2) == both(ERR_DECODE)              # NULL buffers with n > 0
        assert f(0, q, q + 1) == both(ERR_LEN)             # k > q
        assert f((1 << 26) + 1, q, 2, B) == both(ERR_DECODE)  # before anything is read or launched
    assert new(0, q + 1, 2) == both(ERR_LEN) and init(0, q + 1, 2) == both(ERR_LEN)   # q != the params' q
    assert new(1, q + 1, 2, B) == both(ERR_LEN) and init(1, q + 1, 2, B) == both(ERR_LEN)
    assert gen(0, q + 1, 2) == both(OK)                    # gen_proof holds no params to compare with
    assert gen(0, 4097, 2) == both(ERR_DECODE)             # q > CC_MAX_Q
    assert gen(0, 4096, 4097) == both(ERR_LEN)
    bare = coconut.Context(0, coconut.GroupMode(MODES[mode]))  # no request params
    try:
        assert new(0, q, 2, hh=bare.h) == both(ERR_STATE) and init(0, q, 2, hh=bare.h) == both(ERR_STATE)
        assert new(1, q, 2, B, hh=bare.h) == both(ERR_STATE) and init(1, q, 2, B, hh=bare.h) == both(ERR_STATE)
        assert new(1, q, 2, hh=bare.h) == both(ERR_DECODE)  # the NULL check comes first
        assert gen(0, q, 2, hh=bare.h) == both(OK)
        # cc_set_request_params
        g, hv = ctypes.c_char_p(w.g_enc), ctypes.c_char_p(b"".join(w.h_enc))
        assert lib.cc_set_request_params(bare.h, q, N, hv, 8) == ERR_DECODE
        assert lib.cc_set_request_params(bare.h, q, g, N, 8) == ERR_DECODE
        assert lib.cc_set_request_params(bare.h, 0, g, hv, 8) == ERR_DECODE
        assert lib.cc_set_request_params(bare.h, 4097, g, hv, 8) == ERR_DECODE
        for bits in (-1, 1, 7, 17, 22):
            assert lib.cc_set_request_params(bare.h, q, g, hv, bits) == ERR_DECODE
        assert new(0, q, 2, hh=bare.h) == both(ERR_STATE)   # none of those bound anything
        assert lib.cc_set_request_params(bare.h, q, g, hv, 8) == OK
        assert new(0, q, 2, hh=bare.h) == both(OK)
        assert lib.cc_set_request_params(bare.h, q, N, hv, 8) == ERR_DECODE
        assert new(0, q, 2, hh=bare.h) == both(OK)          # a refused call leaves the params in place
    finally:
        bare.close()
    # k = 0: elgamal_pk and the ciphertexts may be NULL
    _n0, w0, k0, rows0 = K.expected(mode, "shapes")[0]
    assert k0 == 0
    ctx.set_request_params(w0.g_enc, w0.h_enc, 8)
    a = K.inputs(w0, 0, rows0[:1])
    sb = ctx.mode.sig_bytes
    cm, hh_ = ctypes.create_string_buffer(sb), ctypes.create_string_buffer(sb)
    assert lib.cc_sigreq_new_batch(h, 1, w0.q, 0, a["msgs"], N, a["rand"], cm, hh_, N) == OK
    assert cm.raw == rows0[0]["want"]["commitment"] and hh_.raw == rows0[0]["want"]["h"]
    pr = ctypes.create_string_buffer(2 * sb + 96)
    assert lib.cc_sigreq_pok_init_batch(h, 1, w0.q, 0, N, N, a["blind"], pr) == OK
    assert pr.raw == rows0[0]["want"]["init"]
    with pytest.raises(coconut.CoconutError):
        coconut.sigreq_new_batch(ctx, 1, w0.q + 1, 0, bytes((w0.q + 1) * 48), b"", bytes(48))


def _chain(ctx, w, k, rows, sk=None):
    """new -> init -> the challenge hashed on the GPU -> gen_proof, every step on the GPU."""
    import coconut
    n, q = len(rows), w.q
    a = K.inputs(w, k, rows)
    cm, h, ct, rand = coconut.sigreq_new_batch(ctx, n, q, k, a["msgs"], a["pk"])
    init, blind = coconut.sigreq_pok_init_batch(ctx, n, q, k, h, a["pk"])
    chal = coconut.sigreq_challenge_batch(ctx, n, k, w.g_enc, w.h_enc, h, a["pk"], init)
    rec = coconut.sigreq_pok_gen_proof_batch(ctx, n, q, k, a["msgs"], rand, blind, a["sk"] if sk is None else sk, chal,
                                             init)
    return dict(a, commitment=cm, h=h, cts=ct, init=init, record=rec, chal=chal)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_chain(ctxs, mode):
    """GPU new -> GPU init -> sigreq_challenge_batch -> GPU gen_proof: cc_sigreq_verify_batch accepts every
    request (fresh randomness from `secrets`); one flipped response byte, or a gen_proof with the wrong
    elgamal_sk, is refused."""
    ctx = ctxs[mode]
    for idx in (1, 4):  # (3, 1) and (6, 5)
        _name, w, k, rows = K.expected(mode, "shapes")[idx]
        ctx.set_request_params(w.g_enc, w.h_enc, 8)
        n = len(rows)
        got = _chain(ctx, w, k, rows)
        assert _verify(ctx, w, k, got, n).all()
        again = _chain(ctx, w, k, rows)
        assert again["commitment"] != got["commitment"] and again["init"] != got["init"]  # fresh draws
        sb = ctx.mode.sig_bytes
        pb = len(got["record"]) // n
        for off in (sb + 47, 2 * sb + 48 + 47, pb - 1):  # r_sk, r_comm[0], the last r_2b of request 0
            bad = bytearray(got["record"])
            bad[off] ^= 1
            v = _verify(ctx, w, k, got, n, bytes(bad))
            assert v[0] == 0 and v[1:].all(), off
        wrong = _chain(ctx, w, k, rows, sk=got["sk"][48:] + got["sk"][:48])  # the keys of the two rows swapped
        assert not _verify(ctx, w, k, wrong, n).any()


class DeviceIssuanceFlow(Flow):
    def blind_signatures(self, msgs, k, signers):
        """Flow.blind_signatures with the holder's side on the GPU: ElGamal keygen by fixed_base_mul,
        SignatureRequest.new, SignatureRequestPoK.init / to_bytes / gen_proof, the challenge by hash_msg,
        then the signers' verify and blind_sign batches and one unblind_batch."""
        co, ctx = self.co, self.ctx
        sg = 3 - self.og
        sk = _fr(self.rng.fr())
        pk = co.fixed_base_mul(ctx, sg, self.params.g, sk)
        req, rnd = co.SignatureRequest.new(msgs, k, pk, self.params, ctx=ctx)
        pok = co.SignatureRequestPoK.init(req, pk, self.params, ctx=ctx)
        chal = co.hash_msg(ctx, [pok.to_bytes()])[0]
        assert chal == co.sigreq_challenge_batch(ctx, 1, k, self.params.g, self.params.h, req.h, pk, pok.proof)
        chal = _fr(int.from_bytes(chal, "big"))
        proof = pok.gen_proof(msgs[:k], rnd, sk, chal)
        t = len(signers)
        v = co.sigreq_verify_batch(ctx, self.q, k, self.params.g, self.params.h, [req.commitment] * t,
                                   [req.known_messages] * t, [req.ciphertexts] * t, [pk] * t, [proof] * t, [chal] * t)
        assert v.all()
        hs, c1s, c2s = [], [], []
        for s in signers:
            h, c1, c2 = co.blind_sign_batch(ctx, self.q, k, [req.commitment], [req.known_messages], [req.ciphertexts],
                                            _fr(s["x"]), [_fr(y) for y in s["y"]])
            assert h[0] == req.h
            hs.append(h[0])
            c1s.append(c1[0])
            c2s.append(c2[0])
        s2s = co.unblind_batch(ctx, c1s, c2s, [sk] * t)
        return [co.Signature(h, s2) for h, s2 in zip(hs, s2s)]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_full_flow_on_the_device(ctxs, mode):
    """check_signing_on_random_msgs (signature.rs:582-638) with two signers (t = 2 of 3, q = 5, 2 hidden)
    and nothing from the oracle but the keys: keygen by fixed_base_mul -> new -> proof -> blind_sign_batch
    per signer -> unblind_batch -> Signature.verify -> aggregate -> verify."""
    f = DeviceIssuanceFlow(ctxs[mode], mode, seed=911, q=5)
    f.ctx.set_request_params(f.params.g, f.params.h, 8)  # SignatureRequest.new keeps these small tables
    _, _, signers = f.sss_keygen(2, 3)
    check_signing_on_random_msgs(f, 2, 5, 2, signers)
