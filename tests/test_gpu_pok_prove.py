"""GPU tests of the holder side (csrc/pok_prove.hip): cc_pok_init_batch / cc_pok_gen_proof_batch, their
*_device forms and cc_unblind_batch, byte for byte against oracle/coconut_ref.py (pok_init / pok_to_bytes /
pok_gen_proof) and oracle/issuance.py (unblind), in both group modes.  Small forced tables (8-bit unless
a test says otherwise), never the memory-chosen width.  Inputs and oracle expectations:
tests/pok_prove_cases.py (the CPU model check of the same inputs: tests/test_pok_prove_abi.py)."""
import ctypes

import numpy as np
import pytest

import pok_prove_cases as K
from conftest import golden
from test_gpu_parity import MODES

pytestmark = pytest.mark.gpu

R = K.R
OK, ERR_LEN, ERR_BASES, ERR_DECODE, ERR_STATE = 0, -1, -2, -4, -7


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    for x in c.values():
        x.set_table_bits(8, 0)
    yield c
    for x in c.values():
        x.close()


def _load(ctx, w, bits=8):
    g, X, Y = w.vk_bytes()
    if ctx.table_bits()[0] not in (0, bits):
        ctx.set_table_bits(bits, 0)
    ctx.set_params(g)
    ctx.set_verkey(X, Y)
    assert ctx.table_bits()[0] == bits
    return g, X, Y


def _inputs(rows):
    return (b"".join(c["s1"] for c in rows), b"".join(c["s2"] for c in rows),
            b"".join(K.fr(m) for c in rows for m in c["msgs"]), b"".join(K.be48(v) for c in rows for v in c["rand"]),
            b"".join(K.be48(c["chal"]) for c in rows))


def _prove(ctx, q, rev, rows):
    """init + gen_proof through the host forms -> dict of byte strings (n rows each)."""
    import coconut
    n = len(rows)
    s1, s2, msgs, rand, chal = _inputs(rows)
    o1, o2, J, T, rand_back = coconut.pok_init_batch(ctx, n, q, list(rev), s1, s2, msgs, rand)
    assert rand_back == rand
    resp = coconut.pok_gen_proof_batch(ctx, n, q, list(rev), msgs, rand, chal)
    return dict(s1=o1, s2=o2, J=J, T=T, resp=resp, chal=chal,
                rev=b"".join(K.fr(c["msgs"][i]) for c in rows for i in rev))


def _check_bytes(ctx, got, rows, nresp):
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    for i, c in enumerate(rows):
        name = c.get("name", i)
        w = c["want"]
        assert got["s1"][i * sb:(i + 1) * sb] == w["s1"], ("sigma'_1", name)
        assert got["s2"][i * sb:(i + 1) * sb] == w["s2"], ("sigma'_2", name)
        assert got["J"][i * ob:(i + 1) * ob] == w["J"], ("J", name)
        assert got["T"][i * ob:(i + 1) * ob] == w["T"], ("T", name)
        assert got["resp"][i * nresp * 48:(i + 1) * nresp * 48] == w["resp"], ("responses", name)


def _verify(ctx, q, rev, got, n, resp=None):
    import coconut
    nresp = q - len(rev) + 1
    chal = b"".join(K.fr(int.from_bytes(got["chal"][48 * i:48 * i + 48], "big")) for i in range(n))
    return coconut.pok_verify_batch(ctx, n, q, list(rev), nresp, got["s1"], got["s2"], got["J"], got["T"],
                                    got["resp"] if resp is None else resp, chal, got["rev"])


def _oracle_case(ctx, mode, q, rev, n, bits=8):
    import coconut
    w, rows = K.drbg_batch(mode, q, tuple(rev), n, 11)
    g, X, Y = _load(ctx, w, bits)
    nresp = q - len(rev) + 1
    got = _prove(ctx, q, rev, rows)
    _check_bytes(ctx, got, rows, nresp)
    rows_tb = coconut.pok_to_bytes_batch(ctx, n, q, list(rev), g, Y, got["s1"], got["s2"], got["J"], got["T"])
    for i, c in enumerate(rows):
        assert rows_tb[i] == c["want"]["to_bytes"], i
    assert _verify(ctx, q, rev, got, n).all()
    bad = bytearray(got["resp"])
    bad[(nresp - 1) * 48 + 47] ^= 1  # proof 0's last response
    v = _verify(ctx, q, rev, got, n, bytes(bad))
    assert v[0] == 0 and v[1:].all()


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("shape", ["q6", "q32"])
def test_bytes_against_the_oracle(ctxs, mode, shape):
    """sigma'_1, sigma'_2, J, T, the responses and to_bytes equal the oracle's for the same draws; the
    verifier accepts every proof and rejects one with a changed response."""
    if shape == "q6":
        _oracle_case(ctxs[mode], mode, 6, (3, 5), 6)
    else:
        _oracle_case(ctxs[mode], mode, 32, K.CONFIG5_REVEALED, 3)


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("bits", [10, 16])
def test_table_widths(ctxs, mode, bits):
    """The q = 6 case over 10-bit (ft_digit's generic path) and 16-bit tables."""
    ctx = ctxs[mode]
    try:
        _oracle_case(ctx, mode, 6, (3, 5), 6, bits)
    finally:
        ctx.set_table_bits(8, 0)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_block_and_pair_boundaries(ctxs, mode):
    """n = 1, 2 and B + 1 for the kernels' proofs per block (64 and 128), expected bytes from known
    discrete logs through cc_fixed_base_mul (k_fixed_mul over 8-bit tables: an independent path), as
    bench_modes.make_pok_batch builds its proofs: sigma_1 = k G, sigma_2 = k s G, vk = gk (x, y) G."""
    import coconut
    ctx = ctxs[mode]
    ctx.set_table_bits(8, 0)
    og, sg = (1, 2) if MODES[mode] == 0 else (2, 1)
    gen = {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    q, rev, N = 4, (2,), 129
    hidden = [i for i in range(q) if i not in rev]
    nresp = len(hidden) + 1
    rng = K.C.Drbg("boundaries-" + mode)
    x, gk = rng.fr(), rng.fr()
    y = [rng.fr() for _ in range(q)]
    vk = coconut.fixed_base_mul(ctx, og, gen[og], b"".join(K.fr(v * gk) for v in [x] + y + [1]))
    X, Y, g_tilde = vk[:ob], [vk[ob * (1 + j):ob * (2 + j)] for j in range(q)], vk[ob * (q + 1):]
    ctx.set_params(g_tilde)
    ctx.set_verkey(X, Y)
    e1, e2, w1, w2, wj, wt, msgs, rand, chal, wresp = [], [], [], [], [], [], [], [], [], []
    for _ in range(N):
        m = [rng.fr() for _ in range(q)]
        k, c = rng.fr(), rng.fr()
        rd = [rng.fr() for _ in range(nresp + 2)]
        r1, r2, bl = rd[0], rd[1], rd[2:]
        s = (x + sum(a * b for a, b in zip(y, m))) % R
        secrets = [r2] + [m[i] for i in hidden]
        ylog = [1] + [y[i] for i in hidden]
        e1.append(K.fr(k))
        e2.append(K.fr(k * s))
        w1.append(K.fr(k * r1))
        w2.append(K.fr(r1 * k * (s + r2)))
        wj.append(K.fr(gk * sum(a * b for a, b in zip(ylog, secrets))))
        wt.append(K.fr(gk * sum(a * b for a, b in zip(ylog, bl))))
        wresp.append(b"".join(K.fr(b - c * sc) for b, sc in zip(bl, secrets)))
        msgs.append(b"".join(K.fr(v) for v in m))
        rand.append(b"".join(K.fr(v) for v in rd))
        chal.append(K.fr(c))
    mul = lambda g, sc: coconut.fixed_base_mul(ctx, g, gen[g], b"".join(sc))  # noqa: E731
    S1, S2, W1, W2, WJ, WT = mul(sg, e1), mul(sg, e2), mul(sg, w1), mul(sg, w2), mul(og, wj), mul(og, wt)
    for n in (1, 2, 65, 129):
        o1, o2, J, T, _ = coconut.pok_init_batch(ctx, n, q, list(rev), S1[:n * sb], S2[:n * sb], b"".join(msgs[:n]),
                                                 b"".join(rand[:n]))
        resp = coconut.pok_gen_proof_batch(ctx, n, q, list(rev), b"".join(msgs[:n]), b"".join(rand[:n]),
                                           b"".join(chal[:n]))
        assert o1 == W1[:n * sb] and o2 == W2[:n * sb], n
        assert J == WJ[:n * ob] and T == WT[:n * ob], n
        assert resp == b"".join(wresp[:n]), n
    rv = b"".join(m[48 * i:48 * i + 48] for m in msgs for i in rev)
    v = coconut.pok_verify_batch(ctx, N, q, list(rev), nresp, o1, o2, J, T, resp, b"".join(chal), rv)
    assert v.all()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_edges(ctxs, mode):
    """The edge inputs of pok_prove_cases.edge_batches, one proof each, the cases that share a verkey and
    a revealed set in one batch: bytes from the oracle, the verifier's verdict as the oracle's."""
    ctx = ctxs[mode]
    seen = 0
    for _name, w, rev, cases in K.edge_expected(mode):
        _load(ctx, w)
        nresp = w.q - len(rev) + 1
        got = _prove(ctx, w.q, rev, cases)
        _check_bytes(ctx, got, cases, nresp)
        v = _verify(ctx, w.q, rev, got, len(cases))
        assert [int(x) for x in v] == [int(c["valid"]) for c in cases], [c["name"] for c in cases]
        seen += len(cases)
    assert seen == 16


def test_responses_against_python_integers(ctxs):
    """gen_proof alone (needs neither params nor verkey): q = 1, nothing revealed, so each row has the
    response of r2 (slot 0) and of the hidden message (slot 1); both get the case's (b, chal, secret)."""
    import coconut
    ctx = coconut.Context(0, coconut.GroupMode.SIG_G2)  # a context with nothing set
    try:
        cases = K.response_cases()
        msgs = b"".join(K.be48(s) for _, _, _, s in cases)
        rand = b"".join(K.be48(v) for _, b, _, s in cases for v in (7, s, b, b))
        chal = b"".join(K.be48(c) for _, _, c, _ in cases)
        resp = coconut.pok_gen_proof_batch(ctx, len(cases), 1, [], msgs, rand, chal)
        for i, (name, b, c, s) in enumerate(cases):
            want = K.fr(b - c * s)
            assert resp[96 * i:96 * i + 48] == want, name
            assert resp[96 * i + 48:96 * i + 96] == want, name
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_device_forms(ctxs, mode):
    """The *_device forms on a caller stream give the host forms' bytes; then once more with
    cc_set_concurrency(2) and a verify batch in flight on another stream before them."""
    import torch
    from coconut._lib import lib
    ctx = ctxs[mode]
    q, rev, n = 6, (3, 5), 6
    w, rows = K.drbg_batch(mode, q, rev, n, 11)
    _load(ctx, w)
    nresp = q - len(rev) + 1
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    host = _prove(ctx, q, rev, rows)
    dev = torch.device("cuda", 0)
    to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    s1, s2, msgs, rand, chal = (to(x) for x in _inputs(rows))
    ridx = (ctypes.c_uint64 * len(rev))(*rev)

    def run(st):
        o = [torch.zeros(n * k, dtype=torch.uint8, device=dev) for k in (sb, sb, ob, ob, nresp * 48)]
        st.wait_stream(torch.cuda.current_stream(dev))
        sp = ctypes.c_void_p(st.cuda_stream)
        assert lib.cc_pok_init_batch_device(ctx.h, n, q, len(rev), nresp, P(s1), P(s2), P(msgs), ridx, P(rand), P(o[0]),
                                            P(o[1]), P(o[2]), P(o[3]), sp) == OK
        assert lib.cc_pok_gen_proof_batch_device(ctx.h, n, q, len(rev), nresp, P(msgs), ridx, P(rand), P(chal), P(o[4]),
                                                 sp) == OK
        return o

    def same(o):
        for k, t in zip(("s1", "s2", "J", "T", "resp"), o):
            assert bytes(t.cpu().numpy()) == host[k], k

    st = torch.cuda.Stream(dev)
    o = run(st)
    st.synchronize()
    same(o)
    ctx.set_concurrency(2)
    try:
        other = torch.cuda.Stream(dev)
        D = {k: to(host[k]) for k in ("s1", "s2", "J", "T", "resp", "rev")}
        D["chal"] = to(b"".join(K.fr(c["chal"]) for c in rows))
        v = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert lib.cc_pok_verify_batch_device(ctx.h, n, q, len(rev), nresp, P(D["s1"]), P(D["s2"]), P(D["J"]), P(D["T"]),
                                              P(D["resp"]), P(D["chal"]), ridx, P(D["rev"]), P(v), None,
                                              ctypes.c_void_p(other.cuda_stream)) == OK
        o = run(st)
        torch.cuda.synchronize()
        same(o)
        assert v.cpu().numpy().all()
    finally:
        ctx.set_concurrency(1)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_errors(ctxs, mode):
    """The checks of cc_pok_verify_batch_device, in its order and before the n = 0 shortcut."""
    import coconut
    from coconut._lib import lib
    ctx = ctxs[mode]
    w, _rows = K.drbg_batch(mode, 6, (3, 5), 6, 11)
    _load(ctx, w)
    h, q, N = ctx.h, 6, None
    one = ctypes.create_string_buffer(8)
    B = ctypes.cast(one, ctypes.c_void_p)
    idx = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731

    def init(n, q_, r, nresp, ix, p=N, hh=h):
        return (lib.cc_pok_init_batch(hh, n, q_, r, nresp, p, p, p, ix, p, p, p, p, p),
                lib.cc_pok_init_batch_device(hh, n, q_, r, nresp, p, p, p, ix, p, p, p, p, p, N))

    def gen(n, q_, r, nresp, ix, p=N, hh=h):
        return (lib.cc_pok_gen_proof_batch(hh, n, q_, r, nresp, p, ix, p, p, p),
                lib.cc_pok_gen_proof_batch_device(hh, n, q_, r, nresp, p, ix, p, p, p, N))

    two = idx(3, 5)
    assert init(0, q, 2, 5, two) == (OK, OK) and gen(0, q, 2, 5, two) == (OK, OK)  # n = 0 with NULLs
    assert init(0, q, 0, 7, N) == (OK, OK) and gen(0, q, 0, 7, N) == (OK, OK)
    assert init(0, q + 1, 2, 6, two) == (ERR_LEN, ERR_LEN)            # wrong q (UnsupportedNoOfMessages)
    assert gen(0, q + 1, 2, 6, two) == (OK, OK)                        # gen_proof holds no verkey to compare with
    assert init(0, q, 2, 6, two) == (ERR_BASES, ERR_BASES) and gen(0, q, 2, 6, two) == (ERR_BASES, ERR_BASES)
    assert init(0, q, 2, 5, idx(3, 6)) == (ERR_LEN, ERR_LEN) and gen(0, q, 2, 5, idx(3, 6)) == (ERR_LEN, ERR_LEN)
    assert init(0, q, 2, 5, idx(3, 3)) == (ERR_DECODE, ERR_DECODE)    # repeated index
    assert gen(0, q, 2, 5, idx(3, 3)) == (ERR_DECODE, ERR_DECODE)
    assert init(0, q, 2, 5, N) == (ERR_DECODE, ERR_DECODE)            # r > 0 without indices
    assert init(1, q, 2, 5, two) == (ERR_DECODE, ERR_DECODE)          # NULL buffers with n > 0
    assert gen(1, q, 2, 5, two) == (ERR_DECODE, ERR_DECODE)
    big = (1 << 26) + 1
    assert init(big, q, 2, 5, two, B) == (ERR_DECODE, ERR_DECODE)     # before anything is read or launched
    assert gen(big, q, 2, 5, two, B) == (ERR_DECODE, ERR_DECODE)
    assert lib.cc_unblind_batch(h, big, B, B, B, B) == ERR_DECODE
    assert lib.cc_unblind_batch(h, 0, N, N, N, N) == OK
    assert lib.cc_unblind_batch(h, 1, N, B, B, B) == ERR_DECODE
    bare = coconut.Context(0, coconut.GroupMode(MODES[mode]))  # no params, no verkey
    try:
        assert init(0, q, 2, 5, two, hh=bare.h) == (ERR_STATE, ERR_STATE)
        assert init(1, q, 2, 5, two, B, hh=bare.h) == (ERR_STATE, ERR_STATE)
        assert gen(0, q, 2, 5, two, hh=bare.h) == (OK, OK)
        assert lib.cc_unblind_batch(bare.h, 0, N, N, N, N) == OK
    finally:
        bare.close()
    with pytest.raises(coconut.CoconutError):
        coconut.pok_init_batch(ctx, 1, q, [3, 3], bytes(ctx.mode.sig_bytes), bytes(ctx.mode.sig_bytes), bytes(q * 48),
                               bytes(7 * 48))


@pytest.mark.parametrize("name", ["issuance_g1.json", "issuance_g2.json"])
def test_unblind(ctxs, name):
    """Every request of the issuance fixtures (k = 2, k = 0 where c1 is the identity, k = 3):
    unblind_batch(c1, c2, elgamal_sk) is the file's sigma2; then sk = 0, sk = r - 1 and c2 = sk c1 (the
    identity) against the oracle's unblind."""
    import coconut
    from oracle import issuance as I
    d = golden(name)
    for case in d["cases"]:
        mode = case["mode"]
        ctx = ctxs[mode]
        rq = case["requests"]
        hx = bytes.fromhex
        if case["k"] == 0:
            ident = K.C.Groups(mode).sig_to_bytes(None)
            assert all(hx(r["c1"]) == ident for r in rq)
        got = coconut.unblind_batch(ctx, [hx(r["c1"]) for r in rq], [hx(r["c2"]) for r in rq],
                                    [hx(r["elgamal_sk"]) for r in rq])
        assert [g.hex() for g in got] == [r["sigma2"] for r in rq], (mode, case["k"])
    grp = K.C.Groups(mode)
    rng = K.C.Drbg("unblind-" + mode)
    c1, c2 = grp.sig.mul(grp.sig.gen, rng.fr()), grp.sig.mul(grp.sig.gen, rng.fr())
    sk = rng.fr()
    rows = [(c1, c2, 0), (c1, c2, R - 1), (c1, grp.sig.mul(c1, sk), sk), (None, c2, sk), (c1, c2, sk)]
    se = grp.sig_to_bytes
    got = coconut.unblind_batch(ctx, [se(a) for a, _, _ in rows], [se(b) for _, b, _ in rows],
                                [K.fr(k) for _, _, k in rows])
    want = [se(I.unblind(grp, (None, a, b), k)[1]) for a, b, k in rows]
    assert got == want
    assert got[0] == se(c2) and got[2] == se(None) and got[3] == se(c2)
    # a key handed over as r + sk in 48 bytes is reduced
    assert coconut.unblind_batch(ctx, [se(c1)], [se(c2)], [K.be48(R + sk)]) == [want[4]]
