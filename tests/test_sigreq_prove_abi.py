"""CPU tests of the holder-side issuance entry points' boundary (cc_set_request_params, cc_sigreq_new_batch,
cc_sigreq_pok_init_batch, cc_sigreq_pok_gen_proof_batch and their *_device forms): the header declares
them, the library exports them, a NULL context is refused without touching a GPU, the Python wrappers
refuse a short buffer before calling C, the Rust shim calls them behind its length asserts — and the
oracle alone accepts what the inputs of test_gpu_sigreq_prove.py produce (signature_request_new ->
sigreq_pok_init -> sigreq_gen_proof -> sigreq_proof_verify, then blind_sign -> unblind -> verify), so
those inputs are valid expectations before the GPU sees them."""
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
RS = os.path.join(ROOT, "integration", "rust", "src")
NAMES = ("cc_set_request_params", "cc_sigreq_new_batch", "cc_sigreq_new_batch_device", "cc_sigreq_pok_init_batch",
         "cc_sigreq_pok_init_batch_device", "cc_sigreq_pok_gen_proof_batch", "cc_sigreq_pok_gen_proof_batch_device")


def test_header_declares_the_seven_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bcc_status\s+%s\s*\(" % name, src), name


def test_library_exports_the_seven_entry_points():
    from coconut._lib import lib
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name  # declared in coconut/_lib.py


@pytest.mark.parametrize("n", [1, 0])
def test_null_context_is_a_decode_error_without_gpu(n):
    from coconut._lib import lib
    N = None
    assert lib.cc_set_request_params(N, 3, N, N, 0) == -4
    assert lib.cc_sigreq_new_batch(N, n, 3, 2, N, N, N, N, N, N) == -4
    assert lib.cc_sigreq_new_batch_device(N, n, 3, 2, N, N, N, N, N, N, N) == -4
    assert lib.cc_sigreq_pok_init_batch(N, n, 3, 2, N, N, N, N) == -4
    assert lib.cc_sigreq_pok_init_batch_device(N, n, 3, 2, N, N, N, N, N) == -4
    assert lib.cc_sigreq_pok_gen_proof_batch(N, n, 3, 2, N, N, N, N, N, N) == -4
    assert lib.cc_sigreq_pok_gen_proof_batch_device(N, n, 3, 2, N, N, N, N, N, N, N) == -4


def test_python_names_are_exported():
    import coconut
    for name in ("SignatureRequest", "SignatureRequestPoK", "sigreq_new_batch", "sigreq_pok_init_batch",
                 "sigreq_pok_gen_proof_batch", "sigreq_pok_to_bytes_batch", "sigreq_challenge_batch"):
        assert hasattr(coconut, name), name
    assert "new" in dir(coconut.SignatureRequest)
    assert {"init", "to_bytes", "gen_proof"} <= set(dir(coconut.SignatureRequestPoK))
    assert "set_request_params" in dir(coconut.Context)


class _Ctx:
    """Enough of a Context for the wrappers' length checks, which run before any C call (h = None would
    be refused by the library as a NULL context anyway)."""
    h = None

    def __init__(self, mode):
        import coconut
        self.mode = coconut.GroupMode(mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_python_wrappers_refuse_a_short_buffer_before_calling_c(mode):
    import coconut
    from coconut import CoconutError
    ctx = _Ctx(mode)
    sb = ctx.mode.sig_bytes
    n, q, k = 2, 3, 2
    pb = 2 * sb + 48 * (k + 2) + k * (2 * sb + 144)
    assert coconut.sigreq_proof_bytes(ctx, k) == pb
    good = dict(msgs=bytes(n * q * 48), pk=bytes(n * sb), rand=bytes(n * (k + 1) * 48))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.sigreq_new_batch(ctx, n, q, k, a["msgs"], a["pk"], a["rand"])
    good = dict(h=bytes(n * sb), pk=bytes(n * sb), blind=bytes(n * (3 * k + 2) * 48))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.sigreq_pok_init_batch(ctx, n, q, k, a["h"], a["pk"], a["blind"])
    good = dict(msgs=bytes(n * q * 48), rand=bytes(n * (k + 1) * 48), blind=bytes(n * (3 * k + 2) * 48),
                sk=bytes(n * 48), chal=bytes(n * 48), proofs=bytes(n * pb))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.sigreq_pok_gen_proof_batch(ctx, n, q, k, a["msgs"], a["rand"], a["blind"], a["sk"], a["chal"],
                                               a["proofs"])
    good = dict(g=bytes(sb), hs=bytes(n * sb), pk=bytes(n * sb), proofs=bytes(n * pb))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.sigreq_pok_to_bytes_batch(ctx, n, k, a["g"], [bytes(sb)] * q, a["hs"], a["pk"], a["proofs"])
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.sigreq_pok_to_bytes_batch(ctx, n, k, bytes(sb), [bytes(sb), bytes(sb - 1)], bytes(n * sb), bytes(n * sb),
                                          bytes(n * pb))
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.Context.set_request_params(ctx, bytes(sb - 1), [bytes(sb)] * q)
    # to_bytes lays a request's row out as g | T_sk | h_0 .. | g | T_comm | k x (g | T_1 | pk | h | T_2)
    rows = coconut.sigreq_pok_to_bytes_batch(ctx, n, k, b"g" * sb, [b"a" * sb, b"b" * sb, b"c" * sb], b"h" * (n * sb),
                                             b"p" * (n * sb), bytes(range(256)) * (n * pb // 256 + 1))
    assert len(rows) == n and all(len(r) == (4 + 6 * k) * sb for r in rows)
    assert rows[0][:sb] == b"g" * sb and rows[0][2 * sb:4 * sb] == b"a" * sb + b"b" * sb
    assert rows[0][4 * sb:5 * sb] == b"g" * sb and rows[0][8 * sb:10 * sb] == b"p" * sb + b"h" * sb


def _fn_body(src, name):
    i = src.index(f"pub fn {name}(")
    k = src.find("\npub fn ", i + 1)
    return src[i:k if k > 0 else len(src)]


def test_rust_shim_calls_the_entry_points_behind_its_length_asserts():
    b = open(os.path.join(RS, "batch.rs")).read()
    h = open(os.path.join(RS, "hip.rs")).read()
    for name in NAMES:
        assert len(re.findall(r"pub fn %s\(" % name, h)) == 1, name
    prove = _fn_body(b, "sigreq_prove_batch")
    calls = ("cc_set_request_params(", "cc_sigreq_new_batch(", "cc_sigreq_pok_init_batch(",
             "cc_sigreq_pok_gen_proof_batch(")
    at = 0
    for call in calls:
        u = prove.index("unsafe", at)
        assert call in prove[u:], call
        assert "assert" in prove[at:u], call  # every unsafe block has its length asserts before it
        at = prove.index(call, u)
    first = prove.index("unsafe")
    for g in ("params.h.len(), q", "gb.len() == sb && hb.len() == q * sb"):
        assert g in prove[:first], g
    new_at = prove.index("cc_sigreq_new_batch(")
    for g in ("m.len() == q", "elgamal_pks.len(), n", "m.len() == n * q * 48 && pk.len() == n * sb",
              "rand.len() == n * (k + 1) * 48"):
        assert g in prove[:new_at], g
    init_at = prove.index("cc_sigreq_pok_init_batch(")
    assert "blind.len() == n * (3 * k + 2) * 48" in prove[:init_at]
    assert "h.len() == n * sb" in prove[:init_at] and "proofs.len() == n * pb" in prove[:init_at]
    gen_at = prove.index("cc_sigreq_pok_gen_proof_batch(")
    assert "sk.len() == n * 48 && ch.len() == n * 48" in prove[:gen_at]


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("which", ["shapes", "edges"])
def test_oracle_accepts_the_inputs(mode, which):
    """Model check with the oracle alone: every row's proof is what the reference's verifier accepts, and
    for the rows whose elgamal_pk is sk g the issuance flow ends in a signature that verifies."""
    from oracle import coconut_ref as C
    from oracle import issuance as I
    import sigreq_prove_cases as K
    seen = 0
    for _name, w, k, rows in K.expected(mode, which):
        grp = w.grp
        rng = C.Drbg(f"sigreq-model-{mode}-{_name}")
        x, y = rng.fr(), [rng.fr() for _ in range(w.q)]
        vk = (grp.other.mul(w.g_tilde, x), [grp.other.mul(w.g_tilde, v) for v in y])
        for r in rows:
            want = r["want"]
            chal = r["chal"] % K.R
            ok = I.sigreq_proof_verify(grp, want["proof"], want["req"], r["pk"], chal, w.params())
            if r["valid"]:
                assert ok, r["name"]
            else:
                # pk is not sk g: every Schnorr check but the ElGamal key's holds
                assert not ok, r["name"]
                for i, (p1, p2) in enumerate(want["proof"]["cts"]):
                    assert I.schnorr_verify(grp, [w.g], want["req"]["ciphertexts"][i][0], p1, chal), r["name"]
                    assert I.schnorr_verify(grp, [r["pk"], want["h_pt"]], want["req"]["ciphertexts"][i][1], p2, chal)
                assert I.schnorr_verify(grp, list(w.h[:k]) + [w.g], want["req"]["commitment"], want["proof"]["comm"],
                                        chal), r["name"]
            if r["valid"] and (which == "shapes" or r["name"] in ("m=0,1,r-1", "blindings=0", "known m0=r+5")):
                blinded = I.blind_sign(grp, want["req"], (x, y))
                sig = I.unblind(grp, blinded, r["sk"] % K.R)
                assert C.verify(grp, sig, [m % K.R for m in r["msgs"]], vk, w.g_tilde), r["name"]
            seen += 1
    assert seen == (10 if which == "shapes" else 15)
    if which == "edges":
        by = {r["name"]: (w, r) for _n, w, _k, rows in K.expected(mode, which) for r in rows}
        ident = C.Groups(mode).sig_to_bytes(None)
        sb = len(ident)
        w, r = by["r=0,k0=0,m0=0,m2>=r"]
        assert r["want"]["cts"][:2 * sb] == ident + ident  # c1_0 and c2_0
        w, r = by["blindings=0"]
        rec, k = r["want"]["init"], r["k"]
        assert rec[:sb] == ident and rec[sb + 48:2 * sb + 48] == ident
        for i in range(k):
            o = 2 * sb + 48 * (k + 2) + i * (2 * sb + 144)
            assert rec[o:o + sb] == ident and rec[o + sb + 48:o + 2 * sb + 48] == ident
        w, r = by["pk=-h"]
        assert r["want"]["cts"][sb:2 * sb] == ident  # c2_0 = m (pk + h)
        w, r = by["h1=-h0, equal messages"]
        assert r["want"]["commitment"] == w.grp.sig_to_bytes(w.grp.sig.mul(w.g, r["rand"][0]))
        w, r = by["h0 identity, h1 off-curve"]
        assert r["want"]["commitment"] == w.grp.sig_to_bytes(w.grp.sig.mul(w.g, r["rand"][0]))
        assert by["known m0=r+5"][1]["msgs"][0] >= K.R
