"""CPU tests of the holder-side entry points' boundary (cc_pok_init_batch, cc_pok_gen_proof_batch, their
*_device forms and cc_unblind_batch): the header declares them, the library exports them, a NULL context
is refused without touching a GPU, the Python wrappers refuse a short buffer before calling C, the Rust
shim calls them behind its length asserts — and the oracle alone accepts what the edge inputs of
test_gpu_pok_prove.py produce (pok_init -> pok_gen_proof -> pok_verify_gt), so those inputs are valid
expectations before the GPU sees them."""
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
RS = os.path.join(ROOT, "integration", "rust", "src")
NAMES = ("cc_pok_init_batch", "cc_pok_init_batch_device", "cc_pok_gen_proof_batch", "cc_pok_gen_proof_batch_device",
         "cc_unblind_batch")


def test_header_declares_the_five_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bcc_status\s+%s\s*\(" % name, src), name


def test_library_exports_the_five_entry_points():
    from coconut._lib import lib
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name  # declared in coconut/_lib.py


@pytest.mark.parametrize("n", [1, 0])
def test_null_context_is_a_decode_error_without_gpu(n):
    from coconut._lib import lib
    N = None
    assert lib.cc_pok_init_batch(N, n, 6, 0, 7, N, N, N, N, N, N, N, N, N) == -4
    assert lib.cc_pok_init_batch_device(N, n, 6, 0, 7, N, N, N, N, N, N, N, N, N, N) == -4
    assert lib.cc_pok_gen_proof_batch(N, n, 6, 0, 7, N, N, N, N, N) == -4
    assert lib.cc_pok_gen_proof_batch_device(N, n, 6, 0, 7, N, N, N, N, N, N) == -4
    assert lib.cc_unblind_batch(N, n, N, N, N, N) == -4


def test_python_names_are_exported():
    import coconut
    for name in ("PoKOfSignature", "pok_init_batch", "pok_gen_proof_batch", "pok_challenge_batch", "unblind_batch"):
        assert hasattr(coconut, name), name
    assert {"init", "to_bytes", "gen_proof"} <= set(dir(coconut.PoKOfSignature))


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
    n, q, rev = 2, 3, [1]
    nresp = q - len(rev) + 1
    good = dict(sigma1=bytes(n * sb), sigma2=bytes(n * sb), msgs=bytes(n * q * 48), rand=bytes(n * (nresp + 2) * 48))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.pok_init_batch(ctx, n, q, rev, a["sigma1"], a["sigma2"], a["msgs"], a["rand"])
    good = dict(msgs=bytes(n * q * 48), rand=bytes(n * (nresp + 2) * 48), chal=bytes(n * 48))
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.pok_gen_proof_batch(ctx, n, q, rev, a["msgs"], a["rand"], a["chal"])
    for c1, c2, sk in ((bytes(sb - 1), bytes(sb), bytes(48)), (bytes(sb), bytes(sb - 1), bytes(48)),
                       (bytes(sb), bytes(sb), bytes(47))):
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.unblind_batch(ctx, [c1], [c2], [sk])
    with pytest.raises(ValueError):
        coconut.unblind_batch(ctx, [bytes(sb)], [bytes(sb)], [])


def _fn_body(src, name):
    i = src.index(f"pub fn {name}(")
    k = src.find("\npub fn ", i + 1)
    return src[i:k if k > 0 else len(src)]


def test_rust_shim_calls_the_entry_points_behind_its_length_asserts():
    b = open(os.path.join(RS, "batch.rs")).read()
    h = open(os.path.join(RS, "hip.rs")).read()
    for name in NAMES:
        assert len(re.findall(r"pub fn %s\(" % name, h)) == 1, name
    prove = _fn_body(b, "pok_prove_batch")
    first = prove.index("unsafe")
    for g in ("messages.len(), n", "m.len() == q", "(i as usize) < q", "s1.len() == n * sb && s2.len() == n * sb",
              "m.len() == n * q * 48 && rand.len() == n * (nresp + 2) * 48"):
        assert g in prove[:first], g
    assert "cc_pok_init_batch(" in prove[first:]
    second = prove.index("unsafe", first + 1)
    assert "ch.len(), n * 48" in prove[:second] and "cc_pok_gen_proof_batch(" in prove[second:]
    unb = _fn_body(b, "unblind_batch")
    cut = unb.index("unsafe")
    for g in ("sks.len(), n", "c1.len() == n * sb && c2.len() == n * sb && sk.len() == n * 48"):
        assert g in unb[:cut], g
    assert "cc_unblind_batch(" in unb[cut:]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_oracle_accepts_the_edge_inputs(mode):
    """Model check with the oracle alone: every edge case's proof is what ps_sig's verifier accepts — or,
    where the inputs make sigma' the identity or are no signature at all, what it refuses (the case's
    `valid` says which, and why is written next to the case)."""
    from oracle import coconut_ref as C
    import pok_prove_cases as K
    seen = 0
    for _name, w, rev, cases in K.edge_expected(mode):
        for c in cases:
            revealed = {i: c["msgs"][i] % K.R for i in rev}
            ok, _ = C.pok_verify_gt(w.grp, c["proof"], w.vk, w.g_tilde, revealed, c["chal"] % K.R)
            assert ok == c["valid"], c["name"]
            # the Schnorr relation holds whatever the signature is: bases . responses + chal J == T
            bases = [w.g_tilde] + [w.vk[1][i] for i in range(w.q) if i not in rev]
            chk = w.grp.other.msm(bases + [c["proof"]["J"]], list(c["proof"]["responses"]) + [c["chal"] % K.R])
            assert w.grp.oth_to_bytes(chk) == c["want"]["T"], c["name"]
            seen += 1
    assert seen == 16
    by = {c["name"]: c for _n, _w, _r, cs in K.edge_expected(mode) for c in cs}
    ident = w.grp.sig_to_bytes(None)
    assert by["r1=0"]["want"]["s1"] == ident and by["r1=0"]["want"]["s2"] == ident
    assert by["s2=s1,r2=r-1"]["want"]["s2"] == ident and by["s2=-s1,r2=1"]["want"]["s2"] == ident
    assert by["blindings=0"]["want"]["T"] == w.grp.oth_to_bytes(None)
    assert by["r1=r+5"]["rand"][0] >= K.R


def test_response_cases_cover_the_borrow():
    import pok_prove_cases as K
    names = [c[0] for c in K.response_cases()]
    assert {"chal=0", "chal=r-1", "secret=0", "b<chal*secret", "b=chal*secret"} <= set(names)
    for name, b, c, s in K.response_cases():
        if name == "b<chal*secret":
            assert b % K.R < (c * s) % K.R
        if name == "b=chal*secret":
            assert (b - c * s) % K.R == 0
