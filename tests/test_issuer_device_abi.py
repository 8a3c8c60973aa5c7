"""CPU tests of the boundary of the issuer's device forms (cc_sigreq_verify_batch_device,
cc_blind_sign_batch_device): the header declares them, the library exports them, a NULL context is refused
without touching a GPU, the Python wrappers refuse a short buffer before calling C, and the Rust shim calls
them behind its length asserts."""
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
RS = os.path.join(ROOT, "integration", "rust", "src")
NAMES = ("cc_sigreq_verify_batch_device", "cc_blind_sign_batch_device")


def test_header_declares_both_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bcc_status\s+%s\s*\(" % name, src), name


def test_library_exports_both_entry_points():
    from coconut._lib import lib
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name  # declared in coconut/_lib.py


@pytest.mark.parametrize("n", [1, 0])
def test_null_arguments_are_a_decode_error_without_gpu(n):
    import ctypes
    from coconut._lib import lib
    N = None
    assert lib.cc_sigreq_verify_batch_device(N, n, 3, 2, N, N, N, N, N, N, N, N, N) == -4
    assert lib.cc_blind_sign_batch_device(N, n, 3, 2, N, N, N, N, N, N, N, N, N, N) == -4
    b = ctypes.create_string_buffer(4 * 48)
    p = ctypes.cast(b, ctypes.c_void_p)
    assert lib.cc_blind_sign_batch_device(N, n, 3, 2, p, p, p, p, p, p, p, p, p, N) == -4  # the context alone


def test_python_names_are_exported():
    import coconut
    for name in ("sigreq_verify_batch_device", "blind_sign_batch_device"):
        assert hasattr(coconut, name), name


class _Ctx:
    """Enough of a Context for the wrappers' length checks, which run before any C call."""
    h = None

    def __init__(self, mode):
        import coconut
        self.mode = coconut.GroupMode(mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_python_wrappers_refuse_a_short_buffer_before_calling_c(mode):
    import torch
    import coconut
    from coconut import CoconutError
    ctx = _Ctx(mode)
    sb = ctx.mode.sig_bytes
    n, q, k = 2, 3, 2
    pb = coconut.sigreq_proof_bytes(ctx, k)
    z = lambda c: torch.zeros(c, dtype=torch.uint8)  # noqa: E731
    good = dict(commitments=z(n * sb), known=z(n * (q - k) * 48), ciphertexts=z(n * k * 2 * sb), pks=z(n * sb),
                proofs=z(n * pb), chals=z(n * 48))
    order = ("commitments", "known", "ciphertexts", "pks", "proofs", "chals")
    for short in good:
        a = dict(good, **{short: good[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.sigreq_verify_batch_device(ctx, n, q, k, *[a[key] for key in order])
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.sigreq_verify_batch_device(ctx, n, q, k, *[None if key == "known" else good[key] for key in order])
    with pytest.raises(CoconutError, match="torch.uint8"):
        coconut.sigreq_verify_batch_device(ctx, n, q, k, good["commitments"].to(torch.int32),
                                           *[good[key] for key in order[1:]])
    with pytest.raises(CoconutError, match="device tensor"):  # full-length host tensors: not what the C side reads
        coconut.sigreq_verify_batch_device(ctx, n, q, k, *[good[key] for key in order])
    x, y = bytes(48), [bytes(48)] * q
    sign = dict(commitments=good["commitments"], known=good["known"], ciphertexts=good["ciphertexts"])
    for short in sign:
        a = dict(sign, **{short: sign[short][:-1]})
        with pytest.raises(CoconutError, match="the call reads"):
            coconut.blind_sign_batch_device(ctx, n, q, k, a["commitments"], a["known"], a["ciphertexts"], x, y)
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.blind_sign_batch_device(ctx, n, q, k, None, sign["known"], sign["ciphertexts"], x, y, h=z(n * sb - 1))
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.blind_sign_batch_device(ctx, n, q, k, *sign.values(), x[:-1], y)
    with pytest.raises(CoconutError, match="the call reads"):
        coconut.blind_sign_batch_device(ctx, n, q, k, *sign.values(), x, y[:-1])


def _fn_body(src, name):
    i = src.index(f"pub fn {name}(")
    k = src.find("\npub fn ", i + 1)
    return src[i:k if k > 0 else len(src)]


def test_rust_shim_calls_the_entry_points_behind_its_length_asserts():
    b = open(os.path.join(RS, "batch.rs")).read()
    h = open(os.path.join(RS, "hip.rs")).read()
    for name in NAMES:
        assert len(re.findall(r"pub fn %s\(" % name, h)) == 1, name
    body = _fn_body(b, "issuer_verify_sign_device")
    at = 0
    for call in ("cc_set_request_params(", "cc_sigreq_verify_batch_device(", "cc_blind_sign_batch_device("):
        u = body.rindex("unsafe {", 0, body.index(call, at))  # the block the call sits in
        assert "assert" in body[at:u], call  # length asserts before every call
        at = body.index(call, u)
    verify_at = body.index("cc_sigreq_verify_batch_device(")
    for g in ("commitment.len() >= n * sb", "known.len() >= n * (q - k) * 48", "ciphertexts.len() >= n * k * 2 * sb",
              "elgamal_pk.len() >= n * sb", "proofs.len() >= n * pb", "chal.len() >= n * 48", "verdicts.len() >= n",
              "h.len() >= n * sb", "c1.len() >= n * sb && c2.len() >= n * sb", "gb.len() == sb && hb.len() == q * sb"):
        assert g in body[:verify_at], g
    sign_at = body.index("cc_blind_sign_batch_device(")
    assert "x.len() == 48 && y.len() == q * 48" in body[:sign_at]
    assert "sigkey.y.len(), q" in body[:sign_at]
    assert "pub unsafe fn new(ptr: *mut u8, len: usize)" in b  # a DeviceBytes is vouched for once, by its maker
