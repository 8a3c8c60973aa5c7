"""CPU tests of the per-proof-verkey PoK verify's boundary: the header, coconut/_lib.py and the Rust
binding declare both entry points with the same arity, the library exports them and rejects a NULL context
without touching a GPU, and the Python vk= path checks its byte counts."""
import os
import re
import types

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
HIP_RS = os.path.join(ROOT, "integration", "rust", "src", "hip.rs")
BATCH_RS = os.path.join(ROOT, "integration", "rust", "src", "batch.rs")
ARITY = {"cc_pok_verify_batch_pervk_device": 18, "cc_pok_verify_batch_pervk": 17}


def _c_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    m = re.search(r"\bcc_status\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def _rust_params(name):
    src = re.sub(r"//[^\n]*", "", open(HIP_RS).read())
    m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, src, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", sorted(ARITY))
def test_header_python_and_rust_declare_the_same_arity(name):
    from coconut._lib import _SIGS, lib
    c = _c_params(name)
    assert len(c) == ARITY[name], c
    assert len(_SIGS[name][1]) == ARITY[name]
    assert len(_rust_params(name)) == ARITY[name]
    assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == ARITY[name]
    # the verkey arguments come after the revealed messages, before the outputs
    names = [p.split()[-1].lstrip("*") for p in c]
    i = names.index("d_revealed_msgs" if name.endswith("_device") else "revealed_msgs")
    assert [n.lower().replace("d_", "") for n in names[i + 1:i + 3]] == ["vk_x", "vk_y"]


def test_the_device_form_is_the_shared_verkey_form_plus_two_verkey_pointers():
    a, b = _c_params("cc_pok_verify_batch_device"), _c_params("cc_pok_verify_batch_pervk_device")
    assert len(b) == len(a) + 2
    assert b[:13] == a[:13] and b[15:] == a[13:]
    assert b[13:15] == ["const uint8_t* d_vk_X", "const uint8_t* d_vk_Y"]


def test_rust_wrapper_guards_its_lengths_before_the_call():
    src = open(BATCH_RS).read()
    body = src[src.index("pub fn pok_verify_batch_pervk("):]
    body = body[:body.index("\npub ", 1)]
    head = body[:body.index("unsafe")]
    for g in ("vks.len(), n", "v.Y_tilde.len() == q", "chal.len(), n", "revealed_msgs.len() == n", "m.len() == r",
              "p.4.len() == nresp", "p.0.len() == sb", "p.2.len() == ob", "vx.len() == n * ob && vy.len() == n * q * ob"):
        assert g in head, g
    assert "cc_pok_verify_batch_pervk(" in body and "set_verkey" not in body


def test_null_context_is_a_decode_error_without_gpu():
    from coconut._lib import lib
    N = None
    for n in (1, 0):
        assert lib.cc_pok_verify_batch_pervk_device(N, n, 6, 0, 7, N, N, N, N, N, N, N, N, N, N, N, N, N) == -4
        assert lib.cc_pok_verify_batch_pervk(N, n, 6, 0, 7, N, N, N, N, N, N, N, N, N, N, N, N) == -4


def test_python_vk_path_checks_byte_counts():
    import coconut
    from coconut import pok_verify_batch
    from coconut.errors import CoconutError, CoconutErrorKind
    ctx = types.SimpleNamespace(mode=coconut.GroupMode.SIG_G2, h=None)
    n, q, sb, ob = 2, 3, 192, 97
    ok = dict(sigma1=bytes(n * sb), sigma2=bytes(n * sb), J=bytes(n * ob), T=bytes(n * ob), responses=bytes(n * 3 * 48),
              chal=bytes(n * 48), revealed_msgs=bytes(n * 48))
    for vk in ((bytes(n * ob - 1), bytes(n * q * ob)), (bytes(n * ob), bytes(n * q * ob - 1)), (None, bytes(n * q * ob)),
               (bytes(n * ob), None)):
        with pytest.raises(CoconutError) as e:
            pok_verify_batch(ctx, n, q, [1], 3, vk=vk, **ok)
        assert e.value.kind is CoconutErrorKind.Decode
    with pytest.raises(ValueError):
        pok_verify_batch(ctx, n, q, [1], 3, vk=(bytes(n * ob), bytes(n * q * ob)), rlc=True, **ok)
