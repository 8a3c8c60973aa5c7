"""CPU tests of the keygen entry points' boundary: the header, coconut/_lib.py, the loaded library and the
Rust binding agree on the five names and their arity, a NULL context is rejected without touching a GPU, the
Python wrappers check their byte counts, and the Rust wrapper guards its lengths before the call."""
import os
import re
import types

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
HIP_RS = os.path.join(ROOT, "integration", "rust", "src", "hip.rs")
BATCH_RS = os.path.join(ROOT, "integration", "rust", "src", "batch.rs")
ARITY = {"cc_set_keygen_params": 5, "cc_keygen_deal_batch": 14, "cc_keygen_deal_batch_device": 15,
         "cc_keygen_combine_batch": 18, "cc_keygen_combine_batch_device": 19}


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
def test_header_python_library_and_rust_agree_on_the_arity(name):
    from coconut._lib import _SIGS, lib
    c = _c_params(name)
    assert len(c) == ARITY[name], c
    assert len(_SIGS[name][1]) == ARITY[name]
    assert len(_rust_params(name)) == ARITY[name]
    assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == ARITY[name]


def test_the_device_forms_are_the_host_forms_plus_a_stream():
    strip = lambda ps: [p.replace(" d_", " ").replace("*d_", "*") for p in ps]  # noqa: E731
    for host in ("cc_keygen_deal_batch", "cc_keygen_combine_batch"):
        a, b = _c_params(host), _c_params(host + "_device")
        assert b[-1] == "void* stream" and strip(b[:-1]) == a
    deal = [p.split()[-1].lstrip("*") for p in _c_params("cc_keygen_deal_batch")]
    assert deal == ["ctx", "m", "q", "t", "total", "coeffs", "coeffs_t", "out_x", "out_y", "out_xt", "out_yt",
                    "out_comm", "out_X", "out_Y"]
    comb = [p.split()[-1].lstrip("*") for p in _c_params("cc_keygen_combine_batch")]
    assert comb == ["ctx", "m", "d", "q", "t", "total", "x", "y", "xt", "yt", "comm", "out_x", "out_y", "out_xt",
                    "out_yt", "out_comm", "out_X", "out_Y"]


def test_null_context_is_a_decode_error_without_gpu():
    from coconut._lib import lib
    N = None
    b = bytes(192)
    assert lib.cc_set_keygen_params(N, b, N, N, 0) == -4
    for m in (1, 0):
        assert lib.cc_keygen_deal_batch(N, m, 1, 1, 1, N, N, N, N, N, N, N, N, N) == -4
        assert lib.cc_keygen_deal_batch_device(N, m, 1, 1, 1, N, N, N, N, N, N, N, N, N, N) == -4
        assert lib.cc_keygen_combine_batch(N, m, 1, 1, 1, 1, N, N, N, N, N, N, N, N, N, N, N, N) == -4
        assert lib.cc_keygen_combine_batch_device(N, m, 1, 1, 1, 1, N, N, N, N, N, N, N, N, N, N, N, N, N) == -4


def test_python_wrappers_reject_short_buffers():
    import coconut
    from coconut import keygen_combine_batch, keygen_deal_batch
    from coconut.errors import CoconutError, CoconutErrorKind
    ctx = types.SimpleNamespace(mode=coconut.GroupMode.SIG_G2, h=None)
    m, q, t, total = 2, 1, 3, 4
    cb = m * (q + 1) * t * 48
    for cf, ct in ((bytes(cb - 1), None), (None, None), (bytes(cb), bytes(cb - 1))):
        with pytest.raises(CoconutError) as e:
            keygen_deal_batch(ctx, m, q, t, total, cf, ct)
        assert e.value.kind is CoconutErrorKind.Decode
    d = 2
    xb, yb, mb = d * m * total * 48, d * m * total * q * 48, d * m * (q + 1) * t * 97
    ok = dict(x=bytes(xb), y=bytes(yb), xt=bytes(xb), yt=bytes(yb), comm=bytes(mb))
    for key in ok:
        bad = dict(ok, **{key: ok[key][:-1]})
        with pytest.raises(CoconutError) as e:
            keygen_combine_batch(ctx, m, d, q, t, total, **bad)
        assert e.value.kind is CoconutErrorKind.Decode
    with pytest.raises(CoconutError) as e:  # one Pedersen buffer given makes all of them required
        keygen_combine_batch(ctx, m, d, q, t, total, ok["x"], ok["y"], comm=ok["comm"])
    assert e.value.kind is CoconutErrorKind.Decode
    sctx = types.SimpleNamespace(mode=coconut.GroupMode.SIG_G1, h=None, _kg=None)
    for args in ((bytes(191),), (bytes(192), bytes(96), bytes(97)), (bytes(192), bytes(97), None)):
        with pytest.raises(CoconutError) as e:
            coconut.Context.set_keygen_params(sctx, *args)
        assert e.value.kind is CoconutErrorKind.Decode


def test_rust_wrapper_guards_its_lengths_before_the_call():
    src = open(BATCH_RS).read()
    body = src[src.index("pub fn keygen_deal_batch("):]
    body = body[:body.index("\npub ", 1)]
    head = body[:body.index("cc_keygen_deal_batch(")]
    for g in ("t > 0 && t <= total", "gt.len(), ob", "g.len() == 97 && h.len() == 97", "cf.len() == nc * 48",
              "ct.len() == nc * 48", "x.len() == ns * 48 && y.len() == ns * q * 48",
              "xk.len() == ns * ob && yk.len() == ns * q * ob",
              "xt.len() == ns * 48 && yt.len() == ns * q * 48 && cm.len() == nc * 97"):
        assert g in head, g
    assert head.count("// len-guard") >= 6
    # the params call's own guards precede it too
    params = body[:body.index("cc_set_keygen_params(")]
    assert "gt.len(), ob" in params and "g.len() == 97 && h.len() == 97" in params
