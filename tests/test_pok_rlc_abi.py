"""CPU tests of the PoK RLC entry points' boundary: the header declares them, the library exports
them, both reject a NULL context without touching a GPU, and the Python form refuses a GT request."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
NAMES = ("cc_pok_rlc_partial_device", "cc_pok_verify_batch_rlc")


def test_header_declares_both_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bcc_status\s+%s\s*\(" % name, src), name


def test_library_exports_both_entry_points():
    from coconut._lib import lib
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name  # declared in coconut/_lib.py


def test_null_context_is_a_decode_error_without_gpu():
    from coconut._lib import lib
    N = None
    seed = bytes(32)
    part = (ctypes.c_uint32 * 929)()
    assert lib.cc_pok_rlc_partial_device(N, 1, 6, 0, 7, 0, seed, N, N, N, N, N, N, N, N,
                                         ctypes.cast(part, ctypes.c_void_p), N) == -4
    assert lib.cc_pok_rlc_partial_device(N, 0, 6, 0, 7, 0, seed, N, N, N, N, N, N, N, N,
                                         ctypes.cast(part, ctypes.c_void_p), N) == -4
    assert lib.cc_pok_verify_batch_rlc(N, 1, 6, 0, 7, N, N, N, N, N, N, N, N, N) == -4
    assert lib.cc_pok_verify_batch_rlc(N, 0, 6, 0, 7, N, N, N, N, N, N, N, N, N) == -4


def test_rlc_with_gt_output_is_refused():
    from coconut import pok_verify_batch
    with pytest.raises(ValueError):
        pok_verify_batch(None, 0, 6, [], 7, b"", b"", b"", b"", b"", b"", b"", want_gt=True, rlc=True)


def test_engine_is_exported():
    import coconut
    from coconut.dist import DeviceEngine
    assert issubclass(coconut.PokDeviceEngine, DeviceEngine)
