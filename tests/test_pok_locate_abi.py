"""CPU tests of the PoK RLC locate entry points' boundary: the header declares them, the library exports them,
and all three reject a NULL context without touching a GPU."""
import ctypes
import os
import re

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "coconut_hip.h")
NAMES = ("cc_pok_rlc_partial_seg_device", "cc_pok_verify_batch_locate_device", "cc_pok_verify_batch_locate")


def test_header_declares_the_entry_points_and_the_defaults():
    raw = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bcc_status\s+%s\s*\(" % name, src), name
    for mode in ("G2", "G1"):
        m = re.search(r"#define\s+CC_POK_LOCATE_SEG_DEFAULT_%s\s+(\d+)" % mode, src)
        assert m, mode
        seg = int(m.group(1))
        assert seg >= 4 and seg & (seg - 1) == 0, seg   # a segment length the partial takes


def test_library_exports_the_entry_points():
    from coconut._lib import lib
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name  # declared in coconut/_lib.py


def test_null_context_is_a_decode_error_without_gpu():
    from coconut._lib import lib
    N = None
    seed = bytes(32)
    part = (ctypes.c_uint32 * 929)()
    out = ctypes.cast(part, ctypes.c_void_p)
    stats = (ctypes.c_uint32 * 3)(7, 7, 7)
    for n in (1, 0):
        assert lib.cc_pok_rlc_partial_seg_device(N, n, 6, 0, 7, 16, 0, seed, N, N, N, N, N, N, N, N, out, N) == -4
        assert lib.cc_pok_verify_batch_locate_device(N, n, 6, 0, 7, 16, seed, N, N, N, N, N, N, N, N, out, stats, N) == -4
        assert lib.cc_pok_verify_batch_locate(N, n, 6, 0, 7, 16, N, N, N, N, N, N, N, N, out, stats) == -4
    assert list(stats) == [7, 7, 7]   # refused before anything is written


def test_python_forms_are_exported():
    import coconut
    assert callable(coconut.pok_verify_batch_locate)
    assert callable(coconut.PokDeviceEngine.partial_seg) and callable(coconut.PokDeviceEngine.locate)
    assert coconut.PokDeviceEngine.partial_seg is not coconut.DeviceEngine.partial_seg
    assert coconut.PokDeviceEngine.locate is not coconut.DeviceEngine.locate
    assert coconut.PokDeviceEngine.finish_each is coconut.DeviceEngine.finish_each
