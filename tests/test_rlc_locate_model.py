"""CPU side of the RLC locate mode (cc_verify_batch_locate*): the planning header under sanitizers, the
product tree's alignment that the segmented partial relies on, and the inputs of tests/test_gpu_rlc_locate.py
checked against the C oracle, so a GPU failure there is the library's and not the test's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rlc_locate_cases as L
from conftest import host_threads, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def _san_env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locate") / "test_locate_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-I",
                           os.path.join(ROOT, "coconut-rust_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "test_locate_plan.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=_san_env())
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr
    return p.stdout


def test_planner_builtin_cases_under_asan_ubsan(planner):
    """No segment rejected, every segment rejected, alternating, adjacent ones merging, the short tail,
    S = 1, an empty batch, and the segment lengths the partial takes."""
    assert "all checks passed" in _run(planner)


def _brute(n, seg, bits):
    """The plan restated per credential: mark every credential of a rejected segment, then read the runs
    off the marks."""
    S = -(-n // seg)
    mark = np.zeros(n, bool)
    for s in range(S):
        if bits[s] == "0":
            mark[s * seg:min(n, (s + 1) * seg)] = True
    runs, i, off = [], 0, 0
    while i < n:
        if not mark[i]:
            i += 1
            continue
        j = i
        while j < n and mark[j]:
            j += 1
        runs.append((i, j, off))
        off += j - i
        i = j
    rej = bits.count("0")
    return (S, rej, int(mark.sum()), int(rej == S)), runs


def test_planner_counts_against_a_brute_force_restatement(planner):
    rng = np.random.default_rng(7)
    cases = [(150, 16, "1" * 10), (150, 16, "0" * 10), (128, 16, "01" * 4), (150, 16, "1100111011"),
             (150, 16, "1111111110"), (7, 16, "0"), (7, 16, "1"), (12, 4, "010")]
    for n, seg in L.SHAPES + ((300, 4), (257, 32)):
        S = -(-n // seg)
        for _ in range(3):
            cases.append((n, seg, "".join(rng.choice(["0", "1"], size=S, p=[0.4, 0.6]))))
    for n, seg, bits in cases:
        out = _run(planner, n, seg, bits).split("\n")
        head, runs = _brute(n, seg, bits)
        assert tuple(map(int, out[0].split())) == head, (n, seg, bits)
        got = [tuple(map(int, ln.split())) for ln in out[1:] if ln.strip()]
        assert got == runs, (n, seg, bits)


def test_planner_merges_as_the_gpu_test_expects(planner):
    for bad, segs, runs in L.LOCATE_TWO:
        bits = "".join("0" if s in segs else "1" for s in range(-(-L.N // L.SEG)))
        out = _run(planner, L.N, L.SEG, bits).split("\n")
        got = [tuple(map(int, ln.split()))[:2] for ln in out[1:] if ln.strip()]
        assert got == list(runs), bad


@pytest.mark.parametrize("n,seg", L.SHAPES + L.WIDE_SHAPES + ((300, 4), (131072, 4096), (131071, 1024)))
def test_product_tree_keeps_segments_aligned(n, seg):
    """k_miller4 puts credentials 4 j .. 4 j + 3 into Miller value j; the tree is pairwise with the tail kept
    alone.  After k levels (seg = 4 * 2^k) element t must hold exactly the Miller values [t 2^k, (t + 1) 2^k),
    i.e. the credentials of segment t, and the level must have S = ceil(n / seg) elements."""
    k = (seg // 4).bit_length() - 1
    assert 4 << k == seg
    nv = (n + 3) // 4
    if nv > 4096:  # the big shapes: the index arithmetic alone (lists of 32,768 leaves per level are slow)
        size = nv
        for _ in range(k):
            size = (size + 1) // 2
        assert size == -(-n // seg)
        return
    level = L.tree_level(nv, k)
    assert len(level) == -(-n // seg)
    for t, idx in enumerate(level):
        assert idx == list(range(t << k, min(nv, (t + 1) << k)))
        creds = [c for j in idx for c in range(4 * j, min(n, 4 * j + 4))]
        assert creds == list(range(t * seg, min(n, (t + 1) * seg)))


def test_bad_indices_fall_in_the_expected_segments():
    S = -(-L.N // L.SEG)
    assert S == 10 and L.N - (S - 1) * L.SEG == 6
    for i, s, length in L.LOCATE_ONE:
        assert i // L.SEG == s and min(L.N, (s + 1) * L.SEG) - s * L.SEG == length
    assert [i % 4 for i, _, _ in L.LOCATE_ONE[2:6]] == [0, 1, 2, 3]
    assert L.LOCATE_ONE[0][0] % L.SEG == 0 and L.LOCATE_ONE[1][0] % L.SEG == L.SEG - 1
    for bad, segs, runs in L.LOCATE_TWO:
        assert tuple(i // L.SEG for i in bad) == segs
    assert L.FLAG_AT // L.FLAG_SEG == 1 and -(-L.FLAG_N // L.FLAG_SEG) == 4


def _oracle_verdicts(mode, n, s1, s2, ms):
    b = L.batch(mode)
    ver = ctypes.create_string_buffer(n)
    oracle_lib().oc_verify_batch(mode, ctypes.c_size_t(n), ctypes.c_size_t(L.Q), s1, s2, ms, b["X"], b["Y"], 0,
                                 b["g_tilde"], ver, None, host_threads())
    return np.frombuffer(ver.raw, np.uint8)


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_verdicts_of_the_corrupted_batches_equal_construction(mode):
    """The C oracle's per-credential verdicts on every batch the GPU test corrupts equal the verdicts the
    GPU test expects by construction."""
    assert _oracle_verdicts(mode, L.N, *L.head(mode, L.N)).all()
    for bad in [(i,) for i, _, _ in L.LOCATE_ONE] + [b for b, _, _ in L.LOCATE_TWO]:
        s1, s2, ms, expect = L.swap_sigma2(mode, L.N, bad)
        assert np.array_equal(_oracle_verdicts(mode, L.N, s1, s2, ms), expect), bad
    for kind in L.FLAG_KINDS:
        s1, s2, ms, expect = L.flag_case(mode, kind)
        assert np.array_equal(_oracle_verdicts(mode, L.FLAG_N, s1, s2, ms), expect), kind
