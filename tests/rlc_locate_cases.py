"""Inputs shared by tests/test_gpu_rlc_locate.py (GPU) and tests/test_rlc_locate_model.py (CPU): the shapes,
the batches (C oracle, test_gpu_parity._gen_batch, generated once a mode), where the bad credentials go and
which segment each must land in.  The CPU test checks these inputs (segments, oracle verdicts); the GPU test
uses them."""
import functools

import numpy as np

from conftest import golden
from test_gpu_parity import _gen_batch

Q = 6
N = 150                # the largest batch: 9 full segments of 16 and a tail of 6
SEG = 16
SEED = bytes(range(1, 33))
BASE_INDEX = (1 << 40) + 12345   # a non-zero, wider-than-32-bit start of the delta schedule
# (n, seg) of the partial comparison: several segments with a tail; exact multiples; one credential in the
# tail; a batch shorter than the segment; seg = 4 (tree level 0: no product); a longer segment
SHAPES = ((150, 16), (64, 16), (65, 16), (7, 16), (12, 4), (129, 64))
# the segmented bucket reduce sizes its lane groups by seg (fold.hip fold_seg_group: one lane or lane pair a
# bucket up to 2,048, doubling up to the whole wave at 65,536): one segment of each width
WIDE_SHAPES = ((150, 2048), (150, 4096), (150, 16384), (150, 131072))

# one swapped sigma_2 at a time in the (150, 16) batch: (index, segment it must clear, segment length)
LOCATE_ONE = (
    (32, 2, 16),    # the first credential of a segment
    (47, 2, 16),    # the last credential of a segment
    (64, 4, 16), (65, 4, 16), (66, 4, 16), (67, 4, 16),   # the four quad positions (k_miller4)
    (147, 9, 6),    # the 6-credential tail segment
)
# two at a time: (indices, rejected segments, merged runs as (lo, hi))
LOCATE_TWO = (
    ((47, 48), (2, 3), ((32, 64),)),              # adjacent segments: one run
    ((10, 100), (0, 6), ((0, 16), (96, 112))),    # far apart: two runs
)
FLAG_N, FLAG_SEG, FLAG_AT = 64, 16, 21   # the per-segment flag cases: credential 21 (segment 1 of 4)
FLAG_KINDS = ("sigma1_inf", "sigma2_inf", "sigma1_outside", "sigma2_outside")


def sig_bytes(mode):
    return 192 if mode == 0 else 97


@functools.lru_cache(maxsize=None)
def batch(mode):
    """N valid credentials of q = Q messages (mode 0 SigG2, 1 SigG1)."""
    return _gen_batch(mode, N, Q, seed=301 + mode, bad_every=N + 1)


def head(mode, n):
    """(sigma_1, sigma_2, msgs) of the first n credentials of batch(mode)."""
    b, sb = batch(mode), sig_bytes(mode)
    return b["s1"][:n * sb], b["s2"][:n * sb], b["msgs"][:n * Q * 48]


def swap_sigma2(mode, n, bad):
    """The first n credentials with sigma_2 of every index in `bad` replaced by its successor's (mod n):
    -> (sigma_1, sigma_2, msgs, expected verdicts)."""
    s1, s2, ms = head(mode, n)
    sb = sig_bytes(mode)
    out = bytearray(s2)
    expect = np.ones(n, np.uint8)
    for i in bad:
        j = (i + 1) % n
        out[i * sb:(i + 1) * sb] = s2[j * sb:(j + 1) * sb]
        expect[i] = 0
    return s1, bytes(out), ms, expect


def special_points(mode):
    """The signature group's identity encoding and a curve point outside its order-r subgroup."""
    g = "G2" if mode == 0 else "G1"
    d = golden(f"verify_{g.lower()}_q6.json")
    inf = bytes.fromhex(next(c for c in d["creds"] if c["kind"] == "sigma1_inf")["sigma1"])
    outside = bytes.fromhex(next(r["point"] for r in golden("subgroup.json")[g] if r["status"] == 1))
    assert len(inf) == len(outside) == sig_bytes(mode)
    return inf, outside


def flag_case(mode, kind):
    """FLAG_N valid credentials with credential FLAG_AT's sigma_1 or sigma_2 the identity or outside the
    subgroup -> (sigma_1, sigma_2, msgs, expected verdicts): that credential alone fails."""
    s1, s2, ms = head(mode, FLAG_N)
    inf, outside = special_points(mode)
    sb = sig_bytes(mode)
    s1, s2 = bytearray(s1), bytearray(s2)
    pt = inf if kind.endswith("_inf") else outside
    (s1 if kind.startswith("sigma1") else s2)[FLAG_AT * sb:(FLAG_AT + 1) * sb] = pt
    expect = np.ones(FLAG_N, np.uint8)
    expect[FLAG_AT] = 0
    return bytes(s1), bytes(s2), ms, expect


def tree_level(n_values, k):
    """The index sets of the pairwise product tree (tail kept alone) after k levels over n_values leaves."""
    level = [[i] for i in range(n_values)]
    for _ in range(k):
        level = [level[2 * t] + (level[2 * t + 1] if 2 * t + 1 < len(level) else []) for t in range((len(level) + 1) // 2)]
    return level
