"""Inputs for the direct test of the wide Miller loop (tests/test_gpu_miller_wide_direct.py; the recipe
of tests/golden/miller_wide_words.json in tests/golden/make_golden.py uses the same builder).

PAIRS is 16 pairs (P in G1, Q in G2) from a seeded random.Random, built with oracle/bls12_381.py; the
last two are (a P0, Q0) and (P0, a Q0) for the small scalar A, so every launch of 16 or more also holds
the bilinearity check.  Larger launches tile them.

Encoding (csrc/soa.h, the comment above k_wide_pairs in csrc/miller_wide.hip).  The kernels read the
prep structure of arrays: word w of Fp slot s of pair i at ((s * 12 + w) * n + i).  Q is affine in slots
S_Q1..S_Q1+3 (x real, x imaginary, y real, y imaginary); P is in evaluation form k (x, y, 1) in
S_P1..S_P1+2 for any k in Fp* (the final exponentiation removes k).  Every Fp value v is stored as
v 2^406 mod p (tests/fexp_direct_cases.py).  One flag word per pair.  The Miller value of pair i leaves
in the 144-word element form of fexp_direct_cases.encode at element foff + i of stride fstride.
"""
import functools
import random

import numpy as np

import fexp_direct_cases as C
from oracle import bls12_381 as B

P = B.P
NW = C.NW
S_Q1, S_P1, PREP_SLOTS = 0, 8, 14  # csrc/soa.h
NPAIR = 16
A = 5             # the bilinearity pair's scalar
SKIP_MASK = 5     # flag bits 0 and 2 skip the pair (Miller value exactly 1)
ONE_WORDS = C.element_words(C.ONE)


@functools.lru_cache(maxsize=None)
def pairs():
    rnd = random.Random(0x3117E7)
    out = [(B.G1.mul(B.G1.gen, rnd.randrange(1, B.R)), B.G2.mul(B.G2.gen, rnd.randrange(1, B.R)))
           for _ in range(NPAIR - 2)]
    p0, q0 = out[0]
    out.append((B.G1.mul(p0, A), q0))
    out.append((p0, B.G2.mul(q0, A)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def scales():
    """One random k in Fp* per pair (the evaluation form's scaling)."""
    rnd = random.Random(0x5CA1E)
    return tuple(rnd.randrange(2, P) for _ in range(NPAIR))


@functools.lru_cache(maxsize=None)
def gt_of_pair(t):
    """The oracle's GT bytes of PAIRS[t]."""
    p, q = pairs()[t]
    return B.gt_to_bytes(B.pairing(p, q))


def _words(v):
    v = v * C.R_STORE % P
    return [(v >> (32 * w)) & 0xFFFFFFFF for w in range(NW)]


def pair_words(p, q, k=1):
    """The PREP_SLOTS x 12 words of one pair, slot major (unused slots zero)."""
    out = np.zeros(PREP_SLOTS * NW, dtype=np.uint32)
    (xa, xb), (ya, yb) = q
    vals = {S_Q1: xa, S_Q1 + 1: xb, S_Q1 + 2: ya, S_Q1 + 3: yb,
            S_P1: k * p[0] % P, S_P1 + 1: k * p[1] % P, S_P1 + 2: k % P}
    for s, v in vals.items():
        out[s * NW:(s + 1) * NW] = _words(v)
    return out


def encode_prep(items):
    """items: [(P, Q, k)] -> the prep structure of arrays of the launch, stride len(items)."""
    n = len(items)
    a = np.empty((PREP_SLOTS * NW, n), dtype=np.uint32)
    for i, (p, q, k) in enumerate(items):
        a[:, i] = pair_words(p, q, k)
    return np.ascontiguousarray(a.reshape(-1))


# ---------------------------------------------------------------- the tiled launches
# blocks of 16 elements: block 0 is the 16 pairs plain (k = 1, no flags: what the recorded words pin),
# odd blocks scale P by the pair's random k, and from block 1 on the flag words below rotate through the
# elements, so skipped and computed pairs alternate inside every wave-pair of a launch
FLAG_WORDS = (0, 1, 2, 4, 8, 16, 32, 5, 0x3A, 0xFFFFFFFA, 0x80000001)


def layout(n):
    """[(pair index, k, flag word)] of a launch of n."""
    out = []
    for i in range(n):
        b, t = divmod(i, NPAIR)
        k = scales()[t] if b % 2 else 1
        fl = FLAG_WORDS[(i + b) % len(FLAG_WORDS)] if b else 0
        out.append((t, k, fl))
    return out
