"""Inputs for the direct tests of the final exponentiation and the Fp12 product tree
(tests/test_fexp_direct_model.py on the CPU, tests/test_gpu_fexp_direct.py on the device).

Every input is an oracle Fp12: six Fp2 coefficients of W^0..W^5 (oracle/bls12_381.py, W^6 = xi), drawn
from a seeded random.Random, every Fp value canonical (< p).  `encode` writes a batch in the kernels'
input form; `expected` gives the oracle's GT bytes and verdict for one input (computed once per
distinct input).  Each case carries the regime its construction claims (KINDS); the model test walks the
chain the kernels run and asserts the claim, so the device test can place cases by kind.

Encoding.  The kernels read the 12 x 32-bit structure of arrays of csrc/soa.h: word w of Fp slot k of
element i at ((k * 12 + w) * n + i), the twelve Fp slots being the two halves (real, imaginary) of the
Fp2 values a.a, a.b, b.a, b.b, c.a, c.b of the AMCL tower, which are the coefficients of
W^0, W^3, W^1, W^4, W^2, W^5 (oracle AMCL_SLOT_TO_W).  Each Fp value x is stored as x R mod p with the
storage constant R = 2^406 of csrc/field.h (csrc/lazy.h: "12 x 32 canonical, R = 2^406"), not 2^384.
final_exp is invariant under scaling by Fp*, so a wrong R would pass every final-exponentiation test
here unnoticed; the product-tree test (out = a b R, not a b R^2) is what pins the constant.
"""
import functools
import random

import numpy as np

from oracle import bls12_381 as B

P = B.P
R_STORE = pow(2, 406, P)
R_STORE_INV = pow(R_STORE, -1, P)
NW = 12          # 32-bit words per Fp
F12_WORDS = 144  # 12 Fp slots x 12 words
GT_BYTES = 576
ZERO_GT = bytes(GT_BYTES)
ONE_GT = B.gt_to_bytes(B.f12_one())

F2Z = (0, 0)
ZERO = (F2Z,) * 6
ONE = ((1, 0),) + (F2Z,) * 5

# regimes: the easy part is exactly 1 and every pow-by-x takes the Granger-Scott fallback; the normal
# path ending at exactly one; the normal path ending elsewhere; f = 0
FALLBACK, RTH, GENERIC, ZERO_KIND = "fallback", "rth", "generic", "zero"
KINDS = (FALLBACK, ZERO_KIND, RTH, GENERIC)


def f12(x):
    return tuple((int(a) % P, int(b) % P) for a, b in x)


def support_of(f):
    return tuple(k for k in range(6) if f[k] != F2Z)


def support_in_subfield_coset(sup):
    """The support lies in W^j times a proper subfield (over Fp2: Fp2 itself = {0}, Fp4 = {0, 3},
    Fp6 = {0, 2, 4}): such an element is killed by the easy part, W^j included."""
    s = set(sup)
    for j in range(6):
        for sub in ({0}, {0, 3}, {0, 2, 4}):
            if s <= {(k + j) % 6 for k in sub}:
                return True
    return False


def _f2(rnd):
    return (rnd.randrange(1, P), rnd.randrange(1, P))


def _dense(rnd):
    return tuple(_f2(rnd) for _ in range(6))


class Case:
    def __init__(self, name, family, f, kind, same_as=None):
        self.name, self.family, self.f, self.kind, self.same_as = name, family, f12(f), kind, same_as

    def __repr__(self):
        return f"Case({self.name})"


@functools.lru_cache(maxsize=None)
def cases():
    rnd = random.Random(0xFE12)
    out = []
    # supports: every non-empty support pattern with random non-zero coefficients
    for m in range(1, 64):
        sup = tuple(k for k in range(6) if m >> k & 1)
        f = tuple(_f2(rnd) if k in sup else F2Z for k in range(6))
        kind = FALLBACK if support_in_subfield_coset(sup) else GENERIC
        out.append(Case("sup" + "".join(map(str, sup)), "supports", f, kind))
    # ... and patterns of each regime with every non-zero Fp half p - 1, and with every one 1
    for sup in ((0, 1, 2, 3, 4, 5), (0, 1), (1, 3, 5), (2, 5), (4,)):
        kind = FALLBACK if support_in_subfield_coset(sup) else GENERIC
        for tag, v in (("pm1", P - 1), ("ones", 1)):
            f = tuple((v, v) if k in sup else F2Z for k in range(6))
            out.append(Case(f"sup{''.join(map(str, sup))}_{tag}", "supports", f, kind))
    # units: the 12 single-Fp basis elements and their negations
    for k in range(6):
        for h in range(2):
            for sign, v in (("+", 1), ("-", P - 1)):
                c = (v, 0) if h == 0 else (0, v)
                f = tuple(c if j == k else F2Z for j in range(6))
                out.append(Case(f"unit{sign}W{k}{'i' if h else ''}", "units", f, FALLBACK))
    # subfield: Fp, Fp2, Fp4 (the tower's a only: W^0, W^3) and Fp6 (W^0, W^2, W^4)
    out.append(Case("sub_fp", "subfield", ((rnd.randrange(2, P), 0),) + (F2Z,) * 5, FALLBACK))
    out.append(Case("sub_fp2", "subfield", (_f2(rnd),) + (F2Z,) * 5, FALLBACK))
    out.append(Case("sub_fp4", "subfield", tuple(_f2(rnd) if k in (0, 3) else F2Z for k in range(6)), FALLBACK))
    out.append(Case("sub_fp6", "subfield", tuple(_f2(rnd) if k in (0, 2, 4) else F2Z for k in range(6)), FALLBACK))
    out.append(Case("one", "one", ONE, FALLBACK))
    # scale: c f has the GT of f
    g = _dense(rnd)
    out.append(Case("scale_base", "scale", g, GENERIC))
    for tag, c in (("2", 2), ("pm1", P - 1), ("rnd", rnd.randrange(3, P - 1))):
        out.append(Case("scale_" + tag, "scale", tuple(B.f2_muls(x, c) for x in g), GENERIC, same_as="scale_base"))
    # rth-power: h^r, whose GT is exactly one through the normal path
    for k in range(2):
        out.append(Case(f"rth{k}", "rth-power", B.f12_pow(list(_dense(rnd)), B.R), RTH))
    for k in range(3):
        out.append(Case(f"generic{k}", "generic", _dense(rnd), GENERIC))
    out.append(Case("zero", "zero", ZERO, ZERO_KIND))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def of_kind(kind):
    return [c for c in cases() if c.kind == kind]


@functools.lru_cache(maxsize=None)
def expected(f):
    """(GT bytes, GT == 1) of the oracle for one input; f = 0 gives the all-zero GT the order-13 twist
    point already pins (tests/test_gpu_torsion_edges.py; the oracle's inversion raises on 0)."""
    if f == ZERO:
        return ZERO_GT, False
    gt = B.gt_to_bytes(B.final_exp(list(f)))
    return gt, gt == ONE_GT


# ---------------------------------------------------------------- the kernels' input form
def _fp_words(x):
    v = x * R_STORE % P
    return [(v >> (32 * w)) & 0xFFFFFFFF for w in range(NW)]


@functools.lru_cache(maxsize=None)
def element_words(f):
    """The 144 words of one element, Fp slot major: slot 2 s + h is half h of AMCL Fp2 slot s."""
    out = []
    for s in range(6):
        c = f[B.AMCL_SLOT_TO_W[s]]
        out += _fp_words(c[0]) + _fp_words(c[1])
    return np.array(out, dtype=np.uint32)


def encode(fs):
    """Structure of arrays of a batch: word ((k * 12 + w) * n + i) is word w of Fp slot k of element i."""
    n = len(fs)
    a = np.empty((F12_WORDS, n), dtype=np.uint32)
    for i, f in enumerate(fs):
        a[:, i] = element_words(f12(f))
    return np.ascontiguousarray(a.reshape(-1))


def decode(words, n):
    """Inverse of encode; every stored Fp value must be canonical."""
    a = np.asarray(words, dtype=np.uint32).reshape(F12_WORDS, n)
    out = []
    for i in range(n):
        fp = []
        for k in range(12):
            v = sum(int(a[k * NW + w, i]) << (32 * w) for w in range(NW))
            assert v < P, "non-canonical stored value"
            fp.append(v * R_STORE_INV % P)
        f = [None] * 6
        for s in range(6):
            f[B.AMCL_SLOT_TO_W[s]] = (fp[2 * s], fp[2 * s + 1])
        out.append(tuple(f))
    return out
