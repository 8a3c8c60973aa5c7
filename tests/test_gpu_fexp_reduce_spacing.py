"""The quad final exponentiation alone (csrc/fexp_q.hip k_fexp_q) around its compressed-squaring runs and
their value reductions: a pow-by-x is 16 + 32 + 9 compressed squarings with the snapshots g^(2^16), g^(2^48)
and g^(2^57) between the runs, so the inputs here are the ones whose compressed states are extreme or
degenerate.  (Spacing the value reductions three squarings apart was measured and not kept,
profiles/r07/valu_trim; any respacing has to pass this file.)

Inputs: 1 and -1; a non-trivial element of Fp, of Fp2 and of Fp6 (the easy part sends these five to 1, and
every pow-by-x then takes the zero-denominator fallback: tests/fexp_direct_cases.py kind FALLBACK, with
further members of that kind); 0; Miller values of a valid credential (the product of the Miller values of
(a P, Q) and (-P, a Q): GT exactly one through the normal path) and of corrupted ones (the second pair's Q
replaced; and values the Miller kernels recorded in tests/golden/miller_lz_words.json), all through the
normal path.  Sizes n = 1, 17 (16 quads a wave) and 65 (64 quads a block), the inputs rotating element by
element so that quads of one wave take different paths.  GT bytes against the oracle's final
exponentiation; each verdict is "GT == 1 and (flags & 11) == 0"; the verdicts with a null GT buffer are
the same.  The expectations and every input's regime are asserted on the CPU first (test_inputs).
"""
import functools
import json
import os

import numpy as np
import pytest

import fexp_direct_cases as C
import miller_wide_cases as W
from oracle import bls12_381 as B

MINUS_ONE = ((C.P - 1, 0),) + (C.F2Z,) * 5
FLAG_WORDS = (0, 1, 2, 4, 8, 16, 32, 11)
SIZES = (1, 17, 65)


@functools.lru_cache(maxsize=None)
def inputs():
    """((name, f, GT is one), ...)."""
    pr = W.pairs()
    (ap0, q0), (p0, aq0), (_, q1) = pr[W.NPAIR - 2], pr[W.NPAIR - 1], pr[2]  # (A P0, Q0), (P0, A Q0)
    m0 = B.miller_loop(q0, ap0)
    valid = C.f12(B.f12_mul(m0, B.miller_loop(aq0, B.G1.neg(p0))))
    corrupted = C.f12(B.f12_mul(m0, B.miller_loop(q1, B.G1.neg(p0))))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "miller_lz_words.json")
    with open(path) as f:
        rec = json.load(f)["words"]
    words = lambda k, e: np.frombuffer(bytes.fromhex(rec[k][e]), dtype="<u4")  # noqa: E731
    out = [("one", C.ONE, True), ("minus_one", MINUS_ONE, True)]
    out += [(x, C.by_name(x).f, True) for x in ("sub_fp", "sub_fp2", "sub_fp6")]
    out += [("zero", C.ZERO, False), ("valid", valid, True), ("corrupted", corrupted, False)]
    out += [(f"recorded_{k}{e}", C.decode(words(k, e), 1)[0], False) for k, e in (("lz_g2", 0), ("lz_g1", 3), ("quad", 7))]
    out += [(x, C.by_name(x).f, True) for x in ("sub_fp4", "sup024", "unit-W5i", "sup135_pm1", "rth0")]
    out += [(x, C.by_name(x).f, False) for x in ("generic0", "sup01")]
    return tuple(out)


def batch(n, rot):
    ins = inputs()
    pick = [ins[(i + rot) % len(ins)] for i in range(n)]
    flags = [FLAG_WORDS[(i // 2 + rot) % len(FLAG_WORDS)] for i in range(n)]
    return [f for _, f, _ in pick], [x for x, _, _ in pick], flags


def rotations(n):
    return range(len(inputs())) if n == 1 else (0, 7)


def test_inputs():
    ins = inputs()
    assert len({x for x, _, _ in ins}) == len({f for _, f, _ in ins}) == len(ins)
    for name, f, one in ins:
        gt, is_one = C.expected(f)
        assert is_one == one and (gt == C.ONE_GT) == one, name
    by = {x: f for x, f, _ in ins}
    # the easy part f^((p^6 - 1)(p^2 + 1)) of the subfield elements is exactly one: the fallback's regime
    for name in ("one", "minus_one", "sub_fp", "sub_fp2", "sub_fp6", "sub_fp4", "sup024", "unit-W5i", "sup135_pm1"):
        f = list(by[name])
        t = B.f12_mul(B.f12_conj(f), B.f12_inv(f))
        assert B.f12_is_one(B.f12_mul(B.f12_frob(B.f12_frob(t)), t)), name
        assert name in ("one", "minus_one") or C.by_name(name).kind == C.FALLBACK
    assert by["sub_fp"][0][1] == 0 and by["sub_fp"][0][0] not in (0, 1, C.P - 1) and C.support_of(by["sub_fp"]) == (0,)
    assert by["sub_fp2"][0][1] != 0 and C.support_of(by["sub_fp2"]) == (0,)
    assert C.support_of(by["sub_fp6"]) == (0, 2, 4)
    for name in ("valid", "corrupted", "recorded_lz_g20", "rth0", "generic0"):  # the normal path: easy part not one
        f = list(by[name])
        t = B.f12_mul(B.f12_conj(f), B.f12_inv(f))
        assert not B.f12_is_one(B.f12_mul(B.f12_frob(B.f12_frob(t)), t)), name
    assert C.expected(C.ZERO) == (C.ZERO_GT, False)
    for n in SIZES:  # every input and every flag word at every size
        names, flags = set(), set()
        for rot in rotations(n):
            _, nm, fl = batch(n, rot)
            names |= set(nm)
            flags |= set(fl)
        assert names == set(by), n
        assert n == 1 or flags == set(FLAG_WORDS)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_quad_fexp(n):
    import test_gpu_fexp_direct as D
    from coconut._lib import lib
    sz, p, i = D.ctypes.c_size_t, D.ctypes.c_void_p, D.ctypes.c_int
    lib.cck_fexp_q.argtypes, lib.cck_fexp_q.restype = [sz, p, p, p, p, p], i
    for rot in rotations(n):
        fs, names, flags = batch(n, rot)
        exp = [C.expected(f) for f in fs]
        v, gt = D.run_fexp(lib, "quad", fs, flags, want_gt=True)
        for k in range(n):
            assert gt[576 * k:576 * (k + 1)] == exp[k][0], (n, rot, k, names[k])
            assert v[k] == int(gt[576 * k:576 * (k + 1)] == C.ONE_GT and (flags[k] & 11) == 0), (n, rot, k, names[k])
            assert v[k] == int(exp[k][1] and (flags[k] & 11) == 0)
        v2, none = D.run_fexp(lib, "quad", fs, flags, want_gt=False)
        assert none is None and v2 == v, (n, rot)
