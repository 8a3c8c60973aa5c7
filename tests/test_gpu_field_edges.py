"""The canonical 12 x 32 Fp (csrc/field.h, through the out-of-line fp_mul_call), its Fp2 helpers and the
scalar field (csrc/fr.h, csrc/codec.h) on the device, at their edges.

cc_selftest_field (csrc/selftest.hip) runs the project's own functions one row per lane.  Every op runs
on its list from tests/field_edges.py (tests/test_field_edges_model.py shows on the CPU which branch each
row takes), padded with seeded random rows to a multiple of 256 plus one so that a second block and a
partial block run, and every output word is compared with the Python-integer expectation; words beyond a
result's width must be zero.
"""
import ctypes

import numpy as np
import pytest

import field_edges as F

pytestmark = pytest.mark.gpu
P, R = F.P, F.R


def run(op, a, b=None, out_rows=1):
    """One cc_selftest_field call on rows of integers (or of 12 words); returns the out_rows * n output
    rows as 12-word lists.  The output is filled with 0xC3 first: every word must be written."""
    from coconut._lib import lib
    n = len(a)
    assert n == F.padded(n - 1) and n % 256 == 1, n
    ha = np.array([x if isinstance(x, list) else F.words(x) for x in a], dtype=np.uint32)
    hb = None if b is None else np.array([F.words(x) for x in b], dtype=np.uint32)
    assert ha.shape == (n, F.NW) and (hb is None or hb.shape == (n, F.NW))
    out = np.full((out_rows * n, F.NW), 0xC3C3C3C3, dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.cc_selftest_field(op, n, ptr(ha), ptr(hb), ptr(out)) == 0
    return [[int(w) for w in row] for row in out]


def check(op, a, b, want, width=F.NW):
    got = run(op, a, b)
    for k, (row, w) in enumerate(zip(got, want)):
        assert row == F.words(w, width) + [0] * (F.NW - width), (op, k, hex(F.value(row)), hex(w))


def _fp_pairs(rows, seed):
    rows = F.pad(rows, lambda g: (F.rand_fp(g), F.rand_fp(g)), seed)
    return [a for a, _ in rows], [b for _, b in rows]


def _fr_pairs(rows, seed):
    rows = F.pad(rows, lambda g: (F.rand_fr(g), F.rand_fr(g)), seed)
    return [a for a, _ in rows], [b for _, b in rows]


# ---------------------------------------------------------------- Fp
def test_fp_add_sub_neg_dbl():
    a, b = _fp_pairs([(x, y) for _, x, y in F.fp_add_rows()], 1)
    check(F.FP_ADD, a, b, [(x + y) % P for x, y in zip(a, b)])
    a, b = _fp_pairs([(x, y) for _, x, y in F.fp_sub_rows()], 2)
    check(F.FP_SUB, a, b, [(x - y) % P for x, y in zip(a, b)])
    a = F.pad([x for _, x in F.fp_neg_rows()], F.rand_fp, 3)
    check(F.FP_NEG, a, None, [-x % P for x in a])
    a = F.pad([x for _, x in F.fp_dbl_rows()], F.rand_fp, 4)
    check(F.FP_DBL, a, None, [2 * x % P for x in a])


def test_fp_mul_sqr_and_the_montgomery_conversions():
    a, b = _fp_pairs(F.fp_mul_rows(), 5)
    check(F.FP_MUL, a, b, [F.fp_mul_expected(x, y) for x, y in zip(a, b)])
    a = F.pad(F.fp_sqr_rows(), F.rand_fp, 6)
    check(F.FP_SQR, a, None, [F.fp_mul_expected(x, x) for x in a])
    a = F.pad(F.FP_OPERANDS, F.rand_fp, 7)
    check(F.FP_TO_MONT, a, None, [x * F.RP % P for x in a])
    check(F.FP_FROM_MONT, a, None, [x * F.RPINV % P for x in a])


def test_fp_raw_reduce():
    a = F.pad(F.fp_raw_rows(), lambda g: g.randrange(1 << 384), 8)
    check(F.FP_RAW_REDUCE, a, None, [x % P for x in a])


def test_fp_inv_and_fr_inversions_on_the_inversion_lists():
    """fp_inv (x^-1 R^2 with CC_R3_LIMBS), fr_inv_int (plain) and fm_inv (x^-1 R^2 with R3) over the lists
    whose rows reach every batch count and correction of the divstep loops."""
    a = F.pad(F.inv_list(P), F.rand_fp, 9)
    check(F.FP_INV, a, None, [pow(x, -1, P) * F.RP * F.RP % P if x else 0 for x in a])
    a = F.pad(F.inv_list(R), F.rand_fr, 10)
    check(F.FR_INV_INT, a, None, [pow(x, -1, R) if x else 0 for x in a], 8)
    check(F.FM_INV, a, None, [pow(x, -1, R) * F.RR * F.RR % R if x else 0 for x in a], 8)


def _lazy_rows(vals):
    rows = [F.words(v) + [0, 0] for v in vals]
    return np.array(rows, dtype=np.uint32).view(np.int32)


def _lazy(op, rows):
    from coconut._lib import lib
    out = np.full(rows.shape, -1, dtype=np.int32)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.cc_selftest_lazy(op, len(rows), ptr(rows), None, None, None, ptr(out)) == 0
    return [[int(w) for w in row] for row in out.view(np.uint32)]


def test_fp_inv_int_and_its_quad_form_on_the_inversion_list():
    """cc_selftest_lazy ops 4 (field.h fp_inv_int) and 5 (tower_q.h fp_inv_int_quad, one value a quad)
    over the p list, ordered by field_edges.quad_order(): the one-batch input and a largest-count input
    in adjacent quads of a half-wave and across the two halves of a wave."""
    vals = F.pad(F.quad_order(), F.rand_fp, 11)
    want = [F.words(pow(v, -1, P) if v else 0) + [0, 0] for v in vals]
    assert _lazy(4, _lazy_rows(vals)) == want
    quads = [v for v in vals[:len(vals) - 1] for _ in range(4)]        # whole quads, whole waves
    assert len(quads) % 64 == 0
    assert _lazy(5, _lazy_rows(quads)) == [w for w in want[:len(vals) - 1] for _ in range(4)]


# ---------------------------------------------------------------- Fp2
def _f2(op, rows):
    n = len(rows)
    got = run(op, [x for x, _ in rows], [y for _, y in rows], out_rows=2)
    return [(F.value(got[k]), F.value(got[n + k])) for k in range(n)]


def test_f2_mul_sqr_inv_mul_xi():
    rows = F.pad(F.f2_rows(), lambda g: (F.rand_fp(g), F.rand_fp(g)), 12)
    n = len(rows)
    assert _f2(F.F2_MUL, rows) == [F.f2_mul_expected(rows[k], rows[(k + 1) % n]) for k in range(n)]
    assert _f2(F.F2_SQR, rows) == [F.f2_mul_expected(x, x) for x in rows]
    assert _f2(F.F2_MUL_XI, rows) == [((x - y) % P, (x + y) % P) for x, y in rows]
    inv = _f2(F.F2_INV, rows)
    assert inv == [F.f2_inv_expected(x) for x in rows]
    for x, y in zip(rows, inv):   # multiplied back: the Montgomery one, or 0 for 0
        assert F.f2_mul_expected(x, y) == ((F.RP % P, 0) if x != (0, 0) else (0, 0))


# ---------------------------------------------------------------- Fr
def test_fm_mul_sub_and_the_canonical_product():
    a, b = _fr_pairs(F.FR_PAIRS, 13)
    check(F.FM_MUL, a, b, [x * y * F.RRINV % R for x, y in zip(a, b)], 8)
    check(F.FM_SUB, a, b, [(x - y) % R for x, y in zip(a, b)], 8)
    check(F.FR_MUL_CANON, a, b, [x * y % R for x, y in zip(a, b)], 8)


def test_fm_reduce_once_to_canon_from_u64():
    a = F.pad([s for _, s in F.fr_sum_rows()], lambda g: F.rand_fr(g) + F.rand_fr(g), 14)
    check(F.FM_REDUCE_ONCE, a, None, [s - R if s >= R else s for s in a], 8)
    a = F.pad(F.FR_OPERANDS, F.rand_fr, 15)
    check(F.FM_TO_CANON, a, None, [x * F.RRINV % R for x in a], 8)
    a = F.pad(F.U64_ROWS, lambda g: g.randrange(1 << 64), 16)
    check(F.FM_FROM_U64, a, None, [x * F.RR % R for x in a], 8)


def test_rlc_delta_abs():
    d = F.pad(F.delta_rows(), F.rand_delta, 17)
    check(F.RLC_DELTA_ABS, [x % R for x in d], None, [abs(x) | (int(x < 0) << 256) for x in d], 9)


def test_fr_from_be48():
    v = F.pad(F.be48_rows(), lambda g: g.randrange(1 << g.choice((255, 256, 300, 384))), 18)
    check(F.FR_FROM_BE48, [F.be48_words(x) for x in v], None, [x % R for x in v], 8)


def test_bad_ops_and_empty_calls_are_rejected():
    from coconut._lib import lib
    buf = np.zeros((1, F.NW), dtype=np.uint32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.cc_selftest_field(-1, 1, p, p, p) == -1
    assert lib.cc_selftest_field(24, 1, p, p, p) == -1
    assert lib.cc_selftest_field(0, 0, p, p, p) == -1
