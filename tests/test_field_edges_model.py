"""CPU checks of tests/field_edges.py: the committed inputs reach every branch and boundary they are
built for, and the Python restatement of the divstep inversion agrees with pow() on all of them.  No
product code runs here; tests/test_gpu_field_edges.py and tests/test_gpu_lagrange_direct.py run the same
lists on the device."""
import ctypes
import random

import pytest

import field_edges as F

P, R = F.P, F.R
MODULI = [pytest.param(R, id="r"), pytest.param(P, id="p")]


# ---------------------------------------------------------------- constants
def test_moduli_and_radices_are_the_products():
    from oracle import bls12_381 as B
    assert B.P == P and B.R == R
    # field.h CC_ONE_LIMBS / CC_R2_LIMBS / CC_R3_LIMBS and fr.h CC_RONE / CC_RR2 / R3, low words
    assert F.RP % P & F.M32 == 0x03a9fb84 and F.RP ** 2 % P & F.M32 == 0xd5bef7ae and F.RP ** 3 % P & F.M32 == 0x49217d6a
    assert F.RR % R & F.M32 == 0xfffffffe and F.RR ** 2 % R & F.M32 == 0xf3f29c6d and F.RR ** 3 % R & F.M32 == 0x439b73af
    assert pow(P, -1, 1 << 30) == 0x30003 and pow(R, -1, 1 << 30) == 1   # PINV30; "r^-1 = 1 mod 2^30"


# ---------------------------------------------------------------- the inversion lists
@pytest.mark.parametrize("m", MODULI)
def test_inversion_list_contents(m):
    vals = set(F.inv_list(m))
    assert len(vals) == len(F.inv_list(m)) and 300 < len(vals) < 1500
    assert {0, 1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2} <= vals
    for k in range(m.bit_length()):
        assert 1 << k in vals and m - (1 << k) in vals and (1 << k) - 1 in vals
    for x in (2, 3, 5, 7, 255, 256, 257, 1 << 30, (1 << 30) + 1, (1 << 60) - 1):
        assert pow(x, -1, m) in vals
    assert sum(1 for v in vals if v and v & F.M30 == 0 and v & (v - 1)) >= 8   # low limb zero, not a power of two
    assert sum(1 for v in vals if v and v & ((1 << 60) - 1) == 0 and v & (v - 1)) >= 4
    phi = [v for v in vals if abs(v * 1618033988749895 - m * 10 ** 15) < m]     # |v - m / phi| tiny
    assert len(phi) >= 9


@pytest.mark.parametrize("m", MODULI)
def test_inversion_model_agrees_with_pow_and_stays_in_range(m):
    for v, (x, batches, _, in_range) in zip(F.inv_list(m), F.inv_classes(m)):
        assert x == (pow(v, -1, m) if v else 0), v
        assert in_range, v          # d and e inside (-2m, m) after every batch
        assert (batches == 1) == (v == 0) or v == 1, v


@pytest.mark.parametrize("m,bound,lo,hi", [pytest.param(R, 30, 17, 19, id="r"), pytest.param(P, 40, 26, 28, id="p")])
def test_inversion_list_reaches_every_batch_count_and_correction(m, bound, lo, hi):
    """bound: the kernel's loop bound (fr.h fr_inv_int `it < 30`, field.h fp_inv_int `it < 40`)."""
    assert F.LOOP_BOUND[m] == bound
    vals, cls = F.inv_list(m), F.inv_classes(m)
    assert cls[0][1] == 1 and vals[0] == 0                      # the one-batch exit of a = 0
    counts = {c[1] for v, c in zip(vals, cls) if v}
    assert counts == set(range(lo, hi + 1)), sorted(counts)    # every count between the extremes observed
    assert max(counts) <= bound - 10
    combos = {c[2] for c in cls}
    # (f negative, number of +m, final -m): the set the model reports over the list, written out
    assert combos == {(False, 0, False), (False, 1, False), (False, 2, False), (True, 0, False), (True, 0, True),
                      (True, 1, False)} == F.COMBOS
    for want in F.COMBOS:
        assert sum(1 for c in cls if c[2] == want) >= 3, want


def test_quad_order_pairs_the_extremes_within_and_across_half_waves():
    order, by = F.quad_order(), dict(zip(F.inv_list(P), F.inv_classes(P)))
    assert sorted(set(order)) == sorted(F.inv_list(P)) and len(order) == len(F.inv_list(P)) + 2
    top = max(c[1] for c in by.values())
    # quad q of the first wave covers lanes 4q..4q+3; lanes 0..31 are one half
    assert by[order[0]][1] == 1 and by[order[1]][1] == top      # quads 0 | 1: adjacent, lanes 0..7
    assert by[order[7]][1] == 1 and by[order[8]][1] == top      # quads 7 | 8: lanes 28..31 | 32..35
    assert 4 * 7 + 3 == 31 and 4 * 8 == 32 and len(order) > 16


def test_divsteps30_matrix_property():
    """2^30 [f', g'] = t [f, g] on the low words, entries within 32 bits signed, for random odd f."""
    rng = random.Random(3)
    for _ in range(300):
        f, g, eta = rng.randrange(1 << 30) | 1, rng.randrange(1 << 30), rng.randrange(-40, 40)
        eta2, (u, v, q, r) = F.divsteps30(eta, f, g)
        assert (u * f + v * g) % (1 << 30) == 0 and (q * f + r * g) % (1 << 30) == 0
        assert abs(u * r - v * q) == 1 << 30 and all(abs(t) <= 1 << 30 for t in (u, v, q, r))


# ---------------------------------------------------------------- Fp
def test_fp_operands_hold_the_named_values():
    ops = set(F.FP_OPERANDS)
    assert {0, 1, P - 1, F.RP % P, F.RP ** 2 % P} <= ops
    assert all(1 << (29 * k) in ops for k in range(14))
    m29 = (1 << 29) - 1
    full = [x for x in ops if all((x >> (29 * k)) & m29 == m29 for k in range(13))]
    assert full and full[0] + (1 << 377) >= P                   # all limbs ones, the top limb clipped below p
    assert any(all(w == F.M32 for w in F.words(x)[:11]) and F.words(x)[11] for x in ops)
    assert (1 << 352) - 1 in ops


def test_fp_product_rows_sit_on_both_sides_of_p():
    rows = F.fp_mul_rows()
    ts = [F.mont_t(a, b) for a, b in rows]
    assert all(a < 1 << 384 and b < 1 << 384 and t < 2 * P for (a, b), t in zip(rows, ts))
    assert sum(t < P for t in ts) > 400 and sum(P <= t < 2 * P for t in ts) >= 10
    assert sum(P < t for (a, b), t in zip(rows, ts) if a < P and b < P) >= 5      # canonical operands too
    for want in (0, P, P - 1):
        assert sum(t == want for t in ts) >= 2, want
    for (a, b), t in zip(rows, ts):
        assert F.fp_mul_expected(a, b) == (t - P if t >= P else t)
        if t == P:
            assert F.fp_mul_expected(a, b) == 0
    sq = [F.mont_t(a, a) for a in F.fp_sqr_rows()]
    assert P in sq and P + 1 in sq and P + 4 in sq and 0 in sq and sum(t < P for t in sq) > 20 and max(sq) < 2 * P


def test_fp_add_sub_neg_dbl_rows_take_both_branches():
    add = {n: ("reduced" if a + b >= P else "plain") for n, a, b in F.fp_add_rows()}
    assert all(a < P and b < P for _, a, b in F.fp_add_rows())
    assert add["sum p-1"] == add["halves p-1"] == add["0+0"] == add["carry through eleven words"] == "plain"
    assert add["sum p"] == add["sum p+1"] == add["halves p"] == add["(p-1)+(p-1)"] == "reduced"
    assert {a + b for _, a, b in F.fp_add_rows()} >= {P - 1, P, P + 1, 2 * P - 2, 0, 1 << 352}
    assert set(add.values()) == {"reduced", "plain"}
    sub = {n: ("borrowed" if a < b else "plain") for n, a, b in F.fp_sub_rows()}
    assert all(a < P and b < P for _, a, b in F.fp_sub_rows())
    assert sub["a=b=0"] == sub["a=b=p-1"] == sub["borrow through eleven words"] == "plain"
    assert sub["a=b-1 low"] == sub["a=b-1 top"] == sub["0-(p-1)"] == sub["its mirror"] == "borrowed"
    assert F.words((1 << 352) - 1)[:11] == [F.M32] * 11        # 2^352 - 1: the borrow ran through eleven words
    assert set(sub.values()) == {"borrowed", "plain"}
    neg = {n: ("zero" if a == 0 else "nonzero") for n, a in F.fp_neg_rows()}
    assert neg["0"] == "zero" and neg["1"] == neg["p-1"] == "nonzero" and set(neg.values()) == {"zero", "nonzero"}
    dbl = {n: ("reduced" if 2 * a >= P else "plain") for n, a in F.fp_dbl_rows()}
    assert dbl["(p-1)/2"] == "plain" and dbl["(p+1)/2"] == "reduced" and set(dbl.values()) == {"reduced", "plain"}


def test_fp_raw_rows():
    rows = F.fp_raw_rows()
    assert all(v < 1 << 384 for v in rows) and (1 << 384) - 1 in rows
    assert {v // P for v in rows} == set(range(10)) and 9 * P + 1 in rows and 9 * P + P - 1 not in rows
    assert {0, 1, P - 1, P, P + 1, 2 * P - 1} <= set(rows)


def test_f2_rows_are_canonical_and_invertible():
    for x in F.f2_rows():
        assert x[0] < P and x[1] < P
        inv = F.f2_inv_expected(x)
        if x == (0, 0):
            assert inv == (0, 0)
        else:
            assert F.f2_mul_expected(inv, x) == (F.RP % P, 0)   # the Montgomery one
    assert (0, 0) in F.f2_rows()


# ---------------------------------------------------------------- Fr
def test_fr_rows():
    ops = set(F.FR_OPERANDS)
    assert {0, 1, R - 1, F.RR % R, F.RR ** 2 % R, (1 << 64) - 1, 1 << 32} <= ops
    assert any(F.words(x, 8)[:7] == [F.M32] * 7 and F.words(x, 8)[7] for x in ops)
    assert {(1 << 64) - 1, 1 << 32, 0, 1} <= set(F.U64_ROWS)
    sums = dict(F.fr_sum_rows())
    assert {sums[k] for k in ("r-1", "r", "r+1", "2r-2")} == {R - 1, R, R + 1, 2 * R - 2}
    assert all(s <= 2 * R - 2 < 1 << 256 for s in sums.values())
    assert {s >= R for s in sums.values()} == {True, False}


def test_be48_rows_sit_on_every_step_of_the_slow_reduction():
    rows = set(F.be48_rows())
    for s in range(130):
        assert R << s in rows and (R << s) - 1 in rows
        assert ((R << s) + 1 in rows) == ((R << s) + 1 < 1 << 384)
    assert (R << 129) < 1 << 384 < (R << 130)
    assert {1 << 255, (1 << 256) - 1, 1 << 256, (1 << 384) - 1, 0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 3 * R - 1} <= rows
    fast = {v < R for v in rows}        # hi words zero and the low 256 bits below r
    assert fast == {True, False}
    assert all(v < 1 << 384 for v in rows)
    assert F.be48_words(1) == [0] * 11 + [1 << 24] and F.be48_words(0x0102 << 368)[0] == 0x0201


def test_delta_rows():
    rows = F.delta_rows()
    hi, lo = sum(127 << (8 * w) for w in range(16)), sum(-128 << (8 * w) for w in range(16))
    assert {0, 1, -1, 1 << 127, -(1 << 127), 1 << 128, -(1 << 128), hi, lo} <= set(rows)
    for d in rows:
        neg = any(F.words(d % R, 8)[5:])            # the kernel's test: a word above bit 160 set
        assert neg == (d < 0) and abs(d) < 1 << 136


# ---------------------------------------------------------------- k_lagrange
def test_the_lds_switch_from_the_launchers_expression():
    t = F.largest_lds_t()
    assert t == 4032 and F.lds_bytes(t) == 65536 and F.lds_bytes(t + 1) == 65552


def test_lagrange_small_cases_cover_the_shapes():
    cases = F.small_cases()
    assert {t for t, _, _ in cases} == set(F.SMALL_T)
    tasks = {n * t for t, n, _ in cases}
    assert {127, 128, 129} <= tasks
    for t in F.SMALL_T:
        mine = [(n, ln) for tt, n, ln in cases if tt == t]
        assert {ln for _, ln in mine} == {t, t + 3}
        if t % 2:
            assert {n * t % 2 for n, _ in mine} == {0, 1}
        assert any(n * t > F.BLOCK_TASKS for n, _ in mine) and any(n * t <= F.BLOCK_TASKS + 1 for n, _ in mine)
        kinds, ids = F.small_ids(t, 12, t + 3)
        assert kinds == list(F.KINDS) and all(len(r) == t + 3 for r in ids)
        if t >= 3:
            first = [r[:t] for r in ids]
            assert first[1][0] == 0 and first[4][t - 1] == 0 and first[8][t // 2] == 0 and 0 < t // 2 < t - 1
            assert first[3][0] == first[3][t - 1] and len(set(first[3])) == t - 1
            assert first[6][0] == first[6][t // 2] == first[6][t - 1] and len(set(first[6])) == t - 2
            assert first[10][0] == first[10][t - 1] == 0
            assert all(len(set(first[c])) == t and 0 not in first[c] for c in (0, 2, 5, 7, 9, 11))
            if t % 2:   # credentials 2k and 2k + 1 share the lane of tasks (2k + 1) t - 1 | (2k + 1) t
                assert 0 in first[1] and 0 not in first[0]                       # with 0 | without, one lane
                assert len(set(first[3])) < t and len(set(first[2])) == t       # repeats | none, one lane
    used = {x for t, n, ln in cases for r in F.small_ids(t, n, ln)[1] for x in r[:t]}
    assert set(F.EDGE_IDS) <= used and any(x >> 32 for x in used)
    _, ids = F.small_ids(9, 12, 9)
    assert any(a > b and a >> 32 == b >> 32 for r in ids for a in r for b in r)   # differ in the low word only
    assert any(a >> 32 != b >> 32 and a & F.M32 == b & F.M32 for a in F.EDGE_IDS for b in F.EDGE_IDS)


def test_python_lagrange_agrees_with_the_oracle_and_the_power_sums(oc):
    for t, n, ln in ((5, 12, 8), (9, 12, 9)):
        for row in F.small_ids(t, n, ln)[1]:
            ids = row[:t]
            out = ctypes.create_string_buffer(48 * t)
            oc.oc_lagrange(ctypes.c_size_t(t), (ctypes.c_uint64 * t)(*ids), out)
            got = [int.from_bytes(out.raw[48 * k:48 * (k + 1)], "big") for k in range(t)]
            assert got == [F.lagrange_at(ids, i) for i in range(t)]
            first = {x: got[ids.index(x)] for x in F.first_occurrences(ids)}
            for k in range(min(4, len(first))):
                assert sum(l * pow(x, k, R) for x, l in first.items()) % R == (k == 0)


def test_switch_samples():
    t = F.largest_lds_t()
    for tt in (t, t + 1):
        for n in (1, 2):
            rows = F.switch_ids(tt, n)
            assert all(len(r) == tt + 1 for r in rows) and rows[0][5] == rows[0][tt - 3]
            s = F.switch_samples(tt, n, rows)
            assert 128 <= len(s) == len(set(s)) <= 131 and {0, n * tt - 1, 5, tt - 3} <= set(s)
            for e in range(F.BLOCK_TASKS, n * tt, F.BLOCK_TASKS):
                assert e - 1 in s and e in s
            if n == 2:
                assert rows[1][7] == 0 and tt + 7 in s
