"""Inputs at the edges of the scalar field (csrc/fr.h, csrc/codec.h), of the canonical 12 x 32 Fp
(csrc/field.h) and of k_lagrange (csrc/aggregate.hip), with what each must give in Python integers.

Everything here is deterministic and uses `pow` and `%` only for expected values.  inv_model() restates
the divstep inversion (fp_inv_int / fr_inv_int: batches of 30 divsteps, the matrix applied to f, g and
to d, e with the multiple of m that makes the division exact, the final corrections) from the
algorithm; it classifies inputs (batch count, corrections taken) and never produces an expected value.
tests/test_field_edges_model.py asserts on the CPU that the lists reach the branches they are built
for; tests/test_gpu_field_edges.py and tests/test_gpu_lagrange_direct.py run them on the device.
"""
import functools
import math
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
RP_BITS, RR_BITS = 406, 256          # the Montgomery radices of field.h and fr.h
RP, RR = 1 << RP_BITS, 1 << RR_BITS
RPINV, RRINV = pow(RP, -1, P), pow(RR, -1, R)
NW = 12                               # words a row
M32 = 0xFFFFFFFF

# cc_selftest_field ops (csrc/selftest.hip FieldOp)
(FP_ADD, FP_SUB, FP_NEG, FP_DBL, FP_MUL, FP_SQR, FP_TO_MONT, FP_FROM_MONT, FP_RAW_REDUCE, FP_INV, F2_MUL, F2_SQR,
 F2_INV, F2_MUL_XI, FM_MUL, FM_SUB, FM_REDUCE_ONCE, FM_FROM_U64, FM_TO_CANON, FR_MUL_CANON, FR_INV_INT, FM_INV,
 RLC_DELTA_ABS, FR_FROM_BE48) = range(24)


def words(v, n=NW):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * k)) & M32 for k in range(n)]


def value(ws):
    return sum(int(w) << (32 * k) for k, w in enumerate(ws))


def padded(n):
    """The row count a list of n rows is padded to: a multiple of 256 plus one, above n."""
    return (n + 255) // 256 * 256 + 1


def pad(rows, draw, seed):
    """rows + seeded random rows (draw(rng)) up to padded(len(rows)): a second block and a partial block."""
    rng = random.Random(seed)
    return list(rows) + [draw(rng) for _ in range(padded(len(rows)) - len(rows))]


# ---------------------------------------------------------------- the divstep inversion, restated
M30 = (1 << 30) - 1
LOOP_BOUND = {R: 30, P: 40}   # the kernels' loop bounds (fr.h fr_inv_int, field.h fp_inv_int)


def _s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def divsteps30(eta, f, g):
    """30 divsteps on the low words of f and g (f odd): zero runs of g at once, otherwise up to 8 low
    bits of g cancelled by one multiple of f.  Returns eta and the matrix (u, v, q, r), 32-bit signed,
    with 2^30 [f', g'] = [[u, v], [q, r]] [f, g]."""
    u, v, q, r, i = 1, 0, 0, 1, 30
    while True:
        x = (g | (M32 << i)) & M32
        zeros = (x & -x).bit_length() - 1
        g >>= zeros
        u, v = (u << zeros) & M32, (v << zeros) & M32
        eta -= zeros
        i -= zeros
        if i == 0:
            break
        if eta < 0:
            eta = -eta
            f, g = g, -f & M32
            u, q = q, -u & M32
            v, r = r, -v & M32
        limit = min(eta + 1, i)
        mask = (M32 >> (32 - limit)) & 255
        fi = (3 * f ^ 2) & M32                 # f^-1 to 5 bits; one Newton step gives 10
        fi = fi * (2 - f * fi) & M32
        w = g * (-fi & M32) & mask
        g = (g + f * w) & M32
        q = (q + u * w) & M32
        r = (r + v * w) & M32
    return eta, tuple(_s32(t) for t in (u, v, q, r))


def inv_model(a, m):
    """The inversion of a mod m as the kernels run it.  Returns (x, batches, (f negative, number of +m,
    final -m), in_range) with in_range: d and e stayed inside (-2m, m) after every batch."""
    assert 0 <= a < m
    minv = pow(m, -1, 1 << 30)
    d, e, f, g, eta = 0, 1, m, a, -1
    batches, in_range = 0, True
    for _ in range(LOOP_BOUND[m]):
        eta, (u, v, q, r) = divsteps30(eta, f & M30, g & M30)
        md = (u if d < 0 else 0) + (v if e < 0 else 0)
        me = (q if d < 0 else 0) + (r if e < 0 else 0)
        cd, ce = u * d + v * e, q * d + r * e
        md -= (minv * cd + md) & M30
        me -= (minv * ce + me) & M30
        cd, ce = cd + m * md, ce + m * me
        assert cd & M30 == 0 and ce & M30 == 0
        d, e = cd >> 30, ce >> 30
        nf, ng = u * f + v * g, q * f + r * g
        assert nf & M30 == 0 and ng & M30 == 0
        f, g = nf >> 30, ng >> 30
        batches += 1
        in_range = in_range and -2 * m < d < m and -2 * m < e < m
        if g == 0:
            break
    assert g == 0 and (abs(f) == 1 or (a == 0 and f == m))
    neg = f < 0
    if neg:
        d = -d
    adds = 0
    for _ in range(2):
        if d < 0:
            d += m
            adds += 1
    sub = d - m >= 0
    if sub:
        d -= m
    return d, batches, (neg, adds, sub), in_range


# the corrections the issue's survey found for both moduli
COMBOS = {(False, 0, False), (False, 1, False), (False, 2, False), (True, 0, False), (True, 0, True),
          (True, 1, False)}


def _around_golden(m):
    """Nine values around m / phi (consecutive Fibonacci-like quotients: the slowest Euclidean inputs)."""
    k = 400
    s5 = math.isqrt(5 << (2 * k))
    c = m * (s5 - (1 << k)) >> (k + 1)
    return [c + d for d in range(-4, 5)]


@functools.lru_cache(maxsize=None)
def inv_list(m):
    """The inversion inputs for modulus m, each once, 0 first."""
    bits = m.bit_length()
    vals = [0, 1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]
    vals += [1 << k for k in range(bits) if 1 << k < m]
    vals += [m - (1 << k) for k in range(bits) if 1 << k < m]
    vals += [(1 << k) - 1 for k in range(1, bits + 1) if (1 << k) - 1 < m]
    vals += [pow(x, -1, m) for x in (2, 3, 5, 7, 255, 256, 257, 1 << 30, (1 << 30) + 1, (1 << 60) - 1)]
    rng = random.Random(0xD1F5 ^ bits)
    vals += [rng.randrange(1, m >> 30) << 30 for _ in range(8)]      # low 30-bit limb zero
    vals += [rng.randrange(1, m >> 60) << 60 for _ in range(4)]      # two low limbs zero
    vals += [(m - 1) >> 30 << 30, 1 << 30, (1 << 30) * M30]
    vals += _around_golden(m)
    # seeded random values: every one that adds a correction combination or a batch count the list has
    # fewer than three rows of, among the first 3,000 draws, and 32 taken as they come
    have, taken = {}, 0
    for v in vals:
        _, b, c, _ = inv_model(v, m)
        have[c] = have.get(c, 0) + 1
        have[b] = have.get(b, 0) + 1
    for k in range(3000):
        v = rng.randrange(1, m)
        _, b, c, _ = inv_model(v, m)
        if k < 32 or have.get(c, 0) < 3 or have.get(b, 0) < 3:
            vals.append(v)
            have[c] = have.get(c, 0) + 1
            have[b] = have.get(b, 0) + 1
    out, seen = [], set()
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    assert out[0] == 0 and all(0 <= v < m for v in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inv_classes(m):
    """inv_model over inv_list(m): [(x, batches, combination, in_range)]."""
    return tuple(inv_model(v, m) for v in inv_list(m))


@functools.lru_cache(maxsize=None)
def quad_order():
    """inv_list(P) ordered for fp_inv_int_quad (one value a quad, 16 quads a wave): in the first wave
    quads 0 | 1 hold 0 (one batch) | a largest-count input, adjacent in one half-wave, and quads 7 | 8 hold
    the same pair across the two halves of the wave (lanes 28..31 | 32..35)."""
    vals, cls = inv_list(P), inv_classes(P)
    top = max(c[1] for c in cls)
    big = next(v for v, c in zip(vals, cls) if c[1] == top)
    rest = [v for v in vals if v not in (0, big)]
    return tuple([0, big] + rest[:5] + [0, big] + rest[5:])


# ---------------------------------------------------------------- Fp
def _fp_operands():
    ops = [0, 1, P - 1, RP % P, RP * RP % P]
    ops += [1 << (29 * k) for k in range(1, 14)]                    # single 29-bit limbs (1 = limb 0; 2^377 < p)
    ops += [(12 << 377) | ((1 << 377) - 1)]                         # all 29-bit limbs at 2^29 - 1, top clipped
    ops += [((P >> 352) - 1) << 352 | ((1 << 352) - 1), (1 << 352) - 1]   # 32-bit words of all ones
    assert all(0 <= x < P for x in ops) and len(set(ops)) == len(ops)
    return ops


FP_OPERANDS = tuple(_fp_operands())


def mont_t(a, b):
    """The unreduced Montgomery product of fp_mul_v: t = (a b + m p) >> 406, m = a b (-p^-1) mod 2^406."""
    m = a * b * (-pow(P, -1, RP)) % RP
    assert (a * b + m * P) % RP == 0
    return (a * b + m * P) >> RP_BITS


def _canonical_pair_over_p(x, s):
    """Canonical a = x, b with a b = s 2^406 + k p, 0 < k < x: the unreduced product is p + s."""
    k = -s * RP * pow(P, -1, x) % x
    b = (s * RP + k * P) // x
    assert x * b == s * RP + k * P and 0 < k and b < P
    return x, b


@functools.lru_cache(maxsize=None)
def fp_mul_rows():
    """[(a, b)]: every pair of FP_OPERANDS, then rows built for their unreduced product t: p - 1, p
    (operand p itself: inputs are taken as given), and p + s from raw and from canonical operands."""
    rows = [(a, b) for a in FP_OPERANDS for b in FP_OPERANDS]
    rows += [(-RP % P, 1), (1, -RP % P)]                             # t = p - 1
    rows += [(P, 1), (1, P), (P, P - 1), (1 << 383, 9 * P)]          # t = p
    rows += [(1 << 383, k * P + (s << 23)) for k, s in ((1, 1), (5, 2), (9, 1 << 300), (9, (1 << 355) - 1))]
    rng = random.Random(0xF9)
    for s in (1, 2, (1 << 29) - 1, 1 << 200, (1 << 352) - 1):
        x = rng.randrange(P >> 1, P) | 1
        while (s * RP + (-s * RP * pow(P, -1, x) % x) * P) // x >= P:   # b must come out canonical
            x = rng.randrange(P >> 1, P) | 1
        rows.append(_canonical_pair_over_p(x, s))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def fp_sqr_rows():
    """[a]: FP_OPERANDS, -R (t = p - 1 only for a product; here a plain row), p (t = p) and p + j 2^203
    (a^2 = j^2 2^406 + p (p + j 2^204): t = p + j^2)."""
    return tuple(list(FP_OPERANDS) + [-RP % P, P] + [P + (j << 203) for j in (1, 2, 3, (1 << 160) + 1)])


def fp_mul_expected(a, b):
    return a * b * RPINV % P


def _named(rows):
    assert len({n for n, *_ in rows}) == len(rows)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def fp_add_rows():
    """[(name, a, b)] for fp_add; the branch is 'reduced' when a + b >= p."""
    h0, h1 = (P - 1) // 2, (P + 1) // 2
    rows = [("sum p-1", 1, P - 2), ("sum p", 1, P - 1), ("sum p+1", 2, P - 1), ("halves p-1", h0, h0),
            ("halves p", h1, h0), ("halves p+1", h1, h1), ("0+0", 0, 0), ("0+(p-1)", 0, P - 1),
            ("(p-1)+(p-1)", P - 1, P - 1), ("carry through eleven words", (1 << 352) - 1, 1),
            ("carry through eleven words, swapped", 1, (1 << 352) - 1),
            ("carry into the reduction", P - (1 << 352), (1 << 352) - 1)]
    rows += [(f"op {i}+{j}", a, b) for i, a in enumerate(FP_OPERANDS) for j, b in enumerate(FP_OPERANDS) if i <= j]
    return _named(rows)


@functools.lru_cache(maxsize=None)
def fp_sub_rows():
    """[(name, a, b)] for fp_sub; the branch is 'borrowed' when a < b."""
    rows = [("a=b=0", 0, 0), ("a=b=1", 1, 1), ("a=b=p-1", P - 1, P - 1), ("a=b-1 low", 0, 1), ("a=b-1 top", P - 2, P - 1),
            ("a=b-1 at a word edge", (1 << 352) - 1, 1 << 352), ("0-(p-1)", 0, P - 1), ("0-2^352", 0, 1 << 352),
            ("borrow through eleven words", 1 << 352, 1), ("its mirror", 1, 1 << 352), ("(p-1)-0", P - 1, 0),
            ("(p-1)-1", P - 1, 1)]
    rows += [(f"op {i}-{j}", a, b) for i, a in enumerate(FP_OPERANDS) for j, b in enumerate(FP_OPERANDS)]
    return _named(rows)


@functools.lru_cache(maxsize=None)
def fp_neg_rows():
    return _named([("0", 0), ("1", 1), ("p-1", P - 1), ("2^352", 1 << 352), ("(p-1)/2", (P - 1) // 2)] +
                  [(f"op {i}", a) for i, a in enumerate(FP_OPERANDS) if a not in (0, 1, P - 1)])


@functools.lru_cache(maxsize=None)
def fp_dbl_rows():
    return _named([("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2), ("0", 0), ("p-1", P - 1),
                   ("2^351", 1 << 351), ("2^352-1", (1 << 352) - 1)] +
                  [(f"op {i}", a) for i, a in enumerate(FP_OPERANDS) if a not in (0, P - 1)])


@functools.lru_cache(maxsize=None)
def fp_raw_rows():
    """k p + d for k = 0..9 and d in {0, 1, p - 1} where below 2^384, and 2^384 - 1."""
    rows = [k * P + d for k in range(10) for d in (0, 1, P - 1) if k * P + d < 1 << 384]
    return tuple(rows + [(1 << 384) - 1])


def rand_fp(rng):
    return rng.randrange(P)


def f2_mul_expected(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) * RPINV % P, (x[0] * y[1] + x[1] * y[0]) * RPINV % P)


def f2_inv_expected(x):
    n = (x[0] * x[0] + x[1] * x[1]) * RPINV % P
    ni = pow(n, -1, P) * RP * RP % P if n else 0
    return (x[0] * ni * RPINV % P, -x[1] * ni * RPINV % P)


@functools.lru_cache(maxsize=None)
def f2_rows():
    """[(re, im)]: canonical halves from FP_OPERANDS (every (x, 0) and (0, x), and neighbours paired)."""
    ops = FP_OPERANDS
    rows = [(x, 0) for x in ops] + [(0, x) for x in ops if x] + [(x, x) for x in ops if x]
    rows += [(ops[i], ops[(i + 1) % len(ops)]) for i in range(len(ops))]
    rows += [(P - 1, P - 1), (P - 1, 1), (1, P - 1), ((P - 1) // 2, (P + 1) // 2)]
    return tuple(rows)


# ---------------------------------------------------------------- Fr
def _fr_operands():
    ops = [0, 1, 2, R - 1, R - 2, RR % R, RR * RR % R, ((R >> 224) - 1) << 224 | ((1 << 224) - 1), (1 << 224) - 1,
           (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 254, (R - 1) // 2, (R + 1) // 2]
    assert all(0 <= x < R for x in ops) and len(set(ops)) == len(ops)
    return ops


FR_OPERANDS = tuple(_fr_operands())
FR_PAIRS = tuple((a, b) for a in FR_OPERANDS for b in FR_OPERANDS)
U64_ROWS = (0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1)


@functools.lru_cache(maxsize=None)
def fr_sum_rows():
    """Raw sums of two canonical values for fm_reduce_once (keygen.hip kg_add): [(name, a + b)]."""
    rows = [("0", 0), ("1", 1), ("r-1", R - 1), ("r", R), ("r+1", R + 1), ("2r-2", 2 * R - 2), ("2r-3", 2 * R - 3),
            ("2^255", 1 << 255), ("2^255-1", (1 << 255) - 1)]
    rows += [(f"op {i}+{j}", a + b) for i, a in enumerate(FR_OPERANDS) for j, b in enumerate(FR_OPERANDS) if i <= j]
    return _named(rows)


def rand_fr(rng):
    return rng.randrange(R)


@functools.lru_cache(maxsize=None)
def be48_rows():
    """The 48-byte scalars for fr_from_be48 (codec.h): around every r << s of fr_reduce_slow's 130 steps."""
    rows = [v for s in range(130) for v in ((R << s) - 1, R << s, (R << s) + 1) if v < 1 << 384]
    rows += [1 << 255, (1 << 256) - 1, 1 << 256, (1 << 384) - 1]
    rows += [k * R + d for k in (0, 1, 2) for d in (0, 1, R - 1)]
    return tuple(rows)


def be48_words(v):
    """v as 48 big-endian bytes, read back as the row's 12 little-endian words."""
    b = v.to_bytes(48, "big")
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(12)]


@functools.lru_cache(maxsize=None)
def delta_rows():
    """The RLC coefficients (16 signed base-256 digits) for rlc_delta_abs."""
    hi = sum(127 << (8 * w) for w in range(16))
    lo = sum(-128 << (8 * w) for w in range(16))
    rows = [0, 1, -1, 1 << 127, -(1 << 127), 1 << 128, -(1 << 128), hi, lo, 2, -2, (1 << 64) - 1, -(1 << 64)]
    assert hi < 1 << 136 and -lo < 1 << 136
    return tuple(rows)


def rand_delta(rng):
    return sum(rng.randrange(-128, 128) << (8 * w) for w in range(16))


# ---------------------------------------------------------------- k_lagrange
LT = 2                       # tasks a lane (aggregate.hip cck_lagrange lt)
BLOCK_TASKS = 64 * LT        # tasks a block
EDGE_IDS = (1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1)
SMALL_T = (1, 2, 3, 5, 9, 33, 67)
KINDS = ("plain", "zero first", "edge", "first equals last", "zero last", "plain", "triple", "edge", "zero mid",
         "plain", "zero repeated", "edge")


def lds_bytes(t):
    """The launcher's dynamic LDS request: ids of the 64 lt / t + 2 rows of t a block may touch."""
    return (64 * LT + 2 * t) * 8


def largest_lds_t():
    """The largest t staged in LDS: (64 lt + 2 t) 8 <= 64 KiB, t <= (65536 / 8 - 64 lt) / 2."""
    t = (64 * 1024 // 8 - 64 * LT) // 2
    assert lds_bytes(t) <= 64 * 1024 < lds_bytes(t + 1)
    return t


def _distinct(rng, t, avoid=()):
    """t distinct non-zero ids: the edge ids first (shuffled), then random 64-bit values."""
    pool = [x for x in EDGE_IDS if x not in avoid]
    rng.shuffle(pool)
    out = pool[:t]
    while len(out) < t:
        x = rng.randrange(1, 1 << 64)
        if x not in out and x not in avoid:
            out.append(x)
    rng.shuffle(out)
    return out


def lagrange_row(kind, t, ln, rng):
    """One credential's ln ids: the first t shaped by `kind` (where t allows it, else plain), the rest
    filled with ids the kernel must not read (a 0 and copies of used ids among them)."""
    if kind == "plain" or t == 1 and kind != "zero first":
        ids = [rng.randrange(1, 1 << 64) for _ in range(t)]
        while len(set(ids)) < t:
            ids = [rng.randrange(1, 1 << 64) for _ in range(t)]
    else:
        ids = _distinct(rng, t)
        if kind == "zero first":
            ids[0] = 0
        elif kind == "zero last":
            ids[t - 1] = 0
        elif kind == "zero mid":
            ids[t // 2] = 0
        elif kind == "first equals last":
            ids[t - 1] = ids[0]
        elif kind == "triple":
            ids[t // 2] = ids[t - 1] = ids[0]
        elif kind == "zero repeated":
            ids[0] = ids[t - 1] = 0
        else:
            assert kind == "edge"
    tail = [0, ids[0], ids[-1], (1 << 64) - 1]
    return ids + [tail[k % 4] for k in range(ln - t)]


def small_ns(t):
    """Credential counts for a small t: n t at 127, 128, 129 where t divides them, else the counts either
    side of the 128-task block edge, with an odd and an even n t wherever t is odd, and 12 (every kind)."""
    ns = {n for n in (127 // t, -(-128 // t), -(-129 // t), 129 // t + 1, len(KINDS)) if n >= 1}
    return tuple(sorted(ns))


def small_cases():
    return tuple((t, n, ln) for t in SMALL_T for n in small_ns(t) for ln in (t, t + 3))


def small_ids(t, n, ln):
    """(kinds, ids) of the launch (t, n, ln): credential c takes KINDS[c mod 12]."""
    rng = random.Random(1000003 * t + 1009 * n + ln)
    kinds = [KINDS[c % len(KINDS)] for c in range(n)]
    return kinds, [lagrange_row(k, t, ln, rng) for k in kinds]


def switch_ids(t, n):
    """The launches either side of the LDS switch: ln = t + 1, random 64-bit ids; the first credential
    holds a repeat (positions 5 and t - 3), the last (n = 2) the id 0 at position 7."""
    rng = random.Random(77 + 2 * t + n)
    rows = []
    for c in range(n):
        ids = [rng.randrange(1, 1 << 64) for _ in range(t + 1)]
        assert len(set(ids)) == t + 1
        rows.append(ids)
    rows[0][t - 3] = rows[0][5]
    if n == 2:
        rows[1][7] = 0
    else:
        rows[0][t] = 0   # past t: never read
    return rows


def first_occurrences(ids):
    seen, out = set(), []
    for x in ids:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def lagrange_at(ids, i):
    """l_i(0) over the distinct ids of `ids` (HashSet semantics: a repeated id counts once)."""
    xi, num, den = ids[i], 1, 1
    for x in first_occurrences(ids):
        if x != xi:
            num = num * x % R
            den = den * (x - xi) % R
    return num * pow(den, -1, R) % R


def switch_samples(t, n, rows):
    """At least 128 task indices of an (n, t) launch: the first and last entry, both sides of every
    128-task block edge, the repeated and zero positions (131 in all for n = 2), then seeded random
    ones up to 128."""
    tot = n * t
    s = [0, tot - 1, 5, t - 3] + ([t + 7] if n == 2 else [])
    for e in range(BLOCK_TASKS, tot, BLOCK_TASKS):
        s += [e - 1, e]
    s = sorted(set(s))
    rng = random.Random(t + n)
    while len(s) < 128:
        k = rng.randrange(tot)
        if k not in s:
            s.append(k)
    return s
