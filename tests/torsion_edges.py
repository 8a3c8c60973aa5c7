"""Curve points of small order outside G1 / G2 (tests/golden/torsion.json) as inputs of the pairing, the
subgroup tests and the fixed-base tables, with a model of which exceptional steps each double-and-add
chain takes on them, and a homogeneous-projective Miller loop that is a third opinion between the device
and the C oracle.

Plain Python over integers plus oracle/bls12_381.py's field arithmetic; no product code and no context.

POINTS.  The twist's cofactor h2 is divisible by 13^2 and 23^2 and E'[13] has rank 2, G1's cofactor h1 by
3 and 11^2: [h r / l^k] of a random curve point has order l.  The decoders check the curve equation, not
the subgroup, and the reference never tests membership on verify, so these are inputs a verifier is given.
A point of order m is 1 in Z_m; a mixed point k G + T is 1 in Z_(m r) (its order), so the walks below take
the order alone.

WALKS.  chain_events(n, m) follows acc = 1, then for every bit of n below the top one acc <- 2 acc and, for
a set bit, acc <- acc + 1 (mod m), as the Miller loop, the psi-test ladder (subgroup.h jac_mul_xabs over
|x|) and both halves of the phi-test ladder [x^2] P do, and names what each step meets:

    add-to-inverse      acc = -base before an addition    (lambda = 0 in line_add; h = 0, r != 0 in jac_add)
    double-at-identity  acc = O before a doubling         ((0 : Y : 0) in line_dbl; Z = 0 in jac_dbl)
    add-at-identity     acc = O before an addition        (leaves T = (0, 0, 0) in line_add; r = q in jac_add)
    add-of-equal        acc = base before an addition     (theta = lambda = 0 in line_add; the doubling
                                                           branch of jac_add)

The Miller loop's formulas are not a group law at the identity: after add-at-identity T is (0, 0, 0) for
good and every later line is zero (dead=True stops the walk there); the Jacobian ladders go on from the
base.  table_events() is the same for kernels.hip k_table_fill: per run of FILL_RUN digits the first entry
by double-and-add from the identity, the rest by one mixed addition each, and which entries are the
identity (written (0, 0), skipped by Montgomery's trick and by every consumer's ft_is_empty).

MILLER MODEL.  miller() restates the formulas in the comments of csrc/pairing.inc / tower_lz.h (line_dbl:
l0 = 3 b' Z^2 - Y^2, l2 = 3 X^2 x_P, l3 = -2 Y Z y_P; line_add: theta = Y - y_Q Z, lambda = X - x_Q Z,
l0 = theta x_Q - lambda y_Q, l2 = -theta x_P, l3 = lambda y_P) with no special case, so at T = (0, 0, 0) it
returns zero lines as the formulas do, and ends with the conjugation for x < 0.  final_exp() takes no
inversion and no shortcut: conj(f)^(3 (p^12 - 1) / r) by pow, which maps 0 to 0 where the device's and the
oracle's inversions of zero have to.
"""
import ctypes
import json
import os

from fixed_edges import G1_IDENTITY, G2_IDENTITY, R, be48  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_ABS = 0xD201000000010000
EVENTS = ("add-to-inverse", "double-at-identity", "add-at-identity", "add-of-equal")
FILL_RUN = 32  # kernels.hip


def fixture():
    """{group: {name: dict(point bytes, order, k or None)}} of tests/golden/torsion.json."""
    with open(os.path.join(ROOT, "tests", "golden", "torsion.json")) as f:
        d = json.load(f)
    return {g: {r["name"]: dict(point=bytes.fromhex(r["point"]), order=int(r["order"], 16),
                                k=int(r["k"], 16) if "k" in r else None) for r in d[g]} for g in ("G1", "G2")}


# ---------------------------------------------------------------- walks in discrete-log space
def chain_events(n, m, dead=False):
    """[(bit, op, event)] of the double-and-add chain of n on a base of order m, bits counted from n's
    top bit (the start, acc = base) downwards; dead: stop after add-at-identity (the Miller loop)."""
    acc, out = 1 % m, []
    for b in range(n.bit_length() - 2, -1, -1):
        if acc == 0:
            out.append((b, "dbl", "double-at-identity"))
        acc = 2 * acc % m
        if (n >> b) & 1:
            if acc == 0:
                out.append((b, "add", "add-at-identity"))
                if dead:
                    return out
            elif acc == m - 1:
                out.append((b, "add", "add-to-inverse"))
            elif acc == 1:
                out.append((b, "add", "add-of-equal"))
            acc = (acc + 1) % m
    return out


def miller_events(m):
    return chain_events(X_ABS, m, dead=True)


def psi_events(m):
    """subgroup.h g2_in_subgroup / curve_pl.h g2_in_subgroup_lz: [|x|] Q (the closing + psi(Q) is not a
    multiple of Q in general and is not part of the walk; oracle/subgroup.py in_g2_endo decides it on the
    points)."""
    return chain_events(X_ABS, m)


def phi_events(m):
    """subgroup.h g1_in_subgroup: [|x|] P, then [|x|] of that.  The second ladder's base |x| P has the
    order m / gcd(m, |x|)."""
    import math
    m2 = m // math.gcd(m, X_ABS)
    return chain_events(X_ABS, m) + ([] if m2 == 1 else chain_events(X_ABS, m2))


def add_prefixes(n):
    """The multiples k of the base held before each addition of n's chain (acc = k base)."""
    out, k = [], 1
    for b in range(n.bit_length() - 2, -1, -1):
        k *= 2
        if (n >> b) & 1:
            out.append(k)
            k += 1
    assert k == n
    return out


def table_events(wbits, run, m):
    """k_table_fill on a window whose point P = 2^(wbits w) B has order m (2 is a unit mod an odd m, so
    the window's order is the base's): dict(identity: indices in the run whose entry is the identity,
    adds: {branch: count} of the jac_add_aff calls (acc = +P 'add-of-equal', acc = -P 'add-to-inverse',
    acc = O 'add-at-identity'), dbl_at_identity, cnt, d0)."""
    went = (1 << wbits) - 1
    d0 = run * FILL_RUN + 1
    assert d0 <= went
    cnt = min(FILL_RUN, went - d0 + 1)
    adds = {"add-of-equal": 0, "add-to-inverse": 0, "add-at-identity": 0}
    dbl0 = 0

    def add(acc):
        if acc == 0:
            adds["add-at-identity"] += 1
        elif acc == 1 % m:
            adds["add-of-equal"] += 1
        elif acc == m - 1:
            adds["add-to-inverse"] += 1
        return (acc + 1) % m

    acc = 0
    for b in range(wbits - 1, -1, -1):
        dbl0 += acc == 0
        acc = 2 * acc % m
        if (d0 >> b) & 1:
            acc = add(acc)
    assert acc == d0 % m
    ident = []
    for i in range(cnt):
        if i:
            acc = add(acc)
        if acc == 0:
            ident.append(i)
    return dict(identity=ident, adds=adds, dbl_at_identity=dbl0, cnt=cnt, d0=d0)


def window_is_identity(wbits, w, m, base_inf=False):
    """k_table_pow2 / k_table_fill: the window point 2^(wbits w) B of a base of order m is the identity, so
    jac_to_aff fails and the whole window is written (0, 0): for an identity base (inf[j]) and for no other
    base of odd order."""
    return base_inf or (1 << (wbits * w)) % m == 0


def table_positions(wbits, m):
    """{'first' / 'inside' / 'last': [(run, index)]} of the identity entries of one window."""
    out = {"first": [], "inside": [], "last": []}
    for run in range(((1 << wbits) - 1 + FILL_RUN - 1) // FILL_RUN):
        t = table_events(wbits, run, m)
        for i in t["identity"]:
            out["first" if i == 0 else "last" if i == t["cnt"] - 1 else "inside"].append((run, i))
    return out


# ---------------------------------------------------------------- the projective Miller loop
def _B():
    from oracle import bls12_381 as B
    return B


def line_dbl(T):
    """pairing.inc line_dbl: (T', (l0, l2c, l3c))."""
    B = _B()
    X, Y, Z = T
    half = (B.P + 1) // 2
    a = B.f2_muls(B.f2_mul(X, Y), half)
    b = B.f2_sqr(Y)
    c = B.f2_sqr(Z)
    e = B.f2_muls(B.f2_mul(c, B.B2), 3)  # 3 b' Z^2
    f = B.f2_muls(e, 3)
    g = B.f2_muls(B.f2_add(b, f), half)
    h = B.f2_sub(B.f2_sub(B.f2_sqr(B.f2_add(Y, Z)), b), c)  # 2 Y Z
    e2 = B.f2_sqr(e)
    T2 = (B.f2_mul(a, B.f2_sub(b, f)), B.f2_sub(B.f2_sqr(g), B.f2_muls(e2, 3)), B.f2_mul(b, h))
    return T2, (B.f2_sub(e, b), B.f2_muls(B.f2_sqr(X), 3), B.f2_neg(h))


def line_add(T, Q):
    """pairing.inc line_add: (T', (l0, l2c, l3c))."""
    B = _B()
    X, Y, Z = T
    xq, yq = Q
    theta = B.f2_sub(Y, B.f2_mul(yq, Z))
    lam = B.f2_sub(X, B.f2_mul(xq, Z))
    c, d = B.f2_sqr(theta), B.f2_sqr(lam)
    e = B.f2_mul(lam, d)
    f = B.f2_mul(Z, c)
    g = B.f2_mul(X, d)
    h = B.f2_sub(B.f2_sub(B.f2_add(e, f), g), g)
    T2 = (B.f2_mul(lam, h), B.f2_sub(B.f2_mul(theta, B.f2_sub(g, h)), B.f2_mul(e, Y)), B.f2_mul(Z, e))
    return T2, (B.f2_sub(B.f2_mul(theta, xq), B.f2_mul(lam, yq)), B.f2_neg(theta), lam)


def miller(Q, Pt, trace=None):
    """conj of f_{|x|, Q}(P) by the projective formulas; Q, P affine or None (a pair with the identity
    contributes one).  trace: a list that receives T after every step."""
    B = _B()
    if Q is None or Pt is None:
        return B.f12_one()
    xp, yp = Pt
    f, T = B.f12_one(), (Q[0], Q[1], B.F2_ONE)

    def ev(l):
        return [l[0], B.F2_ZERO, B.f2_muls(l[1], xp), B.f2_muls(l[2], yp), B.F2_ZERO, B.F2_ZERO]

    for b in range(X_ABS.bit_length() - 2, -1, -1):
        T, l = line_dbl(T)
        f = B.f12_mul(B.f12_sqr(f), ev(l))
        if trace is not None:
            trace.append(T)
        if (X_ABS >> b) & 1:
            T, l = line_add(T, Q)
            f = B.f12_mul(f, ev(l))
            if trace is not None:
                trace.append(T)
    return B.f12_conj(f)


def final_exp(f):
    B = _B()
    return B.f12_pow(f, 3 * (B.P ** 12 - 1) // B.R)


def gt_bytes(pairs):
    """GT bytes of prod e(P_k, Q_k) over [(P, Q)] as the verify equation takes it."""
    B = _B()
    f = B.f12_one()
    for Pt, Q in pairs:
        f = B.f12_mul(f, miller(Q, Pt))
    return B.gt_to_bytes(final_exp(f))


# ---------------------------------------------------------------- the C oracle
def _sz(n):
    return ctypes.c_size_t(n)


def oc_pairing(oc, Pb, Qb):
    out = ctypes.create_string_buffer(576)
    oc.oc_pairing(Pb, Qb, out)
    return out.raw


def oracle_verify(oc, mode, n, q, s1, s2, msgs, X, Y, g, per_cred, nthreads=8):
    ver = ctypes.create_string_buffer(n)
    gts = ctypes.create_string_buffer(576 * n)
    oc.oc_verify_batch(mode, _sz(n), _sz(q), s1, s2, msgs, X, Y, int(per_cred), g, ver, gts, nthreads)
    return list(ver.raw), gts.raw


def oracle_msm(oc, group, pts, scalars):
    eb = 97 if group == 1 else 192
    out = ctypes.create_string_buffer(eb)
    oc.oc_msm(group, _sz(len(scalars)), pts, b"".join(be48(s) for s in scalars), out)
    return out.raw
