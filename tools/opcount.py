#!/usr/bin/env python3
"""Instrumented op-count mirror of the HIP verify path (measurement infrastructure).

Runs the SAME algorithm as the device code — the AMCL Fp2 -> Fp4 -> Fp12 tower of tower.inc, the
line functions / sparse line multiply of pairing.inc, the Frobenius maps of tower_lz.h, the
shared-squaring 2-pair Miller loop of miller_lz.hip, the final-exponentiation chain of fexp_q.hip /
fexp_pl.hip and the fixed-base window MSM of kernels.hip — on Python integers, counting every Montgomery multiplication the kernels execute.
Because it computes real values, tests/test_opcount.py checks its GT bytes against the golden
fixtures: the counts belong to the algorithm that produces the reference's GT, not to a formula.

Unit: M = one 381-bit Montgomery multiplication (squarings included) = 12x12 a*b + 12x12 m*p
32x32->64 products = 288 "algorithmic mads" (the radix-2^29 device form issues 392 per M).
Counting rules (per credential, useful work — the lane-pair duplication of a step both lanes need
is counted once):
  Fp2 mul 3 M (pair-lane: two lanes x (2 products + 1 reduction) = 4 half-M + 2 half-M),
  Fp2 sqr 2 M, Fp2 x Fp 2 M,
  Fp inversion (field.h fp_inv: Bernstein-Yang divsteps) 14 M: the closing multiplication by R^3 plus
  ~25 batches x ~130 signed 32x32->64 mads of matrix updates (~3.6k mads = 12.6 M-equivalents),
  G1/G2 formulas as written in curve.h (jac_add_aff 7M+4S, jac_add 12M+4S, jac_dbl 2M+5S).

    python tools/opcount.py            # writes tests/fixtures/opcount.json
"""
import json
import os
import random
import sys

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000


class Counter:
    def __init__(self):
        self.M = 0

    def take(self):
        m, self.M = self.M, 0
        return m


C = Counter()


def fmul(a, b):
    C.M += 1
    return a * b % P


# A one-lane Fp squaring (the G1 code's: lazy.h lz_sqr1, upper-triangle product scanning) is counted at
# its algorithmic minimum, 78 products + 144 reduction mads = 222 of a multiplication's 288: a squaring
# counted as a full M would overstate the work and with it the roofline fraction of G1-heavy kernels.
SQR_M = 222 / 288


def fsqr(a):
    C.M += SQR_M
    return a * a % P


SAFEGCD_M = 14  # field.h fp_inv (see the counting rules above)


def finv_pair(a):  # tower_pl.h fp_inv_pair = field.h fp_inv on both lanes of the pair (counted once)
    C.M += SAFEGCD_M
    return pow(a, P - 2, P)


def finv_fermat(a):  # field.h fp_inv (one lane): the same divstep inversion
    C.M += SAFEGCD_M
    return pow(a, P - 2, P)


def f2_inv_lane(x):  # field.h f2_inv (one credential per lane: prep kernels)
    C.M += 4
    n = (x[0] * x[0] + x[1] * x[1]) % P
    ni = finv_fermat(n)
    return (x[0] * ni % P, -x[1] * ni % P)


# ---------------------------------------------------------------- Fp2 = Fp[i]/(i^2+1)
def f2_add(x, y): return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)
def f2_sub(x, y): return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
def f2_neg(x): return (-x[0] % P, -x[1] % P)
def f2_conj(x): return (x[0], -x[1] % P)
def f2_dbl(x): return f2_add(x, x)
def f2_xi(x): return ((x[0] - x[1]) % P, (x[0] + x[1]) % P)


def f2_mul(x, y):
    C.M += 3
    a, b = x
    c, d = y
    return ((a * c - b * d) % P, (a * d + b * c) % P)


def f2_sqr(x):
    C.M += 2
    a, b = x
    return ((a + b) * (a - b) % P, 2 * a * b % P)


def f2_mul_fp(x, k):
    C.M += 2
    return (x[0] * k % P, x[1] * k % P)


def f2_half(x):
    h = pow(2, P - 2, P)
    return (x[0] * h % P, x[1] * h % P)


def f2_inv(x):  # tower_pl.h f2_inv: norm as one fused pair product (3 half-M per lane pair), split inversion
    C.M += 3
    n = (x[0] * x[0] + x[1] * x[1]) % P
    ni = finv_pair(n)
    t = f2_mul_fp(x, ni)
    return f2_conj(t)


F2_ZERO, F2_ONE = (0, 0), (1, 0)


# ---------------------------------------------------------------- Fp4 = Fp2[s]/(s^2 - xi)   (tower.inc)
def f4_add(x, y): return (f2_add(x[0], y[0]), f2_add(x[1], y[1]))
def f4_sub(x, y): return (f2_sub(x[0], y[0]), f2_sub(x[1], y[1]))
def f4_neg(x): return (f2_neg(x[0]), f2_neg(x[1]))
def f4_conj(x): return (x[0], f2_neg(x[1]))
def f4_dbl(x): return f4_add(x, x)
def f4_mul_s(x): return (f2_xi(x[1]), x[0])


def f4_mul(x, y):
    t0 = f2_mul(x[0], y[0])
    t1 = f2_mul(x[1], y[1])
    s = f2_mul(f2_add(x[0], x[1]), f2_add(y[0], y[1]))
    return (f2_add(t0, f2_xi(t1)), f2_sub(f2_sub(s, t0), t1))


def f4_sqr(x):
    a, b = x
    ab = f2_mul(a, b)
    s0 = f2_mul(f2_add(a, b), f2_add(f2_xi(b), a))
    return (f2_sub(f2_sub(s0, ab), f2_xi(ab)), f2_dbl(ab))


def f4_mul_f2(x, c): return (f2_mul(x[0], c), f2_mul(x[1], c))


def f4_inv(x):
    a, b = x
    n = f2_sub(f2_sqr(a), f2_xi(f2_sqr(b)))
    ni = f2_inv(n)
    return (f2_mul(a, ni), f2_neg(f2_mul(b, ni)))


F4_ZERO = (F2_ZERO, F2_ZERO)
F4_ONE = (F2_ONE, F2_ZERO)


# ---------------------------------------------------------------- Fp12 = Fp4[w]/(w^3 - s)
def f12_one(): return (F4_ONE, F4_ZERO, F4_ZERO)
def f12_conj(x): return (f4_conj(x[0]), f4_neg(f4_conj(x[1])), f4_conj(x[2]))


def f12_mul(x, y):
    t0 = f4_mul(x[0], y[0])
    t1 = f4_mul(x[1], y[1])
    t2 = f4_mul(x[2], y[2])
    s = f4_mul(f4_add(x[1], x[2]), f4_add(y[1], y[2]))
    ra = f4_add(f4_mul_s(f4_sub(f4_sub(s, t1), t2)), t0)
    s = f4_mul(f4_add(x[0], x[1]), f4_add(y[0], y[1]))
    rb = f4_add(f4_sub(f4_sub(s, t0), t1), f4_mul_s(t2))
    s = f4_mul(f4_add(x[0], x[2]), f4_add(y[0], y[2]))
    rc = f4_add(f4_sub(f4_sub(s, t0), t2), t1)
    return (ra, rb, rc)


def f12_sqr(x):  # Chung-Hasan SQR2 as tower.inc
    a, b, c = x
    s2 = f4_sqr(f4_add(f4_sub(a, b), c))
    s0 = f4_sqr(a)
    s1 = f4_dbl(f4_mul(a, b))
    s3 = f4_dbl(f4_mul(b, c))
    s4 = f4_sqr(c)
    ra = f4_add(f4_mul_s(s3), s0)
    rc = f4_sub(f4_add(f4_sub(f4_add(s2, s1), s0), s3), s4)
    rb = f4_add(s1, f4_mul_s(s4))
    return (ra, rb, rc)


def f12_cyc_sqr(x):  # Granger-Scott (AMCL FP12::usqr)
    a, b, c = x
    A = f4_sqr(a)
    C_ = f4_sqr(b)
    B = f4_mul_s(f4_sqr(c))
    ra = f4_add(f4_dbl(f4_sub(A, f4_conj(a))), A)
    rb = f4_add(f4_dbl(f4_add(B, f4_conj(b))), B)
    rc = f4_add(f4_dbl(f4_sub(C_, f4_conj(c))), C_)
    return (ra, rb, rc)


def f12_inv(x):
    a, b, c = x
    A = f4_sub(f4_sqr(a), f4_mul_s(f4_mul(b, c)))
    B = f4_sub(f4_mul_s(f4_sqr(c)), f4_mul(a, b))
    Cc = f4_sub(f4_sqr(b), f4_mul(a, c))
    F = f4_add(f4_mul_s(f4_add(f4_mul(c, B), f4_mul(b, Cc))), f4_mul(a, A))
    F = f4_inv(F)
    return (f4_mul(A, F), f4_mul(B, F), f4_mul(Cc, F))


def _xi_pow(e):
    r = (1, 0)
    b = (1, 1)
    while e:
        if e & 1:
            a0, a1 = r
            r = ((a0 * b[0] - a1 * b[1]) % P, (a0 * b[1] + a1 * b[0]) % P)
        b = ((b[0] * b[0] - b[1] * b[1]) % P, 2 * b[0] * b[1] % P)
        e >>= 1
    return r


GAMMA1 = [_xi_pow(k * (P - 1) // 6) for k in range(6)]
GAMMA2 = [_xi_pow(k * (P * P - 1) // 6)[0] for k in range(6)]
# AMCL slots -> W power: a.a 0, a.b 3, b.a 1, b.b 4, c.a 2, c.b 5


def f12_frob(x):
    def fc(c, k): return f2_mul(f2_conj(c), GAMMA1[k])
    (aa, ab), (ba, bb), (ca, cb) = x
    return ((f2_conj(aa), fc(ab, 3)), (fc(ba, 1), fc(bb, 4)), (fc(ca, 2), fc(cb, 5)))


def f12_frob2(x):
    (aa, ab), (ba, bb), (ca, cb) = x
    return ((aa, f2_mul_fp(ab, GAMMA2[3])), (f2_mul_fp(ba, GAMMA2[1]), f2_mul_fp(bb, GAMMA2[4])),
            (f2_mul_fp(ca, GAMMA2[2]), f2_mul_fp(cb, GAMMA2[5])))


def f12_is_one(x):
    return x == f12_one()


# ---------------------------------------------------------------- lines (pairing.inc)
def f12_mul_line(f, l0, l2, l3):
    a, b, c = f
    A = (l0, l3)
    t0 = f4_mul(a, A)
    t2 = f4_mul_f2(c, l2)
    s = f4_mul(f4_add(a, c), (f2_add(l0, l2), l3))
    rc = f4_sub(f4_sub(s, t0), t2)
    ra = f4_add(t0, f4_mul_s(f4_mul_f2(b, l2)))
    rb = f4_add(f4_mul(b, A), f4_mul_s(t2))
    return (ra, rb, rc)


B_TW = (4, 4)  # twist b' = 4(1+i)


def line_dbl(T):
    X, Y, Z = T
    a = f2_half(f2_mul(X, Y))
    b = f2_sqr(Y)
    c = f2_sqr(Z)
    e = f2_xi(c)
    e = f2_add(f2_dbl(f2_dbl(f2_dbl(e))), f2_dbl(f2_dbl(e)))  # x 12
    f = f2_add(f2_dbl(e), e)
    g = f2_half(f2_add(b, f))
    h = f2_sub(f2_sub(f2_sqr(f2_add(Y, Z)), b), c)
    l0 = f2_sub(e, b)
    t = f2_sqr(X)
    l2 = f2_add(f2_dbl(t), t)
    l3 = f2_neg(h)
    nX = f2_mul(a, f2_sub(b, f))
    t = f2_sqr(e)
    nY = f2_sub(f2_sub(f2_sub(f2_sqr(g), t), t), t)
    nZ = f2_mul(b, h)
    return (nX, nY, nZ), l0, l2, l3


def line_add(T, Q):
    X, Y, Z = T
    qx, qy = Q
    theta = f2_sub(Y, f2_mul(qy, Z))
    lam = f2_sub(X, f2_mul(qx, Z))
    c = f2_sqr(theta)
    d = f2_sqr(lam)
    e = f2_mul(lam, d)
    f = f2_mul(Z, c)
    g = f2_mul(X, d)
    h = f2_sub(f2_sub(f2_add(e, f), g), g)
    l0 = f2_sub(f2_mul(theta, qx), f2_mul(lam, qy))
    l2 = f2_neg(theta)
    l3 = lam
    nX = f2_mul(lam, h)
    nY = f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, Y))
    nZ = f2_mul(Z, e)
    return (nX, nY, nZ), l0, l2, l3


def eval_mul(f, l0, l2, l3, Pe):
    """Pe = (px, py, pz or None for affine)"""
    px, py, pz = Pe
    a0 = l0 if pz is None else f2_mul_fp(l0, pz)
    return f12_mul_line(f, a0, f2_mul_fp(l2, px), f2_mul_fp(l3, py))


def miller2(pairs):
    """miller_lz.hip k_miller: pairs = [(Q affine G2, P eval form, skip)]; shared squaring."""
    Ts = [(q[0], q[1], F2_ONE) for q, _, _ in pairs]
    f = f12_one()
    for bit in range(62, -1, -1):
        if bit != 62:
            f = f12_sqr(f)
        for k, (q, pe, skip) in enumerate(pairs):
            Ts[k], l0, l2, l3 = line_dbl(Ts[k])
            if not skip:
                f = eval_mul(f, l0, l2, l3, pe)
        if (X_ABS >> bit) & 1:
            for k, (q, pe, skip) in enumerate(pairs):
                Ts[k], l0, l2, l3 = line_add(Ts[k], q)
                if not skip:
                    f = eval_mul(f, l0, l2, l3, pe)
    return f12_conj(f)


def cyc_pow_x_gs(y):  # fexp_pl.hip fx_pow_x_gs (the zero-denominator fallback)
    acc = y
    for bit in range(62, -1, -1):
        acc = f12_cyc_sqr(acc)
        if (X_ABS >> bit) & 1:
            acc = f12_mul(acc, y)
    return f12_conj(acc)


def _3u(u, v, plus):  # f2_3u_p2v / f2_3u_m2v: u + 2 (u +- v)
    return f2_add(f2_dbl(f2_add(u, v) if plus else f2_sub(u, v)), u)


def cyc4_sqr(x):  # compressed cyclotomic squaring, six Fp2 squarings (fexp_q.hip qz_sqr, fexp_pl.hip cyc4_sqr_dist_lz)
    b0, b1, c0, c1 = x
    s0, s1 = f2_sqr(b0), f2_sqr(b1)
    Xb = f2_sub(f2_sub(f2_sqr(f2_add(b0, b1)), s0), s1)
    Tb = f2_add(s0, f2_xi(s1))
    s0, s1 = f2_sqr(c0), f2_sqr(c1)
    Xc = f2_xi(f2_sub(f2_sub(f2_sqr(f2_add(c0, c1)), s0), s1))
    Tc = f2_add(s0, f2_xi(s1))
    return (_3u(Xc, b0, True), _3u(Tc, b1, False), _3u(Tb, c0, False), _3u(Xb, c1, True))


def cyc4_num(x):  # the decompression's numerators and denominator (fexp_q.hip qz_num, fexp_pl.hip decompress3_wide)
    b0, b1, c0, c1 = x
    Nb = f2_sub(f2_sqr(b0), f2_xi(f2_sqr(b1)))
    Nc = f2_sub(f2_sqr(c0), f2_xi(f2_sqr(c1)))
    n0 = f2_add(f2_mul(b0, Nb), f2_xi(f2_mul(c1, Nc)))
    n1 = f2_add(f2_mul(c0, Nc), f2_mul(b1, Nb))
    den = f2_dbl(f2_sub(f2_mul(b0, c0), f2_xi(f2_mul(b1, c1))))
    return n0, n1, den


def cyc4_expand(x, n0, n1, inv):
    return ((f2_mul(n0, inv), f2_mul(n1, inv)), (x[0], x[1]), (x[2], x[3]))


def cyc_pow_x(y):  # fexp_pl.hip fx_pow_x: 57 compressed squarings, 3 decompressions, 6 Granger-Scott
    c = (y[1][0], y[1][1], y[2][0], y[2][1])
    snaps = {}
    for k in range(1, 58):
        c = cyc4_sqr(c)
        if k in (16, 48):
            snaps[k] = c
    n16, n48, n57 = cyc4_num(snaps[16]), cyc4_num(snaps[48]), cyc4_num(c)
    p1 = f2_mul(n16[2], n48[2])
    p2 = f2_mul(p1, n57[2])
    if p2 == F2_ZERO:
        return cyc_pow_x_gs(y)
    inv = f2_inv(p2)
    yy = cyc4_expand(c, n57[0], n57[1], f2_mul(inv, p1))
    inv = f2_mul(inv, n57[2])
    acc = cyc4_expand(snaps[16], n16[0], n16[1], f2_mul(inv, n48[2]))
    t = cyc4_expand(snaps[48], n48[0], n48[1], f2_mul(inv, n16[2]))
    acc = f12_mul(f12_mul(acc, t), yy)
    for _ in range(3):
        yy = f12_cyc_sqr(yy)
    acc = f12_mul(acc, yy)
    for _ in range(2):
        yy = f12_cyc_sqr(yy)
    acc = f12_mul(acc, yy)
    yy = f12_cyc_sqr(yy)
    acc = f12_mul(acc, yy)
    return f12_conj(acc)


def final_exp(f):  # the chain of k_fexp_q / k_fexp1 (fexp_pl.hip fexp_chain), step for step
    t = f12_inv(f)
    f = f12_mul(f12_conj(f), t)
    f = f12_mul(f12_frob2(f), f)
    r = f12_mul(f12_cyc_sqr(f), f)
    t = cyc_pow_x(f)
    t = f12_mul(t, f12_conj(f))
    a = cyc_pow_x(t)
    a = f12_mul(a, f12_conj(t))
    s = f12_mul(f12_frob2(a), f12_conj(a))
    r = f12_mul(f12_frob(s), r)
    t = cyc_pow_x(a)
    s = f12_mul(f12_frob2(t), f12_conj(t))
    r = f12_mul(s, r)
    a = cyc_pow_x(t)
    r = f12_mul(f12_frob(a), r)
    t = cyc_pow_x(a)
    r = f12_mul(t, r)
    return r


def gt_bytes(f):
    out = b""
    for f4 in f:
        for f2 in f4:
            out += f2[0].to_bytes(48, "big") + f2[1].to_bytes(48, "big")
    return out


# ---------------------------------------------------------------- curves (curve.h), generic over Fp / Fp2
class G:
    def __init__(self, two):
        self.two = two
        if two:
            self.mul, self.sqr = f2_mul, f2_sqr
            self.add, self.sub, self.dbl, self.neg = f2_add, f2_sub, f2_dbl, f2_neg
            self.zero, self.one, self.b = F2_ZERO, F2_ONE, B_TW
            self.inv = f2_inv_lane
        else:
            self.mul, self.sqr = fmul, fsqr
            self.add = lambda a, b: (a + b) % P
            self.sub = lambda a, b: (a - b) % P
            self.dbl = lambda a: 2 * a % P
            self.neg = lambda a: -a % P
            self.zero, self.one, self.b = 0, 1, 4
            self.inv = finv_fermat

    def mul2(self, a, b, c, d):
        """a b + c d: G1 (curve_lz.h jg_add*: lazy.h mul2) shares one reduction between the two products,
        2 x 144 product mads + 144 reduction mads = 1.5 M; G2 runs two products."""
        if self.two:
            return self.add(self.mul(a, b), self.mul(c, d))
        C.M += 1.5
        return (a * b + c * d) % P

    def is_inf(self, p): return p[2] == self.zero
    def inf(self): return (self.one, self.one, self.zero)

    def dbl_j(self, p):
        x, y, z = p
        A = self.sqr(x); B = self.sqr(y); Cc = self.sqr(B)
        t = self.sub(self.sub(self.sqr(self.add(x, B)), A), Cc)
        D = self.dbl(t); E = self.add(self.dbl(A), A); Gg = self.sqr(E)
        z3 = self.dbl(self.mul(y, z))
        x3 = self.sub(self.sub(Gg, D), D)
        y3 = self.sub(self.mul(E, self.sub(D, x3)), self.dbl(self.dbl(self.dbl(Cc))))
        return (x3, y3, z3)

    def add_aff(self, p, q):
        if self.is_inf(p):
            return (q[0], q[1], self.one)
        x, y, z = p
        z1z1 = self.sqr(z)
        u2 = self.mul(q[0], z1z1)
        s2 = self.mul(self.mul(q[1], z), z1z1)
        h = self.sub(u2, x)
        rr = self.sub(s2, y)
        if h == self.zero:
            return self.dbl_j(p) if rr == self.zero else self.inf()
        rr = self.dbl(rr)
        hh = self.sqr(h)
        i = self.dbl(self.dbl(hh))
        j = self.mul(h, i)
        v = self.mul(x, i)
        x3 = self.sub(self.sub(self.sub(self.sqr(rr), j), v), v)
        y3 = self.mul2(rr, self.sub(v, x3), self.neg(self.dbl(y)), j)
        z3 = self.sub(self.sub(self.sqr(self.add(z, h)), z1z1), hh)
        return (x3, y3, z3)

    def add_j(self, p, q):
        if self.is_inf(p):
            return q
        if self.is_inf(q):
            return p
        z1z1 = self.sqr(p[2]); z2z2 = self.sqr(q[2])
        u1 = self.mul(p[0], z2z2); u2 = self.mul(q[0], z1z1)
        s1 = self.mul(self.mul(p[1], q[2]), z2z2)
        s2 = self.mul(self.mul(q[1], p[2]), z1z1)
        h = self.sub(u2, u1); rr = self.sub(s2, s1)
        if h == self.zero:
            return self.dbl_j(p) if rr == self.zero else self.inf()
        rr = self.dbl(rr)
        i = self.sqr(self.dbl(h))
        j = self.mul(h, i); v = self.mul(u1, i)
        x3 = self.sub(self.sub(self.sub(self.sqr(rr), j), v), v)
        y3 = self.mul2(rr, self.sub(v, x3), self.neg(self.dbl(s1)), j)
        z3 = self.mul(self.sub(self.sub(self.sqr(self.add(p[2], q[2])), z1z1), z2z2), h)
        return (x3, y3, z3)

    def to_aff(self, p):
        if self.is_inf(p):
            return None
        zi = self.inv(p[2])
        zi2 = self.sqr(zi)
        zi3 = self.mul(zi2, zi)
        return (self.mul(p[0], zi2), self.mul(p[1], zi3))

    def on_curve(self, a):
        l = self.sqr(a[1])
        r = self.add(self.mul(self.sqr(a[0]), a[0]), self.b)
        return l == r


G1, G2 = G(False), G(True)


def decode(g, enc):
    """codec.h g1_decode / g2_decode: raw -> Montgomery (1 M per coordinate), on-curve check."""
    if g.two:
        v = [int.from_bytes(enc[48 * k:48 * k + 48], "big") % P for k in range(4)]
        C.M += 4
        a = ((v[0], v[1]), (v[2], v[3]))
    else:
        ok0 = enc[0] == 4
        a = (int.from_bytes(enc[1:49], "big") % P, int.from_bytes(enc[49:97], "big") % P)
        C.M += 2
        if not ok0:
            g.on_curve(a)
            return None
    return a if g.on_curve(a) else None


VK_WBITS = 22  # shared-verkey tables (fixed.h; capi_ctx.cpp rebuild_tables: the widest of 22 / 20 / 16 bits whose
# tables fit the HBM budget -- 22 for configs 2 and 3 (8 / 18 G1 bases), 20 for config 5 (34 bases); main()
# sets it per config)


def fixed_table_mul_add(g, acc, k, base_aff, w0, w1, wbits=8):
    """fixed.h ft_add: acc += sum over wbits-bit windows w0..w1-1 of digit * 2^(wbits w) * base."""
    mask = (1 << wbits) - 1
    for w in range(w0, w1):
        d = (k >> (wbits * w)) & mask
        if d:
            e = mul_aff(g, base_aff, d << (wbits * w))  # the table entry (precomputed, not counted)
            acc = g.add_aff(acc, e)
    return acc


def mul_aff(g, base, k):
    """uncounted scalar multiplication (table entries are precomputed at cc_set_verkey)."""
    m = C.M
    acc = g.inf()
    for b in range(k.bit_length() - 1, -1, -1):
        acc = g.dbl_j(acc)
        if (k >> b) & 1:
            acc = g.add_aff(acc, base)
    a = g.to_aff(acc)
    C.M = m
    return a


# ---------------------------------------------------------------- verify (SigG2 shared verkey, pair prep)
def verify_sigg2(cred, vk_aff, gtil_aff, q):
    """k_prep_sigg2_pair -> k_miller<2,false> -> k_fexp_q.  Returns (verdict, gt, {kernel: M})."""
    counts = {}
    s1 = decode(G2, bytes.fromhex(cred["sigma1"]))
    s2 = decode(G2, bytes.fromhex(cred["sigma2"]))
    msgs = [int.from_bytes(bytes.fromhex(m), "big") % R for m in cred["msgs"]]
    X, Ys = vk_aff
    # lane pair: windows 0..15 (with X) on the even lane, 16..31 on the odd lane, then one jac_add
    lo = (X[0], X[1], 1) if X else G1.inf()
    hi = G1.inf()
    nw = -(-256 // VK_WBITS)
    for j in range(q):
        lo = fixed_table_mul_add(G1, lo, msgs[j], Ys[j], 0, nw // 2, VK_WBITS)
        hi = fixed_table_mul_add(G1, hi, msgs[j], Ys[j], nw // 2, nw, VK_WBITS)
    pr = G1.add_j(lo, hi)
    return _pair_sigg2(s1, s2, pr, gtil_aff, counts)


def _pair_sigg2(s1, s2, pr, gtil_aff, counts):
    """The Miller loop and final exponentiation of a SigG2 verify after its prep (pr Jacobian G1)."""
    pr_inf = G1.is_inf(pr)
    pe = None
    if not pr_inf:  # affine in the R' form (curve_lz.h jg_to_aff_rp: one inversion): l0 needs no product
        a = G1.to_aff(pr)
        pe = (a[0], a[1], None)
    counts["prep"] = C.take()
    skip0 = s1 is None or pr_inf
    skip1 = s2 is None
    q0 = s1 if s1 else ((0, 0), (0, 0))
    q1 = (s2[0], f2_neg(s2[1])) if s2 else ((0, 0), (0, 0))
    f = miller2([(q0, pe if pe else (0, 0, 0), skip0), (q1, (gtil_aff[0], gtil_aff[1], None), skip1)])
    counts["miller"] = C.take()
    r = final_exp(f)
    counts["fexp"] = C.take()
    ok = f12_is_one(r) and s1 is not None and s2 is not None
    return int(ok), gt_bytes(r), counts


def verify_sigg1(cred, vk_aff, gtil_aff, q):
    """k_prep_sigg1<true> -> k_miller<1,false> (g~ lines precomputed) -> k_fexp_q."""
    counts = {}
    s1 = decode(G1, bytes.fromhex(cred["sigma1"]))
    s2 = decode(G1, bytes.fromhex(cred["sigma2"]))
    msgs = [int.from_bytes(bytes.fromhex(m), "big") % R for m in cred["msgs"]]
    X, Ys = vk_aff
    acc = (X[0], X[1], F2_ONE) if X else G2.inf()
    for j in range(q):
        acc = fixed_table_mul_add(G2, acc, msgs[j], Ys[j], 0, -(-256 // VK_WBITS), VK_WBITS)
    pr = G2.to_aff(acc)
    return _pair_sigg1(s1, s2, pr, gtil_aff, counts)


def _pair_sigg1(s1, s2, pr, gtil_aff, counts):
    """The Miller loop (g~ lines precomputed) and final exponentiation of a SigG1 verify after its prep."""
    counts["prep"] = C.take()
    # pair 0: (pr, sigma_1); pair 1: (g~ [precomputed lines: no line cost], -sigma_2)
    skip0 = s1 is None or pr is None
    skip1 = s2 is None
    T = (pr[0], pr[1], F2_ONE) if pr else (F2_ONE, F2_ONE, F2_ONE)
    Tg = (gtil_aff[0], gtil_aff[1], F2_ONE)
    f = f12_one()
    for bit in range(62, -1, -1):
        if bit != 62:
            f = f12_sqr(f)
        T, l0, l2, l3 = line_dbl(T)
        if not skip0:
            f = eval_mul(f, l0, l2, l3, (s1[0], s1[1], None))
        m = C.M
        Tg, g0, g2, g3 = line_dbl(Tg)
        C.M = m
        if not skip1:
            f = eval_mul(f, g0, g2, g3, (s2[0], -s2[1] % P, None))
        if (X_ABS >> bit) & 1:
            T, l0, l2, l3 = line_add(T, pr if pr else (F2_ONE, F2_ONE))
            if not skip0:
                f = eval_mul(f, l0, l2, l3, (s1[0], s1[1], None))
            m = C.M
            Tg, g0, g2, g3 = line_add(Tg, gtil_aff)
            C.M = m
            if not skip1:
                f = eval_mul(f, g0, g2, g3, (s2[0], -s2[1] % P, None))
    f = f12_conj(f)
    counts["miller"] = C.take()
    r = final_exp(f)
    counts["fexp"] = C.take()
    ok = f12_is_one(r) and s1 is not None and s2 is not None
    return int(ok), gt_bytes(r), counts


# ---------------------------------------------------------------- aggregation (aggregate.hip)
def lagrange0(ids_first_t, i):
    S = sorted(set(ids_first_t))
    num, den = 1, 1
    for j in S:
        if j != i:
            num = num * j % R
            den = den * (j - i) % R
    return num * pow(den, R - 2, R) % R


def recode_w4(k):
    d, carry = [], 0
    for w in range(64):
        v = ((k >> (4 * w)) & 0xF) + carry
        carry = 1 if v > 8 else 0
        d.append(v - 16 * carry)
    d.append(carry)
    return d


def straus(g, pts, scalars, to_affine=True):
    """k_msm_straus / straus.h: signed 4-bit windows, multiples 1P..8P batch-normalised with one inversion
    (to_affine=False: the Jacobian sum, as the per-credential-verkey preps use it)."""
    ent = []
    acc_z = g.one
    for P in pts:
        J = (P[0], P[1], g.one) if P else g.inf()
        for d in range(8):
            if d == 1:
                J = g.dbl_j(J)
            elif d > 1 and P:
                J = g.add_aff(J, P)
            ent.append(J)
            if not g.is_inf(J):
                acc_z = g.mul(acc_z, J[2])
    inv = g.inv(acc_z)
    aff = [None] * len(ent)
    for e in range(len(ent) - 1, -1, -1):
        J = ent[e]
        if g.is_inf(J):
            continue
        pz = g.one
        for f in range(e):  # the stored prefix (uncounted: it was recorded on the way up)
            if not g.is_inf(ent[f]):
                pz = _raw_mul(g, pz, ent[f][2])
        zi = g.mul(inv, pz)
        inv = g.mul(inv, J[2])
        zi2 = g.sqr(zi)
        x = g.mul(J[0], zi2)
        zi3 = g.mul(zi2, zi)
        aff[e] = (x, g.mul(J[1], zi3))
    digs = [recode_w4(k) for k in scalars]
    acc = g.inf()
    for win in range(64, -1, -1):
        if win != 64 and not g.is_inf(acc):
            for _ in range(4):
                acc = g.dbl_j(acc)
        for k in range(len(pts)):
            d = digs[k][win]
            if d == 0 or aff[k * 8 + abs(d) - 1] is None:
                continue
            e = aff[k * 8 + abs(d) - 1]
            if d < 0:
                e = (e[0], g.neg(e[1]))
            acc = g.add_aff(acc, e)
    return g.to_aff(acc) if to_affine else acc


def verify_pervk(cred, gtil_aff, mode):
    """pervk.hip k_prep_sig*_var (Straus over [Y~_1..q] with the messages, + X~) -> k_miller -> k_fexp_q.
    Counted as ONE Straus over all q bases: the SigG2 kernel splits the bases over a lane pair and
    repeats the doubling chain on both lanes, which is not counted (the conservative figure)."""
    counts = {}
    gs, go = (G2, G1) if mode == "G2" else (G1, G2)
    s1 = decode(gs, bytes.fromhex(cred["sigma1"]))
    s2 = decode(gs, bytes.fromhex(cred["sigma2"]))
    X = decode(go, bytes.fromhex(cred["vk"]["X"]))
    Ys = [decode(go, bytes.fromhex(y)) for y in cred["vk"]["Y"]]
    msgs = [int.from_bytes(bytes.fromhex(m), "big") % R for m in cred["msgs"]]
    acc = straus(go, Ys, msgs, to_affine=False)
    if X:
        acc = go.add_aff(acc, X)
    if mode == "G2":
        return _pair_sigg2(s1, s2, acc, gtil_aff, counts)
    return _pair_sigg1(s1, s2, go.to_aff(acc), gtil_aff, counts)


def _raw_mul(g, a, b):
    m = C.M
    r = g.mul(a, b)
    C.M = m
    return r


def issuer_wbits(nb, two, budget=16 << 30):
    """capi_aggregate.cpp cc_set_issuers: the widest window in {16, 13, 12, 10} whose tables (nb bases, affine
    entries of 24 / 48 words) fit the default 16 GiB budget, else 8."""
    for w in (16, 13, 12, 10):
        if nb * ((256 + w - 1) // w) * ((1 << w) - 1) * (48 if two else 24) * 4 <= budget:
            return w
    return 8


def fixed_sum(g, pts, scalars, wbits=8):
    """k_vk_agg_fixed / msm_fixed: sum of wbits-window table entries (entries precomputed, uncounted)."""
    acc = g.inf()
    nwin = (256 + wbits - 1) // wbits
    for P, k in zip(pts, scalars):
        if P is None:
            continue
        acc = fixed_table_mul_add(g, acc, k, P, 0, nwin, wbits)
    return g.to_aff(acc)


# issuer-table window width of the aggregate bench modes (bench_modes.py BENCH_ISS_BITS, cc_set_table_bits)
BENCH_ISS_BITS = 16


def aggregate_case(d, case, n_issuers=100, wb=None):
    """Signature::aggregate (Straus, SignatureGroup) + Verkey::aggregate (issuer tables, OtherGroup;
    window width wb, default as cc_set_issuers picks it for n_issuers x (q + 1) bases)."""
    gs, go = (G2, G1) if d["mode"] == "G2" else (G1, G2)
    t, q = d["threshold"], d["q"]
    wb = wb or issuer_wbits(n_issuers * (q + 1), go is G2)
    ids = case["ids"][:t]
    ls = [lagrange0(ids, i) for i in ids]
    s2 = [decode(gs, bytes.fromhex(h)) for h in case["sigma2"][:t]]
    C.take()
    sig = straus(gs, s2, ls)
    straus_m = C.take()
    Xs = [decode(go, bytes.fromhex(h)) for h in case["X"][:t]]
    Ys = [[decode(go, bytes.fromhex(h)) for h in row] for row in case["Y"][:t]]
    C.take()
    vkX = fixed_sum(go, Xs, ls, wb)
    vkY = [fixed_sum(go, [Ys[k][j] for k in range(t)], ls, wb) for j in range(q)]
    fixed_m = C.take()
    return sig, vkX, vkY, {"straus_sigma2": straus_m, "fixed_verkey": fixed_m}


def enc(g, a):
    if a is None:
        return (b"\x04" + b"\x00" * 48 + (1).to_bytes(48, "big")) if not g.two else \
            b"\x00" * 96 + (1).to_bytes(48, "big") + b"\x00" * 48
    if g.two:
        return b"".join(v.to_bytes(48, "big") for v in (a[0][0], a[0][1], a[1][0], a[1][1]))
    return b"\x04" + a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


# ---------------------------------------------------------------- PoK verify (k_prep_pok, SigG2)
def pok_sigg2(d, p, vk_aff, gtil):
    """k_prep_pok<Fp2, Fp> -> k_miller<2,false> -> k_fexp_q."""
    counts = {}
    q, rev = d["q"], d["revealed"]
    X, Ys = vk_aff
    s1 = decode(G2, bytes.fromhex(p["sigma1"]))
    s2 = decode(G2, bytes.fromhex(p["sigma2"]))
    Ja = decode(G1, bytes.fromhex(p["J"]))
    resp = [int(h, 16) % R for h in p["responses"]]
    chal = int(p["chal"], 16) % R
    nw = -(-256 // VK_WBITS)
    acc = fixed_table_mul_add(G1, G1.inf(), resp[0], gtil, 0, nw, VK_WBITS)
    slot = 1
    for h in range(q):
        if h in rev:
            continue
        acc = fixed_table_mul_add(G1, acc, resp[slot], Ys[h], 0, nw, VK_WBITS)
        slot += 1
    if Ja:
        sacc = G1.inf()
        for b in range(254, -1, -1):
            sacc = G1.dbl_j(sacc)
            if (chal >> b) & 1:
                sacc = G1.add_aff(sacc, Ja)
        acc = G1.add_j(acc, sacc)
    Ta = decode(G1, bytes.fromhex(p["T"]))
    if Ta:
        acc = G1.add_aff(acc, (Ta[0], G1.neg(Ta[1])))
    schnorr_ok = G1.is_inf(acc)
    jp = (X[0], X[1], 1)
    if Ja:
        jp = G1.add_aff(jp, Ja)
    for z, h in enumerate(rev):
        jp = fixed_table_mul_add(G1, jp, int(p["revealed_msgs"][z], 16) % R, Ys[h], 0, nw, VK_WBITS)
    jinf = G1.is_inf(jp)
    pe = (0, 0, None)
    if not jinf:  # affine in the R' form (curve_lz.h jg_to_aff_rp)
        a = G1.to_aff(jp)
        pe = (a[0], a[1], None)
    counts["prep"] = C.take()
    skip0 = s1 is None or jinf
    skip1 = s2 is None
    q0 = s1 if s1 else ((0, 0), (0, 0))
    q1 = (s2[0], f2_neg(s2[1])) if s2 else ((0, 0), (0, 0))
    f = miller2([(q0, pe, skip0), (q1, (gtil[0], gtil[1], None), skip1)])
    counts["miller"] = C.take()
    r = final_exp(f)
    counts["fexp"] = C.take()
    ok = f12_is_one(r) and s1 is not None and s2 is not None and schnorr_ok
    return int(ok), counts


def pok_sigg1(d, p, vk_aff, gtil):
    """k_prep_pok_g1pl (SigG1: the Schnorr MSM and J' in G2 on lane pairs) -> k_miller<1,false> -> k_fexp_q."""
    counts = {}
    q, rev = d["q"], d["revealed"]
    X, Ys = vk_aff
    s1 = decode(G1, bytes.fromhex(p["sigma1"]))
    s2 = decode(G1, bytes.fromhex(p["sigma2"]))
    Ja = decode(G2, bytes.fromhex(p["J"]))
    resp = [int(h, 16) % R for h in p["responses"]]
    chal = int(p["chal"], 16) % R
    nw = -(-256 // VK_WBITS)
    acc = fixed_table_mul_add(G2, G2.inf(), resp[0], gtil, 0, nw, VK_WBITS)
    slot = 1
    for h in range(q):
        if h in rev:
            continue
        acc = fixed_table_mul_add(G2, acc, resp[slot], Ys[h], 0, nw, VK_WBITS)
        slot += 1
    if Ja:  # chal J in fixed 4-bit windows from a per-lane table of d J, d = 1..15
        tab = [(Ja[0], Ja[1], F2_ONE)]
        for _ in range(14):
            tab.append(G2.add_aff(tab[-1], Ja))
        sacc = G2.inf()
        for win in range(63, -1, -1):
            for _ in range(4):
                sacc = G2.dbl_j(sacc)
            dd = (chal >> (4 * win)) & 15
            if dd:
                sacc = G2.add_j(sacc, tab[dd - 1])
        acc = G2.add_j(acc, sacc)
    Ta = decode(G2, bytes.fromhex(p["T"]))
    if Ta:
        acc = G2.add_aff(acc, (Ta[0], G2.neg(Ta[1])))
    schnorr_ok = G2.is_inf(acc)
    jp = (X[0], X[1], F2_ONE)
    if Ja:
        jp = G2.add_aff(jp, Ja)
    for z, h in enumerate(rev):
        jp = fixed_table_mul_add(G2, jp, int(p["revealed_msgs"][z], 16) % R, Ys[h], 0, nw, VK_WBITS)
    pr = G2.to_aff(jp)
    v, _, cnt = _pair_sigg1(s1, s2, pr, gtil, counts)
    return int(v and schnorr_ok), cnt


# ---------------------------------------------------------------- RLC batch mode (rlc.hip + fold.hip, SigG2)
def _f2_inv_plain(x):
    n = (x[0] * x[0] + x[1] * x[1]) % P
    ni = pow(n, P - 2, P)
    return (x[0] * ni % P, -x[1] * ni % P)


PSI_CX = _f2_inv_plain(_xi_pow((P - 1) // 3))
PSI_CY = _f2_inv_plain(_xi_pow((P - 1) // 2))


def g2_in_subgroup(a):  # curve_pl.h pl::g2_in_subgroup: psi(Q) == [x] Q on the pair-lane Fp2
    J = (a[0], a[1], F2_ONE)
    t = J
    for bit in range(62, -1, -1):
        t = G2.dbl_j(t)
        if (X_ABS >> bit) & 1:
            t = G2.add_j(t, J)
    ps = (f2_mul(f2_conj(a[0]), PSI_CX), f2_mul(f2_conj(a[1]), PSI_CY))
    return G2.is_inf(G2.add_aff(t, ps))


RLC_N, RLC_PSEUDO = 131072, 16  # credentials per GPU (config 3), fold pseudo-credentials (one per window)


def rlc_sigg2(cred, vk_aff, gtil_aff, q, rnd):
    """k_rlc_check_sigg2 + k_rlc_msm_sigg2 -> fold (fold.hip) -> k_miller4<2> (four
    credentials' first pairs per shared-squaring loop) -> the product tree over RLC_N / 4 values; the
    finish's 16 window pairs (one-pair loops, miller_wide.hip k_miller_wide) and the batch's one final
    exponentiation are outside the partial's phases (amortised over RLC_N they are < 0.1 %).
    delta is a random 128-bit value here (the counts do not depend on the key stream)."""
    counts = {}
    s1 = decode(G2, bytes.fromhex(cred["sigma1"]))
    s2 = decode(G2, bytes.fromhex(cred["sigma2"]))
    assert g2_in_subgroup(s2)  # sigma_1's test comes from the Miller loop's T (counted there)
    msgs = [int.from_bytes(bytes.fromhex(m), "big") % R for m in cred["msgs"]]
    X, Ys = vk_aff
    delta = rnd.getrandbits(128) - (1 << 127)
    d = delta % R
    nw = -(-256 // VK_WBITS)
    acc = fixed_table_mul_add(G1, G1.inf(), abs(delta), X, 0, nw, VK_WBITS)  # +-|delta| X~ (fr.h rlc_delta_abs)
    if delta < 0:
        acc = (acc[0], G1.neg(acc[1]), acc[2])
    for j in range(q):
        acc = fixed_table_mul_add(G1, acc, d * msgs[j] % R, Ys[j], 0, nw, VK_WBITS)
    a = G1.to_aff(acc)  # affine in the R' form (curve_lz.h jg_to_aff_rp)
    pe = (a[0], a[1], None)
    counts["prep"] = C.take()
    f = miller2([(s1, pe, False)])
    m1 = C.take()  # one pair alone: a window pseudo-credential
    f = miller2([(s1, pe, False), (s1, pe, False)])  # twin: two credentials, one loop
    m2 = C.take() / 2
    f = miller2([(s1, pe, False)] * 4)  # k_miller4: four credentials, one loop
    for _ in range(4):  # miller_t_in_subgroup per credential: psi(sigma_1) against its T, 2 Fp2 products + psi
        f2_mul(s1[0], s1[0])
        f2_mul(s1[0], s1[0])
        f2_mul(s1[0], s1[0])
        f2_mul(s1[0], s1[0])
    m4 = C.take() / 4
    # fold: one signed point per nonzero digit into a 16-entry chunk (the chunk's first addition is
    # free), then one Jacobian addition of the chunk partial into its bucket
    neg2 = (s2[0], f2_neg(s2[1]))
    G2.add_aff((neg2[0], neg2[1], F2_ONE), s1)
    add_m = C.take()
    G2.add_j((neg2[0], neg2[1], F2_ONE), (s1[0], s1[1], F2_ONE))
    addj_m = C.take()
    fold = 16 * add_m * 15 / 16 + addj_m
    counts["prep"] = round(counts["prep"] + fold, 1)  # the fold runs between the checks and the MSM
    counts["miller"] = round(m4, 1)
    f12_mul(f, f)
    counts["reduce"] = round(C.take() * (RLC_N / 4) / RLC_N, 1)
    counts["miller_twin_per_credential"] = m2
    counts["miller_one_pair"] = m1
    return counts


def vk_from_fixture(d):
    g = G1 if d["mode"] == "G2" else G2
    dec = lambda h: decode(g, bytes.fromhex(h))  # noqa: E731
    X = dec(d["vk"]["X"])
    Ys = [dec(y) for y in d["vk"]["Y"]]
    gt = dec(d["g_tilde"])
    C.take()
    return (X, Ys), gt


def run_fixture(d, limit=None):
    vk, gt = vk_from_fixture(d)
    fn = verify_sigg2 if d["mode"] == "G2" else verify_sigg1
    out = []
    for c in d["creds"][:limit]:
        out.append((c, fn(c, vk, gt, d["q"])))
    return out


def main():
    global VK_WBITS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {"unit": "M = one 381-bit Montgomery multiplication = 288 algorithmic 32x32->64 mads",
           "mads_per_M": 288,
           "source": "tools/opcount.py (instrumented mirror of the HIP kernels; GT bytes pinned to "
                     "tests/golden/verify_g*_q6.json by tests/test_opcount.py)",
           "configs": {}}
    for name, key in (("verify_g2_q6.json", "verify_sigg2_q6_shared_vk"),
                      ("verify_g1_q6.json", "verify_sigg1_q6_shared_vk")):
        with open(os.path.join(root, "tests", "golden", name)) as f:
            d = json.load(f)
        rows = [r for c, r in run_fixture(d) if c["kind"] == "valid"]
        ks = rows[0][2].keys()
        avg = {k: sum(r[2][k] for r in rows) / len(rows) for k in ks}
        res["configs"][key] = {"credentials_averaged": len(rows),
                               "M_per_credential": {k: round(v, 1) for k, v in avg.items()},
                               "mads_per_credential": {k: round(v * 288) for k, v in avg.items()}}
    with open(os.path.join(root, "tests", "golden", "aggregate_g2_t67_subsets.json")) as f:
        d = json.load(f)
    sig, vkX, vkY, cnt = aggregate_case(d, d["cases"][0], wb=BENCH_ISS_BITS)
    assert enc(G2, sig).hex() == d["cases"][0]["out_sigma2"] and enc(G1, vkX).hex() == d["cases"][0]["out_X"]
    res["configs"]["aggregate_sigg2_t67"] = {
        "credentials_averaged": 1, "M_per_credential": {k: round(v, 1) for k, v in cnt.items()},
        "mads_per_credential": {k: round(v * 288) for k, v in cnt.items()},
        "note": "straus_sigma2 = Signature::aggregate (67-point G2 Straus MSM); fixed_verkey = Verkey::aggregate "
                "(q+1 = 7 67-point G1 fixed-base MSMs from the issuer tables, 16-bit windows: the width the bench "
                "opts into, BENCH_ISS_BITS; the library's <= 16 GiB default picks 13); case 0 of "
                "tests/golden/aggregate_g2_t67_subsets.json, outputs checked against the fixture"}
    with open(os.path.join(root, "tests", "golden", "pok_g2_q32.json")) as f:
        d = json.load(f)
    VK_WBITS = 20  # q = 32: 34 bases, 22-bit tables would exceed the 96 GiB budget
    vk, gt = vk_from_fixture(d)
    rows = []
    for p in d["proofs"]:
        v, cnt = pok_sigg2(d, p, vk, gt)
        assert v == p["verdict"], p["kind"]
        if p["kind"] == "valid":
            rows.append(cnt)
    res["configs"]["pok_sigg2_q32_r8"] = {
        "credentials_averaged": len(rows),
        "M_per_credential": {k: round(sum(r[k] for r in rows) / len(rows), 1) for k in rows[0]},
        "mads_per_credential": {k: round(sum(r[k] for r in rows) / len(rows) * 288) for k in rows[0]},
        "note": "valid proofs of tests/golden/pok_g2_q32.json (verdicts of every kind checked)"}
    with open(os.path.join(root, "tests", "golden", "verify_g2_q16.json")) as f:
        d = json.load(f)
    VK_WBITS = 22
    vk, gt = vk_from_fixture(d)
    rnd = random.Random(3)
    rows = [rlc_sigg2(c, vk, gt, d["q"], rnd) for c in d["creds"] if c["kind"] == "valid"]
    res["configs"]["rlc_sigg2_q16"] = {
        "credentials_averaged": len(rows),
        "M_per_credential": {k: round(sum(r[k] for r in rows) / len(rows), 1) for k in rows[0]},
        "mads_per_credential": {k: round(sum(r[k] for r in rows) / len(rows) * 288) for k in rows[0]},
        "note": "valid credentials of tests/golden/verify_g2_q16.json; prep = decode + sigma_2's G2 subgroup check + "
                "the fold's bucket additions + delta-scaled fixed-base MSM (sigma_1's check comes from the Miller "
                "loop's T); miller = a quarter of a four-credential shared-squaring Miller loop (k_miller4, with the four subgroup tests); the finish's 16 window pairs and its one final exponentiation are amortised over 131,072 credentials (< 0.1 %) and not counted; reduce = the partial's product tree over 32,768 values, per credential"}
    # per-credential verkeys (Signature::verify with the caller's verkey; pervk.hip), q = 6
    VK_WBITS = 22
    for name, key, mode in (("verify_g2_q6_pervk.json", "verify_sigg2_q6_pervk", "G2"),
                            ("verify_g1_q6_pervk.json", "verify_sigg1_q6_pervk", "G1")):
        with open(os.path.join(root, "tests", "golden", name)) as f:
            d = json.load(f)
        gt = decode(G1 if mode == "G2" else G2, bytes.fromhex(d["g_tilde"]))
        C.take()
        rows = []
        for c in d["creds"]:
            v, gtb, cnt = verify_pervk(c, gt, mode)
            assert v == c["verdict"] and gtb.hex() == c["gt"], c["kind"]
            if c["kind"] == "valid":
                rows.append(cnt)
        res["configs"][key] = {
            "credentials_averaged": len(rows),
            "M_per_credential": {k: round(sum(r[k] for r in rows) / len(rows), 1) for k in rows[0]},
            "mads_per_credential": {k: round(sum(r[k] for r in rows) / len(rows) * 288) for k in rows[0]},
            "note": f"valid credentials of tests/golden/{name} (verdicts and GT bytes of every kind checked); prep = "
                    "one signed-4-bit Straus over the q bases + X~ (the kernel's repeated doubling chain on the "
                    "second lane of a SigG2 pair is not counted)"}
    # SigG1 forms of configs 4 and 5
    with open(os.path.join(root, "tests", "golden", "aggregate_g1_t67_subsets.json")) as f:
        d = json.load(f)
    sig, vkX, vkY, cnt = aggregate_case(d, d["cases"][0], wb=BENCH_ISS_BITS)
    assert enc(G1, sig).hex() == d["cases"][0]["out_sigma2"] and enc(G2, vkX).hex() == d["cases"][0]["out_X"]
    res["configs"]["aggregate_sigg1_t67"] = {
        "credentials_averaged": 1, "M_per_credential": {k: round(v, 1) for k, v in cnt.items()},
        "mads_per_credential": {k: round(v * 288) for k, v in cnt.items()},
        "note": "SigG1: straus_sigma2 = Signature::aggregate (67-point G1 Straus MSM); fixed_verkey = Verkey::aggregate "
                "(q+1 = 7 67-point G2 fixed-base MSMs from the issuer tables, 16-bit windows: the width the bench "
                "opts into, BENCH_ISS_BITS; the library's default picks 12); case 0 of "
                "tests/golden/aggregate_g1_t67_subsets.json, outputs checked"}
    with open(os.path.join(root, "tests", "golden", "pok_g1_q32.json")) as f:
        d = json.load(f)
    VK_WBITS = 20
    g2 = lambda h: decode(G2, bytes.fromhex(h))  # noqa: E731
    vk, gt = (g2(d["vk"]["X"]), [g2(y) for y in d["vk"]["Y"]]), g2(d["g_tilde"])
    C.take()
    rows = []
    for p in d["proofs"]:
        v, cnt = pok_sigg1(d, p, vk, gt)
        assert v == p["verdict"], p["kind"]
        if p["kind"] == "valid":
            rows.append(cnt)
    res["configs"]["pok_sigg1_q32_r8"] = {
        "credentials_averaged": len(rows),
        "M_per_credential": {k: round(sum(r[k] for r in rows) / len(rows), 1) for k in rows[0]},
        "mads_per_credential": {k: round(sum(r[k] for r in rows) / len(rows) * 288) for k in rows[0]},
        "note": "SigG1, valid proofs of tests/golden/pok_g1_q32.json (verdicts of every kind checked), 20-bit tables"}
    out = os.path.join(root, "tests", "fixtures", "opcount.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    sys.exit(main())
