// One Fp12 element on a whole wave: the wide forms of the pair-lane tower (tower_pl.h) — device code.
//
// A latency-bound chain (the RLC batch's one final exponentiation and product tree, every credential of
// a small batch, the wide Miller loop) runs one element per wave instead of one per lane pair.  The
// contract of everything in this file:
//   * every one of the wave's 32 lane pairs holds the SAME values on entry and on return;
//   * the independent Fp2 products of a step are spread over the pairs, ONE product a pair a level —
//     the 18 of f12_mul, the 6 of f12_cyc_sqr, f4_mul's 3 — as one call (same instructions, different
//     data), so a step's latency holds one product instead of 6 or 18;
//   * the results are gathered with ds_bpermute shuffles (bcast_f2), and the combinations are spread
//     too: a lone wave's time is its instruction count, so no pair redoes what another computes;
//   * pair_idx() is threadIdx.x / 2 and the shuffles address lanes of the calling wave, so the code is
//     valid only in 64-lane blocks, or in a wave-uniform half of a 128-lane block: in wave 0 as it
//     stands, in wave 1 only the functions that take the pair index as an argument (k_miller_wide2).
// Users: fexp_pl.hip (k_fexp1, k_f12_reduce_wide) and miller_wide.hip.
#pragma once
#include "tower_pl.h"
#include "tower_q.h"  // lz::fp_inv_int_quad (f2_inv_q)

namespace cc {
namespace pl {

// an Fp12 operand's map on its way into a product (the final exponentiation's steps; f12_frobs_wide
// takes OP_FROB / OP_FROB2)
enum FxOp { OP_ID = 0, OP_CONJ = 1, OP_FROB = 2, OP_FROB2 = 3 };

DEV int pair_idx() { return (int)(threadIdx.x >> 1); }
// tower_pl.h f2_inv for a value every pair of the wave holds: the norm is then the same on all four
// lanes of each quad, so its divstep inversion runs in the quad form (tower_q.h fp_inv_int_quad: the
// iteration's f, g, d, e one per lane, one update chain a lane instead of four)
DEV void f2_inv_q(Fp2& r, const Fp2& x) {
    const Fp xs = swp(x.c);
    Fp n = fp_mul2_v(x.c, x.c, xs, xs), ni;
    lz::fp_inv_int_quad(ni, n);  // plain integer inverse of the Montgomery residue
    constexpr uint32_t R3[NL] = {CC_R3_LIMBS};
    Fp r3;
#pragma unroll
    for (int j = 0; j < NL; j++) r3.v[j] = R3[j];
    fp_mul(n, ni, r3);  // (n R)^-1 R^3 R^-1 = n^-1 R (field.h fp_inv)
    Fp2 t;
    fp_mul(t.c, x.c, n);
    f2_conj(r, t);
}
DEV Fp2 bcast_f2(const Fp2& v, int src_pair) {
    const int lane = 2 * src_pair + (int)half_id();
    Fp2 r;
#pragma unroll
    for (int k = 0; k < NL; k++) r.c.v[k] = (uint32_t)__shfl((int)v.c.v[k], lane);
    return r;
}
DEV Fp2 f2_pick(int j, const Fp2* opts, int nopt) {
    Fp2 r = opts[0];
    for (int k = 1; k < nopt; k++) r.c = fp_sel(j == k, opts[k].c, r.c);
    return r;
}
// pair j's operands: opts1[j], opts2[j] for j < n (pair-uniform j); o1, o2 unchanged elsewhere
DEV void pick2(Fp2& o1, Fp2& o2, int j, const Fp2* a, const Fp2* b, int n) {
    for (int k = 0; k < n; k++) {
        o1.c = fp_sel(j == k, a[k].c, o1.c);
        o2.c = fp_sel(j == k, b[k].c, o2.c);
    }
}
// an Fp factor multiplies as the Fp2 (k, 0)
DEV Fp2 f2_of_fp(const Fp& k) {
    Fp z;
    fp_zero(z);
    Fp2 r;
    r.c = fp_sel(half_id() != 0, z, k);
    return r;
}
DEV void line_fp12(Fp12& L, const Fp2& a0, const Fp2& a2, const Fp2& a3) {  // A + C w^2 (pairing.inc)
    L.a.a = a0;
    L.a.b = a3;
    f2_zero(L.b.a);
    f2_zero(L.b.b);
    L.c.a = a2;
    f2_zero(L.c.b);
}

// f4_mul's three products of operand set m, spread: pair 3m + p computes product p
DEV void f4_from_products(Fp4& r, const Fp2& p0, const Fp2& p1, const Fp2& p2) {
    Fp2 t;
    f2_mul_xi(t, p1);
    f2_add(r.a, p0, t);
    f2_sub(t, p2, p0);
    f2_sub(r.b, t, p1);
}

// = f12_mul (tower.inc): the six f4 products (t0, t1, t2 and the three cross terms) as 18 Fp2
// products on pairs 0..17 — f12w_operands picks pair j's two factors, f12w_assemble combines the
// products (so a caller can run other independent products on pairs 18..31 in the same call).
// Operand m of the six (a, b, c, b + c, a + b, a + c) is formed by each pair for its own m only: one
// pick of its first term, one of its second (zero for m < 3), one f4 addition.
DEV Fp4 f4_pick3(int k, const Fp4& a, const Fp4& b, const Fp4& c) {  // k in {0, 1, 2}
    Fp4 r = a;
    r.a.c = fp_sel(k == 1, b.a.c, r.a.c);
    r.b.c = fp_sel(k == 1, b.b.c, r.b.c);
    r.a.c = fp_sel(k == 2, c.a.c, r.a.c);
    r.b.c = fp_sel(k == 2, c.b.c, r.b.c);
    return r;
}
DEV Fp4 f12w_term(int m, const Fp12& x) {
    // first term a b c b a a, second - - - c b c (m = 0..5)
    Fp4 u = f4_pick3((0x001210 >> (4 * m)) & 15, x.a, x.b, x.c);
    Fp4 v = f4_pick3((0x212000 >> (4 * m)) & 15, x.a, x.b, x.c);
    Fp4 r;
    f4_add(r, u, v);
    r.a.c = fp_sel(m < 3, u.a.c, r.a.c);
    r.b.c = fp_sel(m < 3, u.b.c, r.b.c);
    return r;
}
DEV void f12w_operands(Fp2& o1, Fp2& o2, int j, const Fp12& x, const Fp12& y) {
    j %= 18;
    const int m = j / 3, p = j % 3;
    const Fp4 U = f12w_term(m, x), V = f12w_term(m, y);
    Fp2 s1, s2;
    o1 = U.a;
    o2 = V.a;
    f2_add_lz(s1, U.a, U.b);
    f2_add_lz(s2, V.a, V.b);
    o1.c = fp_sel(p == 1, U.b.c, o1.c);
    o2.c = fp_sel(p == 1, V.b.c, o2.c);
    o1.c = fp_sel(p == 2, s1.c, o1.c);
    o2.c = fp_sel(p == 2, s2.c, o2.c);
}
// The combination, spread: (1) pair k < 12 forms component k & 1 of Fp4 result k / 2 (t0, t1, t2 and
// the three cross products, f4_mul's (p0 + xi p1, p2 - p0 - p1)) from its three products, gathered
// with one shuffle each; (2) pair q < 6 forms Fp12 coefficient q (a.a, a.b, b.a, b.b, c.a, c.b) as
// xi^[q = 0] (G1 - G2 - G3) + xi^[q = 2] G4 from four components of step 1:
//     a.a = xi (s_bc.b - t1.b - t2.b) + t0.a     a.b = s_bc.a - t1.a - t2.a + t0.b
//     b.a = s_ab.a - t0.a - t1.a + xi t2.b       b.b = s_ab.b - t0.b - t1.b + t2.a
//     c.a = s_ac.a - t0.a - t2.a + t1.a          c.b = s_ac.b - t0.b - t2.b + t1.b
// (3) the six coefficients broadcast to every pair.  Same field values as the sequential assembly.
DEV void f12w_assemble(Fp12& r, const Fp2& prod, int base = 0) {
    const int j = pair_idx();
    Fp2 C;
    {
        const int k = j % 12, m = k >> 1;
        const Fp2 p0 = bcast_f2(prod, base + 3 * m), p1 = bcast_f2(prod, base + 3 * m + 1),
                  p2 = bcast_f2(prod, base + 3 * m + 2);
        Fp2 t, ca, cb;
        f2_mul_xi(t, p1);
        f2_add(ca, p0, t);
        f2_sub(t, p2, p0);
        f2_sub(cb, t, p1);
        C = ca;
        C.c = fp_sel(k & 1, cb.c, ca.c);
    }
    Fp2 O;
    {
        const int q = j % 6;
        const Fp2 G1 = bcast_f2(C, (0xBA9867 >> (4 * q)) & 15), G2 = bcast_f2(C, (0x101023 >> (4 * q)) & 15),
                  G3 = bcast_f2(C, (0x543245 >> (4 * q)) & 15);
        Fp2 G4 = bcast_f2(C, (0x324510 >> (4 * q)) & 15), u, v;
        f2_sub(u, G1, G2);
        f2_sub(u, u, G3);
        f2_mul_xi(v, u);
        u.c = fp_sel(q == 0, v.c, u.c);
        f2_mul_xi(v, G4);
        G4.c = fp_sel(q == 2, v.c, G4.c);
        f2_add(O, u, G4);
    }
    r.a.a = bcast_f2(O, 0);
    r.a.b = bcast_f2(O, 1);
    r.b.a = bcast_f2(O, 2);
    r.b.b = bcast_f2(O, 3);
    r.c.a = bcast_f2(O, 4);
    r.c.b = bcast_f2(O, 5);
}
DEV void f12_mul_wide(Fp12& r, const Fp12& x, const Fp12& y) {
    Fp2 o1, o2, prod;
    f12w_operands(o1, o2, pair_idx(), x, y);
    f2_mul(prod, o1, o2);
    f12w_assemble(r, prod);
}

// Granger-Scott squaring for elements of the cyclotomic subgroup (AMCL FP12::usqr):
//   a' = 3 a^2 - 2 conj(a), b' = 3 s c^2 + 2 conj(b), c' = 3 b^2 - 2 conj(c)
// with f4_sqr of a, b, c as 6 products on pairs 0..5 (pair 2m: ab, pair 2m + 1: (a + b)(a + xi b) of
// operand m)
DEV void f12_cyc_sqr_wide(Fp12& r, const Fp12& x) {
    const int j = pair_idx() % 6;
    const int m = j >> 1;
    Fp2 oa[3] = {x.a.a, x.b.a, x.c.a}, ob[3] = {x.a.b, x.b.b, x.c.b};
    const Fp2 a = f2_pick(m, oa, 3), b = f2_pick(m, ob, 3);
    Fp2 o1 = a, o2 = b, s0, s1, prod;
    f2_add_lz(s0, a, b);
    f2_mul_xi(s1, b);
    f2_add_lz(s1, s1, a);
    o1.c = fp_sel(j & 1, s0.c, o1.c);
    o2.c = fp_sel(j & 1, s1.c, o2.c);
    f2_mul(prod, o1, o2);
    // the combination, spread: pair q < 6 forms coefficient q (a.a, a.b, b.a, b.b, c.a, c.b) of
    //   a' = 3A - 2 conj(a), b' = 3 s C + 2 conj(b), c' = 3 B - 2 conj(c)   (A, B, C the f4 squares:
    //   (t - ab - xi ab, 2ab) from pair 2m's ab and pair 2m + 1's t = (a + b)(a + xi b))
    // as 3u - 2y with u = t - ab - xi ab (a.a, b.b, c.a) or 3u + 2y with u = 2ab (xi 2ab for b.a)
    const int q = pair_idx() % 6;
    const Fp2 Gab = bcast_f2(prod, (0x224400 >> (4 * q)) & 15), Gt = bcast_f2(prod, (0x135111 >> (4 * q)) & 15);
    const bool fa = q == 0 || q == 3 || q == 4;
    Fp2 u, v, w, y;
    f2_sub(u, Gt, Gab);
    f2_mul_xi(v, Gab);
    f2_sub(u, u, v);
    f2_dbl(w, Gab);
    f2_mul_xi(v, w);
    w.c = fp_sel(q == 2, v.c, w.c);
    u.c = fp_sel(fa, u.c, w.c);
    const Fp2 cs[6] = {x.a.a, x.a.b, x.b.a, x.b.b, x.c.a, x.c.b};
    y = f2_pick(q, cs, 6);
    f2_neg(v, y);
    y.c = fp_sel(fa, v.c, y.c);
    f2_add(w, u, y);  // u +- y
    f2_dbl(w, w);
    f2_add(v, w, u);  // 3u +- 2y
    r.a.a = bcast_f2(v, 0);
    r.a.b = bcast_f2(v, 1);
    r.b.a = bcast_f2(v, 2);
    r.b.b = bcast_f2(v, 3);
    r.c.a = bcast_f2(v, 4);
    r.c.b = bcast_f2(v, 5);
}

// acc <- x z (f12_mul_wide, pairs 0..17) and y <- y^2 (f12_cyc_sqr_wide, pairs 18..23) in ONE level:
// pow-by-x's tail multiplies acc by snapshots of y while y keeps squaring (each operand read before
// either result is written, so z may be y)
DEV void f12_mul_cs_wide(Fp12& acc, const Fp12& x, const Fp12& z, Fp12& y) {
    const int j = pair_idx();
    Fp2 o1, o2, prod;
    f12w_operands(o1, o2, j, x, z);
    {
        const int jc = j % 6;  // pairs 18..23: product jc = j - 18
        const int m = jc >> 1;
        Fp2 oa[3] = {y.a.a, y.b.a, y.c.a}, ob[3] = {y.a.b, y.b.b, y.c.b};
        const Fp2 a = f2_pick(m, oa, 3), b = f2_pick(m, ob, 3);
        Fp2 c1 = a, c2 = b, s0, s1;
        f2_add_lz(s0, a, b);
        f2_mul_xi(s1, b);
        f2_add_lz(s1, s1, a);
        c1.c = fp_sel(jc & 1, s0.c, c1.c);
        c2.c = fp_sel(jc & 1, s1.c, c2.c);
        o1.c = fp_sel(j >= 18, c1.c, o1.c);
        o2.c = fp_sel(j >= 18, c2.c, o2.c);
    }
    f2_mul(prod, o1, o2);
    Fp2 v;
    {  // f12_cyc_sqr_wide's combination, its products on pairs 18..23
        const int q = j % 6;
        const Fp2 Gab = bcast_f2(prod, 18 + ((0x224400 >> (4 * q)) & 15)),
                  Gt = bcast_f2(prod, 18 + ((0x135111 >> (4 * q)) & 15));
        const bool fa = q == 0 || q == 3 || q == 4;
        Fp2 u, w, t;
        f2_sub(u, Gt, Gab);
        f2_mul_xi(t, Gab);
        f2_sub(u, u, t);
        f2_dbl(w, Gab);
        f2_mul_xi(t, w);
        w.c = fp_sel(q == 2, t.c, w.c);
        u.c = fp_sel(fa, u.c, w.c);
        const Fp2 cs[6] = {y.a.a, y.a.b, y.b.a, y.b.b, y.c.a, y.c.b};
        Fp2 yy = f2_pick(q, cs, 6);
        f2_neg(t, yy);
        yy.c = fp_sel(fa, t.c, yy.c);
        f2_add(w, u, yy);
        f2_dbl(w, w);
        f2_add(v, w, u);
    }
    f12w_assemble(acc, prod);
    y.a.a = bcast_f2(v, 0);
    y.a.b = bcast_f2(v, 1);
    y.b.a = bcast_f2(v, 2);
    y.b.b = bcast_f2(v, 3);
    y.c.a = bcast_f2(v, 4);
    y.c.b = bcast_f2(v, 5);
}

// x^p (OP_FROB) / x^(p^2) (OP_FROB2), spread: pair q < 6 maps coefficient q (a.a, a.b, b.a, b.b, c.a,
// c.b; the coefficient of W^k, k = 0 3 1 4 2 5) to conj(c) gamma1_k, or c gamma2_k (pairing.h kGamma1 /
// kGamma2, gamma_0 = 1), then the six are broadcast
DEV void f12_frobs_wide(Fp12& x, int op) {
    const int q = pair_idx() % 6, k = (0x524130 >> (4 * q)) & 15;
    const Fp2 cs[6] = {x.a.a, x.a.b, x.b.a, x.b.b, x.c.a, x.c.b};
    Fp2 c = f2_pick(q, cs, 6), r;
    if (op == OP_FROB) {  // wave-uniform
        Fp2 g, t;
        load_f2c(g, kGamma1[k]);
        f2_conj(t, c);
        f2_mul(r, t, g);
    } else {
        Fp g;
#pragma unroll
        for (int j = 0; j < NL; j++) g.v[j] = kGamma2[k][j];
        f2_mul_fp(r, c, g);
    }
    x.a.a = bcast_f2(r, 0);
    x.a.b = bcast_f2(r, 1);
    x.b.a = bcast_f2(r, 2);
    x.b.b = bcast_f2(r, 3);
    x.c.a = bcast_f2(r, 4);
    x.c.b = bcast_f2(r, 5);
}

// k Fp4 products x_m y_m (m < k <= 10) as 3k Fp2 products on pairs 0..3k-1 (f4_mul's Karatsuba: pair
// 3m + p forms x.a y.a, x.b y.b, (x.a + x.b)(y.a + y.b) for p = 0, 1, 2); every pair gets all k results
DEV void f4w_mul(Fp4* r, const Fp4* x, const Fp4* y, int k) {
    const int j = pair_idx() % (3 * k), m = j / 3, p = j % 3;
    Fp2 xa[10], xb[10], ya[10], yb[10];
    for (int t = 0; t < k; t++) {
        xa[t] = x[t].a; xb[t] = x[t].b; ya[t] = y[t].a; yb[t] = y[t].b;
    }
    const Fp2 Xa = f2_pick(m, xa, k), Xb = f2_pick(m, xb, k), Ya = f2_pick(m, ya, k), Yb = f2_pick(m, yb, k);
    Fp2 o1 = Xa, o2 = Ya, s1, s2, pr;
    f2_add_lz(s1, Xa, Xb);
    f2_add_lz(s2, Ya, Yb);
    o1.c = fp_sel(p == 1, Xb.c, o1.c);
    o2.c = fp_sel(p == 1, Yb.c, o2.c);
    o1.c = fp_sel(p == 2, s1.c, o1.c);
    o2.c = fp_sel(p == 2, s2.c, o2.c);
    f2_mul(pr, o1, o2);
    for (int t = 0; t < k; t++) f4_from_products(r[t], bcast_f2(pr, 3 * t), bcast_f2(pr, 3 * t + 1), bcast_f2(pr, 3 * t + 2));
}

// x^-1 over the cubic extension: with A0 = a^2 - s bc, B0 = s c^2 - ab, C0 = b^2 - ac and
// F = s (c B0 + b C0) + a A0 in Fp4, x^-1 = (A0 + B0 w + C0 w^2) / F.  Its 40 Fp2 products as five
// spread calls and the one inversion (a^2, bc, c^2, ab, b^2, ac | c B0, b C0, a A0 | F.a^2, F.b^2 |
// inverse | A0, B0, C0 by 1/F)
DEV void f12_inv_wide(Fp12& r, const Fp12& x) {
    Fp4 P[6];
    {
        const Fp4 X[6] = {x.a, x.b, x.c, x.a, x.b, x.a}, Y[6] = {x.a, x.c, x.c, x.b, x.b, x.c};
        f4w_mul(P, X, Y, 6);
    }
    Fp4 A0, B0, C0, t;
    f4_mul_s(t, P[1]);
    f4_sub(A0, P[0], t);  // a^2 - s bc
    f4_mul_s(t, P[2]);
    f4_sub(B0, t, P[3]);  // s c^2 - ab
    f4_sub(C0, P[4], P[5]);  // b^2 - ac
    Fp4 F;
    {
        const Fp4 X[3] = {x.c, x.b, x.a}, Y[3] = {B0, C0, A0};
        f4w_mul(P, X, Y, 3);
        f4_add(F, P[0], P[1]);
        f4_mul_s(F, F);
        f4_add(F, F, P[2]);
    }
    Fp2 n, pr, u, v;
    {  // (a + b s)^-1 = (a - b s) / (a^2 - xi b^2): pairs 0, 1 square F.a, F.b
        const int j = pair_idx() & 1;
        Fp2 in = F.a;
        in.c = fp_sel(j == 1, F.b.c, in.c);
        f2_sqr(pr, in);
        f2_mul_xi(u, bcast_f2(pr, 1));
        f2_sub(n, bcast_f2(pr, 0), u);  // a^2 - xi b^2
    }
    f2_inv_q(n, n);
    {
        const int j = pair_idx() & 1;
        Fp2 in = F.a;
        in.c = fp_sel(j == 1, F.b.c, in.c);
        f2_mul(pr, in, n);
        u = bcast_f2(pr, 0);
        v = bcast_f2(pr, 1);
    }
    Fp4 Fi;
    Fi.a = u;
    f2_neg(Fi.b, v);
    {
        const Fp4 X[3] = {A0, B0, C0}, Y[3] = {Fi, Fi, Fi};
        f4w_mul(P, X, Y, 3);
    }
    r.a = P[0];
    r.b = P[1];
    r.c = P[2];
}

}  // namespace pl
}  // namespace cc
