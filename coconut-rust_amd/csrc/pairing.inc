// Optimal-ate pieces written only in terms of the tower primitives (f2_*, f4_*, f12_*, f2_half):
// the sparse line multiply and the doubling/addition line functions.  Textually included inside
// namespace cc (pairing.h) and cc::pl (tower_pl.h); see pairing.h for the algorithm notes.  No include
// guard.  (The Frobenius maps and the cyclotomic steps live with the towers that run them: tower_lz.h,
// tower_q.h, tower_wide.h.)
// ---------------------------------------------------------------- sparse line multiply
// f *= (A + C w^2) with A = (l0, l3) in Fp4 and C = (l2, 0): 13 Fp2 multiplications.
DEV void f12_mul_line(Fp12& f, const Fp2& l0, const Fp2& l2, const Fp2& l3) {
    Fp4 A;
    A.a = l0;
    A.b = l3;
    // ordered so a and c die after the Karatsuba cross term and b last (low peak liveness)
    Fp4 t0, t2, s;
    f4_mul(t0, f.a, A);       // a A
    f4_mul_f2(t2, f.c, l2);   // c C
    f4_add(s, f.a, f.c);
    {
        Fp4 AC = A;
        f2_add(AC.a, AC.a, l2);
        f4_mul(s, s, AC);     // (a + c)(A + C)
    }
    f4_sub(s, s, t0);
    f4_sub(f.c, s, t2);       // r.c = c A + a C
    f4_mul_f2(s, f.b, l2);    // b C
    f4_mul_s(s, s);
    f4_add(f.a, t0, s);       // r.a = a A + s (b C)
    f4_mul(s, f.b, A);        // b A
    f4_mul_s(t2, t2);
    f4_add(f.b, s, t2);       // r.b = b A + s (c C)
}

// ---------------------------------------------------------------- line functions
struct G2Proj {
    Fp2 x, y, z;  // homogeneous projective on the twist
};

// x * 12
DEV void f2_mul12(Fp2& r, const Fp2& x) {
    Fp2 t4;
    f2_dbl(t4, x);
    f2_dbl(t4, t4);
    Fp2 t8;
    f2_dbl(t8, t4);
    f2_add(r, t8, t4);
}

// Doubling step: T <- 2T; line coefficients before evaluation at P:
//   l0 = 3b'Z^2 - Y^2, l2c = 3X^2 (times x_P), l3c = -2YZ (times y_P).   b' = 4(1+i).
DEV void line_dbl(G2Proj& T, Fp2& l0, Fp2& l2c, Fp2& l3c) {
    Fp2 a, b, c, e, f, g, h, t;
    f2_mul(a, T.x, T.y);
    f2_half(a, a);
    f2_sqr(b, T.y);
    f2_sqr(c, T.z);
    // e = 3 b' c = 12 (1 + i) c
    f2_mul_xi(e, c);
    f2_mul12(e, e);
    f2_dbl(f, e);
    f2_add(f, f, e);
    f2_add(g, b, f);
    f2_half(g, g);
    f2_add_lz(h, T.y, T.z);
    f2_sqr(h, h);
    f2_sub(h, h, b);
    f2_sub(h, h, c);
    f2_sub(l0, e, b);
    f2_sqr(t, T.x);
    f2_dbl(l2c, t);
    f2_add(l2c, l2c, t);
    f2_neg(l3c, h);
    // T
    f2_sub(t, b, f);
    f2_mul(T.x, a, t);
    f2_sqr(t, e);
    f2_sqr(T.y, g);
    f2_sub(T.y, T.y, t);
    f2_sub(T.y, T.y, t);
    f2_sub(T.y, T.y, t);
    f2_mul(T.z, b, h);
}

// Addition step with affine Q: T <- T + Q;
//   l0 = theta x_Q - lambda y_Q, l2c = -theta (times x_P), l3c = lambda (times y_P).
DEV void line_add(G2Proj& T, const Aff<Fp2>& Q, Fp2& l0, Fp2& l2c, Fp2& l3c) {
    Fp2 theta, lambda, c, d, e, f, g, h, t;
    f2_mul(t, Q.y, T.z);
    f2_sub(theta, T.y, t);
    f2_mul(t, Q.x, T.z);
    f2_sub(lambda, T.x, t);
    f2_sqr(c, theta);
    f2_sqr(d, lambda);
    f2_mul(e, lambda, d);
    f2_mul(f, T.z, c);
    f2_mul(g, T.x, d);
    f2_add(h, e, f);
    f2_sub(h, h, g);
    f2_sub(h, h, g);
    f2_mul(l0, theta, Q.x);
    f2_mul(t, lambda, Q.y);
    f2_sub(l0, l0, t);
    f2_neg(l2c, theta);
    l3c = lambda;
    f2_mul(T.x, lambda, h);
    f2_sub(t, g, h);
    f2_mul(t, theta, t);
    f2_mul(c, e, T.y);
    f2_sub(T.y, t, c);
    f2_mul(T.z, T.z, e);
}

// P in G1 prepared for line evaluation: line = l0*pz + l2c*px W^2 + l3c*py W^3.
// Affine P: (x, y, 1).  Jacobian (X, Y, Z): (X Z, Y, Z^3) — the line times Z^3 (an Fp factor).
struct G1Eval {
    Fp px, py, pz;
};

template <bool kAffine>
DEV void eval_line(Fp12& f, const Fp2& l0, const Fp2& l2c, const Fp2& l3c, const G1Eval& P) {
    Fp2 a0, a2, a3;
    if (kAffine) {
        a0 = l0;
    } else {
        f2_mul_fp(a0, l0, P.pz);
    }
    f2_mul_fp(a2, l2c, P.px);
    f2_mul_fp(a3, l3c, P.py);
    f12_mul_line(f, a0, a2, a3);
}
