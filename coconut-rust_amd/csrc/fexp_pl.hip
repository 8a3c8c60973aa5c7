// The one-wave final exponentiation and product tree for gfx950 (AMCL `pair::fexp` via amcl_wrapper
// `GT::ate_2_pairing`, reference src/lib.rs:13): k_fexp1, one element per wave in the
// wide form of tower_wide.h (every lane pair holds the element, a step's independent Fp2 products spread
// over the pairs), for the latency-bound cases — the RLC batch mode's one final exponentiation a batch
// and every credential of a small batch — and k_f12_reduce_wide, one level of the RLC product tree in
// the same form.  Larger batches run the quad-lane lazy-field kernel of fexp_q.hip (cck_fexp picks).
//
// CC_FP_INLINE: the multiplications are inlined inside each step function; the steps themselves are
// out of line and exchange Fp12 values through a per-lane SoA scratch (one load/store per step,
// against thousands of Fp multiplications per step), so each step's code exists once.
#ifdef CC_HOT_INLINE  // build option (Makefile HOT_INLINE=1): inline every Fp multiplication
#define CC_FP_INLINE 1
#endif
#include <cstdlib>
#include <cstring>
#include "codec.h"
#include "launch.h"
#include "lazy.h"  // the compressed squarings run on the lazy field
#include "tower_wide.h"

namespace cc {
namespace pl {

// ================================================================ final exponentiation
// f^((p^6-1)(p^2+1)) then the hard part 3 + (x-1)^2 [p^3 + x p^2 + (x^2-1) p + x^3 - x]
// (= 3*Phi_12(p)/r, AMCL's exponent).  Each step below is one out-of-line function reading its
// Fp12 operands from, and writing its result to, a per-lane SoA slot (12 Fp slots each).
DEV void fx_apply(Fp12& x, int op) {
    if (op == OP_FROB || op == OP_FROB2) f12_frobs_wide(x, op);
    else if (op == OP_CONJ) f12_conj(x, x);
}

// dst <- src^-1
static __device__ __noinline__ void fx_inv(Soa src, Soa dst, size_t i) {
    Fp12 f, t;
    ld_f12(f, src, i);
    f12_inv_wide(t, f);
    st_f12(dst, i, t);
}

// dst <- src^3 (cyclotomic)
static __device__ __noinline__ void fx_cube(Soa src, Soa dst, size_t i) {
    Fp12 f, r;
    ld_f12(f, src, i);
    f12_cyc_sqr_wide(r, f);
    f12_mul_wide(r, r, f);
    st_f12(dst, i, r);
}

// dst <- src^x, x = -|x| (cyclotomic square-and-multiply, then conj).  The base is re-read from src at
// each of the 5 multiplications instead of being held in registers across the 63 squarings.
// Fallback of fx_pow_x below for the (never honestly reached) case of a zero decompression
// denominator.
static __device__ __noinline__ void fx_pow_x_gs(Soa src, Soa dst, size_t i) {
    Fp12 acc;
    ld_f12(acc, src, i);
    for (int b = 62; b >= 0; b--) {
        f12_cyc_sqr_wide(acc, acc);
        if ((X_ABS >> b) & 1ull) {
            asm volatile("" ::: "memory");  // keep the reload inside the loop
            Fp12 y;
            ld_f12(y, src, i);
            f12_mul_wide(acc, acc, y);
        }
    }
    f12_conj(acc, acc);
    st_f12(dst, i, acc);
}

// ---------------------------------------------------------------- compressed cyclotomic squaring
// Karabina's compression (eprint 2010/542) restated for this tower.  For x = a + b w + c w^2 in the
// cyclotomic subgroup (a = a0 + a1 s, b = b0 + b1 s, c = c0 + c1 s), Granger-Scott's b', c' depend on
// b and c only:
//     b0' = 6 xi c0 c1 + 2 b0      b1' = 3 (c0^2 + xi c1^2) - 2 b1
//     c0' = 3 (b0^2 + xi b1^2) - 2 c0      c1' = 6 b0 b1 + 2 c1
// with 2 uv = (u + v)^2 - u^2 - v^2: six Fp2 squarings against Granger-Scott's six Fp2
// multiplications.  a is recovered from x conj(x) = 1 (its w and w^2 coefficients are linear in
// a0, a1):
//     a0 = (b0 Nb + xi c1 Nc) / D,  a1 = (c0 Nc + b1 Nb) / D,
//     Nb = b0^2 - xi b1^2,  Nc = c0^2 - xi c1^2,  D = 2 (b0 c0 - xi b1 c1)
// (decompress3_wide below; tests/test_fexp_algebra.py checks both against the oracle's Fp12
// arithmetic; fexp_q.hip runs the same formulas one component a lane).
//
// The squaring with the state spread: pair q (mod 4) holds component q of (b0, b1, c0, c1).  Pair t
// (mod 6) squares b0, b1, b0 + b1, c0, c1, c0 + c1 (its inputs gathered from pairs 0..3), then pair q
// forms its new component from three gathered squares S_t:
//     b0' = 3 xi (S5 - S3 - S4) + 2 b0     b1' = 3 (S3 + xi S4) - 2 b1
//     c0' = 3 (S0 + xi S1) - 2 c0          c1' = 3 (S2 - S0 - S1) + 2 c1
// so no pair redoes another's combination.  It runs on the lazy field (lazy.h: 14 signed 28-bit limbs,
// R' form, bounds in the types): the squaring's Montgomery product and the combination's additions in
// the lazy form (carry-free additions, one reduction a step) instead of the storage form's canonical
// ones.
using LzF2 = lz::F2<lz::AN, 9>;
DEV LzF2 bcast_lz(const LzF2& v, int src_pair) {
    const int lane = 2 * src_pair + (int)half_id();
    LzF2 r;
#pragma unroll
    for (int k = 0; k < lz::LN; k++) r.c.v[k] = __shfl(v.c.v[k], lane);
    return r;
}
template <int A, int B>
DEV lz::F2<A, B> sel2(bool c, const lz::F2<A, B>& x, const lz::F2<A, B>& y) { return {lz::sel(c, x.c, y.c)}; }
DEV void cyc4_sqr_dist_lz(LzF2& V) {
    using namespace lz;
    const int j = pair_idx(), t = j % 6, q = j & 3;
    const LzF2 a = bcast_lz(V, (0x232010 >> (4 * t)) & 15), b = bcast_lz(V, (0x300100 >> (4 * t)) & 15);
    const auto s = add(a, b);
    const auto in = sel2(t == 2 || t == 5, s, fit<decltype(s)::AV, decltype(s)::BV>(a));
    const LzF2 sq = reduce(sqrr_in(in));
    const LzF2 G1 = bcast_lz(sq, (0x2035 >> (4 * q)) & 15), G2 = bcast_lz(sq, (0x0143 >> (4 * q)) & 15),
               G3 = bcast_lz(sq, (0x1004 >> (4 * q)) & 15);
    const bool xf = q == 0 || q == 3;  // X family: G1 - G2 - G3 (times xi for b0'); else T: G1 + xi G2
    const auto x = sub(sub(G1, G2), G3);
    const auto xx = xi(x);
    const auto w = add(G1, xi(G2));
    using U = F2<decltype(xx)::AV, decltype(xx)::BV>;
    const U u0 = sel2(q == 0, xx, fit<U::AV, U::BV>(x));
    const auto u = squeeze(sel2(xf, u0, fit<U::AV, U::BV>(w)));
    const auto y = sel2(xf, V, neg(V));  // 3u + 2V = u + 2 (u + V) (X family), 3u - 2V = u + 2 (u - V) (T)
    V = reduce(add(u, dbl(add(u, y))));
}
// the full compressed state (b0, b1, c0, c1) in the storage form at K slots base.. (each pair converts
// its own component, then four broadcasts)
DEV void st_cyc4_dist_lz(const Soa& K, int base, size_t i, const LzF2& V) {
    const Fp2 own = lz::out_r2(V);
    const Fp2 b0 = bcast_f2(own, 0), b1 = bcast_f2(own, 1), c0 = bcast_f2(own, 2), c1 = bcast_f2(own, 3);
    st_f2(K, base + 0, i, b0);
    st_f2(K, base + 2, i, b1);
    st_f2(K, base + 4, i, c0);
    st_f2(K, base + 6, i, c1);
}

// The decompression of pow-by-x's three snapshots: their 12 squarings, then their 18 products, as two
// spread calls (pair j loads its operands from the scratch by index), the three denominators' pairwise
// products, ONE inversion (Montgomery's trick), the three inverses and the six a-coefficients — six
// product latencies and the inversion.  Snapshots (b0 b1 c0 c1, 8 slots each) at K slots 0
// (g^(2^16)), 8 (g^(2^48)), 16 (g^(2^57)); N_b, N_c and then the numerators in the scratch region X
// (12 slots; the chain's S, free during a pow-by-x).  Returns false on a zero denominator (the
// Granger-Scott fallback).
DEV bool decompress3_wide(Fp12& a16, Fp12& a48, Fp12& a57, const Soa& K, const Soa& X, size_t i) {
    const int j = pair_idx();
    {  // squarings of b0, b1, c0, c1 of each snapshot (pairs 0..11)
        const int jj = j % 12;
        Fp2 in, sq;
        ld_f2(in, K, 8 * (jj >> 2) + 2 * (jj & 3), i);
        f2_sqr(sq, in);
        for (int s = 0; s < 3; s++) {
            Fp2 t, u;
            f2_mul_xi(t, bcast_f2(sq, 4 * s + 1));
            f2_sub(u, bcast_f2(sq, 4 * s), t);  // N_b = b0^2 - xi b1^2
            st_f2(X, 4 * s, i, u);
            f2_mul_xi(t, bcast_f2(sq, 4 * s + 3));
            f2_sub(u, bcast_f2(sq, 4 * s + 2), t);  // N_c = c0^2 - xi c1^2
            st_f2(X, 4 * s + 2, i, u);
        }
    }
    Fp2 d[3];
    {  // per snapshot: b0 N_b, c1 N_c, c0 N_c, b1 N_b, b0 c0, b1 c1 (pairs 0..17)
        const int jj = j % 18, s = jj / 6, t = jj % 6;
        const int c1 = (0x101230 >> (4 * t)) & 15;  // first factor's component: b0 c1 c0 b1 b0 b1
        Fp2 o1, o2, pr;
        ld_f2(o1, K, 8 * s + 2 * c1, i);
        if (t < 4) ld_f2(o2, X, 4 * s + (t == 1 || t == 2 ? 2 : 0), i);
        else ld_f2(o2, K, 8 * s + (t == 4 ? 4 : 6), i);
        f2_mul(pr, o1, o2);
        for (int s2 = 0; s2 < 3; s2++) {
            Fp2 u, v;
            f2_mul_xi(u, bcast_f2(pr, 6 * s2 + 1));
            f2_add(v, bcast_f2(pr, 6 * s2), u);  // a0 numerator: b0 N_b + xi c1 N_c
            st_f2(X, 4 * s2, i, v);
            f2_add(v, bcast_f2(pr, 6 * s2 + 2), bcast_f2(pr, 6 * s2 + 3));  // a1 numerator: c0 N_c + b1 N_b
            st_f2(X, 4 * s2 + 2, i, v);
            f2_mul_xi(u, bcast_f2(pr, 6 * s2 + 5));
            f2_sub(v, bcast_f2(pr, 6 * s2 + 4), u);
            f2_dbl(d[s2], v);  // D = 2 (b0 c0 - xi b1 c1)
        }
    }
    Fp2 e[3], p2, inv;
    {  // pairs 0..2: d16 d48, d48 d57, d16 d57
        const int jj = j % 3;
        Fp2 pr;
        f2_mul(pr, f2_pick(jj == 1 ? 1 : 0, d, 3), f2_pick(jj == 0 ? 1 : 2, d, 3));
        for (int k = 0; k < 3; k++) e[k] = bcast_f2(pr, k);
    }
    f2_mul(p2, e[0], d[2]);
    if (f2_is_zero(p2)) return false;  // wave-uniform: every pair holds the same values
    f2_inv_q(inv, p2);
    Fp2 iv[3];
    {  // pairs 0..2: 1/d16 = inv d48 d57, 1/d48 = inv d16 d57, 1/d57 = inv d16 d48
        const int jj = j % 3;
        Fp2 pr;
        f2_mul(pr, inv, f2_pick(jj == 0 ? 1 : jj == 1 ? 2 : 0, e, 3));
        for (int k = 0; k < 3; k++) iv[k] = bcast_f2(pr, k);
    }
    {  // pairs 0..5: the a-coefficients, numerator (s, h) times 1/d_s
        const int jj = j % 6, s = jj >> 1;
        Fp2 nm, pr;
        ld_f2(nm, X, 4 * s + 2 * (jj & 1), i);
        f2_mul(pr, nm, f2_pick(s, iv, 3));
        Fp12* outs[3] = {&a16, &a48, &a57};
        for (int s2 = 0; s2 < 3; s2++) {
            Fp12& r = *outs[s2];
            r.a.a = bcast_f2(pr, 2 * s2);
            r.a.b = bcast_f2(pr, 2 * s2 + 1);
            ld_f2(r.b.a, K, 8 * s2, i);
            ld_f2(r.b.b, K, 8 * s2 + 2, i);
            ld_f2(r.c.a, K, 8 * s2 + 4, i);
            ld_f2(r.c.b, K, 8 * s2 + 6, i);
        }
    }
    return true;
}

// dst <- src^x.  |x| = 2^63 + 2^62 + 2^60 + 2^57 + 2^48 + 2^16: 57 compressed squarings, the state
// spread over the pairs, with snapshots g^(2^16), g^(2^48) stored to K; the three compressed values
// g^(2^16), g^(2^48), g^(2^57) decompressed with ONE inversion; then g^(2^60), g^(2^62), g^(2^63) by six
// Granger-Scott squarings of g^(2^57) (cheaper than three more decompressions) and five Fp12
// multiplications.  A zero denominator (b = c = 0 pattern; never reached by honest inputs, e.g.
// src = 1) sends the wave to the Granger-Scott ladder.
static __device__ __noinline__ void fx_pow_x(Soa src, Soa dst, Soa K, size_t i, Soa X) {
    LzF2 V;
    {
        Fp2 v;
        ld_f2(v, src, 4 + 2 * (pair_idx() & 3), i);
        V = lz::reduce(lz::in_r2(v));
    }
    for (int k = 1; k <= 57; k++) {
        cyc4_sqr_dist_lz(V);
        if (k == 16) st_cyc4_dist_lz(K, 0, i, V);
        if (k == 48) st_cyc4_dist_lz(K, 8, i, V);
    }
    st_cyc4_dist_lz(K, 16, i, V);
    Fp12 acc, t, y;
    if (!decompress3_wide(acc, t, y, K, X, i)) {
        fx_pow_x_gs(src, dst, i);
        return;
    }
    // the tail's products of acc and its squarings of y pair up: 7 levels instead of 11
    const Fp12 y57 = y;
    f12_mul_cs_wide(acc, acc, t, y);    // acc = g^(2^16 + 2^48), y = g^(2^58)
    f12_mul_cs_wide(acc, acc, y57, y);  // acc *= g^(2^57), y = g^(2^59)
    f12_cyc_sqr_wide(y, y);             // 2^60
    f12_mul_cs_wide(acc, acc, y, y);    // acc *= g^(2^60), y = g^(2^61)
    f12_cyc_sqr_wide(y, y);             // 2^62
    f12_mul_cs_wide(acc, acc, y, y);    // acc *= g^(2^62), y = g^(2^63)
    f12_mul_wide(acc, acc, y);          // acc *= g^(2^63)
    f12_conj(acc, acc);
    st_f12(dst, i, acc);
}

// dst <- op_a(a) * op_b(b)
static __device__ __noinline__ void fx_mul(Soa a, int opa, Soa b, int opb, Soa dst, size_t i) {
    Fp12 x, y;
    ld_f12(x, a, i);
    fx_apply(x, opa);
    ld_f12(y, b, i);
    fx_apply(y, opb);
    f12_mul_wide(x, x, y);
    st_f12(dst, i, x);
}

// the chain of element i of n on a whole wave
DEV void fexp_chain(size_t n, size_t i, uint32_t* fbuf, uint32_t* scratch) {
    const Soa F{fbuf, n};
    const Soa T{scratch, n}, A{scratch + (size_t)12 * NL * n, n}, S{scratch + (size_t)24 * NL * n, n},
        R{scratch + (size_t)36 * NL * n, n}, K{scratch + (size_t)48 * NL * n, n};
    fx_inv(F, T, i);
    fx_mul(F, OP_CONJ, T, OP_ID, F, i);   // f^(p^6 - 1)
    fx_mul(F, OP_FROB2, F, OP_ID, F, i);  // ^(p^2 + 1)
    fx_cube(F, R, i);                     // res = f^3
    fx_pow_x(F, T, K, i, S);
    fx_mul(T, OP_ID, F, OP_CONJ, T, i);   // t = f^(x-1)
    fx_pow_x(T, A, K, i, S);
    fx_mul(A, OP_ID, T, OP_CONJ, A, i);   // a = f^((x-1)^2)
    fx_mul(A, OP_FROB2, A, OP_CONJ, S, i);
    fx_mul(S, OP_FROB, R, OP_ID, R, i);   // res *= (a^(p^2) a^-1)^p
    fx_pow_x(A, T, K, i, S);              // b = a^x
    fx_mul(T, OP_FROB2, T, OP_CONJ, S, i);
    fx_mul(S, OP_ID, R, OP_ID, R, i);     // res *= b^(p^2) b^-1
    fx_pow_x(T, A, K, i, S);              // c = b^x
    fx_mul(A, OP_FROB, R, OP_ID, R, i);   // res *= c^p
    fx_pow_x(A, T, K, i, S);              // d = c^x
    fx_mul(T, OP_ID, R, OP_ID, R, i);     // res *= d
}

DEV void fexp_out(size_t n, size_t i, const uint32_t* scratch, const uint32_t* flags, uint8_t* verdicts,
                  uint8_t* gt_out, bool writer) {
    Fp12 res;
    ld_f12(res, Soa{const_cast<uint32_t*>(scratch) + (size_t)36 * NL * n, n}, i);
    const uint32_t fl = flags ? flags[i] : 0u;
    const bool ok = f12_is_one(res) && (fl & 11u) == 0;  // sigma_1/sigma_2 = O or PoK Schnorr failure
    if (!writer) return;
    if (!half_id()) verdicts[i] = ok ? 1 : 0;
    if (gt_out) {  // each lane writes its halves: Fp slots 2k + h of the AMCL FP12 order
        const Fp2* v = reinterpret_cast<const Fp2*>(&res);
        uint8_t* o = gt_out + i * 576 + 48 * half_id();
        for (int k = 0; k < 6; k++) {
            Fp c;
            fp_from_mont(c, v[k].c);
            store_be48_aligned(o + 96 * k, c);
        }
    }
}

// one element per wave (64 lanes, all pairs holding the same values; pair 0 writes the outputs):
// element blockIdx.x of n, its chain through SoA scratch of stride n.  One wave per SIMD (HIP's second
// bound): the whole register file.  Latency-bound small batches (cck_fexp: n <= kFexpWideMax) and the
// RLC batch's one product; larger batches run the quad-lane lazy-field kernel of fexp_q.hip.
__global__ __launch_bounds__(64, 1) void k_fexp1(size_t n, uint32_t* __restrict__ fbuf, uint32_t* __restrict__ scratch,
                                              const uint32_t* __restrict__ flags, uint8_t* __restrict__ verdicts,
                                              uint8_t* __restrict__ gt_out) {
    const size_t i = blockIdx.x;
    if (i >= n) return;  // wave-uniform
    fexp_chain(n, i, fbuf, scratch);
    fexp_out(n, i, scratch, flags, verdicts, gt_out, threadIdx.x < 2);
}

// one level of the RLC product tree in the wide form: out[t] = in[2t] in[2t+1] (in[2t] alone for an odd
// tail), one wave per product, the 18 Fp2 products on the wave's lane pairs at once.  The tree's short
// levels are latency-bound (k_f12_reduce: one product on one lane pair, ~45 us a level whatever its
// width); here a level holds about one Fp2 product's latency.
__global__ __launch_bounds__(64, 2) void k_f12_reduce_wide(size_t n_in, const uint32_t* __restrict__ in,
                                                          uint32_t* __restrict__ out) {
    const size_t t = blockIdx.x;
    const size_t n_out = (n_in + 1) / 2;
    if (t >= n_out) return;  // wave-uniform
    const Soa I{const_cast<uint32_t*>(in), n_in}, O{out, n_out};
    Fp12 a;
    ld_f12(a, I, 2 * t);
    if (2 * t + 1 < n_in) {
        Fp12 b;
        ld_f12(b, I, 2 * t + 1);
        f12_mul_wide(a, a, b);
    }
    if (threadIdx.x < 2) st_f12(O, t, a);
}

}  // namespace pl
}  // namespace cc

// one level of the product tree, wide form (k_f12_reduce_wide): (n + 1) / 2 waves
extern "C" int cck_f12_reduce_wide(size_t n, const uint32_t* d_in, uint32_t* d_out, hipStream_t st) {
    if (n < 2) return -1;
    hipLaunchKernelGGL(cc::pl::k_f12_reduce_wide, dim3((unsigned)((n + 1) / 2)), dim3(64), 0, st, n, d_in, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// n <= wide_max (the caller's threshold; d_scratch >= 72 x 12 x n words): one wave per element, the
// latency-bound form (k_fexp1); otherwise the batched kernel: lazy field, one credential per lane quad,
// the chain in registers (fexp_q.hip)
extern "C" int cck_fexp(size_t n, uint32_t* d_f, uint32_t* d_scratch, const uint32_t* d_flags, uint8_t* d_verdicts,
                        uint8_t* d_gt, size_t wide_max, hipStream_t st) {
    if (!n) return 0;
    if (n > wide_max) return cck_fexp_q(n, d_f, d_flags, d_verdicts, d_gt, st);
    hipLaunchKernelGGL(cc::pl::k_fexp1, dim3((unsigned)n), dim3(64), 0, st, n, d_f, d_scratch, d_flags, d_verdicts, d_gt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
