// The wide Miller loop for gfx950: one pair (P in G1, Q in G2) per wave, in the wide form of
// tower_wide.h — the 32 lane pairs hold the same values and a step's independent Fp2 products are spread
// over them.  Two kernels walk the same chain: k_miller_wide (one wave a pair) and k_miller_wide2 (two
// waves a pair, for launches smaller than the chip).  Users: the RLC fold's 16 window pairs (fold.hip)
// and small batches (capi_verify.cpp: n <= kWideMax, laid out by k_wide_pairs below).
//
// CC_FP_INLINE: the Fp multiplications are inlined (Makefile HOT_INLINE=1), as in fexp_pl.hip.
#ifdef CC_HOT_INLINE  // build option (Makefile HOT_INLINE=1): inline every Fp multiplication
#define CC_FP_INLINE 1
#endif
#include <cstdlib>
#include <cstring>
#include "codec.h"
#include "launch.h"
#include "lazy.h"  // LZ_ONE_LIMBS (k_wide_pairs)
#include "tower_wide.h"

namespace cc {
namespace pl {

// ================================================================ wide Miller loop
// The RLC fold's 16 window pairs (fold.hip): few, so each runs alone on a wave in the wide form of
// tower_wide.h — the 32 lane pairs hold the same values and a step's independent Fp2 products (pairing.inc
// line_dbl / line_add / eval_line / f12_mul_line, the same formulas) are spread over them, one
// product a pair, results gathered with shuffles.  The point T's chain and f's chain are independent
// until f takes a line, so the loop runs them as a pipeline of LEVELS, one Fp2 product a pair each:
// pairs 18.. take T's next level — a doubling is two (A: X Y, Y^2, Z^2, (Y + Z)^2, X^2; B: T's a (b -
// 3e), e^2, g^2, b h with the line's evaluation at P), an addition four (Q_y Z, Q_x Z | theta^2,
// lambda^2, theta Q_x, lambda Q_y | lambda d, Z c, X d and the evaluation | T's four products) — and
// pairs 0..17 the oldest of f's pending operations (f^2, or f times a finished line as a full Fp12
// A + C w^2).  f's operations keep their order, so the result is the sequential loop's, in 147 levels
// instead of 209 (a doubling iteration 2 instead of 3): X = T's A | f times the previous doubling's
// line (f^2 after an addition step), Y = T's B | f^2; an addition step's first level takes the
// doubling's line, its last the addition's.
// P (slots S_P1..+2) is in evaluation form (X Z, Y, Z^3); an Fp factor multiplies as the Fp2 (k, 0).
__global__ __launch_bounds__(64, 1) void k_miller_wide(size_t n, const uint32_t* __restrict__ prep,
                                                    const uint32_t* __restrict__ flags, uint32_t* __restrict__ fout,
                                                    size_t fstride, size_t foff) {
    const size_t i = blockIdx.x;  // the pair of this wave (wave-uniform)
    if (i >= n) return;
    const int j = pair_idx();
    const Soa S{const_cast<uint32_t*>(prep), n};
    Fp12 f;
    f12_one(f);
    if (!(flags[i] & 5u)) {
        Aff<Fp2> Q;
        ld_f2(Q.x, S, S_Q1, i);
        ld_f2(Q.y, S, S_Q1 + 2, i);
        Fp px, py, pz;
        cc::ld_fp(px, S, S_P1, i);
        cc::ld_fp(py, S, S_P1 + 1, i);
        cc::ld_fp(pz, S, S_P1 + 2, i);
        const Fp2 PX = f2_of_fp(px), PY = f2_of_fp(py), PZ = f2_of_fp(pz);
        G2Proj T;
        T.x = Q.x;
        T.y = Q.y;
        f2_one(T.z);
        // the doubling line not yet multiplied into f (taken at the next iteration's first level)
        Fp2 lp0, lp2, lp3;
        bool havep = false;
#pragma unroll 1
        for (int b = 62; b >= 0; b--) {
            Fp2 o1, o2, pr, l0, l2c, l3c;
            {  // X: T's A products (pairs 18..22) | f times the pending line, else f^2 (pairs 0..17)
                if (havep) {
                    Fp12 L;
                    line_fp12(L, lp0, lp2, lp3);
                    f12w_operands(o1, o2, j, f, L);
                } else {
                    f12w_operands(o1, o2, j, f, f);
                }
                Fp2 yz;
                f2_add_lz(yz, T.y, T.z);
                const Fp2 a1[5] = {T.x, T.y, T.z, yz, T.x}, a2[5] = {T.y, T.y, T.z, yz, T.x};
                pick2(o1, o2, j - 18, a1, a2, 5);
                f2_mul(pr, o1, o2);
                f12w_assemble(f, pr);
            }
            Fp2 a = bcast_f2(pr, 18), bb = bcast_f2(pr, 19), c = bcast_f2(pr, 20), h = bcast_f2(pr, 21),
                t = bcast_f2(pr, 22), e, ff, g;
            f2_half(a, a);
            f2_sub(h, h, bb);
            f2_sub(h, h, c);
            f2_mul_xi(e, c);
            f2_mul12(e, e);  // e = 3 b' Z^2
            f2_dbl(ff, e);
            f2_add(ff, ff, e);
            f2_add(g, bb, ff);
            f2_half(g, g);
            f2_sub(l0, e, bb);
            f2_dbl(l2c, t);
            f2_add(l2c, l2c, t);
            f2_neg(l3c, h);
            {  // Y: T's B products and the line's evaluation (pairs 18..24) | f^2 if X took the line
                Fp2 bmf;
                f2_sub(bmf, bb, ff);
                const Fp2 a1[7] = {a, e, g, bb, l0, l2c, l3c}, a2[7] = {bmf, e, g, h, PZ, PX, PY};
                if (havep) {
                    f12w_operands(o1, o2, j, f, f);
                } else {
                    o1 = a1[0];
                    o2 = a2[0];
                }
                pick2(o1, o2, j - 18, a1, a2, 7);
                f2_mul(pr, o1, o2);
                if (havep) f12w_assemble(f, pr);
            }
            T.x = bcast_f2(pr, 18);
            {
                const Fp2 e2 = bcast_f2(pr, 19);
                T.y = bcast_f2(pr, 20);
                f2_sub(T.y, T.y, e2);
                f2_sub(T.y, T.y, e2);
                f2_sub(T.y, T.y, e2);
            }
            T.z = bcast_f2(pr, 21);
            lp0 = bcast_f2(pr, 22);
            lp2 = bcast_f2(pr, 23);
            lp3 = bcast_f2(pr, 24);
            havep = true;
            if (!((X_ABS >> b) & 1ull)) continue;
            // addition step (pairing.inc line_add); its first level also takes the doubling's line
            Fp2 theta, lambda;
            {  // D1: Q_y Z, Q_x Z (pairs 18, 19) | f times the doubling's line (pairs 0..17)
                Fp12 L;
                line_fp12(L, lp0, lp2, lp3);
                f12w_operands(o1, o2, j, f, L);
                const Fp2 a1[2] = {Q.y, Q.x}, a2[2] = {T.z, T.z};
                pick2(o1, o2, j - 18, a1, a2, 2);
                f2_mul(pr, o1, o2);
                f12w_assemble(f, pr);
                havep = false;
                f2_sub(theta, T.y, bcast_f2(pr, 18));
                f2_sub(lambda, T.x, bcast_f2(pr, 19));
            }
            {  // D2
                const Fp2 a1[4] = {theta, lambda, theta, lambda}, a2[4] = {theta, lambda, Q.x, Q.y};
                o1 = a1[0];
                o2 = a2[0];
                pick2(o1, o2, j, a1, a2, 4);
                f2_mul(pr, o1, o2);
            }
            c = bcast_f2(pr, 0);
            const Fp2 d = bcast_f2(pr, 1);
            f2_sub(l0, bcast_f2(pr, 2), bcast_f2(pr, 3));
            f2_neg(l2c, theta);
            l3c = lambda;
            {  // D3
                const Fp2 a1[6] = {lambda, T.z, T.x, l0, l2c, l3c}, a2[6] = {d, c, d, PZ, PX, PY};
                o1 = a1[0];
                o2 = a2[0];
                pick2(o1, o2, j, a1, a2, 6);
                f2_mul(pr, o1, o2);
            }
            e = bcast_f2(pr, 0);
            ff = bcast_f2(pr, 1);
            g = bcast_f2(pr, 2);
            f2_add(h, e, ff);
            f2_sub(h, h, g);
            f2_sub(h, h, g);
            {  // D4: T's four products on pairs 0..3, f times the line on pairs 4..21
                Fp12 L;
                line_fp12(L, bcast_f2(pr, 3), bcast_f2(pr, 4), bcast_f2(pr, 5));
                Fp2 gmh;
                f2_sub(gmh, g, h);
                f12w_operands(o1, o2, j - 4, f, L);
                const Fp2 a1[4] = {lambda, theta, e, T.z}, a2[4] = {h, gmh, T.y, e};
                pick2(o1, o2, j, a1, a2, 4);
                f2_mul(pr, o1, o2);
                T.x = bcast_f2(pr, 0);
                f2_sub(T.y, bcast_f2(pr, 1), bcast_f2(pr, 2));
                T.z = bcast_f2(pr, 3);
                f12w_assemble(f, pr, 4);
            }
        }
        if (havep) {  // the last doubling's line
            Fp2 o1, o2, pr;
            Fp12 L;
            line_fp12(L, lp0, lp2, lp3);
            f12w_operands(o1, o2, j, f, L);
            f2_mul(pr, o1, o2);
            f12w_assemble(f, pr);
        }
        f12_conj(f, f);
    }
    if (threadIdx.x < 2) st_f12(Soa{fout, fstride}, foff + i, f);
}

// The same loop on TWO waves a pair, for launches of up to kWide2Max pairs (fewer waves than the chip
// has SIMDs, so the second wave is free): wave 1 walks T's chain (its A / B levels, the addition's four)
// and leaves each iteration's evaluated lines in LDS; wave 0 squares f and multiplies it by them one
// iteration behind.  A block barrier per iteration hands the lines over (two LDS slots).  Wave 0's
// iteration is then its two or three Fp12 operations alone (no T products or glue in its levels).
constexpr size_t kWide2Max = 256;
__global__ __launch_bounds__(128, 1) void k_miller_wide2(size_t n, const uint32_t* __restrict__ prep,
                                                      const uint32_t* __restrict__ flags, uint32_t* __restrict__ fout,
                                                      size_t fstride, size_t foff) {
    const size_t i = blockIdx.x;
    if (i >= n) return;  // block-uniform
    const bool twave = threadIdx.x >= 64;  // wave-uniform
    const int j = (int)((threadIdx.x & 63) >> 1), h = (int)(threadIdx.x & 1);
    __shared__ uint32_t lbuf[2][2][3][2][NL];  // [slot][doubling / addition line][coefficient][half][word]
    const Soa S{const_cast<uint32_t*>(prep), n};
    Fp12 f;
    f12_one(f);
    if (!(flags[i] & 5u)) {  // block-uniform
        if (twave) {
            Aff<Fp2> Q;
            ld_f2(Q.x, S, S_Q1, i);
            ld_f2(Q.y, S, S_Q1 + 2, i);
            Fp px, py, pz;
            cc::ld_fp(px, S, S_P1, i);
            cc::ld_fp(py, S, S_P1 + 1, i);
            cc::ld_fp(pz, S, S_P1 + 2, i);
            const Fp2 PX = f2_of_fp(px), PY = f2_of_fp(py), PZ = f2_of_fp(pz);
            G2Proj T;
            T.x = Q.x;
            T.y = Q.y;
            f2_one(T.z);
            auto put = [&](int slot, int which, const Fp2& x0, const Fp2& x2, const Fp2& x3) {
                if (j == 0) {
#pragma unroll
                    for (int w = 0; w < NL; w++) {
                        lbuf[slot][which][0][h][w] = x0.c.v[w];
                        lbuf[slot][which][1][h][w] = x2.c.v[w];
                        lbuf[slot][which][2][h][w] = x3.c.v[w];
                    }
                }
            };
#pragma unroll 1
            for (int k = 0; k <= 63; k++) {
                if (k <= 62) {
                    const int b = 62 - k;
                    Fp2 o1, o2, pr, l0, l2c, l3c;
                    {  // A: X Y, Y^2, Z^2, (Y + Z)^2, X^2
                        Fp2 yz;
                        f2_add_lz(yz, T.y, T.z);
                        const Fp2 a1[5] = {T.x, T.y, T.z, yz, T.x}, a2[5] = {T.y, T.y, T.z, yz, T.x};
                        o1 = a1[0];
                        o2 = a2[0];
                        pick2(o1, o2, j, a1, a2, 5);
                        f2_mul(pr, o1, o2);
                    }
                    Fp2 a = bcast_f2(pr, 0), bb = bcast_f2(pr, 1), c = bcast_f2(pr, 2), hh = bcast_f2(pr, 3),
                        t = bcast_f2(pr, 4), e, ff, g;
                    f2_half(a, a);
                    f2_sub(hh, hh, bb);
                    f2_sub(hh, hh, c);
                    f2_mul_xi(e, c);
                    f2_mul12(e, e);  // e = 3 b' Z^2
                    f2_dbl(ff, e);
                    f2_add(ff, ff, e);
                    f2_add(g, bb, ff);
                    f2_half(g, g);
                    f2_sub(l0, e, bb);
                    f2_dbl(l2c, t);
                    f2_add(l2c, l2c, t);
                    f2_neg(l3c, hh);
                    {  // B: T's a (b - 3e), e^2, g^2, b h and the line's evaluation at P
                        Fp2 bmf;
                        f2_sub(bmf, bb, ff);
                        const Fp2 a1[7] = {a, e, g, bb, l0, l2c, l3c}, a2[7] = {bmf, e, g, hh, PZ, PX, PY};
                        o1 = a1[0];
                        o2 = a2[0];
                        pick2(o1, o2, j, a1, a2, 7);
                        f2_mul(pr, o1, o2);
                    }
                    T.x = bcast_f2(pr, 0);
                    {
                        const Fp2 e2 = bcast_f2(pr, 1);
                        T.y = bcast_f2(pr, 2);
                        f2_sub(T.y, T.y, e2);
                        f2_sub(T.y, T.y, e2);
                        f2_sub(T.y, T.y, e2);
                    }
                    T.z = bcast_f2(pr, 3);
                    put(b & 1, 0, bcast_f2(pr, 4), bcast_f2(pr, 5), bcast_f2(pr, 6));
                    if ((X_ABS >> b) & 1ull) {  // addition step (pairing.inc line_add)
                        Fp2 theta, lambda;
                        {
                            const Fp2 a1[2] = {Q.y, Q.x}, a2[2] = {T.z, T.z};
                            o1 = a1[0];
                            o2 = a2[0];
                            pick2(o1, o2, j, a1, a2, 2);
                            f2_mul(pr, o1, o2);
                            f2_sub(theta, T.y, bcast_f2(pr, 0));
                            f2_sub(lambda, T.x, bcast_f2(pr, 1));
                        }
                        {
                            const Fp2 a1[4] = {theta, lambda, theta, lambda}, a2[4] = {theta, lambda, Q.x, Q.y};
                            o1 = a1[0];
                            o2 = a2[0];
                            pick2(o1, o2, j, a1, a2, 4);
                            f2_mul(pr, o1, o2);
                        }
                        c = bcast_f2(pr, 0);
                        const Fp2 d = bcast_f2(pr, 1);
                        f2_sub(l0, bcast_f2(pr, 2), bcast_f2(pr, 3));
                        f2_neg(l2c, theta);
                        l3c = lambda;
                        {
                            const Fp2 a1[6] = {lambda, T.z, T.x, l0, l2c, l3c}, a2[6] = {d, c, d, PZ, PX, PY};
                            o1 = a1[0];
                            o2 = a2[0];
                            pick2(o1, o2, j, a1, a2, 6);
                            f2_mul(pr, o1, o2);
                        }
                        e = bcast_f2(pr, 0);
                        ff = bcast_f2(pr, 1);
                        g = bcast_f2(pr, 2);
                        put(b & 1, 1, bcast_f2(pr, 3), bcast_f2(pr, 4), bcast_f2(pr, 5));
                        f2_add(hh, e, ff);
                        f2_sub(hh, hh, g);
                        f2_sub(hh, hh, g);
                        {
                            Fp2 gmh;
                            f2_sub(gmh, g, hh);
                            const Fp2 a1[4] = {lambda, theta, e, T.z}, a2[4] = {hh, gmh, T.y, e};
                            o1 = a1[0];
                            o2 = a2[0];
                            pick2(o1, o2, j, a1, a2, 4);
                            f2_mul(pr, o1, o2);
                            T.x = bcast_f2(pr, 0);
                            f2_sub(T.y, bcast_f2(pr, 1), bcast_f2(pr, 2));
                            T.z = bcast_f2(pr, 3);
                        }
                    }
                }
                __syncthreads();
            }
        } else {
            auto get = [&](int slot, int which) {
                Fp12 L;
                Fp2 x0, x2, x3;
#pragma unroll
                for (int w = 0; w < NL; w++) {
                    x0.c.v[w] = lbuf[slot][which][0][h][w];
                    x2.c.v[w] = lbuf[slot][which][1][h][w];
                    x3.c.v[w] = lbuf[slot][which][2][h][w];
                }
                line_fp12(L, x0, x2, x3);
                return L;
            };
#pragma unroll 1
            for (int k = 0; k <= 63; k++) {
                if (k >= 1) {  // iteration b = 63 - k, its lines written in round k - 1
                    const int b = 63 - k;
                    f12_mul_wide(f, f, f);
                    f12_mul_wide(f, f, get(b & 1, 0));
                    if ((X_ABS >> b) & 1ull) f12_mul_wide(f, f, get(b & 1, 1));
                }
                __syncthreads();
            }
            f12_conj(f, f);
        }
    }
    if (threadIdx.x < 2) st_f12(Soa{fout, fstride}, foff + i, f);
}

// ================================================================ small batches: one wave per pair
// A batch of n credentials fills 2n lanes of the batch Miller kernel (miller_lz.hip k_miller): for small
// n that is a handful of waves, each the latency of a 2-pair loop on one lane pair (~7.5 ms alone on its
// SIMD, whatever n up to ~4k).  For n <= kWideMax (capi_verify.cpp) each credential's two pairs run instead as
// two waves of k_miller_wide (~1.8 ms), and k_f12_reduce_wide (fexp_pl.hip) multiplies each credential's
// two Miller values.  k_wide_pairs lays the pairs out for it: pair 2i = credential i's pair 0, 2i + 1 its
// pair 1, Q affine (storage R form) in slots S_Q1.., P in evaluation form (X Z, Y, Z^3) in S_P1..; wide
// flag bit 0 = skip.
//   SigG2: pair 0 (sigma_1, pr), pair 1 (-sigma_2, g~);  SigG1: pair 0 (pr, sigma_1), pair 1 (g~, -sigma_2)
// The prep's P are affine in the lazy R' form (kAffRp): words x R' mod p, read by the storage-form tower
// as x 2^-14, so P = (x, y) goes in as (x R', y R', R' mod p) = 2^-14 (x, y, 1), a scaling of the
// evaluation form by an Fp constant (the final exponentiation removes it).  g~ (ctx gtilde_aff, AoS,
// R form) goes in as (x, y, 1) in R form.  Verdict flags stay per credential (the prep's).
DEV Fp one_rprime_words() {  // R' mod p (lazy.h LZ_ONE_LIMBS, 14 x 28 bits) as 12 x 32-bit words
    constexpr uint32_t L[14] = {LZ_ONE_LIMBS};
    Fp r;
#pragma unroll
    for (int j = 0; j < NL; j++) {
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const int sh = 28 * k - 32 * j;
            if (sh >= 32 || sh <= -28) continue;
            w |= sh >= 0 ? (uint64_t)L[k] << sh : (uint64_t)L[k] >> -sh;
        }
        r.v[j] = (uint32_t)w;
    }
    return r;
}
template <int MODE>
__global__ __launch_bounds__(64) void k_wide_pairs(size_t n, size_t ps, const uint32_t* __restrict__ prep,
                                                   const uint32_t* __restrict__ flags,
                                                   const uint32_t* __restrict__ gaff, uint32_t* __restrict__ wprep,
                                                   uint32_t* __restrict__ wflags) {
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= 2 * n) return;
    const size_t i = e >> 1;
    const int k = (int)(e & 1);
    const Soa S{const_cast<uint32_t*>(prep), ps}, W{wprep, 2 * n};
    Fp v;
    const bool q_is_g = MODE == 1 && k == 1, p_is_g = MODE == 0 && k == 1;
#pragma unroll
    for (int j = 0; j < 4; j++) {  // Q: x.a, x.b, y.a, y.b
        if (q_is_g) {
#pragma unroll
            for (int l = 0; l < NL; l++) v.v[l] = gaff[NL * j + l];
        } else {
            ld_fp(v, S, (k ? S_Q2 : S_Q1) + j, i);
        }
        st_fp(W, S_Q1 + j, e, v);
    }
    if (p_is_g) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int l = 0; l < NL; l++) v.v[l] = gaff[NL * j + l];
            st_fp(W, S_P1 + j, e, v);
        }
        fp_one(v);
    } else {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            ld_fp(v, S, (k ? S_P2 : S_P1) + j, i);
            st_fp(W, S_P1 + j, e, v);
        }
        v = one_rprime_words();
    }
    st_fp(W, S_P1 + 2, e, v);
    wflags[e] = (flags[i] & (k ? 18u : 5u)) ? 1u : 0u;
}

}  // namespace pl
}  // namespace cc

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// credential i's two Miller pairs as wide pairs 2i, 2i + 1 (k_wide_pairs above); gaff: g~ affine (AoS,
// R form) of the context
extern "C" int cck_wide_pairs(int mode, size_t n, size_t ps, const uint32_t* d_prep, const uint32_t* d_flags,
                              const uint32_t* d_gaff, uint32_t* d_wprep, uint32_t* d_wflags, hipStream_t st) {
    if (!n) return 0;
    if (ps < n) return -1;
    const unsigned g = nblocks(2 * n, 64);
    if (mode == 0)
        hipLaunchKernelGGL(cc::pl::k_wide_pairs<0>, dim3(g), dim3(64), 0, st, n, ps, d_prep, d_flags, d_gaff, d_wprep,
                           d_wflags);
    else
        hipLaunchKernelGGL(cc::pl::k_wide_pairs<1>, dim3(g), dim3(64), 0, st, n, ps, d_prep, d_flags, d_gaff, d_wprep,
                           d_wflags);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// pair i = SoA element i of n (Q: slots S_Q1.., P: S_P1.. in evaluation form; flags bit 0 / 2: skip);
// Miller value i to element foff + i of stride fstride
extern "C" int cck_miller_wide(size_t n, const uint32_t* d_prep, const uint32_t* d_flags, uint32_t* d_f,
                               size_t fstride, size_t foff, hipStream_t st) {
    if (!n) return 0;
    if (fstride < foff + n) return -1;
    if (n <= cc::pl::kWide2Max)  // fewer pairs than SIMDs: a second wave a pair takes T's chain
        hipLaunchKernelGGL(cc::pl::k_miller_wide2, dim3((unsigned)n), dim3(128), 0, st, n, d_prep, d_flags, d_f, fstride,
                           foff);
    else
        hipLaunchKernelGGL(cc::pl::k_miller_wide, dim3((unsigned)n), dim3(64), 0, st, n, d_prep, d_flags, d_f, fstride,
                           foff);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
