// Holder-side device code shared by pok_prove.hip (PoKOfSignature::init) and sigreq_prove.hip
// (SignatureRequest::new, SignatureRequestPoK::init): the two-base table of the signed 4-bit windows
// (straus.h's entry layout: the multiples 1..8 of two points, normalised with ONE inversion), the
// addition of one of its entries, and the encoders of a lazy accumulator and of an Fr value.
//   entries: d B_0 (0..7), d B_1 (8..15), d = 1..8
//   SigG2 (points in G2): one table per lane pair, [entry][half][SEW], 16 Z's and 16 prefix products
//     [entry][half][LN] behind it; SigG1: one table per lane, [entry][SEW], Z's and prefixes [entry][LN].
#pragma once
#include "codec.h"
#include "curve_lz.h"
#include "curve_pl.h"
#include "fr.h"
#include "straus.h"

namespace cc {

constexpr int SP_ENT = 16;  // entries of a two-base table

// words of one two-base table with its Z's and prefix products
__host__ __device__ constexpr size_t sp_table_words_g2() { return (size_t)SP_ENT * 2 * (SEW + 2 * lz::LN); }
__host__ __device__ constexpr size_t sp_table_words_g1() { return (size_t)SP_ENT * (SEW + 2 * lz::LN); }

// the multiples 1..8 of base k (0 or 1), Jacobian, into the pair's table; acc_z: the running product of
// the finite multiples' Z (r_one() before base 0).  An off-curve encoding decodes to the identity.
DEV void sp_fill_g2(uint32_t* ent, uint32_t* zs, uint32_t* pre, int h, int k, const uint8_t* enc, lz::F2R& acc_z) {
    using namespace lz;
    cc::Aff<cc::Fp2> P1;
    const bool ok = pl::pair_all(g2_decode(P1, enc));  // both lanes decode the point
    pl::Fp2 hx, hy;
    hx.c = h ? P1.x.b : P1.x.a;
    hy.c = h ? P1.y.b : P1.y.a;
    const AL P{reduce(in_r2(hx)), reduce(in_r2(hy))};
    JL J = ok ? jl_from_aff(P) : jl_inf();
#pragma unroll 1
    for (int d = 0; d < 8; d++) {
        if (d == 1) J = jl_dbl(J);
        else if (d > 1 && ok) J = jl_add_aff(J, P);
        const int e = k * 8 + d;
        uint32_t* w = ent + (e * 2 + h) * SEW;
        const bool inf = jl_is_inf(J);
        st_w(w, J.x);
        st_w(w + SEY, J.y);
        w[SEF] = inf ? 1u : 0u;
        st_w(zs + (e * 2 + h) * LN, J.z);
        st_w(pre + (e * 2 + h) * LN, acc_z);
        if (!inf) acc_z = reduce(mulr(acc_z, J.z));
    }
}

// one inversion for the ne entries (a two-base table: 16), then walk back: z_e^-1 = inv * prefix_e; inv *= z_e
DEV void sp_norm_g2(uint32_t* ent, const uint32_t* zs, const uint32_t* pre, int h, const lz::F2R& acc_z,
                    int ne = SP_ENT) {
    using namespace lz;
    F2R zinv = reduce(inv(acc_z));
#pragma unroll 1
    for (int e = ne - 1; e >= 0; e--) {
        uint32_t* w = ent + (e * 2 + h) * SEW;
        if (w[SEF]) continue;  // identity multiple (pair-uniform: both halves carry the flag)
        const F2R z = ld_w(zs + (e * 2 + h) * LN);
        const auto zi = mulr(zinv, ld_w(pre + (e * 2 + h) * LN));
        zinv = reduce(mulr(zinv, z));
        const auto zi2 = sqrr(zi);
        st_w(w, reduce(mulr(ld_w(w), zi2)));
        st_w(w + SEY, reduce(mulr(ld_w(w + SEY), mulr(zi2, zi))));
    }
}

// acc += d B_base for a signed digit d != 0
DEV void sp_add_g2(lz::JL& acc, const uint32_t* ent, int h, int base, int d) {
    using namespace lz;
    const uint32_t* w = ent + (((base * 8 + (d < 0 ? -d : d) - 1) * 2) + h) * SEW;
    if (w[SEF]) return;  // identity multiple
    AL e;
    ld16(e.x.c.v, w);
    ld16(e.y.c.v, w + SEY);
    if (d < 0) e = jl_neg_aff(e);
    acc = jl_add_aff(acc, e);
}

DEV void sp_fill_g1(uint32_t* ent, uint32_t* zs, uint32_t* pre, int k, const uint8_t* enc, lz::FR& acc_z) {
    using namespace lz;
    cc::Aff<cc::Fp> P1;
    const bool ok = g1_decode(P1, enc);
    const FR px = reduce(in_r(P1.x)), py = reduce(in_r(P1.y));
    const AG P = ag_of(px, py);
    JG J = ok ? JG{px, py, r1_one()} : jg_inf();
#pragma unroll 1
    for (int d = 0; d < 8; d++) {
        if (d == 1) J = jg_dbl(J);
        else if (d > 1 && ok) J = jg_add_aff(J, P);
        const int e = k * 8 + d;
        uint32_t* w = ent + e * SEW;
        const bool inf = jg_is_inf(J);
        st_r1(w, J.x);
        st_r1(w + SEY, J.y);
        w[SEF] = inf ? 1u : 0u;
        st_r1(zs + e * LN, J.z);
        st_r1(pre + e * LN, acc_z);
        if (!inf) acc_z = reduce(mulr1(acc_z, J.z));
    }
}

DEV void sp_norm_g1(uint32_t* ent, const uint32_t* zs, const uint32_t* pre, const lz::FR& acc_z, int ne = SP_ENT) {
    using namespace lz;
    cc::Fp zinv_s;
    fp_inv(zinv_s, out_r(acc_z));
    FR zinv = reduce(in_r(zinv_s));
#pragma unroll 1
    for (int e = ne - 1; e >= 0; e--) {
        uint32_t* w = ent + e * SEW;
        if (w[SEF]) continue;  // identity multiple
        const FR z = ld_r1(zs + e * LN);
        const FR zi = reduce(mulr1(zinv, ld_r1(pre + e * LN)));
        zinv = reduce(mulr1(zinv, z));
        const FR zi2 = reduce(sqrr1(zi));
        st_r1(w, reduce(mulr1(ld_r1(w), zi2)));
        st_r1(w + SEY, reduce(mulr1(ld_r1(w + SEY), mulr1(zi2, zi))));
    }
}

DEV void sp_add_g1(lz::JG& acc, const uint32_t* ent, int base, int d) {
    using namespace lz;
    const uint32_t* w = ent + (base * 8 + (d < 0 ? -d : d) - 1) * SEW;
    if (w[SEF]) return;  // identity multiple
    FR ex, ey;
    ld16(ex.v, w);
    ld16(ey.v, w + SEY);
    acc = jg_add_aff(acc, ag_of(ex, d < 0 ? neg(ey) : ey));
}

// affine encoding (amcl_wrapper to_bytes) of a lane-pair point; lane h = 0 writes
DEV void g2lz_out(const lz::JL& acc, int h, uint8_t* out) {
    using namespace lz;
    cc::Aff<cc::Fp2> o;
    const bool fin = !jl_is_inf(acc);
    pl::Fp2 x, y;
    if (fin) {
        const auto zi = inv(acc.z);
        const auto zi2 = sqrr(zi);
        x = out_r2(mulr(acc.x, zi2));
        y = out_r2(mulr(acc.y, mulr(zi2, zi)));
    } else {
        fp_zero(x.c);
        fp_zero(y.c);
    }
    const Fp xs = pl::swp(x.c), ys = pl::swp(y.c);
    o.x.a = h ? xs : x.c;
    o.x.b = h ? x.c : xs;
    o.y.a = h ? ys : y.c;
    o.y.b = h ? y.c : ys;
    if (!h) g2_encode(out, o, fin);
}

DEV void g1lz_out(const lz::JG& acc, uint8_t* out) {
    Jac<Fp> s = lz::jg_to(acc);
    Aff<Fp> a;
    const bool fin = jac_to_aff(a, s);
    g1_encode(out, a, fin);
}

// a canonical Fr value as 48 bytes big-endian at a 4-byte-aligned address
DEV void store_fr_be48(uint8_t* p, const uint32_t v[8]) {
    Fp c;
#pragma unroll
    for (int k = 0; k < NL; k++) c.v[k] = k < 8 ? v[k] : 0u;
    store_be48_aligned(p, c);
}

}  // namespace cc
