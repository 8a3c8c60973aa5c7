// PoKOfSignatureProof::verify with the CALLER's verkey per proof (cc_pok_verify_batch_pervk_device).
//
// Reference: src/pok_sig.rs:103-105 -> ps_sig PoKOfSignatureProof::verify(&vk, &params, revealed_msgs,
// &chal) [EXT]: per call, with that call's verkey (X~, Y~_0..q-1) and the params' g~,
//   Schnorr:  resp_0 g~ + sum_hidden resp_j Y~_j + chal J - T == O
//   J'     :  X~ + J + sum_revealed m_z Y~_idx[z]
// then the 2-pairing check e(sigma'_1, J') e(-sigma'_2, g~) == 1 of the shared-verkey PoK prep
// (aggregate.hip k_prep_pok_split / k_prep_pok_g1pl), whose SoA operands and flag bits (1, 2: a sigma'
// that does not decode; 4: J' is the identity; 8: the Schnorr relation failed) this prep writes, so
// launch_miller and cck_fexp finish unchanged.
//
// With a verkey per proof no base is fixed, so there are no window tables.  Every Y~_j belongs to
// exactly one of the two sums (hidden -> Schnorr, revealed -> J'), so ONE Straus table per proof serves
// both: the signed-window multiples 1..8 of the q + 2 bases [g~, Y~_0..q-1, J], batch-normalised with
// one inversion (straus.h's layout and steps), then two 65-window chains over disjoint subsets of it:
//   chain A  g~, the hidden Y~_j and J with the digits of the responses and of chal; then + (-T);
//   chain B  the revealed Y~_j with the digits of the revealed messages; then + X~ + J.
// k_pok_var_scalars writes the canonical scalar (mod r, fr_from_be48) of every base in table order and
// each base's chain (its role) from the uploaded index list.  No endomorphism and no subgroup
// assumption: bases and J may lie outside the order-r subgroup, and the digits are those of the integer
// scalar mod r, so a small-order base gives its integer multiple as AMCL's MSM does.
// Identity accumulators and equal or opposite operands are the additions' own cases (jg_add_aff,
// jl_add_aff); identity bases and identity multiples are flagged in the table and skipped.
//
// Lanes: SigG2 (bases in G1) one proof per LANE on the lazy field (as k_prep_sigg2_var); SigG1 (bases in
// G2) one proof per lane PAIR on the lazy pair-lane field (as k_prep_sigg1_var).  One path for every n.
//
// Scratch per proof: straus_g1lz_words(q + 2) words (SigG2), straus_lz_words(q + 2) (SigG1).  At q = 32
// (34 bases) that is 16,896 words = 67,584 bytes and 33,216 words = 132,864 bytes a proof: 4.43 GB and
// 8.71 GB at 65,536 proofs, from the slot's vkb buffer (plus 34 x 32 bytes of scalars a proof).
#include "codec.h"
#include "curve_lz.h"
#include "curve_pl.h"
#include "fr.h"
#include "launch.h"
#include "pairing.h"
#include "soa.h"
#include "straus.h"

using namespace cc;

namespace {
using namespace cc::lz;

// Table order: base 0 = g~ (resp_0), base 1 + j = Y~_j (its response if hidden, its message if
// revealed), base q + 1 = J (chal).  role: 0 chain A (Schnorr), 1 chain B (J').
__global__ __launch_bounds__(256) void k_pok_var_scalars(size_t n, int q, int r, const uint8_t* __restrict__ resp,
                                                         const uint8_t* __restrict__ chal,
                                                         const uint8_t* __restrict__ rev_msgs,
                                                         const uint32_t* __restrict__ rev_idx,
                                                         uint32_t* __restrict__ role, uint32_t* __restrict__ out) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t t = (size_t)q + 2;
    if (g >= n * t) return;
    const size_t i = g / t;
    const int k = (int)(g % t);
    const size_t nresp = (size_t)(q - r + 1);
    const uint8_t* src;
    uint32_t ro = 0;
    if (k == 0) {
        src = resp + i * nresp * 48;
    } else if (k == q + 1) {
        src = chal + i * 48;
    } else {
        const uint32_t j = (uint32_t)(k - 1);
        int rev = -1, below = 0;  // j's place in the revealed list; revealed indices below j
        for (int z = 0; z < r; z++) {
            const uint32_t x = rev_idx[z];
            if (x == j) rev = z;
            below += x < j;
        }
        if (rev >= 0) {
            ro = 1;
            src = rev_msgs + (i * (size_t)r + (size_t)rev) * 48;
        } else {  // responses: [g~, Y~_j for hidden j ascending]
            src = resp + (i * nresp + 1 + (size_t)((int)j - below)) * 48;
        }
    }
    Fr m;
    fr_from_be48(m, src);
    uint4* o = reinterpret_cast<uint4*>(out + g * 8);
    o[0] = make_uint4(m.v[0], m.v[1], m.v[2], m.v[3]);
    o[1] = make_uint4(m.v[4], m.v[5], m.v[6], m.v[7]);
    if (i == 0) role[k] = ro;
}

// ---------------------------------------------------------------- G1 bases, one proof per lane
// base k of proof i: storage-form affine coordinates; false: the identity (a point that does not decode)
DEV bool pv_base_g1(cc::Aff<cc::Fp>& P, size_t k, size_t q, const uint32_t* __restrict__ gaff, uint32_t ginf,
                    const uint8_t* __restrict__ Y, const uint8_t* __restrict__ J) {
    if (k == 0) {
        for (int c = 0; c < NL; c++) {
            P.x.v[c] = gaff[c];
            P.y.v[c] = gaff[NL + c];
        }
        return !ginf;
    }
    return g1_decode(P, k == q + 1 ? J : Y + (k - 1) * 97);
}

// the table of straus_g1lz_lane over the t = q + 2 bases: multiples 1..8, normalised with one inversion
DEV void pv_table_g1(size_t q, const uint32_t* __restrict__ gaff, uint32_t ginf, const uint8_t* __restrict__ Y,
                     const uint8_t* __restrict__ J, const uint32_t* __restrict__ scal, uint32_t* __restrict__ ent) {
    const size_t t = q + 2;
    uint32_t* zs = ent + t * 8 * SEW;
    uint32_t* pre = zs + t * 8 * LN;
    int8_t* dig = reinterpret_cast<int8_t*>(pre + t * 8 * LN);
    FR acc_z = r1_one();
#pragma unroll 1
    for (size_t k = 0; k < t; k++) {
        cc::Aff<cc::Fp> P1;
        const bool ok = pv_base_g1(P1, k, q, gaff, ginf, Y, J);
        recode_w4(dig + k * 65, scal + k * 8);
        const FR px = reduce(in_r(P1.x)), py = reduce(in_r(P1.y));
        const AG P = ag_of(px, py);
        JG Jm = ok ? JG{px, py, r1_one()} : jg_inf();
#pragma unroll 1
        for (int d = 0; d < 8; d++) {
            if (d == 1) Jm = jg_dbl(Jm);
            else if (d > 1 && ok) Jm = jg_add_aff(Jm, P);
            const size_t e = k * 8 + d;
            uint32_t* w = ent + e * SEW;
            const bool inf = jg_is_inf(Jm);
            st_r1(w, Jm.x);
            st_r1(w + SEY, Jm.y);
            w[SEF] = inf ? 1u : 0u;
            st_r1(zs + e * LN, Jm.z);
            st_r1(pre + e * LN, acc_z);
            if (!inf) acc_z = reduce(mulr1(acc_z, Jm.z));
        }
    }
    cc::Fp zinv_s;
    fp_inv(zinv_s, out_r(acc_z));
    FR zinv = reduce(in_r(zinv_s));
#pragma unroll 1
    for (long long e = (long long)t * 8 - 1; e >= 0; e--) {
        uint32_t* w = ent + (size_t)e * SEW;
        if (w[SEF]) continue;  // identity multiple
        const FR z = ld_r1(zs + (size_t)e * LN);
        const FR zi = reduce(mulr1(zinv, ld_r1(pre + (size_t)e * LN)));
        zinv = reduce(mulr1(zinv, z));
        const FR zi2 = reduce(sqrr1(zi));
        st_r1(w, reduce(mulr1(ld_r1(w), zi2)));
        st_r1(w + SEY, reduce(mulr1(ld_r1(w + SEY), mulr1(zi2, zi))));
    }
}

// acc += the table's affine entry e (multiple d + 1 of base e / 8), negated if neg; identity entries skipped
DEV void pv_add_entry_g1(JG& acc, const uint32_t* __restrict__ ent, size_t e, bool negate) {
    const uint32_t* w = ent + e * SEW;
    if (w[SEF]) return;
    FR ex, ey;
    ld16(ex.v, w);
    ld16(ey.v, w + SEY);
    acc = jg_add_aff(acc, ag_of(ex, negate ? neg(ey) : ey));
}

// one 65-window chain over the bases whose role is `which`
DEV JG pv_chain_g1(size_t t, const uint32_t* __restrict__ role, uint32_t which, const uint32_t* __restrict__ ent) {
    const int8_t* dig = reinterpret_cast<const int8_t*>(ent + t * 8 * (SEW + 2 * LN));
    JG acc = jg_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jg_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jg_dbl(acc);
#pragma unroll 1
        for (size_t k = 0; k < t; k++) {
            if (role[k] != which) continue;  // uniform
            const int d = dig[k * 65 + win];
            if (!d) continue;
            pv_add_entry_g1(acc, ent, k * 8 + (size_t)(d < 0 ? -d : d) - 1, d < 0);
        }
    }
    return acc;
}

// ---------------------------------------------------------------- G2 bases, one proof per lane pair
// base k as lane h's halves; false (pair-uniform): the identity
DEV bool pv_base_g2(AL& P, int h, size_t k, size_t q, const uint32_t* __restrict__ gaff, uint32_t ginf,
                    const uint8_t* __restrict__ Y, const uint8_t* __restrict__ J) {
    pl::Fp2 hx, hy;
    bool ok;
    if (k == 0) {
        for (int c = 0; c < NL; c++) {
            hx.c.v[c] = gaff[NL * h + c];
            hy.c.v[c] = gaff[2 * NL + NL * h + c];
        }
        ok = !ginf;
    } else {
        cc::Aff<cc::Fp2> P1;
        ok = pl::pair_all(g2_decode(P1, k == q + 1 ? J : Y + (k - 1) * 192));  // both lanes decode the point
        hx.c = h ? P1.x.b : P1.x.a;
        hy.c = h ? P1.y.b : P1.y.a;
    }
    P = AL{reduce(in_r2(hx)), reduce(in_r2(hy))};
    return ok;
}

// the table of straus_g2lz_pair over the t = q + 2 bases
DEV void pv_table_g2(int h, size_t q, const uint32_t* __restrict__ gaff, uint32_t ginf, const uint8_t* __restrict__ Y,
                     const uint8_t* __restrict__ J, const uint32_t* __restrict__ scal, uint32_t* __restrict__ ent) {
    const size_t t = q + 2;
    uint32_t* zs = ent + t * 8 * 2 * SEW;
    uint32_t* pre = zs + t * 8 * 2 * LN;
    int8_t* dig = reinterpret_cast<int8_t*>(pre + t * 8 * 2 * LN);
    F2R acc_z = r_one();
#pragma unroll 1
    for (size_t k = 0; k < t; k++) {
        AL P;
        const bool ok = pv_base_g2(P, h, k, q, gaff, ginf, Y, J);
        recode_w4(dig + k * 65, scal + k * 8);  // both lanes write the same digits
        JL Jm = ok ? jl_from_aff(P) : jl_inf();
#pragma unroll 1
        for (int d = 0; d < 8; d++) {
            if (d == 1) Jm = jl_dbl(Jm);
            else if (d > 1 && ok) Jm = jl_add_aff(Jm, P);
            const size_t e = k * 8 + d;
            uint32_t* w = ent + (e * 2 + h) * SEW;
            const bool inf = jl_is_inf(Jm);
            st_w(w, Jm.x);
            st_w(w + SEY, Jm.y);
            w[SEF] = inf ? 1u : 0u;
            st_w(zs + (e * 2 + h) * LN, Jm.z);
            st_w(pre + (e * 2 + h) * LN, acc_z);
            if (!inf) acc_z = reduce(mulr(acc_z, Jm.z));
        }
    }
    F2R zinv = reduce(inv(acc_z));
#pragma unroll 1
    for (long long e = (long long)t * 8 - 1; e >= 0; e--) {
        uint32_t* w = ent + ((size_t)e * 2 + h) * SEW;
        if (w[SEF]) continue;  // identity multiple (pair-uniform: both halves carry the flag)
        const F2R z = ld_w(zs + ((size_t)e * 2 + h) * LN);
        const auto zi = mulr(zinv, ld_w(pre + ((size_t)e * 2 + h) * LN));
        zinv = reduce(mulr(zinv, z));
        const auto zi2 = sqrr(zi);
        st_w(w, reduce(mulr(ld_w(w), zi2)));
        st_w(w + SEY, reduce(mulr(ld_w(w + SEY), mulr(zi2, zi))));
    }
}

DEV void pv_add_entry_g2(JL& acc, int h, const uint32_t* __restrict__ ent, size_t e, bool negate) {
    const uint32_t* w = ent + (e * 2 + h) * SEW;
    if (w[SEF]) return;
    AL a;
    ld16(a.x.c.v, w);
    ld16(a.y.c.v, w + SEY);
    if (negate) a = jl_neg_aff(a);
    acc = jl_add_aff(acc, a);
}

DEV JL pv_chain_g2(int h, size_t t, const uint32_t* __restrict__ role, uint32_t which,
                   const uint32_t* __restrict__ ent) {
    const int8_t* dig = reinterpret_cast<const int8_t*>(ent + t * 8 * 2 * (SEW + 2 * LN));
    JL acc = jl_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jl_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jl_dbl(acc);
#pragma unroll 1
        for (size_t k = 0; k < t; k++) {
            if (role[k] != which) continue;  // uniform
            const int d = dig[k * 65 + win];
            if (!d) continue;
            pv_add_entry_g2(acc, h, ent, k * 8 + (size_t)(d < 0 ? -d : d) - 1, d < 0);
        }
    }
    return acc;
}
}  // namespace

// SigG2 (sigma' in G2; J, T and the verkey in G1): one proof per lane
__global__ __launch_bounds__(256, 2) void k_prep_pok_sigg2_var(
    size_t n, int q, const uint8_t* __restrict__ s1b, const uint8_t* __restrict__ s2b, const uint8_t* __restrict__ Jb,
    const uint8_t* __restrict__ Tb, const uint8_t* __restrict__ vkX, const uint8_t* __restrict__ vkY,
    const uint32_t* __restrict__ gaff, uint32_t ginf, const uint32_t* __restrict__ role,
    const uint32_t* __restrict__ scal, uint32_t* __restrict__ scratch, uint32_t* __restrict__ prep,
    uint32_t* __restrict__ flags) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Soa S{prep, n};
    uint32_t fl = 0;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {  // sigma'_1 -> Q1, -sigma'_2 -> Q2
        Aff<Fp2> a;
        if (!g2_decode(a, (h ? s2b : s1b) + i * 192)) fl |= h ? 2u : 1u;
        if (h) f2_neg(a.y, a.y);
        const int slot = h ? S_Q2 : S_Q1;
        st_f2(S, slot, i, a.x);
        st_f2(S, slot + 2, i, a.y);
    }
    const size_t t = (size_t)q + 2;
    uint32_t* ent = scratch + i * straus_g1lz_words(t);
    pv_table_g1((size_t)q, gaff, ginf, vkY + i * (size_t)q * 97, Jb + i * 97, scal + i * t * 8, ent);
    {  // Schnorr: chain A - T == O ?
        JG a = pv_chain_g1(t, role, 0, ent);
        Aff<Fp> T;
        if (g1_decode(T, Tb + i * 97)) a = jg_add_aff(a, ag_of(reduce(in_r(T.x)), neg(reduce(in_r(T.y)))));
        if (!jg_is_inf(a)) fl |= 8u;
    }
    JG b = pv_chain_g1(t, role, 1, ent);
    {  // J' = chain B + X~ + J (the table's 1 J)
        Aff<Fp> X;
        if (g1_decode(X, vkX + i * 97)) b = jg_add_aff(b, ag_of(reduce(in_r(X.x)), reduce(in_r(X.y))));
        pv_add_entry_g1(b, ent, (t - 1) * 8, false);
    }
    if (jg_is_inf(b)) {
        fl |= 4u;
    } else {  // affine in the R' form (the Miller loop's kAffRp operand)
        Fp x, y;
        jg_to_aff_rp(x, y, b);
        st_fp(S, S_P1, i, x);
        st_fp(S, S_P1 + 1, i, y);
    }
    flags[i] = fl;
}

// SigG1 (sigma' in G1; J, T and the verkey in G2): one proof per lane pair
__global__ __launch_bounds__(256, 2) void k_prep_pok_sigg1_var(
    size_t n, int q, const uint8_t* __restrict__ s1b, const uint8_t* __restrict__ s2b, const uint8_t* __restrict__ Jb,
    const uint8_t* __restrict__ Tb, const uint8_t* __restrict__ vkX, const uint8_t* __restrict__ vkY,
    const uint32_t* __restrict__ gaff, uint32_t ginf, const uint32_t* __restrict__ role,
    const uint32_t* __restrict__ scal, uint32_t* __restrict__ scratch, uint32_t* __restrict__ prep,
    uint32_t* __restrict__ flags) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t i = g >> 1;
    const int h = (int)(g & 1);
    if (i >= n) return;  // pair-uniform
    Soa S{prep, n};
    uint32_t fl = 0;
    {  // sigma'_1 on lane 0 (P1), -sigma'_2 on lane 1 (P2)
        Aff<Fp> a;
        if (!g1_decode(a, (h ? s2b : s1b) + i * 97)) fl |= h ? 2u : 1u;
        if (h) fp_neg(a.y, a.y);
        const int slot = h ? S_P2 : S_P1;
        fp_to_lazy_form(a.x);  // the Miller loop's affine P in the lazy R' form (miller_lz.hip kAffRp)
        fp_to_lazy_form(a.y);
        st_fp(S, slot, i, a.x);
        st_fp(S, slot + 1, i, a.y);
    }
    fl |= pl::swp(fl);
    const size_t t = (size_t)q + 2;
    uint32_t* ent = scratch + i * straus_lz_words(t);
    pv_table_g2(h, (size_t)q, gaff, ginf, vkY + i * (size_t)q * 192, Jb + i * 192, scal + i * t * 8, ent);
    // a G2 encoding as this lane's halves on the lazy field (both lanes decode it)
    auto own = [&](AL& o, const uint8_t* p) {
        Aff<Fp2> a;
        const bool ok = pl::pair_all(g2_decode(a, p));
        pl::Fp2 hx, hy;
        hx.c = h ? a.x.b : a.x.a;
        hy.c = h ? a.y.b : a.y.a;
        o = AL{reduce(in_r2(hx)), reduce(in_r2(hy))};
        return ok;
    };
    {  // Schnorr: chain A - T == O ?
        JL a = pv_chain_g2(h, t, role, 0, ent);
        AL T;
        if (own(T, Tb + i * 192)) a = jl_add_aff(a, jl_neg_aff(T));
        if (!jl_is_inf(a)) fl |= 8u;
    }
    JL b = pv_chain_g2(h, t, role, 1, ent);
    {  // J' = chain B + X~ + J (the table's 1 J)
        AL X;
        if (own(X, vkX + i * 192)) b = jl_add_aff(b, X);
        pv_add_entry_g2(b, h, ent, (t - 1) * 8, false);
    }
    Jac<pl::Fp2> acc = pl::jl_to_pl(b);
    Aff<pl::Fp2> a;
    if (!jac_to_aff(a, acc)) fl |= 4u;
    pl::st_f2(S, S_Q1, i, a.x);
    pl::st_f2(S, S_Q1 + 2, i, a.y);
    if (!h) flags[i] = fl;
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// scratch words of cck_prep_pok_var for n proofs of q messages: the roles, the scalars, the tables
size_t cck_prep_pok_var_words(int mode, size_t n, size_t q) {
    const size_t t = q + 2;
    return straus_round32(t) + straus_round32(n * t * 8) + n * (mode == 0 ? straus_g1lz_words(t) : straus_lz_words(t)) + 64;
}

// Per-proof-verkey PoK prep: d_vkX n x OtherGroup, d_vkY n x q x OtherGroup; d_gaff / ginf: the context's
// g~ (storage-form affine, identity flag); d_rev_idx: r indices (< q, unique) on the device; scratch:
// cck_prep_pok_var_words words.  Writes the Miller-loop operands and flags like cck_prep_pok.
int cck_prep_pok_var(int mode, size_t n, int q, int r, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_J,
                     const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal, const uint8_t* d_rev_msgs,
                     const uint32_t* d_rev_idx, const uint8_t* d_vkX, const uint8_t* d_vkY, const uint32_t* d_gaff,
                     uint32_t ginf, uint32_t* d_scratch, uint32_t* d_prep, uint32_t* d_flags, hipStream_t st) {
    if (!n) return 0;
    const size_t t = (size_t)q + 2;
    uint32_t* role = d_scratch;
    uint32_t* scal = role + straus_round32(t);
    uint32_t* straus = scal + straus_round32(n * t * 8);  // 128-byte-aligned proof regions
    hipLaunchKernelGGL(k_pok_var_scalars, dim3(nblocks(n * t, 256)), dim3(256), 0, st, n, q, r, d_resp, d_chal,
                       d_rev_msgs, d_rev_idx, role, scal);
    if (mode == 0)
        hipLaunchKernelGGL(k_prep_pok_sigg2_var, dim3(nblocks(n, 256)), dim3(256), 0, st, n, q, d_s1, d_s2, d_J, d_T,
                           d_vkX, d_vkY, d_gaff, ginf, role, scal, straus, d_prep, d_flags);
    else
        hipLaunchKernelGGL(k_prep_pok_sigg1_var, dim3(nblocks(2 * n, 256)), dim3(256), 0, st, n, q, d_s1, d_s2, d_J,
                           d_T, d_vkX, d_vkY, d_gaff, ginf, role, scal, straus, d_prep, d_flags);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"
