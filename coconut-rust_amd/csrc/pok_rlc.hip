// RLC batch mode for PoKOfSignatureProof::verify on gfx950: the PoK prep of the RLC partial.
//
// Per proof i the reference checks (ps_sig PoKOfSignatureProof::verify [EXT], reference
// src/pok_sig.rs:103-105) the Schnorr relation g~ resp_0 + sum_hidden Y~_h resp_k + chal J == T and the
// pairing equation e(sigma'_1, J') * e(-sigma'_2, g~) == 1 with J' = X~ + J + sum_revealed m_i Y~_i.
// The pairing equation has the shape of Signature::verify's, so the batch is checked as rlc.hip checks
// signatures:
//
//     prod_i e(sigma'_1,i, delta_i J'_i) * e(-sigma'_2,i, delta_i g~) == 1        (SigG2)
//     prod_i e(delta_i J'_i, sigma'_1,i) * e(g~, -delta_i sigma'_2,i) == 1        (SigG1)
//
// with the delta_i of the same key stream (fr.h rlc_delta_signed), while the Schnorr relation costs no
// pairing and stays an exact per-proof check.  A batch is accepted only if every proof's Schnorr
// relation holds and the delta-weighted product is one; a forged batch passes with probability
// <= 2^-127.  Part 0 of the partial is rlc.hip's k_rlc_check_* on (sigma'_1, sigma'_2) unchanged; the
// kernels here are its part 1; the fold, the Miller loop (two proofs a loop while those waves fit one a
// SIMD, capi_pok.cpp pok_rlc_twin; four beyond) and the product tree follow as for signatures.
//
//   k_rlc_pok_sigg2 / k_rlc_pok_sigg1 : the Schnorr check (flag bit 3), J's subgroup test (flag bit 6)
//                                       and delta J' = delta X~ + sum_revealed (delta m) Y~ + delta J as
//                                       pair 0's other argument in the twin layout (flag bit 2 when
//                                       it is the identity).  Bits 3 and 6 raise the batch's fall-back
//                                       word: the caller then verifies per proof, so verdicts never
//                                       change.  One table of d J, d = 1..15, per proof (jtab) serves
//                                       both chal J (64 windows) and |delta| J (34 windows).
#include "codec.h"
#include "curve_lz.h"
#include "curve_pl.h"
#include "fixed.h"
#include "fr.h"
#include "launch.h"
#include "pairing.h"
#include "soa.h"
#include "subgroup.h"
#include "subgroup_lz.h"

using namespace cc;

namespace {

DEV int twin_slot(int s0, int s1, size_t i) { return (i & 1) ? s1 : s0; }  // rlc.hip

constexpr int kDeltaWin = 34;  // 4-bit windows of |delta| < 2^136

}  // namespace

// SigG2 (J, T, the verkey in G1), split by WAVE as aggregate.hip k_prep_pok_split: a block of 256
// lanes serves 128 proofs.  Waves 0-1 (role A) add g~ resp_0 and the first `split` hidden responses'
// table terms, build the table of d J and run chal J and |delta| J over it; waves 2-3 (role B) take the
// other hidden responses, -T, J's subgroup test and delta X~ + sum_revealed (delta m) Y~.  The two
// partial results cross in LDS: role A checks the Schnorr sum, role B adds delta J and writes
// delta J' affine in the R' form (the Miller loop's kAffRp operand).  Roles are wave-uniform.
constexpr int PR_PB = 128;  // proofs per block
__global__ __launch_bounds__(256, 2) void k_rlc_pok_sigg2(size_t n, size_t ps, int q, int r, int split,
                                                          uint64_t base_index, const uint32_t* __restrict__ key,
                                                          const uint8_t* __restrict__ Jb,
                                                          const uint8_t* __restrict__ Tb,
                                                          const uint8_t* __restrict__ resp,
                                                          const uint8_t* __restrict__ chal,
                                                          const uint8_t* __restrict__ rev_msgs,
                                                          const uint32_t* __restrict__ rev_idx,
                                                          const uint32_t* __restrict__ table, int wbits,
                                                          const uint32_t* __restrict__ binf,
                                                          uint32_t* __restrict__ prep, uint32_t* __restrict__ flags,
                                                          uint32_t* __restrict__ any, uint32_t* __restrict__ jtab) {
    constexpr int JW = sizeof(Jac<Fp>) / 4, LW = sizeof(lz::JG) / 4;
    __shared__ uint32_t sch[PR_PB][JW + 1];  // role B's partial Schnorr sum (storage form)
    __shared__ uint32_t dj[PR_PB][LW + 1];   // role A's delta J (lazy form)
    const bool roleB = threadIdx.x >= PR_PB;  // wave-uniform
    const int sib = (int)(threadIdx.x & (PR_PB - 1));
    const size_t i = blockIdx.x * (size_t)PR_PB + sib;
    const bool active = i < n;
    const Soa S{prep, ps};
    uint32_t fl = 0;
    Jac<Fp> acc;
    jac_set_inf(acc);
    lz::JG lj = lz::jg_inf();  // role A: delta J; role B: delta X~ + sum_revealed (delta m) Y~
    if (active) {
        Aff<Fp> Ja;
        const bool Jok = g1_decode(Ja, Jb + i * 97);
        const uint8_t* rp = resp + i * (size_t)(q - r + 1) * 48;
        const int nwin = ft_nwin(wbits);
        uint32_t kk[NR], d[NR], w4[4];
        for (int k = 0; k < 8; k++) kk[k] = key[k];
        rlc_delta_signed(d, w4, kk, base_index + i);
        uint32_t da[NR];
        const bool neg = rlc_delta_abs(da, d);
        Fr k;
        lz::JG la = lz::jg_inf();  // the Schnorr table terms on the lazy field (fixed.h ft_add_lz)
        if (!roleB) {
            fr_from_be48(k, rp);
            if (!binf[q]) ft_add_lz(la, k.v, table, wbits, q, 0, nwin);  // table base q = g~
        }
        // hidden responses: role A the first `split`, role B the rest
        int slot = 1, hid = 0;
        for (int h = 0; h < q; h++) {
            bool revealed = false;
            for (int z = 0; z < r; z++) revealed |= rev_idx[z] == (uint32_t)h;
            if (revealed) continue;
            const bool mine = roleB ? hid >= split : hid < split;
            hid++;
            if (mine) {
                fr_from_be48(k, rp + (size_t)slot * 48);
                if (!binf[h]) ft_add_lz(la, k.v, table, wbits, h, 0, nwin);
            }
            slot++;
        }
        acc = lz::jg_to(la);
        if (!roleB) {
            if (Jok) {
                // the table of d J, d = 1..15, in the scratch as lazy points (k_prep_pok_split), built once
                auto tab = [&](int dd, int w) -> uint32_t& { return jtab[((size_t)(dd - 1) * LW + w) * n + i]; };
                const lz::AG Jl = ag_from_aff(Ja);
                lz::JG t = lz::jg_add_aff(lz::jg_inf(), Jl);
#pragma unroll 1
                for (int dd = 1; dd <= 15; dd++) {
                    if (dd > 1) t = lz::jg_add_aff(t, Jl);
                    const uint32_t* tw = reinterpret_cast<const uint32_t*>(&t);
                    for (int w = 0; w < LW; w++) tab(dd, w) = tw[w];
                }
                // chal J (the Schnorr sum) and |delta| J (pair 0's argument) in fixed 4-bit windows
                fr_from_be48(k, chal + i * 48);
                lz::JG sacc = lz::jg_inf();
#pragma unroll 1
                for (int win = 63; win >= 0; win--) {
                    for (int b = 0; b < 4; b++) sacc = lz::jg_dbl(sacc);
                    const uint32_t dd = (k.v[win >> 3] >> ((win & 7) * 4)) & 15u;
                    if (dd) {
                        uint32_t* tw = reinterpret_cast<uint32_t*>(&t);
                        for (int w = 0; w < LW; w++) tw[w] = tab((int)dd, w);
                        sacc = lz::jg_add(sacc, t);
                    }
                }
                jac_add(acc, acc, lz::jg_to(sacc));
#pragma unroll 1
                for (int win = kDeltaWin - 1; win >= 0; win--) {
                    for (int b = 0; b < 4; b++) lj = lz::jg_dbl(lj);
                    const uint32_t dd = (da[win >> 3] >> ((win & 7) * 4)) & 15u;
                    if (dd) {
                        uint32_t* tw = reinterpret_cast<uint32_t*>(&t);
                        for (int w = 0; w < LW; w++) tw[w] = tab((int)dd, w);
                        lj = lz::jg_add(lj, t);
                    }
                }
                if (neg) lj.y = lz::reduce(lz::neg(lj.y));
            }
        } else {
            Aff<Fp> Ta;
            if (g1_decode(Ta, Tb + i * 97)) {
                fp_neg(Ta.y, Ta.y);
                jac_add_aff(acc, acc, Ta);
            }
            // J outside the subgroup: the linear-combination argument does not cover it, the batch falls back
            if (Jok && !g1_in_subgroup_lz(Ja)) fl |= 64u;
            if (!binf[q + 1]) ft_add_lz(lj, da, table, wbits, q + 1, 0, nwin, neg);  // delta X~ as +-|delta| X~
            for (int z = 0; z < r; z++) {
                Fr m;
                fr_from_be48(m, rev_msgs + ((size_t)i * r + z) * 48);
                const int h = (int)rev_idx[z];
                if (binf[h]) continue;
                uint32_t dm[NR];
                fr_mul_canon(dm, d, m.v);
                ft_add_lz(lj, dm, table, wbits, h, 0, nwin);
            }
        }
    }
    {
        const uint32_t* lw = reinterpret_cast<const uint32_t*>(&lj);
        const uint32_t* aw = reinterpret_cast<const uint32_t*>(&acc);
        if (roleB)
            for (int c = 0; c < JW; c++) sch[sib][c] = aw[c];
        else
            for (int c = 0; c < LW; c++) dj[sib][c] = lw[c];
    }
    __syncthreads();
    if (!active) return;
    if (!roleB) {
        Jac<Fp> o;
        uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
        for (int c = 0; c < JW; c++) ow[c] = sch[sib][c];
        jac_add(acc, acc, o);
        if (!jac_is_inf(acc)) fl |= 8u;
    } else {
        lz::JG o;
        uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
        for (int c = 0; c < LW; c++) ow[c] = dj[sib][c];
        lj = lz::jg_add(lj, o);
        if (lz::jg_is_inf(lj)) {
            fl |= 4u;
        } else {  // affine in the R' form (the Miller loop's kAffRp operand)
            Fp x, y;
            lz::jg_to_aff_rp(x, y, lj);
            st_fp(S, twin_slot(S_P1, S_P2, i), i >> 1, x);
            st_fp(S, twin_slot(S_P1, S_P2, i) + 1, i >> 1, y);
        }
    }
    if (fl) atomicOr(flags + i, fl);  // both roles add to part 0's word
    if (fl & 72u) atomicOr(any, 1u);  // a failed Schnorr check or J outside the subgroup: the batch falls back
}

// SigG1 (J, T, the verkey in G2), one proof per lane PAIR (curve_pl.h) as aggregate.hip k_prep_pok_g1pl:
// the sums run on the lazy pair-lane field, the table of d J holds this lane's halves.
__global__ __launch_bounds__(256, 2) void k_rlc_pok_sigg1(size_t n, size_t ps, int q, int r, uint64_t base_index,
                                                          const uint32_t* __restrict__ key,
                                                          const uint8_t* __restrict__ Jb,
                                                          const uint8_t* __restrict__ Tb,
                                                          const uint8_t* __restrict__ resp,
                                                          const uint8_t* __restrict__ chal,
                                                          const uint8_t* __restrict__ rev_msgs,
                                                          const uint32_t* __restrict__ rev_idx,
                                                          const uint32_t* __restrict__ table, int wbits,
                                                          const uint32_t* __restrict__ binf,
                                                          uint32_t* __restrict__ prep, uint32_t* __restrict__ flags,
                                                          uint32_t* __restrict__ any, uint32_t* __restrict__ jtab) {
    using G2 = pl::Fp2;
    constexpr int LW = sizeof(lz::JL) / 4;
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t i = g >> 1;
    const int h = (int)(g & 1);
    if (i >= n) return;  // pair-uniform
    const Soa S{prep, ps};
    uint32_t fl = 0;
    // a G2 point as this lane's halves (both lanes decode it)
    auto own = [&](Aff<G2>& o, const Aff<Fp2>& a) {
        o.x.c = h ? a.x.b : a.x.a;
        o.y.c = h ? a.y.b : a.y.a;
    };
    Aff<Fp2> Jf;
    const bool Jok = pl::pair_all(g2_decode(Jf, Jb + i * 192));
    Aff<G2> Ja;
    own(Ja, Jf);
    // J outside the subgroup: the linear-combination argument does not cover it, the batch falls back
    if (Jok && !pl::g2_in_subgroup_lz(Ja)) fl |= 64u;
    uint32_t kk[NR], d[NR], w4[4];
    for (int k = 0; k < 8; k++) kk[k] = key[k];
    rlc_delta_signed(d, w4, kk, base_index + i);
    uint32_t da[NR];
    const bool neg = rlc_delta_abs(da, d);
    const int nwin = ft_nwin(wbits);
    auto tab = [&](int dd, int w) -> uint32_t& { return jtab[((size_t)(dd - 1) * LW + w) * 2 * n + g]; };
    lz::JL dJ = lz::jl_inf();  // delta J
    {  // Schnorr: g~ resp[0] + sum_hidden Y~_h resp[k] + J chal - T == O ?
        Fr k;
        const uint8_t* rp = resp + i * (size_t)(q - r + 1) * 48;
        fr_from_be48(k, rp);
        lz::JL la = lz::jl_inf();  // the table terms on the lazy pair-lane field
        if (!binf[q]) pl::ft_add_g2_lz(la, k.v, table, wbits, q, 0, nwin);  // table base q = g~
        int slot = 1;
        for (int hh = 0; hh < q; hh++) {
            bool revealed = false;
            for (int z = 0; z < r; z++) revealed |= rev_idx[z] == (uint32_t)hh;
            if (revealed) continue;
            fr_from_be48(k, rp + (size_t)slot * 48);
            slot++;
            if (!binf[hh]) pl::ft_add_g2_lz(la, k.v, table, wbits, hh, 0, nwin);
        }
        fr_from_be48(k, chal + i * 48);
        if (Jok) {
            // the table of d J, d = 1..15, in the scratch as lazy points (k_prep_pok_g1pl), built once;
            // chal J (the Schnorr sum) and |delta| J (pair 0's argument) in fixed 4-bit windows over it
            const lz::AL Jl{lz::reduce(lz::in_r2(Ja.x)), lz::reduce(lz::in_r2(Ja.y))};
            lz::JL t = lz::jl_from_aff(Jl);
#pragma unroll 1
            for (int dd = 1; dd <= 15; dd++) {
                if (dd > 1) t = lz::jl_add_aff(t, Jl);
                const uint32_t* tw = reinterpret_cast<const uint32_t*>(&t);
                for (int w = 0; w < LW; w++) tab(dd, w) = tw[w];
            }
            lz::JL sacc = lz::jl_inf();
#pragma unroll 1
            for (int win = 63; win >= 0; win--) {
                for (int b = 0; b < 4; b++) sacc = lz::jl_dbl(sacc);
                const uint32_t dd = (k.v[win >> 3] >> ((win & 7) * 4)) & 15u;
                if (dd) {
                    uint32_t* tw = reinterpret_cast<uint32_t*>(&t);
                    for (int w = 0; w < LW; w++) tw[w] = tab((int)dd, w);
                    sacc = lz::jl_add(sacc, t);
                }
            }
            la = lz::jl_add(la, sacc);
#pragma unroll 1
            for (int win = kDeltaWin - 1; win >= 0; win--) {
                for (int b = 0; b < 4; b++) dJ = lz::jl_dbl(dJ);
                const uint32_t dd = (da[win >> 3] >> ((win & 7) * 4)) & 15u;
                if (dd) {
                    uint32_t* tw = reinterpret_cast<uint32_t*>(&t);
                    for (int w = 0; w < LW; w++) tw[w] = tab((int)dd, w);
                    dJ = lz::jl_add(dJ, t);
                }
            }
            if (neg) dJ.y = lz::reduce(lz::neg(dJ.y));
        }
        Jac<G2> acc = pl::jl_to_pl(la);
        Aff<Fp2> Tf;
        if (pl::pair_all(g2_decode(Tf, Tb + i * 192))) {
            Aff<G2> Ta;
            own(Ta, Tf);
            FT<G2>::neg(Ta.y, Ta.y);
            jac_add_aff(acc, acc, Ta);
        }
        if (!jac_is_inf(acc)) fl |= 8u;
    }
    // delta J' = delta X~ + sum_revealed (delta m_i) Y~_i + delta J
    if (!binf[q + 1]) pl::ft_add_g2_lz(dJ, da, table, wbits, q + 1, 0, nwin, neg);  // +-|delta| X~
    for (int z = 0; z < r; z++) {
        Fr m;
        fr_from_be48(m, rev_msgs + ((size_t)i * r + z) * 48);
        const int hh = (int)rev_idx[z];
        if (binf[hh]) continue;
        uint32_t dm[NR];
        fr_mul_canon(dm, d, m.v);
        pl::ft_add_g2_lz(dJ, dm, table, wbits, hh, 0, nwin);
    }
    const Jac<G2> jp = pl::jl_to_pl(dJ);
    Aff<G2> a;
    if (!jac_to_aff(a, jp)) fl |= 4u;
    pl::st_f2(S, twin_slot(S_Q1, S_Q2, i), i >> 1, a.x);
    pl::st_f2(S, twin_slot(S_Q1, S_Q2, i) + 2, i >> 1, a.y);
    if (!h && fl) {
        flags[i] |= fl;  // part 0's word
        if (fl & 72u) atomicOr(any, 1u);  // a failed Schnorr check or J outside the subgroup: the batch falls back
    }
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// Part 1 of the PoK RLC partial (part 0: rlc.hip cck_prep_rlc part 0 on sigma'_1 / sigma'_2).  ps: the
// prep SoA's stride (>= (n + 1) / 2, the twin layout); d_jtab: 15 Jacobian points of the other group per
// proof (<= 15 x 84 words, as cck_prep_pok); d_flags / d_any: part 0's words, OR-ed into.
int cck_prep_pok_rlc(int mode, size_t n, size_t ps, int q, int r, uint64_t base_index, const uint32_t* d_key,
                     const uint8_t* d_J, const uint8_t* d_T, const uint8_t* d_resp, const uint8_t* d_chal,
                     const uint8_t* d_rev_msgs, const uint32_t* d_rev_idx, const uint32_t* d_table, int wbits,
                     const uint32_t* d_binf, uint32_t* d_prep, uint32_t* d_flags, uint32_t* d_any, uint32_t* d_jtab,
                     hipStream_t st) {
    if (!n) return 0;
    if (mode == 0) {
        // hidden responses for role A, in mixed-addition units: nwin (1 + split) + ~233 (chal J) + ~123
        // (|delta| J) against nwin (hidden - split) + nwin r (delta m Y~) + ~130 (J's subgroup test, delta X~)
        const int hidden = q - r, nwin = ft_nwin(wbits);
        int split = (nwin * (hidden + r - 1) - 226) / (2 * nwin);
        split = split < 0 ? 0 : (split > hidden ? hidden : split);
        hipLaunchKernelGGL(k_rlc_pok_sigg2, dim3(nblocks(n, PR_PB)), dim3(2 * PR_PB), 0, st, n, ps, q, r, split,
                           base_index, d_key, d_J, d_T, d_resp, d_chal, d_rev_msgs, d_rev_idx, d_table, wbits, d_binf,
                           d_prep, d_flags, d_any, d_jtab);
    } else {
        hipLaunchKernelGGL(k_rlc_pok_sigg1, dim3(nblocks(2 * n, 256)), dim3(256), 0, st, n, ps, q, r, base_index, d_key,
                           d_J, d_T, d_resp, d_chal, d_rev_msgs, d_rev_idx, d_table, wbits, d_binf, d_prep, d_flags,
                           d_any, d_jtab);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
