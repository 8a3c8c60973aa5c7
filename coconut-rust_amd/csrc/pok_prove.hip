// Holder-side batch kernels for gfx950: ps_sig PoKOfSignature::init / gen_proof [EXT] (called at
// reference src/pok_sig.rs:64-100) and BlindSignature::unblind (src/signature.rs:436-443).
//
//   PoKOfSignature::init, per credential with fresh r1, r2 and blindings b_0 .. b_hidden:
//       sigma'_1 = r1 sigma_1,  sigma'_2 = r1 (sigma_2 + r2 sigma_1)
//       J = r2 g~ + sum_hidden m_i Y~_i,  T = b_0 g~ + sum_hidden b_j Y~_i
//     k_sigma_prime_* : both sigma' in ONE pass of the 65 signed 4-bit windows (straus.h's entry layout
//       and digits): the multiples 1..8 of sigma_1 and sigma_2 normalised with one inversion, then two
//       accumulators, A += d(r1) sigma_1 and B += d(r1) sigma_2 + d(r1 r2) sigma_1, sharing sigma_1's
//       table: 520 doublings and at most 195 mixed additions a proof against 780 doublings for three
//       separate scalar multiplications.  SigG2: one proof per lane pair (lazy pair-lane field);
//       SigG1: one proof per lane.
//     k_pok_commit_* : J and T over the verkey's fixed-base tables (table base q = g~), no doublings;
//       the two sums are independent and take wave-uniform roles (waves 0-1 of a block J, waves 2-3 T).
//   gen_proof: k_pok_responses, one lane per (proof, response): b - chal * secret mod r.
//   unblind: k_unblind_assemble lays (c1, c2) and (-sk, 1) out for the windowed Straus MSM
//     (aggregate.hip k_msm_straus, t = 2).
#include "fixed.h"
#include "launch.h"
#include "prove_common.h"

using namespace cc;

namespace {

constexpr int SP_DIGW = (2 * 65 + 3) / 4;   // digits of r1 and of r1 r2
constexpr int SP_PB = 128;                  // SigG2: proofs per block (one lane pair each)
constexpr int SP_LB = 64;                   // SigG1: proofs per block (one lane each)
constexpr int PC_PB_G1 = 128;               // commit kernel, G1 sums: proofs per block (a lane per role)
constexpr int PC_PB_G2 = 64;                // commit kernel, G2 sums: proofs per block (a lane pair per role)

__host__ __device__ inline size_t sp_words_g2() {
    return straus_round32((size_t)SP_ENT * 2 * (SEW + 2 * lz::LN) + SP_DIGW);
}
__host__ __device__ inline size_t sp_words_g1() {
    return straus_round32((size_t)SP_ENT * (SEW + 2 * lz::LN) + SP_DIGW);
}

// r1 and r1 r2 mod r as signed radix-16 digits: dig[0..65) and dig[65..130)
DEV void sp_digits(int8_t* dig, const uint8_t* rnd) {
    Fr r1, r2;
    fr_from_be48(r1, rnd);
    fr_from_be48(r2, rnd + 48);
    alignas(16) uint32_t a[8], b[8];
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = r1.v[w];
    fr_mul_canon(b, r1.v, r2.v);
    recode_w4(dig, a);
    recode_w4(dig + 65, b);
}

DEV bool pp_revealed(int hh, int r, const uint32_t* rev_idx) {
    bool rv = false;
    for (int z = 0; z < r; z++) rv |= rev_idx[z] == (uint32_t)hh;
    return rv;
}

}  // namespace

// ================================================================ sigma' (SigG2: sigma in G2)
// One proof per lane pair, as straus.h straus_g2lz_pair with the two bases sigma_1, sigma_2 on the one
// pair and two accumulators.  Scratch per proof: 16 entries [entry][half][32], 16 Z's, 16 prefix
// products [entry][half][LN], 130 digit bytes.
__global__ __launch_bounds__(256, 2) void k_sigma_prime_g2(size_t n, size_t rstride, const uint8_t* __restrict__ s1b,
                                                          const uint8_t* __restrict__ s2b,
                                                          const uint8_t* __restrict__ rnd,
                                                          uint32_t* __restrict__ scratch, uint8_t* __restrict__ o1,
                                                          uint8_t* __restrict__ o2) {
    using namespace lz;
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t i = g >> 1;
    const int h = (int)(g & 1);
    if (i >= n) return;  // pair-uniform
    uint32_t* ent = scratch + i * sp_words_g2();
    uint32_t* zs = ent + SP_ENT * 2 * SEW;
    uint32_t* pre = zs + SP_ENT * 2 * LN;
    int8_t* dig = reinterpret_cast<int8_t*>(pre + SP_ENT * 2 * LN);
    sp_digits(dig, rnd + i * rstride * 48);  // both lanes write the same digits
    // the multiples 1..8 of sigma_1 (entries 0..7) and sigma_2 (8..15), one inversion (prove_common.h)
    F2R acc_z = r_one();
    sp_fill_g2(ent, zs, pre, h, 0, s1b + i * 192, acc_z);
    sp_fill_g2(ent, zs, pre, h, 1, s2b + i * 192, acc_z);
    sp_norm_g2(ent, zs, pre, h, acc_z);
    // A += d(r1) sigma_1;  B += d(r1) sigma_2 + d(r1 r2) sigma_1
    JL A = jl_inf(), B = jl_inf();
    auto add_entry = [&](JL& acc, int base, int d) { sp_add_g2(acc, ent, h, base, d); };
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64) {
            if (!jl_is_inf(A))
#pragma unroll 1
                for (int z = 0; z < 4; z++) A = jl_dbl(A);
            if (!jl_is_inf(B))
#pragma unroll 1
                for (int z = 0; z < 4; z++) B = jl_dbl(B);
        }
        const int d1 = dig[win], d3 = dig[65 + win];
        if (d1) {
            add_entry(A, 0, d1);
            add_entry(B, 1, d1);
        }
        if (d3) add_entry(B, 0, d3);
    }
    g2lz_out(A, h, o1 + i * 192);
    g2lz_out(B, h, o2 + i * 192);
}

// ================================================================ sigma' (SigG1: sigma in G1)
// One proof per lane, as straus.h straus_g1lz_lane.  Scratch per proof: 16 entries [entry][32], 16 Z's,
// 16 prefix products [entry][LN], 130 digit bytes.
__global__ __launch_bounds__(SP_LB) void k_sigma_prime_g1(size_t n, size_t rstride, const uint8_t* __restrict__ s1b,
                                                          const uint8_t* __restrict__ s2b,
                                                          const uint8_t* __restrict__ rnd,
                                                          uint32_t* __restrict__ scratch, uint8_t* __restrict__ o1,
                                                          uint8_t* __restrict__ o2) {
    using namespace lz;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* ent = scratch + i * sp_words_g1();
    uint32_t* zs = ent + SP_ENT * SEW;
    uint32_t* pre = zs + SP_ENT * LN;
    int8_t* dig = reinterpret_cast<int8_t*>(pre + SP_ENT * LN);
    sp_digits(dig, rnd + i * rstride * 48);
    FR acc_z = r1_one();
    sp_fill_g1(ent, zs, pre, 0, s1b + i * 97, acc_z);
    sp_fill_g1(ent, zs, pre, 1, s2b + i * 97, acc_z);
    sp_norm_g1(ent, zs, pre, acc_z);
    JG A = jg_inf(), B = jg_inf();
    auto add_entry = [&](JG& acc, int base, int d) { sp_add_g1(acc, ent, base, d); };
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64) {
            if (!jg_is_inf(A))
#pragma unroll 1
                for (int z = 0; z < 4; z++) A = jg_dbl(A);
            if (!jg_is_inf(B))
#pragma unroll 1
                for (int z = 0; z < 4; z++) B = jg_dbl(B);
        }
        const int d1 = dig[win], d3 = dig[65 + win];
        if (d1) {
            add_entry(A, 0, d1);
            add_entry(B, 1, d1);
        }
        if (d3) add_entry(B, 0, d3);
    }
    g1lz_out(A, o1 + i * 97);
    g1lz_out(B, o2 + i * 97);
}

// ================================================================ J and T over the verkey tables
// Role J (waves 0-1): r2 g~ + sum_hidden m_i Y~_i; role T (waves 2-3): b_0 g~ + sum_hidden b_j Y~_i.
// rnd: per proof r1 | r2 | b_0 .. b_{nresp-1}.  Bases that are the identity (binf) are skipped.
// SigG2 (the verkey in G1): one lane per (proof, role) on the lazy field (fixed.h ft_add_lz).
__global__ __launch_bounds__(256, 2) void k_pok_commit_g1(size_t n, int q, int r, size_t rstride,
                                                         const uint8_t* __restrict__ msgs,
                                                         const uint8_t* __restrict__ rnd,
                                                         const uint32_t* __restrict__ rev_idx,
                                                         const uint32_t* __restrict__ table, int wbits,
                                                         const uint32_t* __restrict__ binf, uint8_t* __restrict__ oJ,
                                                         uint8_t* __restrict__ oT) {
    const bool roleT = threadIdx.x >= PC_PB_G1;  // wave-uniform
    const size_t i = blockIdx.x * (size_t)PC_PB_G1 + (threadIdx.x & (PC_PB_G1 - 1));
    if (i >= n) return;
    const int nwin = ft_nwin(wbits);
    const uint8_t* rp = rnd + i * rstride * 48;
    lz::JG la = lz::jg_inf();
    Fr k;
    fr_from_be48(k, rp + (roleT ? 96 : 48));  // b_0 or r2
    if (!binf[q]) ft_add_lz(la, k.v, table, wbits, q, 0, nwin);  // table base q = g~
    int slot = 1;
    for (int hh = 0; hh < q; hh++) {
        if (pp_revealed(hh, r, rev_idx)) continue;
        fr_from_be48(k, roleT ? rp + (size_t)(2 + slot) * 48 : msgs + (i * (size_t)q + hh) * 48);
        slot++;
        if (!binf[hh]) ft_add_lz(la, k.v, table, wbits, hh, 0, nwin);
    }
    g1lz_out(la, (roleT ? oT : oJ) + i * 97);
}

// SigG1 (the verkey in G2): one lane pair per (proof, role) on the lazy pair-lane field
// (curve_pl.h ft_add_g2_lz), as aggregate.hip k_prep_pok_g1pl's table terms.
__global__ __launch_bounds__(256, 2) void k_pok_commit_g2(size_t n, int q, int r, size_t rstride,
                                                         const uint8_t* __restrict__ msgs,
                                                         const uint8_t* __restrict__ rnd,
                                                         const uint32_t* __restrict__ rev_idx,
                                                         const uint32_t* __restrict__ table, int wbits,
                                                         const uint32_t* __restrict__ binf, uint8_t* __restrict__ oJ,
                                                         uint8_t* __restrict__ oT) {
    const bool roleT = threadIdx.x >= 2 * PC_PB_G2;  // wave-uniform
    const int lane = (int)(threadIdx.x & (2 * PC_PB_G2 - 1));
    const size_t i = blockIdx.x * (size_t)PC_PB_G2 + (lane >> 1);
    const int h = lane & 1;
    if (i >= n) return;  // pair-uniform
    const int nwin = ft_nwin(wbits);
    const uint8_t* rp = rnd + i * rstride * 48;
    lz::JL la = lz::jl_inf();
    Fr k;
    fr_from_be48(k, rp + (roleT ? 96 : 48));  // b_0 or r2
    if (!binf[q]) pl::ft_add_g2_lz(la, k.v, table, wbits, q, 0, nwin);  // table base q = g~
    int slot = 1;
    for (int hh = 0; hh < q; hh++) {
        if (pp_revealed(hh, r, rev_idx)) continue;
        fr_from_be48(k, roleT ? rp + (size_t)(2 + slot) * 48 : msgs + (i * (size_t)q + hh) * 48);
        slot++;
        if (!binf[hh]) pl::ft_add_g2_lz(la, k.v, table, wbits, hh, 0, nwin);
    }
    g2lz_out(la, h, (roleT ? oT : oJ) + i * 192);
}

// ================================================================ gen_proof responses
// One lane per (proof, response j): b_j - chal * secret_j mod r, secret_0 = r2, secret_{1+j} = the j-th
// hidden message (ascending index).
__global__ __launch_bounds__(256) void k_pok_responses(size_t n, int q, int r, int nresp,
                                                       const uint8_t* __restrict__ msgs,
                                                       const uint8_t* __restrict__ rnd,
                                                       const uint8_t* __restrict__ chal,
                                                       const uint32_t* __restrict__ rev_idx,
                                                       uint8_t* __restrict__ out) {
    const size_t gi = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (gi >= n * (size_t)nresp) return;
    const size_t i = gi / nresp;
    const int j = (int)(gi % nresp);
    const uint8_t* rp = rnd + i * (size_t)(nresp + 2) * 48;
    const uint8_t* sec = rp + 48;  // r2
    if (j) {
        int hid = 0, hh = 0;
        for (; hh < q; hh++) {
            if (pp_revealed(hh, r, rev_idx)) continue;
            if (++hid == j) break;
        }
        sec = msgs + (i * (size_t)q + hh) * 48;
    }
    Fr b, c, s;
    fr_from_be48(b, rp + (size_t)(2 + j) * 48);
    fr_from_be48(c, chal + i * 48);
    fr_from_be48(s, sec);
    Fm x, y, d;
    fr_mul_canon(y.v, c.v, s.v);
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = b.v[w];
    fm_sub(d, x, y);
    store_fr_be48(out + gi * 48, d.v);
}

// ================================================================ unblind
// Straus task i (t = 2): bases (c1_i, c2_i) as encodings, scalars (-sk_i mod r, 1) as canonical 8-limb Fr
template <int SB>
__global__ __launch_bounds__(64) void k_unblind_assemble(size_t n, const uint8_t* __restrict__ c1,
                                                         const uint8_t* __restrict__ c2,
                                                         const uint8_t* __restrict__ sk, uint8_t* __restrict__ pts,
                                                         uint32_t* __restrict__ sc) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* p = pts + i * 2 * SB;
    for (int b = 0; b < SB; b++) {
        p[b] = c1[i * SB + b];
        p[SB + b] = c2[i * SB + b];
    }
    Fr v;
    fr_from_be48(v, sk + i * 48);
    uint32_t o = 0, br = 0;
    uint32_t* s = sc + i * 16;
    for (int w = 0; w < 8; w++) o |= v.v[w];
    for (int w = 0; w < 8; w++) {
        const uint32_t t = __builtin_subc(rl(w), v.v[w], br, &br);
        s[w] = o ? t : 0u;
        s[8 + w] = w == 0 ? 1u : 0u;
    }
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// scratch words of cck_sigma_prime for n proofs (mode 0 SigG2, 1 SigG1)
size_t cck_sigma_prime_words(int mode, size_t n) { return n * (mode == 0 ? sp_words_g2() : sp_words_g1()); }

// d_rnd: n x rstride scalars, r1 | r2 first; d_scratch: cck_sigma_prime_words, 256-byte aligned
int cck_sigma_prime(int mode, size_t n, size_t rstride, const uint8_t* d_s1, const uint8_t* d_s2, const uint8_t* d_rnd,
                    uint32_t* d_scratch, uint8_t* d_o1, uint8_t* d_o2, hipStream_t st) {
    if (!n) return 0;
    if (mode == 0)
        hipLaunchKernelGGL(k_sigma_prime_g2, dim3(nblocks(n, SP_PB)), dim3(2 * SP_PB), 0, st, n, rstride, d_s1, d_s2,
                           d_rnd, d_scratch, d_o1, d_o2);
    else
        hipLaunchKernelGGL(k_sigma_prime_g1, dim3(nblocks(n, SP_LB)), dim3(SP_LB), 0, st, n, rstride, d_s1, d_s2, d_rnd,
                           d_scratch, d_o1, d_o2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_pok_commit(int mode, size_t n, int q, int r, const uint8_t* d_msgs, const uint8_t* d_rnd,
                   const uint32_t* d_rev_idx, const uint32_t* d_table, int wbits, const uint32_t* d_binf, uint8_t* d_J,
                   uint8_t* d_T, hipStream_t st) {
    if (!n) return 0;
    const size_t rstride = (size_t)(q - r + 1) + 2;
    if (mode == 0)
        hipLaunchKernelGGL(k_pok_commit_g1, dim3(nblocks(n, PC_PB_G1)), dim3(2 * PC_PB_G1), 0, st, n, q, r, rstride,
                           d_msgs, d_rnd, d_rev_idx, d_table, wbits, d_binf, d_J, d_T);
    else
        hipLaunchKernelGGL(k_pok_commit_g2, dim3(nblocks(n, PC_PB_G2)), dim3(4 * PC_PB_G2), 0, st, n, q, r, rstride,
                           d_msgs, d_rnd, d_rev_idx, d_table, wbits, d_binf, d_J, d_T);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_pok_responses(size_t n, int q, int r, const uint8_t* d_msgs, const uint8_t* d_rnd, const uint8_t* d_chal,
                      const uint32_t* d_rev_idx, uint8_t* d_out, hipStream_t st) {
    if (!n) return 0;
    const int nresp = q - r + 1;
    hipLaunchKernelGGL(k_pok_responses, dim3(nblocks(n * (size_t)nresp, 256)), dim3(256), 0, st, n, q, r, nresp, d_msgs,
                       d_rnd, d_chal, d_rev_idx, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_unblind_assemble(int group, size_t n, const uint8_t* d_c1, const uint8_t* d_c2, const uint8_t* d_sk,
                         uint8_t* d_pts, uint32_t* d_sc, hipStream_t st) {
    if (!n) return 0;
    if (group == 1)
        hipLaunchKernelGGL(k_unblind_assemble<97>, dim3(nblocks(n, 64)), dim3(64), 0, st, n, d_c1, d_c2, d_sk, d_pts,
                           d_sc);
    else
        hipLaunchKernelGGL(k_unblind_assemble<192>, dim3(nblocks(n, 64)), dim3(64), 0, st, n, d_c1, d_c2, d_sk, d_pts,
                           d_sc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
