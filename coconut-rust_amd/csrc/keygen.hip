// Keygen kernels for gfx950: the dealer's side of reference src/keygen.rs — trusted_party_SSS_keygen (53-71),
// trusted_party_PVSS_keygen (74-122) with keygen_from_shares (17-45), and the last step of the decentralized
// keygen (124-205), for whole batches of independent keygens.  The caller supplies the polynomials.
//
//   deal, per keygen with polynomials f_0 (x), f_{1+j} (y_j) and blinding polynomials f'_p, t coefficients each:
//     k_kg_eval     : one lane per (keygen, polynomial, signer): f_p(id) and f'_p(id), id = 1 .. total, by
//                     Horner over fr.h's Fm.  The accumulator and the coefficients stay canonical: the only
//                     Montgomery value is the id, so acc * id needs no conversion either way.
//     k_kg_commit   : one lane per (keygen, polynomial, coefficient): C_i = f_i g + f'_i h over the two-base
//                     G1 table [g, h] on the lazy field (fixed.h ft_add_lz), no doublings; the mixed addition
//                     handles an identity accumulator and equal and opposite operands (h = +-g).
//     k_kg_derive_* : g~ * share for every share the evaluation wrote: one (keygen, signer, polynomial) per lane
//                     when OtherGroup is G1 (SigG2 mode), per lane pair when it is G2 (SigG1 mode), over g~'s
//                     table.  A launch of its own, with the block sizes of sigreq_prove.hip's k_rq_short_*.
//   combine, m groups of d dealers:
//     k_kg_sum_fr   : one lane per output scalar, the sum of the d dealers' shares mod r.
//     k_kg_sum_g1   : one lane per output commitment, the d dealers' commitments added with the complete
//                     mixed addition (equal addends double, opposite ones cancel, an identity or undecodable
//                     addend is skipped, a sum that returns to the identity restarts).
//     k_kg_derive_* again for g~ * the combined shares.
//
// Tables (cck_build_table, built by cc_set_keygen_params): every one in the lazy form — the G1 tables are
// read by ft_add_lz, a G2 g~ table by the lane-pair consumer curve_pl.h ft_add_g2_lz, which reads the
// lazy form as the request params' and the verkey's G2 tables are read.
//
// Measured on one MI355X (tools/bench_keygen.py, 16-bit tables, inputs in HBM, one batch in flight; DESIGN.md
// "Device keygen"), milliseconds a call, SigG2 / SigG1:
//   4,096 committees of (t, total, q) = (3, 5, 6): deal 1.45 / 2.21 (2.82 M / 1.85 M keygens/s), Shamir deal
//     0.665 / 1.41, combine of d = 5 dealers 0.499 / 0.596, the derivation alone 0.663 / 1.41 for 143,360 scalars
//   8 committees of (67, 100, 32): deal 1.00 / 1.10, Shamir deal 0.415 / 0.511, the derivation alone 0.305 / 0.400
//   the derivation against cc_fixed_base_mul on the same scalars in the same run (upload, an 8-bit table built
//   per call, download): 8.4x / 11.1x at the first shape, 14.2x / 29.7x at the second; spreads below 1 % (the
//   yardstick's below 3 %).
#include "fixed.h"
#include "launch.h"
#include "prove_common.h"

using namespace cc;

namespace {

constexpr int KG_FB_G1 = 256;  // fixed-base kernels, G1 sums: tasks per block (one lane each)
constexpr int KG_FB_G2 = 128;  // fixed-base kernels, G2 sums: tasks per block (one lane pair each)
constexpr int KG_FR = 256;     // scalar kernels: lanes per block

// a + b mod r for canonical a, b (r < 2^255: the sum has no carry word)
DEV void kg_add(uint32_t a[8], const uint32_t b[8]) {
    uint32_t s[8], cy = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) s[w] = __builtin_addc(a[w], b[w], cy, &cy);
    Fm r;
    fm_reduce_once(r, s);
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = r.v[w];
}

// f(id) for the t coefficients at c (48 B each, degree ascending), id in Montgomery form
DEV void kg_horner(uint32_t out[8], const uint8_t* c, int t, const Fm& idm) {
    Fm acc;
    Fr k;
    fr_from_be48(k, c + (size_t)(t - 1) * 48);
#pragma unroll
    for (int w = 0; w < 8; w++) acc.v[w] = k.v[w];
#pragma unroll 1
    for (int i = t - 2; i >= 0; i--) {
        acc = fm_mul_v(acc, idm);  // canonical x Montgomery: acc * id, canonical
        fr_from_be48(k, c + (size_t)i * 48);
        kg_add(acc.v, k.v);
    }
#pragma unroll
    for (int w = 0; w < 8; w++) out[w] = acc.v[w];
}

// where the share of (signer row sr = keygen * total + signer, polynomial p) lives: x for p = 0, y_{p-1}
DEV size_t kg_share_off(size_t sr, int q, int p) { return p == 0 ? sr : sr * (size_t)q + (size_t)(p - 1); }

}  // namespace

// ================================================================ evaluation
// task = (keygen * (q + 1) + p) * total + s; ct, xt, yt: NULL for Shamir
__global__ __launch_bounds__(KG_FR) void k_kg_eval(size_t ntask, int q, int t, int total,
                                                  const uint8_t* __restrict__ cf, const uint8_t* __restrict__ ct,
                                                  uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                  uint8_t* __restrict__ xt, uint8_t* __restrict__ yt) {
    const size_t task = blockIdx.x * (size_t)KG_FR + threadIdx.x;
    if (task >= ntask) return;
    const size_t poly = task / (size_t)total;  // keygen * (q + 1) + p
    const int s = (int)(task % (size_t)total);
    const size_t kg = poly / (size_t)(q + 1);
    const int p = (int)(poly % (size_t)(q + 1));
    const Fm idm = fm_from_u64((uint64_t)s + 1);
    const size_t sr = kg * (size_t)total + s;
    const size_t o = kg_share_off(sr, q, p) * 48;
    uint32_t v[8];
    kg_horner(v, cf + poly * (size_t)t * 48, t, idm);
    store_fr_be48((p == 0 ? x : y) + o, v);
    if (ct) {
        kg_horner(v, ct + poly * (size_t)t * 48, t, idm);
        store_fr_be48((p == 0 ? xt : yt) + o, v);
    }
}

// ================================================================ commitments C = f g + f' h (G1)
// lane = (keygen * (q + 1) + p) * t + i, the index of the coefficient and of its commitment
__global__ __launch_bounds__(KG_FB_G1, 2) void k_kg_commit(size_t n, const uint8_t* __restrict__ cf,
                                                          const uint8_t* __restrict__ ct,
                                                          const uint32_t* __restrict__ table, int wbits,
                                                          const uint32_t* __restrict__ binf,
                                                          uint8_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)KG_FB_G1 + threadIdx.x;
    if (i >= n) return;
    const int nwin = ft_nwin(wbits);
    lz::JG la = lz::jg_inf();
    Fr s;
    if (!binf[0]) {
        fr_from_be48(s, cf + i * 48);
        ft_add_lz(la, s.v, table, wbits, 0, 0, nwin);
    }
    if (!binf[1]) {
        fr_from_be48(s, ct + i * 48);
        ft_add_lz(la, s.v, table, wbits, 1, 0, nwin);
    }
    g1lz_out(la, out + i * 97);
}

// ================================================================ derivation g~ * share
// task = (keygen * total + signer) * (q + 1) + p over nrow = keygens * total signer rows
__global__ __launch_bounds__(KG_FB_G1, 2) void k_kg_derive_g1(size_t nrow, int q, const uint8_t* __restrict__ x,
                                                             const uint8_t* __restrict__ y,
                                                             const uint32_t* __restrict__ table, int wbits,
                                                             const uint32_t* __restrict__ binf,
                                                             uint8_t* __restrict__ X, uint8_t* __restrict__ Y) {
    const size_t task = blockIdx.x * (size_t)KG_FB_G1 + threadIdx.x;
    if (task >= nrow * (size_t)(q + 1)) return;
    const size_t sr = task / (size_t)(q + 1);
    const int p = (int)(task % (size_t)(q + 1));
    const size_t o = kg_share_off(sr, q, p);
    lz::JG la = lz::jg_inf();
    if (!binf[0]) {
        Fr s;
        fr_from_be48(s, (p == 0 ? x : y) + o * 48);
        ft_add_lz(la, s.v, table, wbits, 0, 0, ft_nwin(wbits));
    }
    g1lz_out(la, (p == 0 ? X : Y) + o * 97);
}

__global__ __launch_bounds__(2 * KG_FB_G2, 2) void k_kg_derive_g2(size_t nrow, int q, const uint8_t* __restrict__ x,
                                                                 const uint8_t* __restrict__ y,
                                                                 const uint32_t* __restrict__ table, int wbits,
                                                                 const uint32_t* __restrict__ binf,
                                                                 uint8_t* __restrict__ X, uint8_t* __restrict__ Y) {
    const size_t task = blockIdx.x * (size_t)KG_FB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (task >= nrow * (size_t)(q + 1)) return;  // pair-uniform
    const size_t sr = task / (size_t)(q + 1);
    const int p = (int)(task % (size_t)(q + 1));
    const size_t o = kg_share_off(sr, q, p);
    lz::JL la = lz::jl_inf();
    if (!binf[0]) {
        Fr s;
        fr_from_be48(s, (p == 0 ? x : y) + o * 48);
        pl::ft_add_g2_lz(la, s.v, table, wbits, 0, 0, ft_nwin(wbits));
    }
    g2lz_out(la, h, (p == 0 ? X : Y) + o * 192);
}

// ================================================================ combine: sums over the dealer axis
// in: (m x d) x inner scalars, out: m x inner; lane = group * inner + e
__global__ __launch_bounds__(KG_FR) void k_kg_sum_fr(size_t nout, size_t inner, int d, const uint8_t* __restrict__ in,
                                                    uint8_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)KG_FR + threadIdx.x;
    if (i >= nout) return;
    const size_t g = i / inner, e = i % inner;
    uint32_t acc[8];
    Fr k;
    fr_from_be48(k, in + ((g * (size_t)d) * inner + e) * 48);
#pragma unroll
    for (int w = 0; w < 8; w++) acc[w] = k.v[w];
#pragma unroll 1
    for (int dd = 1; dd < d; dd++) {
        fr_from_be48(k, in + ((g * (size_t)d + dd) * inner + e) * 48);
        kg_add(acc, k.v);
    }
    store_fr_be48(out + i * 48, acc);
}

// in: (m x d) x inner G1 encodings, out: m x inner
__global__ __launch_bounds__(KG_FB_G1, 2) void k_kg_sum_g1(size_t nout, size_t inner, int d,
                                                          const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)KG_FB_G1 + threadIdx.x;
    if (i >= nout) return;
    const size_t g = i / inner, e = i % inner;
    lz::JG la = lz::jg_inf();
#pragma unroll 1
    for (int dd = 0; dd < d; dd++) {
        Aff<Fp> P;
        if (g1_decode(P, in + ((g * (size_t)d + dd) * inner + e) * 97))  // undecodable: the identity
            la = lz::jg_add_aff(la, ag_of(lz::reduce(lz::in_r(P.x)), lz::reduce(lz::in_r(P.y))));
    }
    g1lz_out(la, out + i * 97);
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// shares of m keygens: d_ct, d_xt, d_yt NULL for Shamir; d_y / d_yt unused when q = 0
int cck_kg_eval(size_t m, int q, int t, int total, const uint8_t* d_cf, const uint8_t* d_ct, uint8_t* d_x, uint8_t* d_y,
                uint8_t* d_xt, uint8_t* d_yt, hipStream_t st) {
    const size_t ntask = m * (size_t)(q + 1) * (size_t)total;
    if (!ntask) return 0;
    hipLaunchKernelGGL(k_kg_eval, dim3(nblocks(ntask, KG_FR)), dim3(KG_FR), 0, st, ntask, q, t, total, d_cf, d_ct, d_x,
                       d_y, d_xt, d_yt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// n = m (q + 1) t commitments over the two-base table [g, h]
int cck_kg_commit(size_t n, const uint8_t* d_cf, const uint8_t* d_ct, const uint32_t* d_table, int wbits,
                  const uint32_t* d_binf, uint8_t* d_out, hipStream_t st) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_kg_commit, dim3(nblocks(n, KG_FB_G1)), dim3(KG_FB_G1), 0, st, n, d_cf, d_ct, d_table, wbits,
                       d_binf, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// X, Y of nrow = keygens x total signer rows from their shares (group: OtherGroup, 1 or 2)
int cck_kg_derive(int group, size_t nrow, int q, const uint8_t* d_x, const uint8_t* d_y, const uint32_t* d_table,
                  int wbits, const uint32_t* d_binf, uint8_t* d_X, uint8_t* d_Y, hipStream_t st) {
    const size_t ntask = nrow * (size_t)(q + 1);
    if (!ntask) return 0;
    if (group == 1)
        hipLaunchKernelGGL(k_kg_derive_g1, dim3(nblocks(ntask, KG_FB_G1)), dim3(KG_FB_G1), 0, st, nrow, q, d_x, d_y,
                           d_table, wbits, d_binf, d_X, d_Y);
    else
        hipLaunchKernelGGL(k_kg_derive_g2, dim3(nblocks(ntask, KG_FB_G2)), dim3(2 * KG_FB_G2), 0, st, nrow, q, d_x, d_y,
                           d_table, wbits, d_binf, d_X, d_Y);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// out[g][e] = sum_{dd < d} in[g d + dd][e], e < inner: scalars (g1 = 0) or G1 encodings (g1 = 1)
int cck_kg_sum(int g1, size_t m, size_t inner, int d, const uint8_t* d_in, uint8_t* d_out, hipStream_t st) {
    const size_t nout = m * inner;
    if (!nout) return 0;
    if (g1)
        hipLaunchKernelGGL(k_kg_sum_g1, dim3(nblocks(nout, KG_FB_G1)), dim3(KG_FB_G1), 0, st, nout, inner, d, d_in,
                           d_out);
    else
        hipLaunchKernelGGL(k_kg_sum_fr, dim3(nblocks(nout, KG_FR)), dim3(KG_FR), 0, st, nout, inner, d, d_in, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
