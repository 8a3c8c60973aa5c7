// Issuer-side device forms for gfx950: SignatureRequestProof::verify (reference src/signature.rs:324-377)
// over the request params' fixed-base tables, with every input in HBM.  The verdict is the one issue.hip
// k_sigreq_checks + k_sigreq_combine define (scalars mod r, an undecodable point is the identity and is
// skipped, a check passes iff sum resp B + chal C - T is the identity); the way to each check's sum differs.
//
//   Per request the 2 + 2k Schnorr checks are
//       sk    : r_sk g                              + c pk          - T_sk
//       comm  : sum_{i<k} r_comm[i] h_i + r_comm[k] g + c commitment  - T_comm
//       ct1_i : r_1i g                              + c c1_i        - T_1i
//       ct2_i : r_2a pk + r_2b h                    + c c2_i        - T_2i
//   k_iv_table_* : per request ONE table of the signed 4-bit-window multiples 1..8 of its 3 + 2k variable
//       bases [pk, h, commitment, c1_0, c2_0, ..], normalised with one inversion (prove_common.h sp_fill_*),
//       and the 65 signed digits of the challenge, recoded once.  No endomorphism: keys and ciphertexts may
//       lie outside the subgroup, and the digits are those of the integer c mod r.
//   k_iv_check_* : one check per lane (SigG1) or lane pair (SigG2).  The variable-base terms of a check
//       share ONE chain of 65 windows (4 doublings a window; one digit stream for sk / comm / ct1, three for
//       ct2: r_2a over pk, r_2b over h, c over c2_i); the fixed-base terms (g, h_i) are then added from
//       the request params' window tables with no doubling (fixed.h ft_add_lz / curve_pl.h ft_add_g2_lz),
//       then -T, and the lane writes whether the sum is the identity.  The three kinds of check run as
//       three launches (kind 0: sk and ct1_i, kind 1: comm, kind 2: ct2_i), so no wave mixes one-stream
//       with three-stream chains or one fixed-base term with k + 1.  Every addition is curve_lz.h's mixed
//       addition, which handles an identity accumulator, equal and opposite operands.
//   The verdict is then issue.hip k_sigreq_combine's: a request passes iff its checks passed and
//   r_2b[i] == r_comm[i] as Fr values.
#include "fixed.h"
#include "launch.h"
#include "prove_common.h"
#include "sigreq_layout.h"

using namespace cc;

namespace {

constexpr int IV_TB_G1 = 64;    // requests / checks per block (one lane each)
constexpr int IV_TB_G2 = 128;   // requests / checks per block (one lane pair each)
constexpr int IV_CDIGB = 68;    // digit bytes of a request's challenge (65, rounded to words)
constexpr int IV_DIGB = 132;    // digit bytes of one ct2 check's responses (2 x 65, rounded to words)

__host__ __device__ inline int iv_nbases(int k) { return 3 + 2 * k; }  // pk, h, commitment, k x (c1, c2)
__host__ __device__ inline size_t iv_table_words_g1(int k) { return (size_t)8 * iv_nbases(k) * (SEW + 2 * lz::LN); }
__host__ __device__ inline size_t iv_table_words_g2(int k) { return 2 * iv_table_words_g1(k); }

// the 65 signed digits of a 48-byte scalar, reduced mod r
DEV void iv_digits(int8_t* dig, const uint8_t* s48) {
    Fr a;
    fr_from_be48(a, s48);
    alignas(16) uint32_t x[8];
#pragma unroll
    for (int w = 0; w < 8; w++) x[w] = a.v[w];
    recode_w4(dig, x);
}

// one check of a launch of `kind`: its request, its variable base's table index, its index among the
// request's checks, T and (kinds 0 and 1) the response of g
struct IvTask {
    size_t r;
    int vbase, chk, i;
    const uint8_t *T, *rg;
};
DEV IvTask iv_task(int kind, size_t t, int k, const ProofLayout& L, const uint8_t* proof) {
    IvTask o;
    if (kind == 0) {
        o.r = t / (size_t)(k + 1);
        const int j = (int)(t % (size_t)(k + 1));
        o.i = j - 1;
        const uint8_t* pr = proof + o.r * L.bytes();
        if (j == 0) {
            o.vbase = 0, o.chk = 0, o.T = pr + L.t_sk(), o.rg = pr + L.r_sk();
        } else {
            const uint8_t* rec = pr + L.ct(o.i);
            o.vbase = 3 + 2 * o.i, o.chk = 2 + 2 * o.i, o.T = rec, o.rg = rec + L.sb;
        }
    } else if (kind == 1) {
        o.r = t;
        o.i = 0;
        const uint8_t* pr = proof + o.r * L.bytes();
        o.vbase = 2, o.chk = 1, o.T = pr + L.t_comm(), o.rg = pr + L.r_comm(k);
    } else {
        o.r = t / (size_t)k;
        o.i = (int)(t % (size_t)k);
        const uint8_t* rec = proof + o.r * L.bytes() + L.ct(o.i);
        o.vbase = 4 + 2 * o.i, o.chk = 3 + 2 * o.i, o.T = rec + L.sb + 48, o.rg = nullptr;
    }
    return o;
}
__host__ __device__ inline size_t iv_ntasks(int kind, size_t n, int k) {
    return kind == 0 ? n * (size_t)(k + 1) : kind == 1 ? n : n * (size_t)k;
}

}  // namespace

// ================================================================ the per-request table and challenge digits
__global__ __launch_bounds__(2 * IV_TB_G2, 2) void k_iv_table_g2(size_t n, int k, const uint8_t* __restrict__ pk,
                                                                const uint8_t* __restrict__ hp,
                                                                const uint8_t* __restrict__ comm,
                                                                const uint8_t* __restrict__ cts,
                                                                const uint8_t* __restrict__ chal,
                                                                uint32_t* __restrict__ tab, int8_t* __restrict__ cdig) {
    using namespace lz;
    const size_t r = blockIdx.x * (size_t)IV_TB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (r >= n) return;  // pair-uniform
    const int ne = 8 * iv_nbases(k);
    uint32_t* ent = tab + r * iv_table_words_g2(k);
    uint32_t* zs = ent + (size_t)ne * 2 * SEW;
    uint32_t* pre = zs + (size_t)ne * 2 * LN;
    F2R acc_z = r_one();
    sp_fill_g2(ent, zs, pre, h, 0, pk + r * 192, acc_z);
    sp_fill_g2(ent, zs, pre, h, 1, hp + r * 192, acc_z);
    sp_fill_g2(ent, zs, pre, h, 2, comm + r * 192, acc_z);
#pragma unroll 1
    for (int j = 0; j < 2 * k; j++) sp_fill_g2(ent, zs, pre, h, 3 + j, cts + (r * (size_t)k * 2 + j) * 192, acc_z);
    sp_norm_g2(ent, zs, pre, h, acc_z, ne);
    iv_digits(cdig + r * IV_CDIGB, chal + r * 48);  // both lanes: same digits
}

__global__ __launch_bounds__(IV_TB_G1) void k_iv_table_g1(size_t n, int k, const uint8_t* __restrict__ pk,
                                                          const uint8_t* __restrict__ hp,
                                                          const uint8_t* __restrict__ comm,
                                                          const uint8_t* __restrict__ cts,
                                                          const uint8_t* __restrict__ chal, uint32_t* __restrict__ tab,
                                                          int8_t* __restrict__ cdig) {
    using namespace lz;
    const size_t r = blockIdx.x * (size_t)IV_TB_G1 + threadIdx.x;
    if (r >= n) return;
    const int ne = 8 * iv_nbases(k);
    uint32_t* ent = tab + r * iv_table_words_g1(k);
    uint32_t* zs = ent + (size_t)ne * SEW;
    uint32_t* pre = zs + (size_t)ne * LN;
    FR acc_z = r1_one();
    sp_fill_g1(ent, zs, pre, 0, pk + r * 97, acc_z);
    sp_fill_g1(ent, zs, pre, 1, hp + r * 97, acc_z);
    sp_fill_g1(ent, zs, pre, 2, comm + r * 97, acc_z);
#pragma unroll 1
    for (int j = 0; j < 2 * k; j++) sp_fill_g1(ent, zs, pre, 3 + j, cts + (r * (size_t)k * 2 + j) * 97, acc_z);
    sp_norm_g1(ent, zs, pre, acc_z, ne);
    iv_digits(cdig + r * IV_CDIGB, chal + r * 48);
}

// ================================================================ one Schnorr check per lane pair / lane
__global__ __launch_bounds__(2 * IV_TB_G2, 2) void k_iv_check_g2(int kind, size_t n, int q, int k,
                                                                const uint8_t* __restrict__ proof,
                                                                const uint32_t* __restrict__ tab,
                                                                const int8_t* __restrict__ cdig,
                                                                int8_t* __restrict__ digs,
                                                                const uint32_t* __restrict__ table, int wbits,
                                                                const uint32_t* __restrict__ binf,
                                                                uint8_t* __restrict__ ok) {
    using namespace lz;
    const size_t t = blockIdx.x * (size_t)IV_TB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (t >= iv_ntasks(kind, n, k)) return;  // pair-uniform
    const ProofLayout L{192, (size_t)k};
    const IvTask tk = iv_task(kind, t, k, L, proof);
    const uint32_t* ent = tab + tk.r * iv_table_words_g2(k);
    const int8_t* cd = cdig + tk.r * IV_CDIGB;
    int8_t* dig = digs + t * IV_DIGB;  // kind 2 alone
    if (kind == 2) {
        const uint8_t* rec = tk.T - 192 - 48;
        iv_digits(dig, rec + 2 * 192 + 48);       // r_2a, over pk
        iv_digits(dig + 65, rec + 2 * 192 + 96);  // r_2b, over h
    }
    JL acc = jl_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jl_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jl_dbl(acc);
        if (kind == 2) {
            const int da = dig[win], db = dig[65 + win];
            if (da) sp_add_g2(acc, ent, h, 0, da);
            if (db) sp_add_g2(acc, ent, h, 1, db);
        }
        const int dc = cd[win];
        if (dc) sp_add_g2(acc, ent, h, tk.vbase, dc);
    }
    const int nwin = ft_nwin(wbits);
    Fr s;
    if (kind == 1) {
#pragma unroll 1
        for (int i = 0; i < k; i++) {
            if (binf[i]) continue;
            fr_from_be48(s, proof + tk.r * L.bytes() + L.r_comm(i));
            pl::ft_add_g2_lz(acc, s.v, table, wbits, i, 0, nwin);
        }
    }
    if (kind != 2 && !binf[q]) {  // table base q = g
        fr_from_be48(s, tk.rg);
        pl::ft_add_g2_lz(acc, s.v, table, wbits, q, 0, nwin);
    }
    cc::Aff<cc::Fp2> T1;
    if (pl::pair_all(g2_decode(T1, tk.T))) {
        pl::Fp2 hx, hy;
        hx.c = h ? T1.x.b : T1.x.a;
        hy.c = h ? T1.y.b : T1.y.a;
        acc = jl_add_aff(acc, jl_neg_aff(AL{reduce(in_r2(hx)), reduce(in_r2(hy))}));
    }
    const bool pass = jl_is_inf(acc);
    if (!h) ok[tk.r * (size_t)(2 + 2 * k) + tk.chk] = pass ? 1 : 0;
}

__global__ __launch_bounds__(IV_TB_G1) void k_iv_check_g1(int kind, size_t n, int q, int k,
                                                          const uint8_t* __restrict__ proof,
                                                          const uint32_t* __restrict__ tab,
                                                          const int8_t* __restrict__ cdig, int8_t* __restrict__ digs,
                                                          const uint32_t* __restrict__ table, int wbits,
                                                          const uint32_t* __restrict__ binf, uint8_t* __restrict__ ok) {
    using namespace lz;
    const size_t t = blockIdx.x * (size_t)IV_TB_G1 + threadIdx.x;
    if (t >= iv_ntasks(kind, n, k)) return;
    const ProofLayout L{97, (size_t)k};
    const IvTask tk = iv_task(kind, t, k, L, proof);
    const uint32_t* ent = tab + tk.r * iv_table_words_g1(k);
    const int8_t* cd = cdig + tk.r * IV_CDIGB;
    int8_t* dig = digs + t * IV_DIGB;  // kind 2 alone
    if (kind == 2) {
        const uint8_t* rec = tk.T - 97 - 48;
        iv_digits(dig, rec + 2 * 97 + 48);       // r_2a, over pk
        iv_digits(dig + 65, rec + 2 * 97 + 96);  // r_2b, over h
    }
    JG acc = jg_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jg_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jg_dbl(acc);
        if (kind == 2) {
            const int da = dig[win], db = dig[65 + win];
            if (da) sp_add_g1(acc, ent, 0, da);
            if (db) sp_add_g1(acc, ent, 1, db);
        }
        const int dc = cd[win];
        if (dc) sp_add_g1(acc, ent, tk.vbase, dc);
    }
    const int nwin = ft_nwin(wbits);
    Fr s;
    if (kind == 1) {
#pragma unroll 1
        for (int i = 0; i < k; i++) {
            if (binf[i]) continue;
            fr_from_be48(s, proof + tk.r * L.bytes() + L.r_comm(i));
            ft_add_lz(acc, s.v, table, wbits, i, 0, nwin);
        }
    }
    if (kind != 2 && !binf[q]) {  // table base q = g
        fr_from_be48(s, tk.rg);
        ft_add_lz(acc, s.v, table, wbits, q, 0, nwin);
    }
    cc::Aff<cc::Fp> T1;
    if (g1_decode(T1, tk.T)) {
        const FR tx = reduce(in_r(T1.x)), ty = reduce(in_r(T1.y));
        acc = jg_add_aff(acc, ag_of(tx, neg(ty)));
    }
    ok[tk.r * (size_t)(2 + 2 * k) + tk.chk] = jg_is_inf(acc) ? 1 : 0;
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// scratch of cck_iv_checks for n requests of k ciphertexts (group 1: SigG1): table words, challenge digit
// bytes, response digit bytes, check flags
size_t cck_iv_table_words(int group, size_t n, int k) {
    return n * (group == 1 ? iv_table_words_g1(k) : iv_table_words_g2(k));
}
size_t cck_iv_cdig_bytes(size_t n) { return (n * IV_CDIGB + 255) / 256 * 256; }
size_t cck_iv_dig_bytes(size_t n, int k) { return (n * (size_t)k * IV_DIGB + 255) / 256 * 256; }
size_t cck_iv_ok_bytes(size_t n, int k) { return n * (size_t)(2 + 2 * k); }

// the checks' flags into d_ok (n x (2 + 2k)), for issue.hip k_sigreq_combine (cck_sigreq_combine);
// d_table / d_binf: the request params' tables of [h_0 .. h_{q-1}, g] and their identity flags
int cck_iv_checks(int group, size_t n, int q, int k, const uint8_t* d_comm, const uint8_t* d_cts, const uint8_t* d_pk,
                  const uint8_t* d_proof, const uint8_t* d_chal, const uint8_t* d_h, const uint32_t* d_table,
                  int wbits, const uint32_t* d_binf, uint32_t* d_tab, int8_t* d_cdig, int8_t* d_digs, uint8_t* d_ok,
                  hipStream_t st) {
    if (!n) return 0;
    if (group == 1) {
        hipLaunchKernelGGL(k_iv_table_g1, dim3(nblocks(n, IV_TB_G1)), dim3(IV_TB_G1), 0, st, n, k, d_pk, d_h, d_comm,
                           d_cts, d_chal, d_tab, d_cdig);
        for (int kind = 0; kind < 3; kind++) {
            const size_t nt = iv_ntasks(kind, n, k);
            if (nt)
                hipLaunchKernelGGL(k_iv_check_g1, dim3(nblocks(nt, IV_TB_G1)), dim3(IV_TB_G1), 0, st, kind, n, q, k,
                                   d_proof, d_tab, d_cdig, d_digs, d_table, wbits, d_binf, d_ok);
        }
    } else {
        hipLaunchKernelGGL(k_iv_table_g2, dim3(nblocks(n, IV_TB_G2)), dim3(2 * IV_TB_G2), 0, st, n, k, d_pk, d_h,
                           d_comm, d_cts, d_chal, d_tab, d_cdig);
        for (int kind = 0; kind < 3; kind++) {
            const size_t nt = iv_ntasks(kind, n, k);
            if (nt)
                hipLaunchKernelGGL(k_iv_check_g2, dim3(nblocks(nt, IV_TB_G2)), dim3(2 * IV_TB_G2), 0, st, kind, n, q,
                                   k, d_proof, d_tab, d_cdig, d_digs, d_table, wbits, d_binf, d_ok);
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
