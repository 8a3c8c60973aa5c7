// Holder-side issuance kernels for gfx950: SignatureRequest::new ("PrepareBlindSign", reference
// src/signature.rs:124-192) and SignatureRequestPoK::init / gen_proof (216-320), the steps before
// cc_sigreq_verify_batch and cc_blind_sign_batch.  Every sum is in the SignatureGroup.
//
//   new, per request with fresh r, k_0 .. k_{k-1}:
//       commitment = sum_{i<k} m_i h_i + r g,   h = compute_h(commitment, m_k ..)  (hash.hip, between)
//       c1_i = k_i g,   c2_i = k_i pk + m_i h
//   init, with blindings b_sk | hb_0 .. hb_{k-1} | b_r | k x (b1_i | b2_i):
//       T_sk = b_sk g,  T_comm = sum hb_i h_i + b_r g,  T_1i = b1_i g,  T_2i = b2_i pk + hb_i h
//     k_rq_long_*  : the commitment or T_comm, k + 1 bases over the request params' fixed-base tables
//       (cc_set_request_params: table base q = g), no doublings; one request per lane (SigG1) or per
//       lane pair (SigG2).
//     k_rq_short_* : the single-base sums c1_i, or T_sk and T_1i, over g's table; one (request, j) per
//       lane or lane pair.  A launch of its own: its tasks are a factor k + 1 shorter than the long
//       sums, and no wave holds both kinds.
//     k_rq_table_* : per request the signed 4-bit-window table of (pk, h), the multiples 1..8 of each
//       normalised with one inversion (prove_common.h), written to scratch.
//     k_rq_two_*   : c2_i or T_2i, one (request, i) per lane or lane pair: 65 windows, two digit streams,
//       reading its request's table.
//   gen_proof: k_rq_responses, one lane per (request, response): b - chal * secret mod r into the proof
//     record (sigreq_layout.h).
//   k_rq_h_rows lays commitment || known messages out as compute_h's input rows.
#include "fixed.h"
#include "launch.h"
#include "prove_common.h"
#include "sigreq_layout.h"

using namespace cc;

namespace {

constexpr int RQ_FB_G1 = 256;  // fixed-base kernels, G1 sums: tasks per block (one lane each)
constexpr int RQ_FB_G2 = 128;  // fixed-base kernels, G2 sums: tasks per block (one lane pair each)
constexpr int RQ_TB_G1 = 64;   // two-base kernels, G1: requests / tasks per block (one lane each)
constexpr int RQ_TB_G2 = 128;  // two-base kernels, G2: requests / tasks per block (one lane pair each)
constexpr int RQ_DIGB = 132;   // digit bytes of one two-base task (2 x 65, rounded to words)

// scalars of one request: rnd = r | k_0 .. (k + 1 values), blind = b_sk | hb_0 .. | b_r | k x (b1 | b2)
__host__ __device__ inline size_t rq_blind_stride(int k) { return (size_t)(3 * k + 2); }

// the long sum's scalars: hidden term i < k, then g's
DEV const uint8_t* rq_long_scalar(bool init, size_t r, int q, int k, int i, const uint8_t* msgs, const uint8_t* rnd) {
    if (init) return rnd + (r * rq_blind_stride(k) + 1 + i) * 48;  // hb_i, i == k: b_r
    return i < k ? msgs + (r * (size_t)q + i) * 48 : rnd + r * (size_t)(k + 1) * 48;  // m_i, r
}
DEV uint8_t* rq_long_out(bool init, size_t r, int k, size_t sb, uint8_t* out) {
    const ProofLayout L{sb, (size_t)k};
    return init ? out + r * L.bytes() + L.t_comm() : out + r * sb;
}
// the single-base sums: new has k a request (c1_j), init k + 1 (T_sk, T_1j)
DEV const uint8_t* rq_short_scalar(bool init, size_t r, int k, int j, const uint8_t* rnd) {
    if (!init) return rnd + (r * (size_t)(k + 1) + 1 + j) * 48;  // k_j
    const size_t S = rq_blind_stride(k);
    return j == 0 ? rnd + r * S * 48 : rnd + (r * S + k + 2 + 2 * (size_t)(j - 1)) * 48;  // b_sk, b1_{j-1}
}
DEV uint8_t* rq_short_out(bool init, size_t r, int k, int j, size_t sb, uint8_t* out) {
    if (!init) return out + (r * (size_t)k + j) * 2 * sb;  // c1_j
    const ProofLayout L{sb, (size_t)k};
    return out + r * L.bytes() + (j == 0 ? L.t_sk() : L.ct(j - 1));
}
// the two-base sums: scalar of pk, scalar of h, output
DEV const uint8_t* rq_two_a(bool init, size_t r, int k, int i, const uint8_t* rnd) {
    return init ? rnd + (r * rq_blind_stride(k) + k + 3 + 2 * (size_t)i) * 48  // b2_i
                : rnd + (r * (size_t)(k + 1) + 1 + i) * 48;                      // k_i
}
DEV const uint8_t* rq_two_b(bool init, size_t r, int q, int k, int i, const uint8_t* msgs, const uint8_t* rnd) {
    return init ? rnd + (r * rq_blind_stride(k) + 1 + i) * 48 : msgs + (r * (size_t)q + i) * 48;  // hb_i, m_i
}
DEV uint8_t* rq_two_out(bool init, size_t r, int k, int i, size_t sb, uint8_t* out) {
    if (!init) return out + ((r * (size_t)k + i) * 2 + 1) * sb;  // c2_i
    const ProofLayout L{sb, (size_t)k};
    return out + r * L.bytes() + L.ct(i) + sb + 48;  // T_2i
}

// the digits of the task's two scalars: dig[0..65) for pk, dig[65..130) for h
DEV void rq_digits(int8_t* dig, const uint8_t* a48, const uint8_t* b48) {
    Fr a, b;
    fr_from_be48(a, a48);
    fr_from_be48(b, b48);
    alignas(16) uint32_t x[8], y[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
        x[w] = a.v[w];
        y[w] = b.v[w];
    }
    recode_w4(dig, x);
    recode_w4(dig + 65, y);
}

}  // namespace

// ================================================================ commitment / T_comm (k + 1 bases)
// SigG1: one request per lane on the lazy field (fixed.h ft_add_lz)
__global__ __launch_bounds__(RQ_FB_G1, 2) void k_rq_long_g1(size_t n, int q, int k, bool init,
                                                           const uint8_t* __restrict__ msgs,
                                                           const uint8_t* __restrict__ rnd,
                                                           const uint32_t* __restrict__ table, int wbits,
                                                           const uint32_t* __restrict__ binf,
                                                           uint8_t* __restrict__ out) {
    const size_t r = blockIdx.x * (size_t)RQ_FB_G1 + threadIdx.x;
    if (r >= n) return;
    const int nwin = ft_nwin(wbits);
    lz::JG la = lz::jg_inf();
    Fr s;
    for (int i = 0; i <= k; i++) {
        const int base = i < k ? i : q;  // table base q = g
        if (binf[base]) continue;
        fr_from_be48(s, rq_long_scalar(init, r, q, k, i, msgs, rnd));
        ft_add_lz(la, s.v, table, wbits, base, 0, nwin);
    }
    g1lz_out(la, rq_long_out(init, r, k, 97, out));
}

// SigG2: one request per lane pair on the lazy pair-lane field (curve_pl.h ft_add_g2_lz)
__global__ __launch_bounds__(2 * RQ_FB_G2, 2) void k_rq_long_g2(size_t n, int q, int k, bool init,
                                                               const uint8_t* __restrict__ msgs,
                                                               const uint8_t* __restrict__ rnd,
                                                               const uint32_t* __restrict__ table, int wbits,
                                                               const uint32_t* __restrict__ binf,
                                                               uint8_t* __restrict__ out) {
    const size_t r = blockIdx.x * (size_t)RQ_FB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (r >= n) return;  // pair-uniform
    const int nwin = ft_nwin(wbits);
    lz::JL la = lz::jl_inf();
    Fr s;
    for (int i = 0; i <= k; i++) {
        const int base = i < k ? i : q;  // table base q = g
        if (binf[base]) continue;
        fr_from_be48(s, rq_long_scalar(init, r, q, k, i, msgs, rnd));
        pl::ft_add_g2_lz(la, s.v, table, wbits, base, 0, nwin);
    }
    g2lz_out(la, h, rq_long_out(init, r, k, 192, out));
}

// ================================================================ c1_j / T_sk, T_1j (one base: g)
__global__ __launch_bounds__(RQ_FB_G1, 2) void k_rq_short_g1(size_t n, int q, int k, bool init,
                                                            const uint8_t* __restrict__ rnd,
                                                            const uint32_t* __restrict__ table, int wbits,
                                                            const uint32_t* __restrict__ binf,
                                                            uint8_t* __restrict__ out) {
    const int ns = init ? k + 1 : k;
    const size_t t = blockIdx.x * (size_t)RQ_FB_G1 + threadIdx.x;
    if (t >= n * (size_t)ns) return;
    const size_t r = t / ns;
    const int j = (int)(t % ns);
    lz::JG la = lz::jg_inf();
    if (!binf[q]) {
        Fr s;
        fr_from_be48(s, rq_short_scalar(init, r, k, j, rnd));
        ft_add_lz(la, s.v, table, wbits, q, 0, ft_nwin(wbits));
    }
    g1lz_out(la, rq_short_out(init, r, k, j, 97, out));
}

__global__ __launch_bounds__(2 * RQ_FB_G2, 2) void k_rq_short_g2(size_t n, int q, int k, bool init,
                                                                const uint8_t* __restrict__ rnd,
                                                                const uint32_t* __restrict__ table, int wbits,
                                                                const uint32_t* __restrict__ binf,
                                                                uint8_t* __restrict__ out) {
    const int ns = init ? k + 1 : k;
    const size_t t = blockIdx.x * (size_t)RQ_FB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (t >= n * (size_t)ns) return;  // pair-uniform
    const size_t r = t / ns;
    const int j = (int)(t % ns);
    lz::JL la = lz::jl_inf();
    if (!binf[q]) {
        Fr s;
        fr_from_be48(s, rq_short_scalar(init, r, k, j, rnd));
        pl::ft_add_g2_lz(la, s.v, table, wbits, q, 0, ft_nwin(wbits));
    }
    g2lz_out(la, h, rq_short_out(init, r, k, j, 192, out));
}

// ================================================================ the per-request table of (pk, h)
// SigG2: one request per lane pair; tab: n x sp_table_words_g2()
__global__ __launch_bounds__(2 * RQ_TB_G2, 2) void k_rq_table_g2(size_t n, const uint8_t* __restrict__ pk,
                                                                const uint8_t* __restrict__ hp,
                                                                uint32_t* __restrict__ tab) {
    using namespace lz;
    const size_t r = blockIdx.x * (size_t)RQ_TB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (r >= n) return;  // pair-uniform
    uint32_t* ent = tab + r * sp_table_words_g2();
    uint32_t* zs = ent + SP_ENT * 2 * SEW;
    uint32_t* pre = zs + SP_ENT * 2 * LN;
    F2R acc_z = r_one();
    sp_fill_g2(ent, zs, pre, h, 0, pk + r * 192, acc_z);
    sp_fill_g2(ent, zs, pre, h, 1, hp + r * 192, acc_z);
    sp_norm_g2(ent, zs, pre, h, acc_z);
}

// SigG1: one request per lane; tab: n x sp_table_words_g1()
__global__ __launch_bounds__(RQ_TB_G1) void k_rq_table_g1(size_t n, const uint8_t* __restrict__ pk,
                                                          const uint8_t* __restrict__ hp,
                                                          uint32_t* __restrict__ tab) {
    using namespace lz;
    const size_t r = blockIdx.x * (size_t)RQ_TB_G1 + threadIdx.x;
    if (r >= n) return;
    uint32_t* ent = tab + r * sp_table_words_g1();
    uint32_t* zs = ent + SP_ENT * SEW;
    uint32_t* pre = zs + SP_ENT * LN;
    FR acc_z = r1_one();
    sp_fill_g1(ent, zs, pre, 0, pk + r * 97, acc_z);
    sp_fill_g1(ent, zs, pre, 1, hp + r * 97, acc_z);
    sp_norm_g1(ent, zs, pre, acc_z);
}

// ================================================================ c2_i / T_2i = a pk + b h
// One (request, i) per lane pair (SigG2) or lane (SigG1); digs: n k x RQ_DIGB bytes.
__global__ __launch_bounds__(2 * RQ_TB_G2, 2) void k_rq_two_g2(size_t n, int q, int k, bool init,
                                                              const uint8_t* __restrict__ msgs,
                                                              const uint8_t* __restrict__ rnd,
                                                              const uint32_t* __restrict__ tab,
                                                              int8_t* __restrict__ digs, uint8_t* __restrict__ out) {
    using namespace lz;
    const size_t t = blockIdx.x * (size_t)RQ_TB_G2 + (threadIdx.x >> 1);
    const int h = threadIdx.x & 1;
    if (t >= n * (size_t)k) return;  // pair-uniform
    const size_t r = t / k;
    const int i = (int)(t % k);
    const uint32_t* ent = tab + r * sp_table_words_g2();
    int8_t* dig = digs + t * RQ_DIGB;
    rq_digits(dig, rq_two_a(init, r, k, i, rnd), rq_two_b(init, r, q, k, i, msgs, rnd));  // both lanes: same digits
    JL acc = jl_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jl_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jl_dbl(acc);
        const int da = dig[win], db = dig[65 + win];
        if (da) sp_add_g2(acc, ent, h, 0, da);
        if (db) sp_add_g2(acc, ent, h, 1, db);
    }
    g2lz_out(acc, h, rq_two_out(init, r, k, i, 192, out));
}

__global__ __launch_bounds__(RQ_TB_G1) void k_rq_two_g1(size_t n, int q, int k, bool init,
                                                        const uint8_t* __restrict__ msgs,
                                                        const uint8_t* __restrict__ rnd,
                                                        const uint32_t* __restrict__ tab, int8_t* __restrict__ digs,
                                                        uint8_t* __restrict__ out) {
    using namespace lz;
    const size_t t = blockIdx.x * (size_t)RQ_TB_G1 + threadIdx.x;
    if (t >= n * (size_t)k) return;
    const size_t r = t / k;
    const int i = (int)(t % k);
    const uint32_t* ent = tab + r * sp_table_words_g1();
    int8_t* dig = digs + t * RQ_DIGB;
    rq_digits(dig, rq_two_a(init, r, k, i, rnd), rq_two_b(init, r, q, k, i, msgs, rnd));
    JG acc = jg_inf();
#pragma unroll 1
    for (int win = 64; win >= 0; win--) {
        if (win != 64 && !jg_is_inf(acc))
#pragma unroll 1
            for (int z = 0; z < 4; z++) acc = jg_dbl(acc);
        const int da = dig[win], db = dig[65 + win];
        if (da) sp_add_g1(acc, ent, 0, da);
        if (db) sp_add_g1(acc, ent, 1, db);
    }
    g1lz_out(acc, rq_two_out(init, r, k, i, 97, out));
}

// ================================================================ compute_h's input rows
// row r (len = sb + 48 (q - k) bytes): commitment_r || m_k .. m_{q-1}; offsets[r] = r len, offsets[n] = n len
__global__ __launch_bounds__(64) void k_rq_h_rows(size_t n, int q, int k, size_t sb,
                                                  const uint8_t* __restrict__ commitment,
                                                  const uint8_t* __restrict__ msgs, uint8_t* __restrict__ data,
                                                  uint64_t* __restrict__ offsets) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t kb = (size_t)(q - k) * 48, len = sb + kb;
    uint8_t* row = data + r * len;
    for (size_t b = 0; b < sb; b++) row[b] = commitment[r * sb + b];
    const uint8_t* m = msgs + (r * (size_t)q + k) * 48;
    for (size_t b = 0; b < kb; b++) row[sb + b] = m[b];
    offsets[r] = r * len;
    if (r == 0) offsets[n] = n * len;
}

// ================================================================ gen_proof responses
// One lane per (request, response j), 4k + 2 a request, each b - chal * secret mod r:
//   j = 0: r_sk (b_sk, sk);  j = 1 + i, i < k: r_comm[i] (hb_i, m_i);  j = 1 + k: r_comm[k] (b_r, r);
//   j = k + 2 + 3i + {0, 1, 2}: r_1 (b1_i, k_i), r_2a (b2_i, k_i), r_2b (hb_i, m_i)
__global__ __launch_bounds__(256) void k_rq_responses(size_t n, int q, int k, size_t sb,
                                                      const uint8_t* __restrict__ msgs,
                                                      const uint8_t* __restrict__ rnd,
                                                      const uint8_t* __restrict__ blind,
                                                      const uint8_t* __restrict__ sk,
                                                      const uint8_t* __restrict__ chal, uint8_t* __restrict__ proofs) {
    const int nr = 4 * k + 2;
    const size_t gi = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (gi >= n * (size_t)nr) return;
    const size_t r = gi / nr;
    const int j = (int)(gi % nr);
    const ProofLayout L{sb, (size_t)k};
    const uint8_t* bl = blind + r * rq_blind_stride(k) * 48;
    const uint8_t* rn = rnd + r * (size_t)(k + 1) * 48;
    const uint8_t* ms = msgs + r * (size_t)q * 48;
    const uint8_t *bp, *sp;
    size_t off;
    if (j == 0) {
        bp = bl;
        sp = sk + r * 48;
        off = L.r_sk();
    } else if (j <= k) {
        bp = bl + (size_t)j * 48;
        sp = ms + (size_t)(j - 1) * 48;
        off = L.r_comm(j - 1);
    } else if (j == k + 1) {
        bp = bl + (size_t)(k + 1) * 48;
        sp = rn;
        off = L.r_comm(k);
    } else {
        const int i = (j - k - 2) / 3, w = (j - k - 2) % 3;
        if (w == 0) {
            bp = bl + (size_t)(k + 2 + 2 * i) * 48;
            sp = rn + (size_t)(1 + i) * 48;
            off = L.ct(i) + sb;
        } else if (w == 1) {
            bp = bl + (size_t)(k + 3 + 2 * i) * 48;
            sp = rn + (size_t)(1 + i) * 48;
            off = L.ct(i) + 2 * sb + 48;
        } else {
            bp = bl + (size_t)(1 + i) * 48;
            sp = ms + (size_t)i * 48;
            off = L.ct(i) + 2 * sb + 96;
        }
    }
    Fr b, c, s;
    fr_from_be48(b, bp);
    fr_from_be48(c, chal + r * 48);
    fr_from_be48(s, sp);
    Fm x, y, d;
    fr_mul_canon(y.v, c.v, s.v);
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = b.v[w];
    fm_sub(d, x, y);
    Fp o;
#pragma unroll
    for (int w = 0; w < NL; w++) o.v[w] = w < 8 ? d.v[w] : 0u;
    store_be48_bytes(proofs + r * L.bytes() + off, o);  // SigG1 records (sb = 97) misalign the fields
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

// scratch of cck_rq_two_base for n requests of k ciphertexts (group 1: SigG1): table words, digit bytes
size_t cck_rq_table_words(int group, size_t n) {
    return n * (group == 1 ? sp_table_words_g1() : sp_table_words_g2());
}
size_t cck_rq_digit_bytes(size_t n, int k) { return (n * (size_t)k * RQ_DIGB + 255) / 256 * 256; }

// init = 0: commitment (n x SG at d_long), c1_i (into d_out = the ciphertexts); init = 1: T_comm, T_sk and
// T_1i into the proof records at d_out (d_long = d_out).  d_rnd: rand (new) or blind (init).
int cck_rq_fixed(int group, size_t n, int q, int k, int init, const uint8_t* d_msgs, const uint8_t* d_rnd,
                 const uint32_t* d_table, int wbits, const uint32_t* d_binf, uint8_t* d_long, uint8_t* d_out,
                 hipStream_t st) {
    if (!n) return 0;
    const size_t ns = n * (size_t)(init ? k + 1 : k);
    if (group == 1) {
        hipLaunchKernelGGL(k_rq_long_g1, dim3(nblocks(n, RQ_FB_G1)), dim3(RQ_FB_G1), 0, st, n, q, k, init != 0, d_msgs,
                           d_rnd, d_table, wbits, d_binf, d_long);
        if (ns)
            hipLaunchKernelGGL(k_rq_short_g1, dim3(nblocks(ns, RQ_FB_G1)), dim3(RQ_FB_G1), 0, st, n, q, k, init != 0,
                               d_rnd, d_table, wbits, d_binf, d_out);
    } else {
        hipLaunchKernelGGL(k_rq_long_g2, dim3(nblocks(n, RQ_FB_G2)), dim3(2 * RQ_FB_G2), 0, st, n, q, k, init != 0,
                           d_msgs, d_rnd, d_table, wbits, d_binf, d_long);
        if (ns)
            hipLaunchKernelGGL(k_rq_short_g2, dim3(nblocks(ns, RQ_FB_G2)), dim3(2 * RQ_FB_G2), 0, st, n, q, k,
                               init != 0, d_rnd, d_table, wbits, d_binf, d_out);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// c2_i (init = 0, into the ciphertexts at d_out) or T_2i (init = 1, into the proof records): the
// per-request table of (pk, h) into d_tab, then one task per (request, i)
int cck_rq_two_base(int group, size_t n, int q, int k, int init, const uint8_t* d_pk, const uint8_t* d_h,
                    const uint8_t* d_msgs, const uint8_t* d_rnd, uint32_t* d_tab, int8_t* d_digs, uint8_t* d_out,
                    hipStream_t st) {
    if (!n || !k) return 0;
    const size_t nt = n * (size_t)k;
    if (group == 1) {
        hipLaunchKernelGGL(k_rq_table_g1, dim3(nblocks(n, RQ_TB_G1)), dim3(RQ_TB_G1), 0, st, n, d_pk, d_h, d_tab);
        hipLaunchKernelGGL(k_rq_two_g1, dim3(nblocks(nt, RQ_TB_G1)), dim3(RQ_TB_G1), 0, st, n, q, k, init != 0, d_msgs,
                           d_rnd, d_tab, d_digs, d_out);
    } else {
        hipLaunchKernelGGL(k_rq_table_g2, dim3(nblocks(n, RQ_TB_G2)), dim3(2 * RQ_TB_G2), 0, st, n, d_pk, d_h, d_tab);
        hipLaunchKernelGGL(k_rq_two_g2, dim3(nblocks(nt, RQ_TB_G2)), dim3(2 * RQ_TB_G2), 0, st, n, q, k, init != 0,
                           d_msgs, d_rnd, d_tab, d_digs, d_out);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// d_data: n x (sb + 48 (q - k)) bytes (+ 16), d_offsets: n + 1
int cck_rq_h_rows(int group, size_t n, int q, int k, const uint8_t* d_commitment, const uint8_t* d_msgs,
                  uint8_t* d_data, uint64_t* d_offsets, hipStream_t st) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_rq_h_rows, dim3(nblocks(n, 64)), dim3(64), 0, st, n, q, k, (size_t)(group == 1 ? 97 : 192),
                       d_commitment, d_msgs, d_data, d_offsets);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_rq_responses(int group, size_t n, int q, int k, const uint8_t* d_msgs, const uint8_t* d_rnd,
                     const uint8_t* d_blind, const uint8_t* d_sk, const uint8_t* d_chal, uint8_t* d_proofs,
                     hipStream_t st) {
    if (!n) return 0;
    const size_t nr = n * (size_t)(4 * k + 2);
    hipLaunchKernelGGL(k_rq_responses, dim3(nblocks(nr, 256)), dim3(256), 0, st, n, q, k,
                       (size_t)(group == 1 ? 97 : 192), d_msgs, d_rnd, d_blind, d_sk, d_chal, d_proofs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
