// Pedersen VSS verify_share on the device (secret_sharing PedersenVSS::verify_share [EXT]; reference
// src/keygen.rs:141-157, 334-349), for whole batches of commitment SETS: every share of a set is checked
// against the same t coefficient commitments C_0 .. C_{t-1},
//     sum_{k<t} (id^k mod r) C_k - s g - s' h == O                                  (G1)
// issue.hip's k_vss_verify evaluates that sum bit-serially per share over full-width scalars.  Two facts
// make it cheap when every point lies in the order-r subgroup G1:
//   - the ids are 64-bit, and for points of order r the sum equals the Horner form
//     C_0 + id (C_1 + id (... + id C_{t-1})) with id as a PLAIN INTEGER: t - 1 multiplications by a
//     <= 64-bit integer, and s g + s' h is two lookups in the [g, h] table of cc_set_keygen_params;
//   - with independent 128-bit delta_i all shares of a set hold iff
//     sum_k A_k C_k - U g - U' h == O,  A_k = sum_i delta_i id_i^k, U = sum delta_i s_i, U' = sum delta_i s'_i
//     (mod r), except with probability <= 2^-127: one (t + 2)-term MSM a set, the rest Fr arithmetic.
// Both are false outside G1 (the reference's verdict there depends on id^k mod r), so a set holding a
// decodable point outside G1 is IRREGULAR and keeps the exact route of k_vss_verify.
//
//   k_vss_prep    : one lane a commitment: decoded once, the G1 test (subgroup_lz.h), affine lazy words and a
//                   flag word (0 identity or undecodable: skipped, 1 in G1, 2 outside) in straus.h's entry
//                   layout; a point outside G1 raises its set's word.  Two more lanes test g and h: either one
//                   outside G1 raises the word every set reads.
//   k_vss_exact   : one lane a share of the selected (regular) sets: Horner with the 64-bit id over the set's
//                   prepared points, the id loop on the longest id of the wave, then (-s) g + (-s') h over the
//                   table; the verdict is whether the sum is the identity.  No per-share scratch.
//   k_vss_scalars : one wave a set: A_k, U, U' with the deltas rlc_delta(key, row) of fr.h.
//   k_vss_msm     : VM_NG lanes a set: straus.h's windowed Straus over the set's commitments and A_k, the table
//                   terms of U and U' on two of the lanes, the lanes' sums added; the set's status byte.
//   k_vss_status  : the status bytes without the RLC check (rlc = 0).
//   k_vss_fill    : verdict 1 for every row of an accepted set.
//   k_vss_gather / k_vss_scatter : the irregular sets' rows side by side for cck_vss_verify (shares negated, to go
//                   with -g, -h: the reference's sum whatever the order of g and h), verdicts back.
// Rows are addressed through cck_vss_rows (launch.h): the CSR form, or the keygen outputs in place.
//
// Measured on one MI355X (tools/bench_vss_verify.py, 16-bit tables, shares dealt on the device, one batch in
// flight; DESIGN.md "Device keygen: verify_share"), milliseconds a call, SigG2 (SigG1 within 1 %):
//   4,096 committees of (t, total, q) = (3, 5, 6), 143,360 shares in 28,672 sets: cc_vss_verify_batch from host
//     memory 28.4, cc_vss_verify_sets on the same host rows 4.26, the device form 3.55, with rlc 13.2
//   8 committees of (67, 100, 32), 26,400 shares in 264 sets: 208.8, 13.26, 13.08, with rlc 9.34 (one altered
//     share: 21.4: a rejected set's rows are two waves walking 66 Horner steps, ~12 ms of latency)
#include "fixed.h"
#include "fr.h"
#include "launch.h"
#include "prove_common.h"
#include "subgroup_lz.h"

using namespace cc;

namespace {

constexpr int VS_PB = 256;  // prep, exact, fill, gather: lanes per block
constexpr int VM_NG = 16;   // lanes of one set's MSM

struct VssRow {
    uint64_t id;
    const uint8_t *s, *st;
};

DEV uint64_t vr_begin(const cck_vss_rows& a, size_t j) { return a.set_begin ? a.set_begin[j] : j * (uint64_t)a.total; }

// row `row` of set j: its id and where s and s' lie (keygen.hip kg_share_off for the keygen outputs)
DEV VssRow vr_row(const cck_vss_rows& a, size_t j, uint64_t row) {
    if (a.set_begin) {
        const uint8_t* s = a.shares + row * 96;
        return {a.ids[row], s, s + 48};
    }
    const size_t signer = row - j * (size_t)a.total, kg = j / (a.q + 1), sr = kg * a.total + signer;
    const uint32_t p = (uint32_t)(j % (a.q + 1));
    const size_t o = (p == 0 ? sr : sr * (size_t)a.q + (p - 1)) * 48;
    return {(uint64_t)signer + 1, (p == 0 ? a.x : a.y) + o, (p == 0 ? a.xt : a.yt) + o};
}

// the largest k < cnt with off[k] <= i (off non-decreasing, off[0] <= i)
DEV size_t vr_find(const uint64_t* __restrict__ off, size_t cnt, uint64_t i) {
    size_t lo = 0, hi = cnt;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// lane i of a launch over the selected sets -> (set, row); sel_off: prefix sums of the selected sets' sizes
DEV void vr_select(const cck_vss_rows& a, const uint32_t* __restrict__ sel_set, const uint64_t* __restrict__ sel_off,
                   size_t nsel, uint64_t i, size_t& j, uint64_t& row) {
    const size_t k = vr_find(sel_off, nsel, i);
    j = sel_set[k];
    row = vr_begin(a, j) + (i - sel_off[k]);
}

// the set of row `row` over all sets (empty sets share their begin with the next one: the last of them)
DEV size_t vr_set_of(const cck_vss_rows& a, size_t n_sets, uint64_t row) {
    return a.set_begin ? vr_find(a.set_begin, n_sets, row) : (size_t)(row / a.total);
}

DEV lz::AG vs_load(const uint32_t* w) {
    lz::FR ex, ey;
    ld16(ex.v, w);
    ld16(ey.v, w + SEY);
    return ag_of(ex, ey);
}

DEV uint32_t vs_wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// a + b mod r for canonical a, b (keygen.hip kg_add)
DEV void vs_add(uint32_t a[8], const uint32_t b[8]) {
    uint32_t s[8], cy = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) s[w] = __builtin_addc(a[w], b[w], cy, &cy);
    Fm r;
    fm_reduce_once(r, s);
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = r.v[w];
}

// the sum mod r of v over the wave's 64 lanes, on every lane
DEV void vs_wave_sum(uint32_t v[8]) {
#pragma unroll 1
    for (int m = 32; m > 0; m >>= 1) {
        uint32_t o[8];
#pragma unroll
        for (int w = 0; w < 8; w++) o[w] = (uint32_t)__shfl_xor((int)v[w], m);
        vs_add(v, o);
    }
}

// curve.h lane_group_sum for lazy G1 points over L consecutive lanes
template <int L>
DEV void vs_group_sum(lz::JG& acc) {
#pragma unroll 1
    for (int m = L >> 1; m > 0; m >>= 1) {
        lz::JG o;
#pragma unroll
        for (int k = 0; k < lz::LN; k++) {
            o.x.v[k] = __shfl_xor(acc.x.v[k], m);
            o.y.v[k] = __shfl_xor(acc.y.v[k], m);
            o.z.v[k] = __shfl_xor(acc.z.v[k], m);
        }
        // same operand order on both partners so they hold the same representation
        if (threadIdx.x & m) {
            const lz::JG s = acc;
            acc = o;
            o = s;
        }
        acc = lz::jg_add(acc, o);
    }
}

}  // namespace

// ================================================================ 1. commitment prep
// lanes [0, npts): commitment i of set i / t; lanes npts, npts + 1: g, h (gh: their two encodings; gh_neg: those
// of -g, -h)
__global__ __launch_bounds__(VS_PB, 2) void k_vss_prep(size_t npts, int t, const uint8_t* __restrict__ comms,
                                                   const uint8_t* __restrict__ gh, uint32_t* __restrict__ prep,
                                                   uint32_t* __restrict__ set_flag, uint32_t* __restrict__ gh_flag,
                                                   uint8_t* __restrict__ gh_neg) {
    const size_t i = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    if (i >= npts + 2) return;
    const bool base = i >= npts;
    Aff<Fp> P;
    const bool fin = g1_decode(P, base ? gh + (i - npts) * 97 : comms + i * 97);
    const bool out = fin && !g1_in_subgroup_lz(P);
    if (base) {
        if (out) atomicOr(gh_flag, 1u);
        FT<Fp>::neg(P.y, P.y);  // -g, -h for the irregular sets' route (an undecodable one: the identity encoding)
        g1_encode(gh_neg + (i - npts) * 97, P, fin);
        return;
    }
    uint32_t* w = prep + i * SEW;
    st_r1(w, lz::reduce(lz::in_r(P.x)));
    st_r1(w + SEY, lz::reduce(lz::in_r(P.y)));
    w[SEF] = fin ? (out ? 2u : 1u) : 0u;
    if (out) atomicOr(set_flag + i / (size_t)t, 1u);
}

// ================================================================ 2. exact per-share check, regular sets
__global__ __launch_bounds__(VS_PB, 2) void k_vss_exact(size_t nrow, int t, cck_vss_rows rows,
                                                    const uint32_t* __restrict__ sel_set,
                                                    const uint64_t* __restrict__ sel_off, size_t nsel,
                                                    const uint32_t* __restrict__ prep,
                                                    const uint32_t* __restrict__ table, int wbits,
                                                    const uint32_t* __restrict__ binf, uint8_t* __restrict__ verdicts) {
    const size_t i = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    const bool live = i < nrow;
    size_t j = 0;
    uint64_t row = 0;
    VssRow r{0, nullptr, nullptr};
    if (live) {
        vr_select(rows, sel_set, sel_off, nsel, i, j, row);
        r = vr_row(rows, j, row);
    }
    const uint32_t* C = prep + j * (size_t)t * SEW;
    // the id loop runs on the longest id of the wave: a lane's leading zero bits double the identity
    const int nb = (int)vs_wave_max(live ? (uint32_t)(64 - __builtin_clzll(r.id | 1ull)) : 0u);
    lz::JG acc = lz::jg_inf();
    if (live && C[(size_t)(t - 1) * SEW + SEF]) acc = lz::jg_add_aff(acc, vs_load(C + (size_t)(t - 1) * SEW));
#pragma unroll 1
    for (int k = t - 2; k >= 0; k--) {
        lz::JG m = lz::jg_inf();  // id * acc
#pragma unroll 1
        for (int b = nb - 1; b >= 0; b--) {
            m = lz::jg_dbl(m);
            if ((r.id >> b) & 1ull) m = lz::jg_add(m, acc);
        }
        acc = m;
        if (live && C[(size_t)k * SEW + SEF]) acc = lz::jg_add_aff(acc, vs_load(C + (size_t)k * SEW));
    }
    if (!live) return;
    const int nwin = ft_nwin(wbits);
    Fr s;
    if (!binf[0]) {
        fr_from_be48(s, r.s);
        ft_add_lz(acc, s.v, table, wbits, 0, 0, nwin, true);
    }
    if (!binf[1]) {
        fr_from_be48(s, r.st);
        ft_add_lz(acc, s.v, table, wbits, 1, 0, nwin, true);
    }
    verdicts[row] = lz::jg_is_inf(acc) ? 1 : 0;
}

// ================================================================ 3. RLC scalars
// block = one wave = one set; A: n_sets x t scalars (8 canonical words), UU: n_sets x (U, U')
__global__ __launch_bounds__(64) void k_vss_scalars(size_t n_sets, int t, cck_vss_rows rows,
                                                   const uint32_t* __restrict__ key, uint32_t* __restrict__ A,
                                                   uint32_t* __restrict__ UU) {
    const size_t j = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t b0 = vr_begin(rows, j), b1 = vr_begin(rows, j + 1);
    uint32_t* Aj = A + j * (size_t)t * 8;
    uint32_t u[2][8];
#pragma unroll
    for (int w = 0; w < 8; w++) u[0][w] = u[1][w] = 0;
    bool first = true;
    uint64_t c0 = b0;
    do {  // an empty set writes zeros
        const uint64_t row = c0 + lane;
        const bool live = row < b1;
        Fm p, idm;
#pragma unroll
        for (int w = 0; w < 8; w++) p.v[w] = 0;
        idm = p;
        if (live) {
            const VssRow r = vr_row(rows, j, row);
            rlc_delta(p.v, key, row);
            idm = fm_from_u64(r.id);
#pragma unroll
            for (int z = 0; z < 2; z++) {
                Fr s;
                fr_from_be48(s, z ? r.st : r.s);
                uint32_t ds[8];
                fr_mul_canon(ds, p.v, s.v);
                vs_add(u[z], ds);
            }
        }
        // p = delta id^k (canonical: the only Montgomery value is the id)
#pragma unroll 1
        for (int k = 0; k < t; k++) {
            uint32_t v[8];
#pragma unroll
            for (int w = 0; w < 8; w++) v[w] = p.v[w];
            vs_wave_sum(v);
            if (lane == 0) {
                uint32_t* o = Aj + (size_t)k * 8;
                if (!first) {
                    uint32_t old[8];
#pragma unroll
                    for (int w = 0; w < 8; w++) old[w] = o[w];
                    vs_add(v, old);
                }
#pragma unroll
                for (int w = 0; w < 8; w++) o[w] = v[w];
            }
            if (k + 1 < t) p = fm_mul_v(p, idm);
        }
        first = false;
        c0 += 64;
    } while (c0 < b1);
    vs_wave_sum(u[0]);
    vs_wave_sum(u[1]);
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < 8; w++) {
            UU[(j * 2) * 8 + w] = u[0][w];
            UU[(j * 2 + 1) * 8 + w] = u[1][w];
        }
    }
}

// ================================================================ 4. RLC MSM, status bytes
// status: 0 rejected by the RLC check (or rlc = 0: checked per share), 1 accepted, 2 irregular
// sets [j0, j0 + cnt): scratch holds cnt shares of straus_g1lz_words(t) words
__global__ __launch_bounds__(VS_PB, 2) void k_vss_msm(size_t j0, size_t cnt, int t, const uint8_t* __restrict__ comms,
                                                  const uint32_t* __restrict__ A, const uint32_t* __restrict__ UU,
                                                  const uint32_t* __restrict__ table, int wbits,
                                                  const uint32_t* __restrict__ binf,
                                                  const uint32_t* __restrict__ set_flag,
                                                  const uint32_t* __restrict__ gh_flag, uint32_t* __restrict__ scratch,
                                                  uint8_t* __restrict__ status) {
    const size_t g = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    const size_t task = g / VM_NG;
    const int part = (int)(g % VM_NG);
    if (task >= cnt) return;  // uniform over the lane group (VM_NG divides the block)
    const size_t j = j0 + task;
    if (set_flag[j] | gh_flag[0]) {
        if (part == 0) status[j] = 2;
        return;
    }
    lz::JG acc;
    straus_g1lz_lane(acc, VM_NG, part, (size_t)t, comms + j * (size_t)t * 97, A + j * (size_t)t * 8,
                     scratch + task * straus_g1lz_words((size_t)t));
    if (part < 2 && !binf[part]) ft_add_lz(acc, UU + (j * 2 + part) * 8, table, wbits, part, 0, ft_nwin(wbits), true);
    vs_group_sum<VM_NG>(acc);
    if (part == 0) status[j] = lz::jg_is_inf(acc) ? 1 : 0;
}

__global__ __launch_bounds__(VS_PB) void k_vss_status(size_t n_sets, const uint32_t* __restrict__ set_flag,
                                                     const uint32_t* __restrict__ gh_flag, uint8_t* __restrict__ status) {
    const size_t j = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    if (j < n_sets) status[j] = (set_flag[j] | gh_flag[0]) ? 2 : 0;
}

// ================================================================ 5. the driver's row kernels
__global__ __launch_bounds__(VS_PB) void k_vss_fill(size_t n, size_t n_sets, cck_vss_rows rows,
                                                   const uint8_t* __restrict__ status, uint8_t* __restrict__ verdicts) {
    const size_t row = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    if (row >= n) return;
    if (status[vr_set_of(rows, n_sets, row)] == 1) verdicts[row] = 1;
}

__global__ __launch_bounds__(VS_PB) void k_vss_gather(size_t nrow, cck_vss_rows rows, const uint32_t* __restrict__ sel_set,
                                                     const uint64_t* __restrict__ sel_off, size_t nsel,
                                                     uint32_t* __restrict__ set_of, uint64_t* __restrict__ ids,
                                                     uint8_t* __restrict__ shares, uint64_t* __restrict__ row_of) {
    const size_t i = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    if (i >= nrow) return;
    size_t j;
    uint64_t row;
    vr_select(rows, sel_set, sel_off, nsel, i, j, row);
    const VssRow r = vr_row(rows, j, row);
    set_of[i] = (uint32_t)j;
    ids[i] = r.id;
    row_of[i] = row;
    // k_vss_verify adds (r - s) g + (r - s') h, which is -(s g + s' h) only for g, h of order r: it is handed
    // -g, -h and the shares r - s, r - s', so that it adds s (-g) + s' (-h) whatever their order
    for (int z = 0; z < 2; z++) {
        Fr v;
        fr_from_be48(v, z ? r.st : r.s);
        uint32_t o = 0, neg[8], br = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) o |= v.v[w];
#pragma unroll
        for (int w = 0; w < 8; w++) neg[w] = o ? __builtin_subc(rl(w), v.v[w], br, &br) : 0u;
        store_fr_be48(shares + i * 96 + z * 48, neg);
    }
}

__global__ __launch_bounds__(VS_PB) void k_vss_scatter(size_t nrow, const uint64_t* __restrict__ row_of,
                                                      const uint8_t* __restrict__ ok, uint8_t* __restrict__ verdicts) {
    const size_t i = blockIdx.x * (size_t)VS_PB + threadIdx.x;
    if (i < nrow) verdicts[row_of[i]] = ok[i];
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

extern "C" {

size_t cck_vss_prep_words(size_t npts) { return npts * SEW; }
size_t cck_vss_msm_words(size_t t) { return straus_g1lz_words(t); }

int cck_vss_prep(size_t npts, int t, const uint8_t* d_comms, const uint8_t* d_gh, uint32_t* d_prep, uint32_t* d_set_flag,
                 uint32_t* d_gh_flag, uint8_t* d_gh_neg, hipStream_t st) {
    hipLaunchKernelGGL(k_vss_prep, dim3(nblocks(npts + 2, VS_PB)), dim3(VS_PB), 0, st, npts, t, d_comms, d_gh, d_prep,
                       d_set_flag, d_gh_flag, d_gh_neg);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_exact(size_t nrow, int t, const cck_vss_rows* rows, const uint32_t* d_sel_set, const uint64_t* d_sel_off,
                  size_t nsel, const uint32_t* d_prep, const uint32_t* d_table, int wbits, const uint32_t* d_binf,
                  uint8_t* d_verdicts, hipStream_t st) {
    if (!nrow) return 0;
    hipLaunchKernelGGL(k_vss_exact, dim3(nblocks(nrow, VS_PB)), dim3(VS_PB), 0, st, nrow, t, *rows, d_sel_set, d_sel_off,
                       nsel, d_prep, d_table, wbits, d_binf, d_verdicts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_scalars(size_t n_sets, int t, const cck_vss_rows* rows, const uint32_t* d_key, uint32_t* d_A, uint32_t* d_UU,
                    hipStream_t st) {
    if (!n_sets) return 0;
    hipLaunchKernelGGL(k_vss_scalars, dim3((unsigned)n_sets), dim3(64), 0, st, n_sets, t, *rows, d_key, d_A, d_UU);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_msm(size_t j0, size_t cnt, int t, const uint8_t* d_comms, const uint32_t* d_A, const uint32_t* d_UU,
                const uint32_t* d_table, int wbits, const uint32_t* d_binf, const uint32_t* d_set_flag,
                const uint32_t* d_gh_flag, uint32_t* d_scratch, uint8_t* d_status, hipStream_t st) {
    if (!cnt) return 0;
    hipLaunchKernelGGL(k_vss_msm, dim3(nblocks(cnt * VM_NG, VS_PB)), dim3(VS_PB), 0, st, j0, cnt, t, d_comms, d_A, d_UU,
                       d_table, wbits, d_binf, d_set_flag, d_gh_flag, d_scratch, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_status(size_t n_sets, const uint32_t* d_set_flag, const uint32_t* d_gh_flag, uint8_t* d_status,
                   hipStream_t st) {
    if (!n_sets) return 0;
    hipLaunchKernelGGL(k_vss_status, dim3(nblocks(n_sets, VS_PB)), dim3(VS_PB), 0, st, n_sets, d_set_flag, d_gh_flag,
                       d_status);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_fill(size_t n, size_t n_sets, const cck_vss_rows* rows, const uint8_t* d_status, uint8_t* d_verdicts,
                 hipStream_t st) {
    if (!n) return 0;
    hipLaunchKernelGGL(k_vss_fill, dim3(nblocks(n, VS_PB)), dim3(VS_PB), 0, st, n, n_sets, *rows, d_status, d_verdicts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_gather(size_t nrow, const cck_vss_rows* rows, const uint32_t* d_sel_set, const uint64_t* d_sel_off,
                   size_t nsel, uint32_t* d_set_of, uint64_t* d_ids, uint8_t* d_shares, uint64_t* d_row_of,
                   hipStream_t st) {
    if (!nrow) return 0;
    hipLaunchKernelGGL(k_vss_gather, dim3(nblocks(nrow, VS_PB)), dim3(VS_PB), 0, st, nrow, *rows, d_sel_set, d_sel_off,
                       nsel, d_set_of, d_ids, d_shares, d_row_of);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int cck_vss_scatter(size_t nrow, const uint64_t* d_row_of, const uint8_t* d_ok, uint8_t* d_verdicts, hipStream_t st) {
    if (!nrow) return 0;
    hipLaunchKernelGGL(k_vss_scatter, dim3(nblocks(nrow, VS_PB)), dim3(VS_PB), 0, st, nrow, d_row_of, d_ok, d_verdicts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
