// C ABI, keygen: Pedersen VSS verify_share over commitment sets (vss.hip) — the exact fast path and the
// per-set RLC, in the CSR form and over the keygen outputs in place.  Single-slot calls: they wait for the
// concurrency slots' batches and are ordered on the context's stream.
#include "ctx.h"

namespace {

// the drivers' workspaces (cc_ctx::vss)
enum VssBuf {
    VB_PREP,    // prepared commitments
    VB_FLAG,    // one word a set, then the word of g and h
    VB_STATUS,  // one status byte a set
    VB_KEY,     // the delta key
    VB_SCAL,    // A_k of every set, then U, U'
    VB_MSM,     // the Straus scratch of one MSM launch
    VB_BEGIN,   // set_begin
    VB_SEL,     // the selected sets of the two per-share launches: offsets (8-byte), then set indices
    VB_GHNEG,   // -g | -h encoded, for the irregular sets' route
    VB_G_SET, VB_G_IDS, VB_G_SH, VB_G_ROW, VB_G_OK, VB_G_SCR,  // the irregular sets' gathered rows
    // the host form's device copies
    VB_H_COMM, VB_H_IDS, VB_H_SH, VB_H_VER
};

constexpr size_t kMsmBytes = (size_t)512 << 20;  // Straus scratch of one MSM launch at most (one set at least)

struct Sets {
    size_t n, t, n_sets;
    const uint64_t* set_begin;  // host; NULL: keygen-shaped, sets of `total` rows
    size_t total;
    uint64_t begin(size_t j) const { return set_begin ? set_begin[j] : j * total; }
};

// verdicts of rows [0, n) over the commitment sets at d_comm; rows: device pointers, set_begin filled in here
cc_status vss_sets_device(cc_ctx* c, const Sets& S, cck_vss_rows rows, const uint8_t* d_comm, int rlc,
                          const uint8_t* seed32, uint8_t* d_verdicts, uint32_t* stats4, hipStream_t st) {
    const size_t n = S.n, t = S.t, ns = S.n_sets, npts = ns * t;
    DevBuf* B = c->vss;
    const size_t msm_words = cck_vss_msm_words(t);
    const size_t msm_sets = std::max<size_t>(1, std::min(ns, kMsmBytes / (msm_words * 4)));
    if (B[VB_PREP].ensure(cck_vss_prep_words(npts) * 4) || B[VB_FLAG].ensure((ns + 1) * 4) || B[VB_STATUS].ensure(ns) || B[VB_GHNEG].ensure(2 * 97) ||
        B[VB_SEL].ensure(2 * (ns + 1) * 8 + 2 * ns * 4))
        return CC_ERR_HIP;
    if (S.set_begin && B[VB_BEGIN].ensure((ns + 1) * 8)) return CC_ERR_HIP;
    if (rlc && (B[VB_KEY].ensure(32) || B[VB_SCAL].ensure((npts + 2 * ns) * 32) ||
                B[VB_MSM].ensure(msm_sets * msm_words * 4)))
        return CC_ERR_HIP;
    StreamOrder order(c, st);
    uint32_t* flag = B[VB_FLAG].as<uint32_t>();
    uint8_t* status = B[VB_STATUS].as<uint8_t>();
    const uint32_t *table = c->kg_gh_table.as<uint32_t>(), *binf = c->kg_gh_inf.as<uint32_t>();
    if (S.set_begin) {
        KCK(HipMem::h2d(B[VB_BEGIN].p, S.set_begin, (ns + 1) * 8, st));
        rows.set_begin = B[VB_BEGIN].as<uint64_t>();
    }
    HIPCK(hipMemsetAsync(flag, 0, (ns + 1) * 4, st));
    KCK(cck_vss_prep(npts, (int)t, d_comm, c->kg_gh_enc.as<uint8_t>(), B[VB_PREP].as<uint32_t>(), flag, flag + ns,
                     B[VB_GHNEG].as<uint8_t>(), st));
    if (rlc) {
        uint32_t* A = B[VB_SCAL].as<uint32_t>();
        uint32_t* UU = A + npts * 8;
        KCK(HipMem::h2d(B[VB_KEY].p, seed32, 32, st));
        KCK(cck_vss_scalars(ns, (int)t, &rows, B[VB_KEY].as<uint32_t>(), A, UU, st));
        for (size_t j0 = 0; j0 < ns; j0 += msm_sets)
            KCK(cck_vss_msm(j0, std::min(msm_sets, ns - j0), (int)t, d_comm, A, UU, table, c->kg_wbits, binf, flag,
                            flag + ns, B[VB_MSM].as<uint32_t>(), status, st));
    } else {
        KCK(cck_vss_status(ns, flag, flag + ns, status, st));
    }
    std::vector<uint8_t> stat(ns, 0);
    KCK(HipMem::d2h(stat.data(), status, ns, st));
    KCK(HipMem::sync(st));  // the one synchronisation: the status bytes decide what is launched next
    // the plan: the sets checked per share by k_vss_exact (rlc: the rejected ones) and the irregular ones,
    // each as the prefix sums of their sizes and their indices
    std::vector<uint64_t>& plan = c->vss_plan;  // kept until the next call's synchronisation: the uploads read it
    plan.assign(2 * (ns + 1) + ns, 0);
    uint64_t *off_e = plan.data(), *off_i = off_e + ns + 1;
    uint32_t *set_e = reinterpret_cast<uint32_t*>(off_i + ns + 1), *set_i = set_e + ns;
    size_t ne = 0, ni = 0, rejected = 0, irregular = 0;
    for (size_t j = 0; j < ns; j++) {
        const uint64_t len = S.begin(j + 1) - S.begin(j);
        if (stat[j] == 2) {
            irregular++;
            if (!len) continue;
            set_i[ni] = (uint32_t)j;
            off_i[ni + 1] = off_i[ni] + len;
            ni++;
        } else if (stat[j] == 0) {
            if (rlc) rejected++;
            if (!len) continue;
            set_e[ne] = (uint32_t)j;
            off_e[ne + 1] = off_e[ne] + len;
            ne++;
        }
    }
    const size_t rows_e = (size_t)off_e[ne], rows_i = (size_t)off_i[ni];
    if (stats4)
        stats4[0] = (uint32_t)ns, stats4[1] = (uint32_t)rejected, stats4[2] = (uint32_t)irregular,
        stats4[3] = (uint32_t)(rows_e + rows_i);
    KCK(HipMem::h2d(B[VB_SEL].p, plan.data(), plan.size() * 8, st));
    const uint64_t *d_off_e = B[VB_SEL].as<uint64_t>(), *d_off_i = d_off_e + ns + 1;
    const uint32_t *d_set_e = reinterpret_cast<const uint32_t*>(d_off_i + ns + 1), *d_set_i = d_set_e + ns;
    if (rlc) KCK(cck_vss_fill(n, ns, &rows, status, d_verdicts, st));  // every row of an accepted set verifies
    KCK(cck_vss_exact(rows_e, (int)t, &rows, d_set_e, d_off_e, ne, B[VB_PREP].as<uint32_t>(), table, c->kg_wbits, binf,
                      d_verdicts, st));
    if (rows_i) {
        // the irregular sets' rows side by side through cc_vss_verify_batch's kernel, verdicts back
        if (B[VB_G_SET].ensure(rows_i * 4) || B[VB_G_IDS].ensure(rows_i * 8) || B[VB_G_SH].ensure(rows_i * 96) ||
            B[VB_G_ROW].ensure(rows_i * 8) || B[VB_G_OK].ensure(rows_i) || B[VB_G_SCR].ensure(rows_i * (t + 2) * 33 * 4))
            return CC_ERR_HIP;
        KCK(cck_vss_gather(rows_i, &rows, d_set_i, d_off_i, ni, B[VB_G_SET].as<uint32_t>(), B[VB_G_IDS].as<uint64_t>(),
                           B[VB_G_SH].as<uint8_t>(), B[VB_G_ROW].as<uint64_t>(), st));
        const uint8_t* gh = B[VB_GHNEG].as<uint8_t>();  // -g, -h with the shares k_vss_gather negated
        KCK(cck_vss_verify(rows_i, (int)t, gh, gh + 97, d_comm, B[VB_G_SET].as<uint32_t>(), B[VB_G_IDS].as<uint64_t>(),
                           B[VB_G_SH].as<uint8_t>(), B[VB_G_SCR].as<uint32_t>(), B[VB_G_OK].as<uint8_t>(), st));
        KCK(cck_vss_scatter(rows_i, B[VB_G_ROW].as<uint64_t>(), B[VB_G_OK].as<uint8_t>(), d_verdicts, st));
    }
    return CC_OK;
}

// the checks behind the NULL checks, in the header's order
cc_status sets_checks(const cc_ctx* c, size_t n, size_t t, size_t n_sets, const uint64_t* set_begin) {
    if (!c->have_kg || !c->kg_have_gh) return CC_ERR_STATE;
    if (t == 0 || t > 4096 || n > kMaxBatch || n_sets > kMaxBatch || n_sets * t > kMaxBatch) return CC_ERR_DECODE;
    if (set_begin[0] != 0 || set_begin[n_sets] != n) return CC_ERR_DECODE;
    for (size_t j = 0; j < n_sets; j++)
        if (set_begin[j] > set_begin[j + 1]) return CC_ERR_DECODE;
    return CC_OK;
}

}  // namespace

cc_status cc_vss_verify_sets_device(cc_ctx* c, size_t n, size_t t, size_t n_sets, const uint64_t* set_begin,
                                    const uint8_t* d_commitments, const uint64_t* d_ids, const uint8_t* d_shares,
                                    int rlc, const uint8_t* seed32, uint8_t* d_verdicts, uint32_t* stats4,
                                    void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!d_commitments || !d_ids || !d_shares || !d_verdicts)) || !set_begin || (rlc && !seed32))
        return CC_ERR_DECODE;
    if (cc_status s = sets_checks(c, n, t, n_sets, set_begin)) return s;
    if (stats4) stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    cck_vss_rows rows{nullptr, d_ids, d_shares, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return vss_sets_device(c, Sets{n, t, n_sets, set_begin, 0}, rows, d_commitments, rlc, seed32, d_verdicts, stats4,
                           stream ? (hipStream_t)stream : c->stream);
}

cc_status cc_vss_verify_sets(cc_ctx* c, size_t n, size_t t, size_t n_sets, const uint64_t* set_begin,
                             const uint8_t* commitments, const uint64_t* ids, const uint8_t* shares, int rlc,
                             uint8_t* verdicts, uint32_t* stats4) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (n && (!commitments || !ids || !shares || !verdicts)) || !set_begin) return CC_ERR_DECODE;
    if (cc_status s = sets_checks(c, n, t, n_sets, set_begin)) return s;
    if (stats4) stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
    if (!n) return CC_OK;
    uint8_t seed[32] = {0};
    if (rlc && fresh_seed(seed)) return CC_ERR_HIP;
    HIPCK(hipSetDevice(c->device));
    drain_slots(c);
    hipStream_t st = c->stream;
    DevBuf* B = c->vss;
    if (B[VB_H_COMM].ensure(n_sets * t * 97) || B[VB_H_IDS].ensure(n * 8) || B[VB_H_SH].ensure(n * 96) ||
        B[VB_H_VER].ensure(n))
        return CC_ERR_HIP;
    HostForm f(st);
    f.up(B[VB_H_COMM], commitments, n_sets * t * 97);
    f.up(B[VB_H_IDS], ids, n * 8);
    f.up(B[VB_H_SH], shares, n * 96);
    f.launch([&] {
        cck_vss_rows rows{nullptr, B[VB_H_IDS].as<uint64_t>(), B[VB_H_SH].as<uint8_t>(), nullptr, nullptr, nullptr,
                          nullptr, 0, 0};
        return vss_sets_device(c, Sets{n, t, n_sets, set_begin, 0}, rows, B[VB_H_COMM].as<uint8_t>(), rlc, seed,
                               B[VB_H_VER].as<uint8_t>(), stats4, st);
    });
    f.down(verdicts, B[VB_H_VER], n);
    return f.finish();
}

cc_status cc_keygen_verify_shares_batch_device(cc_ctx* c, size_t m, size_t q, size_t t, size_t total,
                                               const uint8_t* d_x, const uint8_t* d_y, const uint8_t* d_xt,
                                               const uint8_t* d_yt, const uint8_t* d_comm, int rlc,
                                               const uint8_t* seed32, uint8_t* d_verdicts, uint32_t* stats4,
                                               void* stream) {
    c = primary(c);  // a device set forwards to its first device
    if (!c || (m && total && (!d_x || !d_xt || !d_comm || !d_verdicts || (q && (!d_y || !d_yt)))) || (rlc && !seed32))
        return CC_ERR_DECODE;
    if (!c->have_kg || !c->kg_have_gh) return CC_ERR_STATE;
    if (t == 0 || t > 4096) return CC_ERR_DECODE;
    if (t > total) return CC_ERR_THRESHOLD;
    if (total > kMaxIds || q > kMaxQ || m > kMaxBatch) return CC_ERR_DECODE;
    // m <= 2^26, q + 1 < 2^13, total <= 2^16, t < 2^13: the products stay below 2^55
    const size_t n_sets = m * (q + 1), n = n_sets * total;
    if (n_sets > kMaxBatch || n > kMaxBatch || n_sets * t > kMaxBatch) return CC_ERR_DECODE;
    if (stats4) stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
    if (!n) return CC_OK;
    HIPCK(hipSetDevice(c->device));
    cck_vss_rows rows{nullptr, nullptr, nullptr, d_x, d_y, d_xt, d_yt, (uint32_t)q, (uint32_t)total};
    return vss_sets_device(c, Sets{n, t, n_sets, nullptr, total}, rows, d_comm, rlc, seed32, d_verdicts, stats4,
                           stream ? (hipStream_t)stream : c->stream);
}
